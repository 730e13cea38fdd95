// The globe view for hosts without WebGL, a page or a <canvas>: the displaced globe mesh seen through a camera, as RGBA8 pixels and,
// through encodePng (js/map-export.js), a PNG file (ours; csrc/view.hip, the contract is in csrc/view_ops.h).  The reference draws this
// picture with three.js (js/scene.js); its camera (50 degrees at (0, 0.4, 2.8), looking at the centre) and its sun (5, 3, 4) are the
// defaults here, its lighting and tone pipeline are not reproduced: with `shade` each facet is lit by one Lambert term,
// min(255, floor(c * (ambient + diffuse * lambert) + 0.5)) per channel.  The raster, the colouring and the shade pass run in HIP kernels
// on the planet bound to `mesh` (native.js: planetFor); colours, layers and their needs are exportMap's.  No JavaScript fallback.
import addon, { planetFor } from './native.js';
import { MAP_TYPES, MAP_LAYERS, mapTypeId, mapLayerId, exportFilename, layerFilename } from './map-export.js';

export const VIEW_MAX_SIZE = 16384;
export const VIEW_SUN = [5, 3, 4];
export const VIEW_BACKGROUND = 0xFF080303;                                 // the scene colour 0x030308, opaque: R | G << 8 | B << 16 | A << 24
export const VIEW_DEFAULTS = { fov: 50, distance: 2.8, halfHeight: 1.1, exaggeration: 1, ambient: 0.55, diffuse: 0.45 };

// ours: exportFilename's stems (a name that is no type's: the layer's) behind `orogen-globe-`
export function viewFilename(name, seed) {
    const stem = MAP_TYPES.indexOf(name) >= 0 ? exportFilename(name, seed) : layerFilename(name, seed);
    return `orogen-globe-${stem.slice('orogen-'.length)}`;
}

// { lon, lat, distance, fov, halfHeight } (degrees; north is +Y, longitude 0 is +Z) or { eye, fov, halfHeight } -> { eye, fov, halfHeight };
// nothing: the reference's camera.  fov 0 is the orthographic camera of half height halfHeight.  The library checks the values.
export function viewCamera(camera) {
    const c = camera || {};
    const fov = c.fov === undefined || c.fov === null ? VIEW_DEFAULTS.fov : c.fov;
    const halfHeight = c.halfHeight === undefined || c.halfHeight === null ? VIEW_DEFAULTS.halfHeight : c.halfHeight;
    if (typeof fov !== 'number' || typeof halfHeight !== 'number') throw new TypeError('renderGlobe: camera.fov and camera.halfHeight must be numbers');
    if (c.eye !== undefined && c.eye !== null) {
        const eye = Array.from(c.eye);
        if (eye.length !== 3 || eye.some((v) => typeof v !== 'number')) throw new TypeError('renderGlobe: camera.eye must hold three numbers');
        return { eye, fov, halfHeight };
    }
    if (c.lon === undefined && c.lat === undefined) return { eye: [0, 0.4, 2.8], fov, halfHeight };
    const lon = c.lon || 0, lat = c.lat || 0, distance = c.distance === undefined || c.distance === null ? VIEW_DEFAULTS.distance : c.distance;
    if (typeof lon !== 'number' || typeof lat !== 'number' || typeof distance !== 'number') throw new TypeError('renderGlobe: camera.lon, camera.lat and camera.distance must be numbers');
    if (!(lat >= -90 && lat <= 90)) throw new RangeError('renderGlobe: camera.lat must be from -90 to 90 degrees');
    const lo = lon * Math.PI / 180, la = lat * Math.PI / 180;
    return { eye: [distance * Math.cos(la) * Math.sin(lo), distance * Math.sin(la), distance * Math.cos(la) * Math.cos(lo)], fov, halfHeight };
}

function checkSize(width, height) {
    for (const [k, v] of [['width', width], ['height', height]])
        if (!(Number.isInteger(v) && v >= 1 && v <= VIEW_MAX_SIZE)) throw new RangeError(`renderGlobe: ${k} must be an integer from 1 to 16384`);
}

// the thirteen numbers of addon.viewRaster's params (napi/worogen_napi.cc) from { camera, shade, exaggeration, light, ambient, diffuse, background }
export function viewParams(opts) {
    const o = opts || {}, cam = viewCamera(o.camera), pick = (v, d) => (v === undefined || v === null ? d : v);
    const light = Array.from(pick(o.light, VIEW_SUN));
    if (light.length !== 3) throw new TypeError('renderGlobe: light must hold three numbers');
    const background = pick(o.background, VIEW_BACKGROUND);
    if (!(Number.isInteger(background) && background >= 0 && background <= 0xFFFFFFFF)) throw new RangeError('renderGlobe: background must be an integer from 0 to 0xFFFFFFFF (R | G << 8 | B << 16 | A << 24)');
    return Float64Array.from([cam.eye[0], cam.eye[1], cam.eye[2], cam.fov, cam.halfHeight, pick(o.exaggeration, VIEW_DEFAULTS.exaggeration), pick(o.shade, true) ? 1 : 0,
                              light[0], light[1], light[2], pick(o.ambient, VIEW_DEFAULTS.ambient), pick(o.diffuse, VIEW_DEFAULTS.diffuse), background]);
}

// layers: names of MAP_LAYERS other than `debug`, or { name, values } with a Float32Array (under any other name: coloured as `debug`)
function checkedLayers(layers) {
    return Array.from(layers || []).map((l) => {
        const name = typeof l === 'string' ? l : l && l.name, values = typeof l === 'string' ? null : (l && l.values) || null;
        const id = (values && MAP_LAYERS.indexOf(name) < 0) ? 0 : mapLayerId(name);
        if (id === 0 && !values) throw new RangeError("renderGlobe: the map layer 'debug' takes its values from the caller");
        return { name, id, values };
    });
}

// one view raster, one colour pass per type and per layer, on a planet handle (what the worker holds); r_elevation null: the planet's
// resident field; opts.rivers: a minimum flow for the types' maps (the planet's rivers block), null or undefined: off
export function renderGlobeOnPlanet(planet, triangles, halfedges, r_elevation, types, width, height, opts) {
    checkSize(width, height);
    const ids = types.map(mapTypeId), layers = checkedLayers(opts && opts.layers), e = r_elevation || null;
    const rivers = opts && opts.rivers !== undefined && opts.rivers !== null ? opts.rivers : null;
    const r = addon.viewRaster(planet, triangles, halfedges, width, height, viewParams(opts), e, false);
    const maps = ids.map((id, k) => ({ type: types[k], rgba: rivers === null ? addon.mapColor(planet, id, e) : addon.mapColorRivers(planet, id, e, rivers) }));
    for (const l of layers) maps.push({ type: l.name, rgba: addon.mapColorLayer(planet, l.id, l.values, e) });
    return { width: r.width, height: r.height, covered: r.covered, uncovered: r.uncovered, maps };
}

// renderGlobe(mesh, r_xyz, r_elevation, types, width, height, { camera, layers, shade, exaggeration, light, ambient, diffuse, background })
//   -> { width, height, covered, uncovered, maps: [{ type, rgba }] }; types: one name or several
export function renderGlobe(mesh, r_xyz, r_elevation, types, width, height, opts) {
    if (!mesh || !(mesh.triangles instanceof Int32Array) || !(mesh.halfedges instanceof Int32Array)) throw new TypeError('renderGlobe: mesh.triangles and mesh.halfedges must be Int32Arrays');
    if (!(r_elevation instanceof Float32Array) || r_elevation.length !== mesh.numRegions) throw new RangeError(`renderGlobe: r_elevation must be a Float32Array of ${mesh.numRegions} entries`);
    const names = typeof types === 'string' ? [types] : Array.from(types);
    return renderGlobeOnPlanet(planetFor(mesh, r_xyz), mesh.triangles, mesh.halfedges, r_elevation, names, width, height, opts);
}

// the depth map of the planet's last view raster: Float32Array(width * height), NaN where nothing covers the pixel
export function viewDepth(mesh, r_xyz) { return addon.viewDepth(planetFor(mesh, r_xyz)); }
