// Counterpart of the reference's buildMesh, updateMeshColors and updateSuperPlateBorders (js/planet-mesh.js:620-836, :840-957,
// :533-576) on the device, for hosts without WebGL: the displaced Voronoi-fan mesh of a planet as the Float32Arrays the reference
// hands to three.js, bit for bit (csrc/globe_ops.h), its wireframe, its super-plate borders, and all of it as one binary glTF file.
// The mesh and the lines come from HIP kernels (csrc/globe.hip) on the planet bound to `mesh` (native.js: planetFor); there is no
// JavaScript fallback for them.  computePlateColors and the GLB encoder run on the host, here and in globe_export.py, byte for byte alike.
// A view is a map type other than `landmask` (buildMesh has no such branch), a layer of MAP_LAYERS, or `plates`.
import addon, { planetFor } from './native.js';
import { MAP_TYPES, MAP_LAYERS } from './map-export.js';
import { globeFilename, encodeGlb } from './globe-glb.js';
import { windArrowsOnPlanet, oceanCurrentArrowsOnPlanet, itczLine, globeGrid } from './overlay-export.js';
import { riverLinesOnPlanet } from './rivers.js';
import { OUTLINE_GLOBE_BASE, buildOutlineOnPlanet, outlineSegments } from './outline-export.js';

export const GLOBE_PLATES = 'plates';
export const GLOBE_TYPE_VIEWS = MAP_TYPES.filter((t) => t !== 'landmask');
export { LINE_OPACITY, GLB_MAX_BYTES, globeFilename, setHSL, computePlateColors, encodeGlb } from './globe-glb.js';

// ---- the device calls --------------------------------------------------------------------------------------------------------
function checkSides(triangles, halfedges) {
    if (!(triangles instanceof Int32Array) || !(halfedges instanceof Int32Array)) throw new TypeError('buildMesh: mesh.triangles and mesh.halfedges must be Int32Arrays');
}
// view -> what the addon takes; opts: { values, plates: { r_plate, plateSeeds, plateColors } }
function meshOnPlanet(planet, triangles, halfedges, r_elevation, view, opts, positions, colors) {
    checkSides(triangles, halfedges);
    const o = opts || {};
    if (view === GLOBE_PLATES) {
        const pl = o.plates || {};
        const seeds = pl.plateSeeds === undefined || pl.plateSeeds === null ? null : Int32Array.from(pl.plateSeeds);
        return addon.globeMeshPlates(planet, triangles, halfedges, pl.r_plate || null, seeds, pl.plateColors || null, r_elevation || null, positions, colors);
    }
    if (view === 'landmask') throw new RangeError("buildMesh: 'landmask' is no view of the globe: buildMesh has no such branch");
    const type = MAP_TYPES.indexOf(view), layer = MAP_LAYERS.indexOf(view);
    if (type < 0 && layer < 0) throw new RangeError(`buildMesh: unknown globe view '${view}' (one of ${GLOBE_TYPE_VIEWS.concat(MAP_LAYERS, [GLOBE_PLATES]).join(', ')})`);
    return addon.globeMesh(planet, triangles, halfedges, layer >= 0 ? 1 : 0, layer >= 0 ? layer : type, o.values || null, r_elevation || null, positions, colors);
}
// on a planet handle (what the worker holds); r_elevation null: the planet's resident field
export function buildMeshOnPlanet(planet, triangles, halfedges, r_elevation, view, opts) { return meshOnPlanet(planet, triangles, halfedges, r_elevation, view || 'color', opts, true, true); }
export function meshColorsOnPlanet(planet, triangles, halfedges, r_elevation, view, opts) { return meshOnPlanet(planet, triangles, halfedges, r_elevation, view || 'color', opts, false, true).color; }
export function wireframeOnPlanet(planet, triangles, halfedges, r_elevation) {
    checkSides(triangles, halfedges);
    return addon.globeLines(planet, triangles, halfedges, 0, r_elevation || null, null);
}
export function superPlateBordersOnPlanet(planet, triangles, halfedges, r_elevation, superPlates) {
    checkSides(triangles, halfedges);
    if (!(superPlates instanceof Float32Array)) throw new TypeError('updateSuperPlateBorders: superPlates must be a Float32Array of numRegions entries');
    return addon.globeLines(planet, triangles, halfedges, 1, r_elevation || null, superPlates);
}

// buildMesh(mesh, r_xyz, r_elevation, view = 'color', { values, plates }) -> { position, color: Float32Array(numSides * 9), bounds: Float32Array(6) }
export function buildMesh(mesh, r_xyz, r_elevation, view, opts) { return buildMeshOnPlanet(planetFor(mesh, r_xyz), mesh.triangles, mesh.halfedges, r_elevation, view, opts); }
// updateMeshColors(mesh, r_xyz, r_elevation, view, { values, plates }) -> Float32Array(numSides * 9): the colours alone
export function updateMeshColors(mesh, r_xyz, r_elevation, view, opts) { return meshColorsOnPlanet(planetFor(mesh, r_xyz), mesh.triangles, mesh.halfedges, r_elevation, view, opts); }
// buildWireframe(mesh, r_xyz, r_elevation) -> Float32Array(segments * 6)
export function buildWireframe(mesh, r_xyz, r_elevation) { return wireframeOnPlanet(planetFor(mesh, r_xyz), mesh.triangles, mesh.halfedges, r_elevation); }
// updateSuperPlateBorders(mesh, r_xyz, r_elevation, superPlates) -> Float32Array(segments * 6): the globe form
export function updateSuperPlateBorders(mesh, r_xyz, r_elevation, superPlates) { return superPlateBordersOnPlanet(planetFor(mesh, r_xyz), mesh.triangles, mesh.halfedges, r_elevation, superPlates); }

// the globe in one view on a planet handle: { filename, position, color, bounds[, wireframe][, superPlateBorders][, windArrows][, oceanCurrentArrows][, itcz][, grid][, rivers][, outlines][, glb] }
export function exportGlobeOnPlanet(planet, triangles, halfedges, r_elevation, view, seed, opts) {
    const o = opts || {};
    const res = buildMeshOnPlanet(planet, triangles, halfedges, r_elevation, view, o);
    res.filename = globeFilename(view || 'color', seed);
    if (o.wireframe) res.wireframe = wireframeOnPlanet(planet, triangles, halfedges, r_elevation);
    if (o.superPlates) res.superPlateBorders = superPlateBordersOnPlanet(planet, triangles, halfedges, r_elevation, o.superPlates);
    // the overlays (js/overlay-export.js): windArrows, oceanCurrentArrows: 'summer' | 'winter'; itcz: { itczLons, itczLats } of the season; grid: degrees
    if (o.windArrows) res.windArrows = windArrowsOnPlanet(planet, o.windArrows, 0).globe;
    if (o.oceanCurrentArrows) res.oceanCurrentArrows = oceanCurrentArrowsOnPlanet(planet, o.oceanCurrentArrows, 0, r_elevation).globe;
    if (o.itcz) res.itcz = itczLine(o.itcz.itczLons, o.itcz.itczLats).globe;
    if (o.grid !== undefined && o.grid !== null) res.grid = globeGrid(o.grid);
    // rivers: { minFlow }, the segments of the planet's rivers block that reach it (js/rivers.js)
    if (o.rivers !== undefined && o.rivers !== null) res.rivers = riverLinesOnPlanet(planet, o.rivers.minFlow, r_elevation).segments;
    // outlines: { source, values, levels, onlyClass }, the rings of js/outline-export.js at base 1.002 as segments
    if (o.outlines !== undefined && o.outlines !== null) {
        const rings = buildOutlineOnPlanet(planet, triangles, halfedges, o.outlines.source, Object.assign({}, o.outlines, { r_elevation, base: OUTLINE_GLOBE_BASE, lonlat: false }));
        res.outlines = outlineSegments(rings);
    }
    if (o.glb !== false) {
        res.glb = encodeGlb(res, { wireframe: res.wireframe, superPlateBorders: res.superPlateBorders, windArrows: res.windArrows, oceanCurrentArrows: res.oceanCurrentArrows,
                                   itcz: res.itcz, grid: res.grid, rivers: res.rivers, outlines: res.outlines });
    }
    return res;
}
// exportGlobe(mesh, r_xyz, r_elevation, view, seed, { values, plates, wireframe, superPlates, windArrows, oceanCurrentArrows, itcz, grid, rivers, outlines, glb })
export function exportGlobe(mesh, r_xyz, r_elevation, view, seed, opts) {
    return exportGlobeOnPlanet(planetFor(mesh, r_xyz), mesh.triangles, mesh.halfedges, r_elevation, view, seed, opts);
}
