// Counterpart of the reference's exportMap / exportMapBatch (js/planet-mesh.js:1752-2180) on the device, for hosts without WebGL, a
// page or a <canvas>: the equirectangular map of a planet as RGBA8 pixels and, from them, a PNG file.  The raster and the colouring
// run in HIP kernels (csrc/map.hip) on the planet bound to `mesh` (native.js: planetFor); the triangle list and the region colours
// are the reference's bit for bit and the coverage rule is the one csrc/map_ops.h fixes (WebGL's own pixels differ between GPUs).
// `biome` and `koppen` read the Koppen block that classifyKoppen (js/koppen.js) left on the planet; without one the call throws
// `no Koppen result`: the reference's silent fallback to the colour map is not offered.  No JavaScript fallback for the device passes.
// Beyond the export button, the reference's map view (buildMapMesh, :200-382) draws around a centre meridian and shows the layers of
// its debugLayer switch: `centerLon` (radians, within [-pi, pi]) and `layers` offer both.  A climate layer reads the block its stage
// left on the planet (`no wind result` and so on without one); any other array is coloured by debugValueToColor over its own range.
// exportCubeMap / exportCubeMapBatch give the cube map instead (ours; csrc/cube.hip, the contract is in csrc/cube_ops.h): six square faces
// by gnomonic projection, exactly the globe mesh seen from its centre, in the OpenGL order of CUBE_FACES.  The six faces lie stacked in
// one faceSize x 6 faceSize image on the device; each face handed out is a view of that one buffer.
import zlib from 'zlib';
import addon, { planetFor } from './native.js';

// the reference's type names in the order of WO_MAP_COLOR .. WO_MAP_KOPPEN (include/worogen.h)
export const MAP_TYPES = ['color', 'heightmap', 'landheightmap', 'landmask', 'biome', 'koppen'];

// the reference's debugLayer names in the order of WO_MAP_LAYER_DEBUG .. WO_MAP_LAYER_WINDSPEED_WINTER; `debug` is any other array
export const MAP_LAYERS = ['debug', 'continentality', 'tempSummer', 'tempWinter', 'precipSummer', 'precipWinter', 'rainShadowSummer', 'rainShadowWinter',
    'oceanCurrentSummer', 'oceanCurrentWinter', 'pressureSummer', 'pressureWinter', 'windSpeedSummer', 'windSpeedWinter'];

export function mapLayerId(layer) {
    const id = MAP_LAYERS.indexOf(layer);
    if (id < 0) throw new RangeError(`exportMap: unknown map layer '${layer}' (one of ${MAP_LAYERS.join(', ')})`);
    return id;
}

// ours: the reference exports no layer
export function layerFilename(name, seed) { return `orogen-layer-${name}-${seed}.png`; }

export function mapTypeId(type) {
    const id = MAP_TYPES.indexOf(type);
    if (id < 0) throw new RangeError(`exportMap: unknown map type '${type}' (one of ${MAP_TYPES.join(', ')})`);
    return id;
}

// exportFilename(type, seed) (:1952-1961)
export function exportFilename(type, seed) {
    switch (type) {
        case 'landmask':       return `orogen-landmask-${seed}.png`;
        case 'landheightmap':  return `orogen-land-heightmap-${seed}.png`;
        case 'heightmap':      return `orogen-heightmap-${seed}.png`;
        case 'biome':          return `orogen-satellite-${seed}.png`;
        case 'koppen':         return `orogen-climate-${seed}.png`;
        default:               return `orogen-colormap-${seed}.png`;
    }
}

// the cube map's faces in the order +X, -X, +Y, -Y, +Z, -Z (the OpenGL cube-map table; north is +Y, longitude 0 is +Z)
export const CUBE_FACES = ['px', 'nx', 'py', 'ny', 'pz', 'nz'];
export const CUBE_MAX_FACE_SIZE = 16384;

// ours: exportFilename's stems (a name that is no type's: the layer's), then the face
export function cubeFilename(type, face, seed) {
    if (CUBE_FACES.indexOf(face) < 0) throw new RangeError(`exportCubeMap: unknown cube face '${face}' (one of ${CUBE_FACES.join(', ')})`);
    const name = MAP_TYPES.indexOf(type) >= 0 ? exportFilename(type, seed) : layerFilename(type, seed);
    return `${name.slice(0, -4)}-${face}.png`;
}

// the direction of the centre of pixel (column i, row j) of a face (csrc/cube_ops.h: cube_direction); not normalised
export function cubeDirection(face, i, j, faceSize) {
    const f = typeof face === 'number' ? face : CUBE_FACES.indexOf(face);
    if (!(Number.isInteger(f) && f >= 0 && f < 6)) throw new RangeError(`exportCubeMap: unknown cube face '${face}' (one of ${CUBE_FACES.join(', ')})`);
    const a = -1 + 2 * (i + 0.5) / faceSize, b = -1 + 2 * (j + 0.5) / faceSize;
    return [[1, -b, -a], [-1, -b, a], [a, 1, b], [a, -1, -b], [a, -b, 1], [-a, -b, -1]][f];
}

// the six faces of a stacked faceSize x 6 faceSize image: views of its buffer, nothing is copied
export function cubeFaces(rgba, faceSize) {
    const n = faceSize * faceSize * 4;
    if (rgba.length !== 6 * n) throw new RangeError('exportCubeMap: the image does not hold six faces of faceSize x faceSize');
    return CUBE_FACES.map((face, f) => ({ face, rgba: rgba.subarray(f * n, (f + 1) * n) }));
}

function checkFaceSize(faceSize) {
    if (!(Number.isInteger(faceSize) && faceSize >= 1 && faceSize <= CUBE_MAX_FACE_SIZE)) throw new RangeError('exportCubeMap: faceSize must be an integer from 1 to 16384');
}

function checkMesh(mesh, width) {
    if (!mesh || !(mesh.triangles instanceof Int32Array) || !(mesh.halfedges instanceof Int32Array)) throw new TypeError('exportMap: mesh.triangles and mesh.halfedges must be Int32Arrays');
    if (!(Number.isInteger(width) && width >= 2 && width <= 32768 && width % 2 === 0)) throw new RangeError('exportMap: width must be an even integer from 2 to 32768');
}

// the raster of the planet, around a centre meridian when one is given (0, null or undefined: the export's own raster, the same map)
export function rasterOnPlanet(planet, triangles, halfedges, width, centerLon) {
    if (centerLon === undefined || centerLon === null || centerLon === 0) return addon.mapRaster(planet, triangles, halfedges, width, false);
    if (typeof centerLon !== 'number') throw new TypeError('exportMap: centerLon must be a number (radians)');
    return addon.mapRasterCentered(planet, triangles, halfedges, width, centerLon, false);
}

// layers: names of MAP_LAYERS other than `debug`, or { name, values } with a Float32Array that takes the field's place (under any
// other name: coloured as `debug`)
function checkedLayers(layers) {
    return Array.from(layers || []).map((l) => {
        const name = typeof l === 'string' ? l : l && l.name, values = typeof l === 'string' ? null : (l && l.values) || null;
        const id = (values && MAP_LAYERS.indexOf(name) < 0) ? 0 : mapLayerId(name);
        if (id === 0 && !values) throw new RangeError("exportMap: the map layer 'debug' takes its values from the caller");
        return { name, id, values };
    });
}

// one raster, one colour pass per type and per layer, on a planet handle (what the worker holds); r_elevation null: the planet's resident field
export function exportMapsOnPlanet(planet, triangles, halfedges, r_elevation, types, width, opts) {
    const ids = types.map(mapTypeId), layers = checkedLayers(opts && opts.layers);
    const r = rasterOnPlanet(planet, triangles, halfedges, width, opts && opts.centerLon);
    const maps = ids.map((id, k) => ({ type: types[k], rgba: addon.mapColor(planet, id, r_elevation || null, width) }));
    for (const l of layers) maps.push({ type: l.name, rgba: addon.mapColorLayer(planet, l.id, l.values, r_elevation || null, width) });
    return { width: r.width, height: r.height, covered: r.covered, uncovered: r.uncovered, maps };
}

// the cube map's counterpart: one raster of the six faces, one colour pass per type and per layer; rgba is the stacked image, faces its views
export function exportCubeMapsOnPlanet(planet, triangles, halfedges, r_elevation, types, faceSize, opts) {
    checkFaceSize(faceSize);
    const ids = types.map(mapTypeId), layers = checkedLayers(opts && opts.layers);
    const r = addon.mapRasterCube(planet, triangles, halfedges, faceSize, false);
    const maps = ids.map((id, k) => ({ type: types[k], rgba: addon.mapColor(planet, id, r_elevation || null) }));
    for (const l of layers) maps.push({ type: l.name, rgba: addon.mapColorLayer(planet, l.id, l.values, r_elevation || null) });
    for (const m of maps) m.faces = cubeFaces(m.rgba, faceSize);
    return { faceSize: r.faceSize, covered: r.covered, uncovered: r.uncovered, maps };
}

function checkElevation(mesh, r_elevation) {
    if (!(r_elevation instanceof Float32Array) || r_elevation.length !== mesh.numRegions) throw new RangeError(`exportMap: r_elevation must be a Float32Array of ${mesh.numRegions} entries`);
}

// exportMapBatch(mesh, r_xyz, r_elevation, types, width, { layers, centerLon }) -> { width, height, maps: [{ type, rgba }] }: one raster, one
// colour pass per type, then one per layer
export function exportMapBatch(mesh, r_xyz, r_elevation, types, width, opts) {
    checkMesh(mesh, width);
    checkElevation(mesh, r_elevation);
    const res = exportMapsOnPlanet(planetFor(mesh, r_xyz), mesh.triangles, mesh.halfedges, r_elevation, Array.from(types), width, opts);
    return { width: res.width, height: res.height, maps: res.maps };
}

// exportMap(mesh, r_xyz, r_elevation, type, width, { layers, centerLon }) -> { width, height, rgba } (with layers: and maps, as exportMapBatch)
export function exportMap(mesh, r_xyz, r_elevation, type, width, opts) {
    const res = exportMapBatch(mesh, r_xyz, r_elevation, [type], width, opts);
    const out = { width: res.width, height: res.height, rgba: res.maps[0].rgba };
    if (opts && opts.layers && Array.from(opts.layers).length) out.maps = res.maps;
    return out;
}

// exportCubeMapBatch(mesh, r_xyz, r_elevation, types, faceSize, { layers }) -> { faceSize, maps: [{ type, rgba, faces: [{ face, rgba }] }] }
export function exportCubeMapBatch(mesh, r_xyz, r_elevation, types, faceSize, opts) {
    if (!mesh || !(mesh.triangles instanceof Int32Array) || !(mesh.halfedges instanceof Int32Array)) throw new TypeError('exportCubeMap: mesh.triangles and mesh.halfedges must be Int32Arrays');
    checkFaceSize(faceSize);
    checkElevation(mesh, r_elevation);
    const res = exportCubeMapsOnPlanet(planetFor(mesh, r_xyz), mesh.triangles, mesh.halfedges, r_elevation, Array.from(types), faceSize, opts);
    return { faceSize: res.faceSize, maps: res.maps };
}

// exportCubeMap(mesh, r_xyz, r_elevation, type, faceSize, { layers }) -> { faceSize, rgba, faces } (with layers: and maps, as exportCubeMapBatch)
export function exportCubeMap(mesh, r_xyz, r_elevation, type, faceSize, opts) {
    const res = exportCubeMapBatch(mesh, r_xyz, r_elevation, [type], faceSize, opts);
    const out = { faceSize: res.faceSize, rgba: res.maps[0].rgba, faces: res.maps[0].faces };
    if (opts && opts.layers && Array.from(opts.layers).length) out.maps = res.maps;
    return out;
}

// ---- PNG: 8-bit RGBA, filter 0 on every row, one IDAT from zlib.deflateSync; CRC-32 from a table built at load (Node 12 has no
// zlib.crc32) ----
const CRC_TABLE = new Uint32Array(256);
for (let n = 0; n < 256; n++) {
    let c = n;
    for (let k = 0; k < 8; k++) c = (c & 1) ? (0xEDB88320 ^ (c >>> 1)) : (c >>> 1);
    CRC_TABLE[n] = c >>> 0;
}
function crc32(buf, from, to) {
    let c = 0xFFFFFFFF;
    for (let i = from; i < to; i++) c = CRC_TABLE[(c ^ buf[i]) & 0xFF] ^ (c >>> 8);
    return (c ^ 0xFFFFFFFF) >>> 0;
}
function chunk(kind, body) {
    const out = Buffer.alloc(12 + body.length);
    out.writeUInt32BE(body.length, 0);
    out.write(kind, 4, 4, 'latin1');
    body.copy(out, 8);
    out.writeUInt32BE(crc32(out, 4, 8 + body.length), 8 + body.length);
    return out;
}

// the chunk writer and the signature, for the 16-bit encoder of js/relief-export.js
export { chunk as pngChunk };
export const PNG_SIGNATURE = [0x89, 0x50, 0x4E, 0x47, 0x0D, 0x0A, 0x1A, 0x0A];

// encodePng(rgba, width, height) -> Uint8Array (the file's bytes)
export function encodePng(rgba, width, height) {
    if (!(rgba instanceof Uint8Array) && !(rgba instanceof Uint8ClampedArray)) throw new TypeError('encodePng: rgba must be a Uint8Array or Uint8ClampedArray');
    if (!(Number.isInteger(width) && Number.isInteger(height) && width >= 1 && height >= 1) || rgba.length !== width * height * 4) throw new RangeError('encodePng: rgba length must be width*height*4');
    const row = width * 4, raw = Buffer.alloc((row + 1) * height);
    const src = Buffer.from(rgba.buffer, rgba.byteOffset, rgba.byteLength);
    for (let y = 0; y < height; y++) src.copy(raw, y * (row + 1) + 1, y * row, (y + 1) * row);        // byte 0 of each row: filter 0
    const ihdr = Buffer.alloc(13);
    ihdr.writeUInt32BE(width, 0); ihdr.writeUInt32BE(height, 4);
    ihdr[8] = 8; ihdr[9] = 6; ihdr[10] = 0; ihdr[11] = 0; ihdr[12] = 0;                              // 8 bits, RGBA, deflate, adaptive filtering, no interlace
    const png = Buffer.concat([Buffer.from([0x89, 0x50, 0x4E, 0x47, 0x0D, 0x0A, 0x1A, 0x0A]), chunk('IHDR', ihdr), chunk('IDAT', zlib.deflateSync(raw)),
                               chunk('IEND', Buffer.alloc(0))]);
    const out = new Uint8Array(png.length);                                                          // its own ArrayBuffer: the worker transfers it
    out.set(png);
    return out;
}
