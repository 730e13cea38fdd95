// Relief export for hosts without WebGL (ours: the reference exports neither): a smooth height per pixel of the equirectangular map or
// of the cube map, encoded in 16 bits, and RGBA8 normals of the displaced surface.  The rasters, the interpolation and the stencil run
// in HIP kernels (csrc/relief.hip; the contract is in csrc/relief_ops.h) on the planet bound to `mesh` (native.js: planetFor).  The
// height of a pixel is the globe mesh's own flat triangle sampled at the pixel centre; the 16-bit kinds are linear in the reference's
// heightmap and land-heightmap shades, without its gamma table.  No JavaScript fallback for the device passes.
import zlib from 'zlib';
import addon, { planetFor } from './native.js';
import { CUBE_FACES, CUBE_MAX_FACE_SIZE, pngChunk, PNG_SIGNATURE } from './map-export.js';

// the kinds a relief export offers: two 16-bit grey images (WO_RELIEF_HEIGHT, WO_RELIEF_LAND_HEIGHT) and two normal maps
// (WO_RELIEF_NORMAL_TANGENT, WO_RELIEF_NORMAL_OBJECT)
export const RELIEF_KINDS = ['height16', 'landHeight16', 'normal', 'normalObject'];
const STEMS = { height16: 'height16', landHeight16: 'land-height16', normal: 'normal', normalObject: 'normal-object' };
export const RELIEF_FLAT_OCEAN = 1;

export function reliefKindId(kind) {
    const id = RELIEF_KINDS.indexOf(kind);
    if (id < 0) throw new RangeError(`exportRelief: unknown relief kind '${kind}' (one of ${RELIEF_KINDS.join(', ')})`);
    return id;
}
export function reliefIs16(kind) { return reliefKindId(kind) < 2; }

// orogen-<kind>-<seed>.png, and for one face (or the column) of a cube map orogen-cube-<kind>-<face>-<seed>.png
export function reliefFilename(kind, seed, face) {
    const stem = STEMS[RELIEF_KINDS[reliefKindId(kind)]];
    if (face === undefined || face === null) return `orogen-${stem}-${seed}.png`;
    if (face !== 'column' && CUBE_FACES.indexOf(face) < 0) throw new RangeError(`exportRelief: unknown cube face '${face}' (one of ${CUBE_FACES.join(', ')})`);
    return `orogen-cube-${stem}-${face}-${seed}.png`;
}

// one kind of the planet's resident relief: a Uint16Array for the 16-bit kinds, a Uint8ClampedArray of RGBA for the normals
export function reliefImage(planet, kind, opts) {
    const id = reliefKindId(kind);
    if (id < 2) return addon.reliefHeight16(planet, id);
    const strength = opts && opts.strength !== undefined && opts.strength !== null ? opts.strength : 1;
    if (typeof strength !== 'number') throw new TypeError('exportRelief: strength must be a number');
    return addon.reliefNormals(planet, id - 2, strength, opts && opts.flatOcean ? RELIEF_FLAT_OCEAN : 0);
}

// the six faces of a stacked image with `channels` values per pixel: views of its buffer, nothing is copied
export function reliefFaces(data, faceSize, channels) {
    const n = faceSize * faceSize * channels;
    if (data.length !== 6 * n) throw new RangeError('exportRelief: the image does not hold six faces of faceSize x faceSize');
    return CUBE_FACES.map((face, f) => ({ face, data: data.subarray(f * n, (f + 1) * n) }));
}

// one relief raster and one pass per kind, on a planet handle (what the worker holds); r_elevation null: the planet's resident field.
// opts: { centerLon, strength, flatOcean }
export function exportReliefOnPlanet(planet, triangles, halfedges, r_elevation, kinds, width, opts) {
    kinds.forEach(reliefKindId);
    const centerLon = opts && opts.centerLon !== undefined && opts.centerLon !== null ? opts.centerLon : 0;
    if (typeof centerLon !== 'number') throw new TypeError('exportRelief: centerLon must be a number (radians)');
    const r = addon.reliefRaster(planet, triangles, halfedges, width, centerLon, r_elevation || null, false);
    const maps = kinds.map((kind) => ({ kind, data: reliefImage(planet, kind, opts) }));
    return { width: r.width, height: r.height, covered: r.covered, uncovered: r.uncovered, maps };
}
export function exportCubeReliefOnPlanet(planet, triangles, halfedges, r_elevation, kinds, faceSize, opts) {
    kinds.forEach(reliefKindId);
    if (!(Number.isInteger(faceSize) && faceSize >= 1 && faceSize <= CUBE_MAX_FACE_SIZE)) throw new RangeError('exportRelief: faceSize must be an integer from 1 to 16384');
    const r = addon.reliefRasterCube(planet, triangles, halfedges, faceSize, r_elevation || null, false);
    const maps = kinds.map((kind) => {
        const data = reliefImage(planet, kind, opts);
        return { kind, data, faces: reliefFaces(data, faceSize, reliefIs16(kind) ? 1 : 4) };
    });
    return { faceSize: r.faceSize, covered: r.covered, uncovered: r.uncovered, maps };
}

function checkArgs(mesh, r_elevation) {
    if (!mesh || !(mesh.triangles instanceof Int32Array) || !(mesh.halfedges instanceof Int32Array)) throw new TypeError('exportRelief: mesh.triangles and mesh.halfedges must be Int32Arrays');
    if (!(r_elevation instanceof Float32Array) || r_elevation.length !== mesh.numRegions) throw new RangeError(`exportRelief: r_elevation must be a Float32Array of ${mesh.numRegions} entries`);
}

// exportRelief(mesh, r_xyz, r_elevation, kinds, width, { centerLon, strength, flatOcean }) -> { width, height, maps: [{ kind, data }] }
export function exportRelief(mesh, r_xyz, r_elevation, kinds, width, opts) {
    checkArgs(mesh, r_elevation);
    if (!(Number.isInteger(width) && width >= 2 && width <= 32768 && width % 2 === 0)) throw new RangeError('exportRelief: width must be an even integer from 2 to 32768');
    const res = exportReliefOnPlanet(planetFor(mesh, r_xyz), mesh.triangles, mesh.halfedges, r_elevation, Array.from(kinds), width, opts);
    return { width: res.width, height: res.height, maps: res.maps };
}

// exportCubeRelief(mesh, r_xyz, r_elevation, kinds, faceSize, { strength, flatOcean }) -> { faceSize, maps: [{ kind, data, faces: [{ face, data }] }] }
export function exportCubeRelief(mesh, r_xyz, r_elevation, kinds, faceSize, opts) {
    checkArgs(mesh, r_elevation);
    const res = exportCubeReliefOnPlanet(planetFor(mesh, r_xyz), mesh.triangles, mesh.halfedges, r_elevation, Array.from(kinds), faceSize, opts);
    return { faceSize: res.faceSize, maps: res.maps };
}

// encodePng16(gray, width, height) -> Uint8Array (the file's bytes): PNG colour type 0 at bit depth 16, big-endian samples, filter 0 on
// every row, one IDAT from zlib.deflateSync, the chunk writer of encodePng
export function encodePng16(gray, width, height) {
    if (!(gray instanceof Uint16Array)) throw new TypeError('encodePng16: gray must be a Uint16Array');
    if (!(Number.isInteger(width) && Number.isInteger(height) && width >= 1 && height >= 1) || gray.length !== width * height) throw new RangeError('encodePng16: gray length must be width*height');
    const row = width * 2, raw = Buffer.alloc((row + 1) * height);
    for (let y = 0, i = 0; y < height; y++) {
        let o = y * (row + 1) + 1;                                                                   // byte 0 of each row: filter 0
        for (let x = 0; x < width; x++, i++, o += 2) { const v = gray[i]; raw[o] = v >>> 8; raw[o + 1] = v & 0xFF; }
    }
    const ihdr = Buffer.alloc(13);
    ihdr.writeUInt32BE(width, 0); ihdr.writeUInt32BE(height, 4);
    ihdr[8] = 16; ihdr[9] = 0; ihdr[10] = 0; ihdr[11] = 0; ihdr[12] = 0;                             // 16 bits, greyscale, deflate, adaptive filtering, no interlace
    const png = Buffer.concat([Buffer.from(PNG_SIGNATURE), pngChunk('IHDR', ihdr), pngChunk('IDAT', zlib.deflateSync(raw)), pngChunk('IEND', Buffer.alloc(0))]);
    const out = new Uint8Array(png.length);                                                          // its own ArrayBuffer: the worker transfers it
    out.set(png);
    return out;
}
