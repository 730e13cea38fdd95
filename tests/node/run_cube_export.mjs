// Test driver for the exportCubeMap command of planet_heightmap_generation_amd/js/planet-worker.js:
// exportCubeMap with nothing retained -> importHeightmap -> exportCubeMap koppen (no climate yet) -> computeClimate -> exportCubeMap
// (two types and a layer, png) -> the same as one column -> the error answers -> exportMap at the face size's width -> dispose; then the
// module's own exportCubeMap / exportCubeMapBatch on the small mesh.
//   node run_cube_export.mjs <dir>   (reads <dir>/cube_job.json and the image, writes <dir>/cube_result.json and the arrays)
import fs from 'fs';
import path from 'path';
import { fileURLToPath } from 'url';
import { Worker } from 'worker_threads';
import { CUBE_FACES, cubeDirection, cubeFilename, exportCubeMap, exportCubeMapBatch } from '../../planet_heightmap_generation_amd/js/map-export.js';

const here = path.dirname(fileURLToPath(import.meta.url));
const workerFile = path.join(here, '..', '..', 'planet_heightmap_generation_amd', 'js', 'planet-worker.js');
const dir = process.argv[2];
const job = JSON.parse(fs.readFileSync(path.join(dir, 'cube_job.json'), 'utf8'));
function readArr(file, Type) {
    const buf = fs.readFileSync(path.join(dir, file));
    return new Type(buf.buffer.slice(buf.byteOffset, buf.byteOffset + buf.byteLength));
}
function writeArr(file, arr) { fs.writeFileSync(path.join(dir, file), Buffer.from(arr.buffer, arr.byteOffset, arr.byteLength)); }
const img = new Uint8Array(fs.readFileSync(path.join(dir, job.image)));

const w = new Worker(workerFile);
let log = [];
let waiting = null;
w.on('message', (m) => {
    if (m.type === 'progress') { log.push([m.pct, m.label]); return; }
    if (waiting) { const f = waiting; waiting = null; f(m); }
});
w.on('error', (e) => { console.error(e.stack || e); process.exit(1); });
const ask = (msg) => new Promise((resolve) => { waiting = resolve; log = []; w.postMessage(msg); });
const typeName = (v) => (v === null ? 'null' : Array.isArray(v) ? 'Array' : (v && v.constructor ? v.constructor.name : typeof v));

function describe(tag, d) {
    const o = { type: d.type, message: d.message, keys: Object.keys(d), progress: log.slice() };
    if (d.type === 'exportDone') {
        o.width = d.width; o.height = d.height;
        for (const m of d.maps) writeArr(`${tag}_${m.type}.rgba`, m.rgba);
        return o;
    }
    if (d.type !== 'exportCubeDone') return o;
    o.faceSize = d.faceSize;
    o.timingKeys = Object.keys(d._exportTiming); o.timing = d._exportTiming;
    o.maps = d.maps.map((m) => ({
        type: m.type, keys: Object.keys(m),
        // the faces of one map are views of one buffer, in order, without gaps
        oneBuffer: m.faces.every((f, k) => f.rgba.buffer === m.faces[0].rgba.buffer && f.rgba.byteOffset === m.faces[0].rgba.byteOffset + k * f.rgba.byteLength),
        faces: m.faces.map((f) => ({ face: f.face, filename: f.filename, keys: Object.keys(f), rgba: typeName(f.rgba), bytes: f.rgba.byteLength, png: f.png ? typeName(f.png) : null }))
    }));
    for (const m of d.maps) for (const f of m.faces) {
        writeArr(`${tag}_${m.type}_${f.face}.rgba`, f.rgba);
        if (f.png) writeArr(`${tag}_${m.type}_${f.face}.png`, f.png);
    }
    return o;
}

async function main() {
    const out = {};
    const S = job.faceSize;
    out.nothingRetained = describe('none', await ask({ cmd: 'exportCubeMap', type: 'color', faceSize: S }));
    const d = await ask({ cmd: 'importHeightmap', N: job.N, jitter: job.jitter, grayscale: img, imageWidth: job.W, imageHeight: job.H, seed: job.seed, ...job.params });
    out.imported = { type: d.type, message: d.message };
    out.noKoppen = describe('nokoppen', await ask({ cmd: 'exportCubeMap', types: ['color', 'koppen'], faceSize: S }));
    out.noWind = describe('nowind', await ask({ cmd: 'exportCubeMap', type: 'color', layers: job.layers, faceSize: S }));
    const c = await ask({ cmd: 'computeClimate' });
    out.climate = { type: c.type, message: c.message };
    if (c.type === 'climateDone') writeArr('koppen.bin', c.climateDebugLayers.koppen);
    out.faces = describe('faces', await ask({ cmd: 'exportCubeMap', types: job.types, layers: job.layers, faceSize: S, png: true }));
    out.column = describe('column', await ask({ cmd: 'exportCubeMap', types: job.types, layers: job.layers, faceSize: S, png: true, layout: 'column' }));
    out.one = describe('one', await ask({ cmd: 'exportCubeMap', type: 'landmask', faceSize: 5 }));
    out.unknown = describe('unknown', await ask({ cmd: 'exportCubeMap', type: 'plates', faceSize: S }));
    out.unknownLayer = describe('unknownlayer', await ask({ cmd: 'exportCubeMap', type: 'color', layers: ['plates'], faceSize: S }));
    out.zero = describe('zero', await ask({ cmd: 'exportCubeMap', type: 'color', faceSize: 0 }));
    out.tooLarge = describe('large', await ask({ cmd: 'exportCubeMap', type: 'color', faceSize: 16385 }));
    out.badLayout = describe('layout', await ask({ cmd: 'exportCubeMap', type: 'color', faceSize: S, layout: 'cross' }));
    // the map block now holds an S x 6S cube map: an exportMap at width S must not take it for an S x S/2 map
    out.flat = describe('flat', await ask({ cmd: 'exportMap', types: job.types, width: S }));
    out.disposed = (await ask({ cmd: 'dispose' })).type;
    out.afterDispose = describe('gone', await ask({ cmd: 'exportCubeMap', type: 'color', faceSize: S }));
    // the module's own exportCubeMap / exportCubeMapBatch, on this thread, on the small mesh
    const n = job.small.numRegions;
    const whole = { numRegions: n, adjOffset: readArr(job.small.off, Int32Array), adjList: readArr(job.small.adj, Int32Array),
                    triangles: readArr(job.small.tri, Int32Array), halfedges: readArr(job.small.he, Int32Array) };
    const sxyz = readArr(job.small.xyz, Float32Array), se = readArr(job.small.e, Float32Array);
    const one = exportCubeMap(whole, sxyz, se, 'heightmap', 33);
    const batch = exportCubeMapBatch(whole, sxyz, se, ['color', 'landmask'], 33, { layers: [{ name: 'slope', values: se }] });
    out.module = { one: [one.faceSize, one.rgba.constructor.name, one.rgba.length, one.faces.map((f) => f.face)], batch: [batch.faceSize, batch.maps.map((m) => m.type)],
                   faces: CUBE_FACES, filename: cubeFilename('biome', 'ny', 7), layerFilename: cubeFilename('slope', 'pz', 7),
                   direction: CUBE_FACES.map((f) => cubeDirection(f, 3, 8, 33)) };
    writeArr('module_heightmap.rgba', one.rgba);
    for (const m of batch.maps) writeArr(`module_${m.type}.rgba`, m.rgba);
    const threw = {};
    for (const [tag, f] of Object.entries({ noKoppen: () => exportCubeMap(whole, sxyz, se, 'biome', 33), zero: () => exportCubeMap(whole, sxyz, se, 'color', 0),
                                            odd: () => exportCubeMap(whole, sxyz, se, 'color', 2.5) })) {
        try { f(); threw[tag] = null; } catch (e) { threw[tag] = e.message; }
    }
    out.module.threw = threw;
    fs.writeFileSync(path.join(dir, 'cube_result.json'), JSON.stringify(out));
    await w.terminate();
}
main().catch((e) => { console.error(e.stack || e); process.exit(1); });
