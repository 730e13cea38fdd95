// Test driver for the exportMap command of planet_heightmap_generation_amd/js/planet-worker.js:
// exportMap with nothing retained -> retain without triangles -> exportMap -> importHeightmap -> exportMap koppen (no climate yet)
// -> computeClimate -> exportMap (all six, png) -> an unknown type -> reapply (other sliders) -> exportMap heightmap -> dispose.
//   node run_map_export.mjs <dir>   (reads <dir>/map_job.json and the image, writes <dir>/map_result.json and the arrays)
import fs from 'fs';
import path from 'path';
import { fileURLToPath } from 'url';
import { Worker } from 'worker_threads';
import { exportMap, exportMapBatch } from '../../planet_heightmap_generation_amd/js/map-export.js';

const here = path.dirname(fileURLToPath(import.meta.url));
const workerFile = path.join(here, '..', '..', 'planet_heightmap_generation_amd', 'js', 'planet-worker.js');
const dir = process.argv[2];
const job = JSON.parse(fs.readFileSync(path.join(dir, 'map_job.json'), 'utf8'));
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
    if (d.type !== 'exportDone') return o;
    o.width = d.width; o.height = d.height;
    o.timingKeys = Object.keys(d._exportTiming); o.timing = d._exportTiming;
    o.maps = d.maps.map((m) => ({ type: m.type, filename: m.filename, keys: Object.keys(m), rgba: typeName(m.rgba), png: m.png ? typeName(m.png) : null }));
    for (const m of d.maps) {
        writeArr(`${tag}_${m.type}.rgba`, m.rgba);
        if (m.png) writeArr(`${tag}_${m.type}.png`, m.png);
    }
    return o;
}

async function main() {
    const out = {};
    out.nothingRetained = describe('none', await ask({ cmd: 'exportMap', type: 'color', width: 64 }));
    const n = job.small.numRegions;
    const mesh = { numRegions: n, adjOffset: readArr(job.small.off, Int32Array), adjList: readArr(job.small.adj, Int32Array) };
    out.retained = (await ask({ cmd: 'retain', mesh, r_xyz: readArr(job.small.xyz, Float32Array), prePostElev: new Float32Array(n), seed: 1 })).type;
    out.noMesh = describe('nomesh', await ask({ cmd: 'exportMap', type: 'color', width: 64 }));
    out.retained2 = (await ask({ cmd: 'retain', mesh: { ...mesh, triangles: readArr(job.small.tri, Int32Array) }, r_xyz: readArr(job.small.xyz, Float32Array),
                                 prePostElev: new Float32Array(n), seed: 1 })).type;
    out.noHalfedges = describe('nohe', await ask({ cmd: 'exportMap', type: 'color', width: 64 }));
    const d = await ask({ cmd: 'importHeightmap', N: job.N, jitter: job.jitter, grayscale: img, imageWidth: job.W, imageHeight: job.H, seed: job.seed, ...job.params });
    out.imported = { type: d.type, message: d.message };
    out.noKoppen = describe('nokoppen', await ask({ cmd: 'exportMap', types: ['color', 'koppen'], width: job.width }));
    out.noBiome = describe('nobiome', await ask({ cmd: 'exportMap', type: 'biome', width: job.width }));
    const c = await ask({ cmd: 'computeClimate' });
    out.climate = { type: c.type, message: c.message };
    if (c.type === 'climateDone') writeArr('koppen.bin', c.climateDebugLayers.koppen);
    out.all = describe('all', await ask({ cmd: 'exportMap', types: job.types, width: job.width, png: true }));
    out.one = describe('one', await ask({ cmd: 'exportMap', type: 'landmask', width: 64 }));
    out.unknown = describe('unknown', await ask({ cmd: 'exportMap', type: 'plates', width: 64 }));
    out.oddWidth = describe('odd', await ask({ cmd: 'exportMap', type: 'color', width: 63 }));
    const r = await ask({ cmd: 'reapply', ...job.params2 });
    out.reapply = r.type;
    if (r.type === 'reapplyDone') writeArr('re_elevation.bin', r.r_elevation);
    out.afterReapply = describe('after', await ask({ cmd: 'exportMap', types: ['heightmap', 'color'], width: job.width }));
    out.disposed = (await ask({ cmd: 'dispose' })).type;
    out.afterDispose = describe('gone', await ask({ cmd: 'exportMap', type: 'color', width: 64 }));
    // the module's own exportMap / exportMapBatch, on this thread, on the small mesh with its half-edges
    const whole = { ...mesh, triangles: readArr(job.small.tri, Int32Array), halfedges: readArr(job.small.he, Int32Array) };
    const sxyz = readArr(job.small.xyz, Float32Array), se = readArr(job.small.e, Float32Array);
    const one = exportMap(whole, sxyz, se, 'heightmap', 128);
    const batch = exportMapBatch(whole, sxyz, se, ['color', 'landmask'], 128);
    out.module = { one: [one.width, one.height, one.rgba.constructor.name], batch: [batch.width, batch.height, batch.maps.map((m) => m.type)] };
    writeArr('module_heightmap.rgba', one.rgba);
    for (const m of batch.maps) writeArr(`module_${m.type}.rgba`, m.rgba);
    let threw = null;
    try { exportMap(whole, sxyz, se, 'biome', 128); } catch (e) { threw = e.message; }
    out.module.noKoppen = threw;
    fs.writeFileSync(path.join(dir, 'map_result.json'), JSON.stringify(out));
    await w.terminate();
}
main().catch((e) => { console.error(e.stack || e); process.exit(1); });
