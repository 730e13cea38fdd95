// Test driver for the overlay requests of planet_heightmap_generation_amd/js/planet-worker.js: importHeightmap -> an arrow request and
// an ITCZ request (no climate yet) -> computeClimate -> exportGlobe with arrows, ITCZ line and grid as GLB and as arrays ->
// exportOverlays -> the error answers -> an old exportGlobe and an old exportMap command -> dispose.
//   node run_overlays.mjs <dir>   (reads <dir>/overlays_job.json and the image, writes <dir>/overlays_result.json and the arrays)
import fs from 'fs';
import path from 'path';
import { fileURLToPath } from 'url';
import { Worker } from 'worker_threads';

const here = path.dirname(fileURLToPath(import.meta.url));
const workerFile = path.join(here, '..', '..', 'planet_heightmap_generation_amd', 'js', 'planet-worker.js');
const dir = process.argv[2];
const job = JSON.parse(fs.readFileSync(path.join(dir, 'overlays_job.json'), 'utf8'));
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

// every typed array of an answer goes to <tag>.<path>; nested objects are walked
function dump(tag, v, kinds) {
    for (const [k, x] of Object.entries(v)) {
        if (ArrayBuffer.isView(x)) { kinds[`${tag}.${k}`.split('.').slice(1).join('.')] = typeName(x); writeArr(`${tag}.${k}`, x); }
        else if (x && typeof x === 'object' && !Array.isArray(x) && !k.startsWith('_')) dump(`${tag}.${k}`, x, kinds);
    }
}
function describe(tag, d) {
    const o = { type: d.type, message: d.message, keys: Object.keys(d), progress: log.slice(), kinds: {} };
    if (d.type === 'exportDone') { for (const m of d.maps) writeArr(`${tag}_${m.type}.rgba`, m.rgba); o.maps = d.maps.map((m) => [m.type, m.filename]); return o; }
    if (d.type === 'globeDone') { o.view = d.view; o.filename = d.filename; }
    if (d.type === 'overlaysDone') { o.centerLon = d.centerLon; o.counts = {}; for (const k of ['windArrows', 'oceanCurrentArrows']) if (d[k]) o.counts[k] = d[k].count; }
    if (d.type !== 'error') dump(tag, d, o.kinds);
    return o;
}

async function main() {
    const out = {};
    const d = await ask({ cmd: 'importHeightmap', N: job.N, jitter: job.jitter, grayscale: img, imageWidth: job.W, imageHeight: job.H, seed: job.seed, ...job.params });
    out.imported = { type: d.type, message: d.message };
    out.noWind = describe('nowind', await ask({ cmd: 'exportOverlays', windArrows: 'summer' }));
    out.noOcean = describe('noocean', await ask({ cmd: 'exportOverlays', oceanCurrentArrows: 'winter' }));
    out.noWindGlobe = describe('nowindglobe', await ask({ cmd: 'exportGlobe', windArrows: 'summer' }));
    out.noItcz = describe('noitcz', await ask({ cmd: 'exportGlobe', itcz: 'summer' }));
    out.gridOnly = describe('gridonly', await ask({ cmd: 'exportOverlays', grid: job.grid }));      // needs no climate
    const c = await ask({ cmd: 'computeClimate' });
    out.climate = { type: c.type, message: c.message };
    const all = { layer: job.layer, wireframe: true, windArrows: 'summer', oceanCurrentArrows: 'winter', itcz: 'summer', grid: job.grid };
    out.glb = describe('glb', await ask({ cmd: 'exportGlobe', ...all, glb: true }));
    out.arrays = describe('arrays', await ask({ cmd: 'exportGlobe', ...all }));
    out.overlays = describe('overlays', await ask({ cmd: 'exportOverlays', windArrows: 'summer', oceanCurrentArrows: 'winter', itcz: 'winter', grid: job.grid2, centerLon: job.centerLon }));
    out.badSeason = describe('badseason', await ask({ cmd: 'exportOverlays', windArrows: 'spring' }));
    out.badGrid = describe('badgrid', await ask({ cmd: 'exportOverlays', grid: 0 }));
    out.oldGlobe = describe('oldglobe', await ask({ cmd: 'exportGlobe', wireframe: true, glb: true }));
    out.oldGlobeArrays = describe('oldglobearrays', await ask({ cmd: 'exportGlobe', wireframe: true }));
    out.oldMap = describe('oldmap', await ask({ cmd: 'exportMap', types: ['color'], width: job.width }));
    out.disposed = (await ask({ cmd: 'dispose' })).type;
    out.afterDispose = describe('gone', await ask({ cmd: 'exportOverlays', grid: 30 }));
    fs.writeFileSync(path.join(dir, 'overlays_result.json'), JSON.stringify(out));
    await w.terminate();
}
main().catch((e) => { console.error(e.stack || e); process.exit(1); });
