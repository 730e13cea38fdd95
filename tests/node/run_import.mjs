// Test driver for the importHeightmap command of planet_heightmap_generation_amd/js/planet-worker.js:
// import -> reapply (same sliders) -> reapply (other sliders) -> a bad image -> reapply again.
//   node run_import.mjs <dir>   (reads <dir>/import_job.json and the image, writes <dir>/import_result.json and the arrays)
import fs from 'fs';
import path from 'path';
import { fileURLToPath } from 'url';
import { Worker } from 'worker_threads';

const here = path.dirname(fileURLToPath(import.meta.url));
const workerFile = path.join(here, '..', '..', 'planet_heightmap_generation_amd', 'js', 'planet-worker.js');
const dir = process.argv[2];
const job = JSON.parse(fs.readFileSync(path.join(dir, 'import_job.json'), 'utf8'));
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
const ask = (msg, transfer) => new Promise((resolve) => { waiting = resolve; w.postMessage(msg, transfer || []); });
const typeName = (v) => (v === null ? 'null' : Array.isArray(v) ? 'Array' : (v && v.constructor ? v.constructor.name : typeof v));

async function main() {
    const out = {};
    const d = await ask({ cmd: 'importHeightmap', N: job.N, jitter: job.jitter, grayscale: img, imageWidth: job.W, imageHeight: job.H, seed: job.seed, ...job.params });
    out.done = { type: d.type, message: d.message, keys: Object.keys(d), types: Object.fromEntries(Object.keys(d).map((k) => [k, typeName(d[k])])),
                 progress: log.slice(), stages: (d._pipelineTiming || []).map((s) => s.stage), pipelineTiming: d._pipelineTiming, postStages: (d._postTiming || []).map((s) => s.stage),
                 params: d._params, skipClimate: d.skipClimate, seed: d.seed, nMag: d.nMag, numRegions: d.numRegions, debugLayers: d.debugLayers ? Object.keys(d.debugLayers) : null,
                 plateVecSample: d.plateVec ? d.plateVec[d.plateSeeds[0]] : null, workerTotal: d._workerTotal };
    if (d.type === 'done') {
        for (const k of ['prePostElev', 'r_elevation', 't_elevation', 't_xyz', 'r_xyz', 'triangles', 'halfedges', 'r_plate', 'r_stress']) writeArr(`imp_${k}.bin`, d[k]);
        for (const k of ['plateSeeds', 'plateIsOcean', 'mountain_r', 'coastline_r', 'ocean_r']) writeArr(`imp_${k}.bin`, Int32Array.from(d[k]));
        writeArr('imp_erosionDelta.bin', d.debugLayers.erosionDelta);
    }
    const r1 = await ask({ cmd: 'reapply', ...job.params });
    out.reapply1 = r1.type;
    if (r1.type === 'reapplyDone') writeArr('re_same.bin', r1.r_elevation);
    const r2 = await ask({ cmd: 'reapply', ...job.params2 });
    out.reapply2 = r2.type;
    if (r2.type === 'reapplyDone') writeArr('re_other.bin', r2.r_elevation);
    log = [];
    const bad = await ask({ cmd: 'importHeightmap', N: job.N, jitter: job.jitter, grayscale: new Float32Array(job.W * job.H), imageWidth: job.W, imageHeight: job.H, seed: job.seed, ...job.params });
    const bad2 = await ask({ cmd: 'importHeightmap', N: job.N, jitter: job.jitter, grayscale: img.subarray(1), imageWidth: job.W, imageHeight: job.H, seed: job.seed, ...job.params });
    out.bad = [bad.type, bad.message, bad2.type, bad2.message];
    const r3 = await ask({ cmd: 'reapply', ...job.params });
    out.reapply3 = r3.type;
    if (r3.type === 'reapplyDone') writeArr('re_after_bad.bin', r3.r_elevation);
    out.disposed = (await ask({ cmd: 'dispose' })).type;
    fs.writeFileSync(path.join(dir, 'import_result.json'), JSON.stringify(out));
    await w.terminate();
}
main().catch((e) => { console.error(e.stack || e); process.exit(1); });
