// Test driver for the computeClimate command of planet_heightmap_generation_amd/js/planet-worker.js:
// computeClimate with nothing retained -> retain without plates -> computeClimate -> importHeightmap -> computeClimate ->
// computeClimate with another temperatureOffset -> reapply -> computeClimate -> dispose -> computeClimate.
//   node run_climate_worker.mjs <dir>   (reads <dir>/climate_job.json and the image, writes <dir>/climate_result.json and the arrays)
import fs from 'fs';
import path from 'path';
import { fileURLToPath } from 'url';
import { Worker } from 'worker_threads';

const here = path.dirname(fileURLToPath(import.meta.url));
const workerFile = path.join(here, '..', '..', 'planet_heightmap_generation_amd', 'js', 'planet-worker.js');
const dir = process.argv[2];
const job = JSON.parse(fs.readFileSync(path.join(dir, 'climate_job.json'), 'utf8'));
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
const ask = (msg) => new Promise((resolve) => { waiting = resolve; w.postMessage(msg); });
const typeName = (v) => (v === null ? 'null' : Array.isArray(v) ? 'Array' : (v && v.constructor ? v.constructor.name : typeof v));

function describe(tag, d, save) {
    const o = { type: d.type, message: d.message, keys: Object.keys(d), progress: log.slice() };
    log = [];
    if (d.type !== 'climateDone') return o;
    o.types = Object.fromEntries(Object.keys(d).map((k) => [k, typeName(d[k])]));
    o.layers = Object.fromEntries(Object.keys(d.climateDebugLayers).map((k) => [k, typeName(d.climateDebugLayers[k])]));
    o.timing = d._climateTiming;
    o.timingKeys = Object.keys(d._climateTiming);
    // a debug layer that is the very array of a result key, as in the reference
    o.layerIs = { precipSummer: d.climateDebugLayers.precipSummer.every((v, i) => Object.is(v, d.r_precip_summer[i])),
                  tempWinter: d.climateDebugLayers.tempWinter.every((v, i) => Object.is(v, d.r_temperature_winter[i])) };
    if (save) {
        for (const k of Object.keys(d)) if (ArrayBuffer.isView(d[k])) writeArr(`${tag}_${k}.bin`, d[k]);
        for (const k of Object.keys(d.climateDebugLayers)) writeArr(`${tag}_layer_${k}.bin`, d.climateDebugLayers[k]);
    }
    return o;
}

async function main() {
    const out = {};
    out.nothingRetained = describe('none', await ask({ cmd: 'computeClimate' }));
    out.generate = describe('gen', await ask({ cmd: 'generate' }));
    out.editRecompute = describe('edit', await ask({ cmd: 'editRecompute' }));
    // a retained state without plates
    const n = job.small.numRegions;
    const mesh = { numRegions: n, adjOffset: readArr(job.small.off, Int32Array), adjList: readArr(job.small.adj, Int32Array) };
    out.retained = (await ask({ cmd: 'retain', mesh, r_xyz: readArr(job.small.xyz, Float32Array), prePostElev: readArr(job.small.e, Float32Array), seed: 1 })).type;
    out.noPlates = describe('noplates', await ask({ cmd: 'computeClimate' }));
    out.badPlate = describe('badplate', await ask({ cmd: 'retain', mesh, r_xyz: readArr(job.small.xyz, Float32Array), prePostElev: readArr(job.small.e, Float32Array), seed: 1,
                                                    r_plate: new Int32Array(3), plateIsOcean: [] }));
    // retain with plates: climate on the retained field
    out.retained2 = (await ask({ cmd: 'retain', mesh, r_xyz: readArr(job.small.xyz, Float32Array), prePostElev: readArr(job.small.e, Float32Array), seed: job.small.seed,
                                 r_plate: readArr(job.small.plate, Int32Array), plateIsOcean: Array.from(readArr(job.small.ocean, Int32Array)) })).type;
    out.small = describe('small', await ask({ cmd: 'computeClimate' }), true);
    // the imported planet
    const d = await ask({ cmd: 'importHeightmap', N: job.N, jitter: job.jitter, grayscale: img, imageWidth: job.W, imageHeight: job.H, seed: job.seed, ...job.params });
    out.imported = { type: d.type, message: d.message, skipClimate: d.skipClimate };
    if (d.type === 'done') writeArr('imp_r_elevation.bin', d.r_elevation);
    log = [];
    out.first = describe('first', await ask({ cmd: 'computeClimate' }), true);
    out.second = describe('second', await ask({ cmd: 'computeClimate', temperatureOffset: 10 }), true);
    out.third = describe('third', await ask({ cmd: 'computeClimate' }), true);                 // the offset persists in W
    const r = await ask({ cmd: 'reapply', ...job.params });
    out.reapply = { type: r.type, skipClimate: r.skipClimate };
    log = [];
    out.afterReapply = describe('after', await ask({ cmd: 'computeClimate', temperatureOffset: 0 }), true);
    out.disposed = (await ask({ cmd: 'dispose' })).type;
    out.afterDispose = describe('gone', await ask({ cmd: 'computeClimate' }));
    fs.writeFileSync(path.join(dir, 'climate_result.json'), JSON.stringify(out));
    await w.terminate();
}
main().catch((e) => { console.error(e.stack || e); process.exit(1); });
