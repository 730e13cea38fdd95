// Test driver for the computeRivers command of planet_heightmap_generation_amd/js/planet-worker.js and for js/rivers.js:
//   node run_rivers.mjs worker <dir>    computeRivers with nothing retained -> importHeightmap -> the `rivers` option before any rivers
//       result -> computeRivers by precipitation before any climate -> computeRivers uniform, downloaded -> exportGlobe without and with
//       `rivers` (GLB and arrays) -> exportMap and exportCubeMap with `rivers` -> the refusals -> computeClimate -> computeRivers by
//       precipitation -> dispose; then the module's own computeRivers / riverLines on the small mesh
//       (reads <dir>/rivers_job.json, writes <dir>/rivers_result.json and the arrays beside it)
import fs from 'fs';
import path from 'path';
import { fileURLToPath } from 'url';
import { Worker } from 'worker_threads';
import { RIVER_KEYS, computeRivers, riverLines } from '../../planet_heightmap_generation_amd/js/rivers.js';

const here = path.dirname(fileURLToPath(import.meta.url));
const workerFile = path.join(here, '..', '..', 'planet_heightmap_generation_amd', 'js', 'planet-worker.js');
const dir = process.argv[3];
function readArr(file, Type) {
    const buf = fs.readFileSync(path.join(dir, file));
    return new Type(buf.buffer.slice(buf.byteOffset, buf.byteOffset + buf.byteLength));
}
function writeArr(file, arr) { fs.writeFileSync(path.join(dir, file), Buffer.from(arr.buffer, arr.byteOffset, arr.byteLength)); }
const typeName = (v) => (v === null ? 'null' : Array.isArray(v) ? 'Array' : (v && v.constructor ? v.constructor.name : typeof v));
const message = (f) => { try { f(); return null; } catch (e) { return `${e.constructor.name}: ${e.message}`; } };

async function worker() {
    const job = JSON.parse(fs.readFileSync(path.join(dir, 'rivers_job.json'), 'utf8'));
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

    function describe(tag, d) {
        const o = { type: d.type, message: d.message, keys: Object.keys(d), progress: log.slice() };
        if (d.type === 'riversDone') {
            for (const k of ['landCells', 'pits', 'spilledBasins', 'endorheicBasins', 'lakeCells', 'rounds', 'launches']) o[k] = d[k];
            o.fields = {};
            for (const k of RIVER_KEYS) if (d[k]) { o.fields[k] = typeName(d[k]); writeArr(`${tag}_${k}.bin`, d[k]); }
        }
        if (d.type === 'globeDone') {
            o.filename = d.filename;
            for (const k of ['glb', 'rivers', 'position']) if (d[k]) { o[k] = typeName(d[k]); writeArr(`${tag}_${k}.bin`, d[k]); }
        }
        if (d.type === 'exportDone') for (const m of d.maps) writeArr(`${tag}_${m.type}.rgba`, m.rgba);
        if (d.type === 'exportCubeDone') for (const m of d.maps) writeArr(`${tag}_${m.type}.rgba`, m.faces[0].rgba);
        return o;
    }

    const out = {};
    const W = job.width, S = job.faceSize, rivers = { minFlow: job.minFlow };
    out.nothingRetained = describe('none', await ask({ cmd: 'computeRivers', runoff: 'uniform' }));
    const d = await ask({ cmd: 'importHeightmap', N: job.N, jitter: job.jitter, grayscale: img, imageWidth: job.W, imageHeight: job.H, seed: job.seed, ...job.params });
    out.imported = { type: d.type, message: d.message };
    out.mapBefore = describe('mapBefore', await ask({ cmd: 'exportMap', types: ['color'], width: W, rivers }));
    out.globeBefore = describe('globeBefore', await ask({ cmd: 'exportGlobe', glb: true, rivers }));
    out.noClimate = describe('noClimate', await ask({ cmd: 'computeRivers' }));
    out.uniform = describe('uniform', await ask({ cmd: 'computeRivers', runoff: 'uniform', download: true }));
    out.quiet = describe('quiet', await ask({ cmd: 'computeRivers', runoff: 'uniform' }));
    out.globePlain = describe('globePlain', await ask({ cmd: 'exportGlobe', glb: true, wireframe: true }));
    out.globeRivers = describe('globeRivers', await ask({ cmd: 'exportGlobe', glb: true, wireframe: true, rivers }));
    out.globeArrays = describe('globeArrays', await ask({ cmd: 'exportGlobe', rivers }));
    out.map = describe('map', await ask({ cmd: 'exportMap', types: ['color', 'heightmap'], width: W, rivers }));
    out.mapPlain = describe('mapPlain', await ask({ cmd: 'exportMap', types: ['color'], width: W }));
    out.cube = describe('cube', await ask({ cmd: 'exportCubeMap', types: ['color'], faceSize: S, layout: 'column', rivers }));
    out.errors = {};
    out.errors.badRunoff = describe('e1', await ask({ cmd: 'computeRivers', runoff: 'rain' }));
    out.errors.shortValues = describe('e2', await ask({ cmd: 'computeRivers', runoff: new Float32Array(3) }));
    out.errors.badMinFlow = describe('e3', await ask({ cmd: 'exportMap', types: ['color'], width: W, rivers: { minFlow: 'deep' } }));
    out.errors.nanMinFlow = describe('e4', await ask({ cmd: 'exportGlobe', rivers: { minFlow: NaN } }));
    const c = await ask({ cmd: 'computeClimate' });
    out.climate = c.type;
    if (c.type === 'climateDone') { writeArr('precip_summer.bin', c.r_precip_summer); writeArr('precip_winter.bin', c.r_precip_winter); }
    out.precip = describe('precip', await ask({ cmd: 'computeRivers', download: true }));
    out.disposed = (await ask({ cmd: 'dispose' })).type;
    out.afterDispose = describe('gone', await ask({ cmd: 'computeRivers' }));
    await w.terminate();

    // the module's own computeRivers / riverLines, on this thread, on the small mesh
    const n = job.small.numRegions;
    const whole = { numRegions: n, adjOffset: readArr(job.small.off, Int32Array), adjList: readArr(job.small.adj, Int32Array),
                    triangles: readArr(job.small.tri, Int32Array), halfedges: readArr(job.small.he, Int32Array) };
    const sxyz = readArr(job.small.xyz, Float32Array), se = readArr(job.small.e, Float32Array), sv = readArr(job.small.values, Float32Array);
    const res = computeRivers(whole, sxyz, se, { runoff: sv });
    for (const k of RIVER_KEYS) writeArr(`module_${k}.bin`, res[k]);
    const lines = riverLines(whole, sxyz, job.minFlow, se);
    writeArr('module_segments.bin', lines.segments); writeArr('module_flows.bin', lines.flows);
    const counts = computeRivers(whole, sxyz, se, { runoff: 'uniform', download: false });
    out.module = { pits: res.pits, rounds: res.rounds, count: lines.count, types: RIVER_KEYS.map((k) => typeName(res[k])), countsKeys: Object.keys(counts),
                   threw: { runoff: message(() => computeRivers(whole, sxyz, se, { runoff: 'snow' })), minFlow: message(() => riverLines(whole, sxyz, Infinity, se)),
                            precip: message(() => computeRivers(whole, sxyz, se, {})) } };
    fs.writeFileSync(path.join(dir, 'rivers_result.json'), JSON.stringify(out));
}

worker().catch((e) => { console.error(e.stack || e); process.exit(1); });
