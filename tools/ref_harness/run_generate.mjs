// Golden-vector generator for plate generation and the worker's `generate`: runs the REFERENCE's own generateCoarsePlates,
// generatePlates, assignOceanLand and handleGenerate (scratch copy of the reference's js/, prepared by make_golden_generate.py)
// under Node 12, and V8's Math.sin / Math.cos / Math.exp on the math arguments.  Build container only (no GPU).  Test infrastructure.
//
//   node --harmony-optional-chaining --harmony-nullish run_generate.mjs <refJsDir> <job.json>
import fs from 'fs';
import path from 'path';
import { performance } from 'perf_hooks';
import { pathToFileURL } from 'url';

const refDir = process.argv[2];
const job = JSON.parse(fs.readFileSync(process.argv[3], 'utf8'));
const posted = [];
globalThis.performance = performance;
globalThis.self = { postMessage: (m) => posted.push(m) };

function readArr(file, Type) {
    const buf = fs.readFileSync(file);
    return new Type(buf.buffer.slice(buf.byteOffset, buf.byteOffset + buf.byteLength));
}
function writeArr(file, arr) { fs.writeFileSync(file, Buffer.from(arr.buffer, arr.byteOffset, arr.byteLength)); }
const median = (a) => { const s = Array.from(a).sort((x, y) => x - y); return s[s.length >> 1]; };

async function main() {
    globalThis.__woTriangulations = {};
    for (const t of job.triangulations) globalThis.__woTriangulations[t.n + ':' + t.crc] = { triangles: readArr(t.triangles, Int32Array), halfedges: readArr(t.halfedges, Int32Array) };
    const imp = (f) => import(pathToFileURL(path.join(refDir, f)).href);
    await imp('planet-worker.js');                       // installs the stub Delaunay provider and self.onmessage
    const CP = await imp('coarse-plates.js');
    const PL = await imp('plates.js');
    const OL = await imp('ocean-land.js');

    // the case table
    const vecOf = (seeds, vec) => { const v = new Float64Array(4 * seeds.length); seeds.forEach((id, i) => { v.set(vec[id].pole, 4 * i); v[4 * i + 3] = vec[id].omega; }); return v; };
    const thetas = [];                                   // every argument generatePlates hands Math.cos (the Euler pole angles)
    const recordingCos = (fn) => {
        const cos = Math.cos;
        Math.cos = (x) => { thetas.push(x); return cos(x); };
        try { return fn(); } finally { Math.cos = cos; }
    };
    for (const c of job.cases) {
        let r_plate, seeds, vec, ocean;
        if (c.mesh) {                                    // generatePlates / assignOceanLand as functions of a given mesh
            const mesh = { numRegions: c.mesh.numRegions, adjOffset: readArr(c.mesh.adjOffset, Int32Array), adjList: readArr(c.mesh.adjList, Int32Array) };
            const xyz = readArr(c.mesh.xyz, Float32Array);
            const g = recordingCos(() => PL.generatePlates(mesh, xyz, c.P, c.seed));
            r_plate = g.r_plate; seeds = Array.from(g.plateSeeds); vec = g.plateVec;
            ocean = OL.assignOceanLand(mesh, r_plate, g.plateSeeds, xyz, c.seed, c.numContinents, c.variety, c.coverage);
        } else {
            const co = CP.generateCoarsePlates(c.seed, c.P, c.numContinents, c.variety, c.coverage);
            r_plate = co.coarse_r_plate; seeds = Array.from(co.coarsePlateSeeds); vec = co.coarsePlateVec; ocean = co.coarsePlateIsOcean;
            recordingCos(() => PL.generatePlates(co.coarseMesh, co.coarse_xyz, c.P, c.seed));       // the same call again, for its angles
        }
        writeArr(c.out + 'r_plate.bin', r_plate);
        writeArr(c.out + 'seeds.bin', Int32Array.from(seeds));
        writeArr(c.out + 'vec.bin', vecOf(seeds, vec));
        writeArr(c.out + 'ocean.bin', Uint8Array.from(seeds.map((id) => ocean.has(id) ? 1 : 0)));
    }

    // V8's Math.sin / Math.cos / Math.exp
    const tx0 = readArr(job.math.trig_x, Float64Array), ex = readArr(job.math.exp_x, Float64Array);
    const tx = new Float64Array(tx0.length + thetas.length);
    tx.set(thetas, 0); tx.set(tx0, thetas.length);
    writeArr(job.math.trig_x_out, tx);
    writeArr(job.math.sin_out, Float64Array.from(tx, (x) => Math.sin(x)));
    writeArr(job.math.cos_out, Float64Array.from(tx, (x) => Math.cos(x)));
    writeArr(job.math.exp_out, Float64Array.from(ex, (x) => Math.exp(x)));

    // host time of generateCoarsePlates (median of job.timing.runs after one warm-up)
    const times = {};
    for (const t of job.timing.cases) {
        const ms = [];
        for (let i = 0; i <= job.timing.runs; i++) {
            const t0 = performance.now();
            CP.generateCoarsePlates(t.seed, t.P, 4, 0, 0.3);
            if (i > 0) ms.push(performance.now() - t0);
        }
        times['P' + t.P] = { median: median(ms), runs: ms };
    }
    fs.writeFileSync(job.timing.out, JSON.stringify(times));

    // the whole command
    for (const g of job.generate) {
        posted.length = 0;
        self.onmessage({ data: { cmd: 'generate', ...g.message } });
        const done = posted.find((m) => m.type === 'done');
        if (!done) throw new Error('generate did not answer done: ' + JSON.stringify(posted.filter((m) => m.type !== 'progress')));
        const arrays = {};
        for (const k of ['triangles', 'halfedges', 'r_xyz', 't_xyz', 'r_plate', 'prePostElev', 'r_elevation', 't_elevation', 'r_stress']) {
            writeArr(g.out + k + '.bin', done[k]);
            arrays[k] = done[k].constructor.name;
        }
        for (const k of ['plateSeeds', 'plateIsOcean', 'originalPlateIsOcean', 'mountain_r', 'coastline_r', 'ocean_r']) {
            writeArr(g.out + k + '.bin', Int32Array.from(done[k]));
            arrays[k] = done[k].constructor.name;
        }
        writeArr(g.out + 'plateVec.bin', vecOf(done.plateSeeds, done.plateVec));
        for (const k of ['plateDensity', 'plateDensityLand', 'plateDensityOcean']) writeArr(g.out + k + '.bin', Float64Array.from(done.plateSeeds, (id) => done[k][id]));
        for (const k of Object.keys(done.debugLayers)) writeArr(g.out + 'dl_' + k + '.bin', done.debugLayers[k]);
        const meta = {
            keys: Object.keys(done), arrays,
            progress: posted.filter((m) => m.type === 'progress').map((m) => [m.pct, m.label]),
            stages: done._pipelineTiming.map((s) => s.stage), postStages: done._postTiming.map((s) => s.stage),
            elevationStages: done._timing.map((s) => s.stage),
            params: done._params, skipClimate: done.skipClimate, seed: done.seed, nMag: done.nMag, numRegions: done.numRegions,
            debugLayers: Object.keys(done.debugLayers), debugLayerTypes: Object.keys(done.debugLayers).map((k) => done.debugLayers[k].constructor.name),
            nulls: Object.keys(done).filter((k) => done[k] === null),
            tableKeys: ['plateVec', 'plateDensity', 'plateDensityLand', 'plateDensityOcean'].map((k) => [k, Object.keys(done[k]).map(Number)]),
            message: g.message,
        };
        fs.writeFileSync(g.out + 'meta.json', JSON.stringify(meta));
    }
}
main().catch((e) => { console.error(e.stack || e); process.exit(1); });
