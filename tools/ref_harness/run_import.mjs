// Golden-vector generator for the heightmap import: runs the REFERENCE's own handleImportHeightmap, sampleHeightmap and
// deriveSyntheticPlates (scratch copy of the reference's js/, prepared by make_golden_import.py) under Node 12, and
// V8's Math.asin / Math.atan2 on the math arguments.  Build container only (no GPU).  Test infrastructure.
//
//   node --harmony-optional-chaining --harmony-nullish run_import.mjs <refJsDir> <job.json>
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

async function main() {
    // the stub Delaunay module of the scratch copy returns the build's planar triangulation for the point count
    globalThis.__woTriangulations = {};
    for (const t of job.triangulations) globalThis.__woTriangulations[t.n] = { triangles: readArr(t.triangles, Int32Array), halfedges: readArr(t.halfedges, Int32Array) };
    const PW = await import(pathToFileURL(path.join(refDir, 'planet-worker.js')).href);

    // V8's Math.asin / Math.atan2
    const ax = readArr(job.math.asin_x, Float64Array), ay = readArr(job.math.atan2_y, Float64Array), axx = readArr(job.math.atan2_x, Float64Array);
    const oa = new Float64Array(ax.length), ot = new Float64Array(ay.length);
    for (let i = 0; i < ax.length; i++) oa[i] = Math.asin(ax[i]);
    for (let i = 0; i < ay.length; i++) ot[i] = Math.atan2(ay[i], axx[i]);
    writeArr(job.math.asin_out, oa); writeArr(job.math.atan2_out, ot);

    // sampleHeightmap: only mesh.numRegions and r_xyz are read
    for (const s of job.samples) {
        const xyz = readArr(s.xyz, Float32Array);
        const out = PW.sampleHeightmap({ numRegions: xyz.length / 3 }, xyz, readArr(s.image, Uint8Array), s.W, s.H);
        writeArr(s.out, out);
    }
    // deriveSyntheticPlates on given fields
    for (const d of job.plates) {
        const mesh = { numRegions: d.numRegions, adjOffset: readArr(d.adjOffset, Int32Array), adjList: readArr(d.adjList, Int32Array) };
        const res = PW.deriveSyntheticPlates(mesh, readArr(d.field, Float32Array));
        writeArr(d.out + 'r_plate.bin', res.r_plate);
        writeArr(d.out + 'seeds.bin', Int32Array.from(res.plateSeeds));
        writeArr(d.out + 'isOcean.bin', Int32Array.from(res.plateIsOcean));
    }
    // the whole command
    const imp = job.import;
    posted.length = 0;
    self.onmessage({ data: { cmd: 'importHeightmap', N: imp.N, jitter: imp.jitter, grayscale: readArr(imp.image, Uint8Array), imageWidth: imp.W,
                             imageHeight: imp.H, seed: imp.seed, skipClimate: true, ...imp.params } });
    const done = posted.find((m) => m.type === 'done');
    if (!done) throw new Error('importHeightmap did not answer done: ' + JSON.stringify(posted.filter((m) => m.type !== 'progress')));
    const arrays = {};
    for (const k of ['prePostElev', 'r_elevation', 't_elevation', 't_xyz', 'r_xyz', 'triangles', 'halfedges', 'r_plate', 'r_stress']) {
        writeArr(imp.out + k + '.bin', done[k]);
        arrays[k] = done[k].constructor.name;
    }
    for (const k of ['plateSeeds', 'plateIsOcean', 'mountain_r', 'coastline_r', 'ocean_r']) writeArr(imp.out + k + '.bin', Int32Array.from(done[k]));
    writeArr(imp.out + 'erosionDelta.bin', done.debugLayers.erosionDelta);
    const meta = {
        keys: Object.keys(done), arrays,
        progress: posted.filter((m) => m.type === 'progress').map((m) => [m.pct, m.label]),
        stages: done._pipelineTiming.map((s) => s.stage), postStages: done._postTiming.map((s) => s.stage),
        params: done._params, skipClimate: done.skipClimate, seed: done.seed, nMag: done.nMag, numRegions: done.numRegions,
        debugLayers: Object.keys(done.debugLayers), plateVecSample: done.plateVec[done.plateSeeds[0]],
        nulls: Object.keys(done).filter((k) => done[k] === null),
        empties: ['plateDensity', 'plateDensityLand', 'plateDensityOcean', '_timing'].map((k) => [k, JSON.stringify(done[k])]),
    };
    fs.writeFileSync(imp.out + 'meta.json', JSON.stringify(meta));
}
main().catch((e) => { console.error(e.stack || e); process.exit(1); });
