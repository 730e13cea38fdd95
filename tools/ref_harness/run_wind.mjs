// Golden-vector generator for the wind stage: runs the REFERENCE's own, unmodified computeWind (scratch copy of the
// reference's js/, prepared by make_golden_wind.py) under Node 12 on given planets.  Build container only (no GPU).
// Test infrastructure.
//
//   node --harmony-optional-chaining --harmony-nullish run_wind.mjs <refJsDir> <job.json>
import fs from 'fs';
import path from 'path';
import { performance } from 'perf_hooks';
import { pathToFileURL } from 'url';

const refDir = process.argv[2];
const job = JSON.parse(fs.readFileSync(process.argv[3], 'utf8'));
globalThis.performance = performance;            // wind.js times its stages with the browser's global

function readArr(file, Type) {
    const buf = fs.readFileSync(file);
    return new Type(buf.buffer.slice(buf.byteOffset, buf.byteOffset + buf.byteLength));
}
function writeArr(file, arr) { fs.writeFileSync(file, Buffer.from(arr.buffer, arr.byteOffset, arr.byteLength)); }

async function main() {
    const W = await import(pathToFileURL(path.join(refDir, 'wind.js')).href);
    const { SimplexNoise } = await import(pathToFileURL(path.join(refDir, 'simplex-noise.js')).href);
    const meta = { exports: Object.keys(W).sort(), cases: {} };
    for (const c of job.cases) {
        const mesh = { numRegions: c.numRegions, adjOffset: readArr(c.adjOffset, Int32Array), adjList: readArr(c.adjList, Int32Array) };
        const plateIsOcean = new Set(readArr(c.plateIsOcean, Int32Array));
        const t0 = performance.now();
        const res = W.computeWind(mesh, readArr(c.xyz, Float32Array), readArr(c.elevation, Float32Array), plateIsOcean,
                                  readArr(c.r_plate, Int32Array), new SimplexNoise(c.seed), c.axialTilt);
        const ms = performance.now() - t0;
        const keys = Object.keys(res), arrays = {};
        for (const k of keys) {
            if (k === '_windTiming') continue;
            writeArr(c.out + k + '.bin', res[k]);
            arrays[k] = res[k].constructor.name;
        }
        meta.cases[c.name] = { keys, arrays, ms, stages: res._windTiming.map((s) => [s.stage, s.ms]) };
    }
    fs.writeFileSync(job.meta, JSON.stringify(meta));
}
main().catch((e) => { console.error(e.stack || e); process.exit(1); });
