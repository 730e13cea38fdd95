// Golden-vector generator for the ocean-current stage: runs the REFERENCE's own, unmodified computeWind and then
// computeOceanCurrents (scratch copy of the reference's js/, prepared by make_golden_ocean.py) under Node 12 on given
// planets.  The lines the reference logs during computeOceanCurrents are kept.  Build container only (no GPU).
// Test infrastructure.
//
//   node --harmony-optional-chaining --harmony-nullish run_ocean.mjs <refJsDir> <job.json>
import fs from 'fs';
import path from 'path';
import { performance } from 'perf_hooks';
import { pathToFileURL } from 'url';

const refDir = process.argv[2];
const job = JSON.parse(fs.readFileSync(process.argv[3], 'utf8'));
globalThis.performance = performance;            // wind.js and ocean.js time their stages with the browser's global

function readArr(file, Type) {
    const buf = fs.readFileSync(file);
    return new Type(buf.buffer.slice(buf.byteOffset, buf.byteOffset + buf.byteLength));
}
function writeArr(file, arr) { fs.writeFileSync(file, Buffer.from(arr.buffer, arr.byteOffset, arr.byteLength)); }

const WIND_INPUTS = ['r_lat', 'r_lon', 'r_isLand', 'r_eastX', 'r_eastY', 'r_eastZ', 'itczLons', 'itczLatsSummer', 'itczLatsWinter'];

async function main() {
    const W = await import(pathToFileURL(path.join(refDir, 'wind.js')).href);
    const O = await import(pathToFileURL(path.join(refDir, 'ocean.js')).href);
    const { SimplexNoise } = await import(pathToFileURL(path.join(refDir, 'simplex-noise.js')).href);
    const meta = { exports: Object.keys(O).sort(), cases: {} };
    for (const c of job.cases) {
        const mesh = { numRegions: c.numRegions, adjOffset: readArr(c.adjOffset, Int32Array), adjList: readArr(c.adjList, Int32Array) };
        const plateIsOcean = new Set(readArr(c.plateIsOcean, Int32Array));
        const xyz = readArr(c.xyz, Float32Array), elevation = readArr(c.elevation, Float32Array);
        const wind = W.computeWind(mesh, xyz, elevation, plateIsOcean, readArr(c.r_plate, Int32Array), new SimplexNoise(c.seed), c.axialTilt);
        const log = [], plain = console.log;
        console.log = (...a) => { log.push(a.join(' ')); };
        let res, ms;
        try {
            const t0 = performance.now();
            res = O.computeOceanCurrents(mesh, xyz, elevation, wind);
            ms = performance.now() - t0;
        } finally { console.log = plain; }
        const keys = Object.keys(res), arrays = {}, inputs = {};
        for (const k of keys) {
            if (k === '_oceanTiming') continue;
            writeArr(c.out + k + '.bin', res[k]);
            arrays[k] = res[k].constructor.name;
        }
        for (const k of WIND_INPUTS) { writeArr(c.out + 'in_' + k + '.bin', wind[k]); inputs[k] = wind[k].constructor.name; }
        meta.cases[c.name] = { keys, arrays, inputs, ms, log, stages: res._oceanTiming.map((s) => [s.stage, s.ms]) };
    }
    fs.writeFileSync(job.meta, JSON.stringify(meta));
}
main().catch((e) => { console.error(e.stack || e); process.exit(1); });
