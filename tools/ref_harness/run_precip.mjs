// Golden-vector generator for the precipitation stage: runs the REFERENCE's own, unmodified computeWind, computeOceanCurrents
// and then computePrecipitation (scratch copy of the reference's js/, prepared by make_golden_precip.py) under Node 12 on given
// planets.  A case may name `precipitationOffset` / `landCoverage`; without them the call takes its defaults.  With job.pow the
// V8 values of Math.pow(b, 1 / h) are written as well.  Build container only (no GPU).  Test infrastructure.
//
//   node --harmony-optional-chaining --harmony-nullish run_precip.mjs <refJsDir> <job.json>
import fs from 'fs';
import path from 'path';
import { performance } from 'perf_hooks';
import { pathToFileURL } from 'url';

const refDir = process.argv[2];
const job = JSON.parse(fs.readFileSync(process.argv[3], 'utf8'));
globalThis.performance = performance;            // the climate modules time their stages with the browser's global

function readArr(file, Type) {
    const buf = fs.readFileSync(file);
    return new Type(buf.buffer.slice(buf.byteOffset, buf.byteOffset + buf.byteLength));
}
function writeArr(file, arr) { fs.writeFileSync(file, Buffer.from(arr.buffer, arr.byteOffset, arr.byteLength)); }

const WIND_INPUTS = ['r_lat', 'r_lon', 'r_isLand', 'r_continentality', 'r_coastDistLand', 'r_eastX', 'r_eastY', 'r_eastZ', 'r_northX', 'r_northY', 'r_northZ',
    'itczLons', 'itczLatsSummer', 'itczLatsWinter', 'r_wind_east_summer', 'r_wind_north_summer', 'r_pressure_summer',
    'r_wind_east_winter', 'r_wind_north_winter', 'r_pressure_winter'];
const OCEAN_INPUTS = ['r_ocean_warmth_summer', 'r_ocean_warmth_winter'];

async function main() {
    if (job.pow) {
        for (const [base, count, file] of job.pow) {
            const out = new Float64Array(count);
            for (let h = 1; h <= count; h++) out[h - 1] = Math.pow(base, 1 / h);
            writeArr(file, out);
        }
    }
    const W = await import(pathToFileURL(path.join(refDir, 'wind.js')).href);
    const O = await import(pathToFileURL(path.join(refDir, 'ocean.js')).href);
    const P = await import(pathToFileURL(path.join(refDir, 'precipitation.js')).href);
    const { SimplexNoise } = await import(pathToFileURL(path.join(refDir, 'simplex-noise.js')).href);
    const meta = { exports: Object.keys(P).sort(), cases: {} };
    for (const c of job.cases) {
        const mesh = { numRegions: c.numRegions, adjOffset: readArr(c.adjOffset, Int32Array), adjList: readArr(c.adjList, Int32Array) };
        const plateIsOcean = new Set(readArr(c.plateIsOcean, Int32Array));
        const xyz = readArr(c.xyz, Float32Array), elevation = readArr(c.elevation, Float32Array);
        const log = [], plain = console.log;
        console.log = (...a) => { log.push(a.join(' ')); };
        let res, ms, wind, ocean;
        try {
            wind = W.computeWind(mesh, xyz, elevation, plateIsOcean, readArr(c.r_plate, Int32Array), new SimplexNoise(c.seed), c.axialTilt);
            ocean = O.computeOceanCurrents(mesh, xyz, elevation, wind);
            log.length = 0;
            const t0 = performance.now();
            res = c.precipitationOffset === undefined ? P.computePrecipitation(mesh, xyz, elevation, wind, ocean)
                : P.computePrecipitation(mesh, xyz, elevation, wind, ocean, c.precipitationOffset, c.landCoverage);
            ms = performance.now() - t0;
        } finally { console.log = plain; }
        const keys = Object.keys(res), arrays = {}, inputs = {};
        for (const k of keys) {
            if (k === '_precipTiming') continue;
            writeArr(c.out + k + '.bin', res[k]);
            arrays[k] = res[k].constructor.name;
        }
        for (const k of WIND_INPUTS) { writeArr(c.out + 'in_' + k + '.bin', wind[k]); inputs[k] = wind[k].constructor.name; }
        for (const k of OCEAN_INPUTS) { writeArr(c.out + 'in_' + k + '.bin', ocean[k]); inputs[k] = ocean[k].constructor.name; }
        // the scalars of the call, by the reference's formulas under V8 (js/precipitation.js:208-210, :221, :291, :454, :550-551, :577-578, :609, :632)
        const avgEdgeKm = (Math.PI * 6371) / Math.sqrt(c.numRegions);
        const maxHops = Math.max(8, Math.min(20, Math.round(2000 / avgEdgeKm)));
        const shadowHops = Math.max(8, Math.round(2500 / avgEdgeKm)), windwardHops = Math.max(6, Math.round(1500 / avgEdgeKm));
        const scalars = { maxHops, elevSmoothPasses: Math.max(2, Math.round(200 / avgEdgeKm)), convSmoothPasses: Math.max(3, Math.round(400 / avgEdgeKm)),
            shadowHops, windwardHops, rsSmoothPasses: Math.max(2, Math.round(150 / avgEdgeKm)), precipSmoothPasses: Math.max(1, Math.round(100 / avgEdgeKm)),
            wcPasses: Math.max(2, Math.round(300 / avgEdgeKm)), leeCoastHops: Math.max(2, Math.round(200 / avgEdgeKm)) };
        const f64 = new Float64Array([1 - Math.pow(0.78, 1 / maxHops), 1 - Math.pow(0.15, 1 / shadowHops), 1 - Math.pow(0.25, 1 / windwardHops)]);
        writeArr(c.out + 'scalars_f64.bin', f64);
        meta.cases[c.name] = { keys, arrays, inputs, ms, log, scalars, stages: res._precipTiming.map((s) => [s.stage, s.ms]) };
    }
    fs.writeFileSync(job.meta, JSON.stringify(meta));
}
main().catch((e) => { console.error(e.stack || e); process.exit(1); });
