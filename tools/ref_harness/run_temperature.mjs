// Golden-vector generator for the temperature stage and the Koppen classification: runs the REFERENCE's own, unmodified
// computeWind, computeOceanCurrents, computePrecipitation, computeTemperature and classifyKoppen (scratch copy of the reference's
// js/, prepared by make_golden_temperature.py) under Node 12 on given planets.  A case may name `precipitationOffset` /
// `landCoverage` / `temperatureOffset`; without them the calls take their defaults.  job.lattice: classifyKoppen on given arrays.
// job.classes: the module's KOPPEN_CLASSES as JSON.  job.climate: the worker's own importHeightmap followed by computeClimate.
// Build container only (no GPU).  Test infrastructure.
//
//   node --harmony-optional-chaining --harmony-nullish run_temperature.mjs <refJsDir> <job.json>
import fs from 'fs';
import path from 'path';
import { performance } from 'perf_hooks';
import { pathToFileURL } from 'url';

const refDir = process.argv[2];
const job = JSON.parse(fs.readFileSync(process.argv[3], 'utf8'));
const posted = [];
globalThis.performance = performance;            // the climate modules time their stages with the browser's global
globalThis.self = { postMessage: (m) => posted.push(m) };

function readArr(file, Type) {
    const buf = fs.readFileSync(file);
    return new Type(buf.buffer.slice(buf.byteOffset, buf.byteOffset + buf.byteLength));
}
function writeArr(file, arr) { fs.writeFileSync(file, Buffer.from(arr.buffer, arr.byteOffset, arr.byteLength)); }

const WIND_INPUTS = ['r_lat', 'r_lon', 'r_isLand', 'r_continentality', 'r_plateContinentality', 'itczLons', 'itczLatsSummer', 'itczLatsWinter'];
const OCEAN_INPUTS = ['r_ocean_warmth_summer', 'r_ocean_speed_summer', 'r_ocean_warmth_winter', 'r_ocean_speed_winter'];
const PRECIP_INPUTS = ['r_precip_summer', 'r_precip_winter'];

async function main() {
    const load = (f) => import(pathToFileURL(path.join(refDir, f)).href);
    const W = await load('wind.js'), O = await load('ocean.js'), P = await load('precipitation.js'), T = await load('temperature.js'), K = await load('koppen.js');
    const { SimplexNoise } = await load('simplex-noise.js');
    const meta = { exports: Object.keys(T).sort(), koppenExports: Object.keys(K).sort(), cases: {} };
    if (job.classes) fs.writeFileSync(job.classes, JSON.stringify(K.KOPPEN_CLASSES, null, 1) + '\n');
    if (job.lattice) {
        const L = job.lattice, n = L.numRegions;
        const f = (k) => readArr(L[k], Float32Array);
        const out = K.classifyKoppen({ numRegions: n }, f('elevation'), { r_temperature_summer: f('tSummer'), r_temperature_winter: f('tWinter') },
            { r_precip_summer: f('pSummer'), r_precip_winter: f('pWinter') });
        writeArr(L.out, out);
        meta.lattice = { type: out.constructor.name };
    }
    for (const c of job.cases || []) {
        const mesh = { numRegions: c.numRegions, adjOffset: readArr(c.adjOffset, Int32Array), adjList: readArr(c.adjList, Int32Array) };
        const plateIsOcean = new Set(readArr(c.plateIsOcean, Int32Array));
        const xyz = readArr(c.xyz, Float32Array), elevation = readArr(c.elevation, Float32Array);
        const log = [], plain = console.log;
        console.log = (...a) => { log.push(a.join(' ')); };
        let res, koppen, ms, msKoppen, wind, ocean, precip;
        try {
            wind = W.computeWind(mesh, xyz, elevation, plateIsOcean, readArr(c.r_plate, Int32Array), new SimplexNoise(c.seed), c.axialTilt);
            ocean = O.computeOceanCurrents(mesh, xyz, elevation, wind);
            precip = c.precipitationOffset === undefined ? P.computePrecipitation(mesh, xyz, elevation, wind, ocean)
                : P.computePrecipitation(mesh, xyz, elevation, wind, ocean, c.precipitationOffset, c.landCoverage);
            log.length = 0;
            let t0 = performance.now();
            res = c.temperatureOffset === undefined ? T.computeTemperature(mesh, xyz, elevation, wind, ocean, precip)
                : T.computeTemperature(mesh, xyz, elevation, wind, ocean, precip, c.temperatureOffset);
            ms = performance.now() - t0;
            t0 = performance.now();
            koppen = K.classifyKoppen(mesh, elevation, res, precip);
            msKoppen = performance.now() - t0;
        } finally { console.log = plain; }
        const keys = Object.keys(res), arrays = {}, inputs = {};
        for (const k of keys) {
            if (k === '_tempTiming') continue;
            writeArr(c.out + k + '.bin', res[k]);
            arrays[k] = res[k].constructor.name;
        }
        writeArr(c.out + 'koppen.bin', koppen);
        arrays.koppen = koppen.constructor.name;
        const all = { ...wind, ...ocean, ...precip };
        for (const k of [...WIND_INPUTS, ...OCEAN_INPUTS, ...PRECIP_INPUTS]) { writeArr(c.out + 'in_' + k + '.bin', all[k]); inputs[k] = all[k].constructor.name; }
        // the pass count by the reference's formula under V8 (js/temperature.js:100-101)
        const avgEdgeKm = (Math.PI * 6371) / Math.sqrt(c.numRegions);
        const scalars = { oceanWarmthPasses: Math.max(4, Math.round(1400 / avgEdgeKm)) };
        meta.cases[c.name] = { keys, arrays, inputs, ms, msKoppen, log, scalars, stages: res._tempTiming.map((s) => [s.stage, s.ms]) };
    }
    if (job.climate) {
        // the worker's own handlers: importHeightmap (as tools/ref_harness/run_import.mjs runs it), then computeClimate twice
        const imp = job.climate;
        globalThis.__woTriangulations = {};
        for (const t of imp.triangulations) globalThis.__woTriangulations[t.n] = { triangles: readArr(t.triangles, Int32Array), halfedges: readArr(t.halfedges, Int32Array) };
        await load('planet-worker.js');
        self.onmessage({ data: { cmd: 'computeClimate' } });             // nothing retained yet
        const withoutState = posted.filter((m) => m.type === 'error').map((m) => m.message);
        posted.length = 0;
        const plain = console.log;
        console.log = () => {};
        try {
            self.onmessage({ data: { cmd: 'importHeightmap', N: imp.N, jitter: imp.jitter, grayscale: readArr(imp.image, Uint8Array), imageWidth: imp.W,
                                     imageHeight: imp.H, seed: imp.seed, skipClimate: true, ...imp.params } });
            if (!posted.find((m) => m.type === 'done')) throw new Error('importHeightmap did not answer done');
            posted.length = 0;
            self.onmessage({ data: { cmd: 'computeClimate' } });
        } finally { console.log = plain; }
        const done = posted.find((m) => m.type === 'climateDone');
        if (!done) throw new Error('computeClimate did not answer climateDone: ' + JSON.stringify(posted.filter((m) => m.type !== 'progress')));
        const arrays = {}, layers = {};
        for (const k of Object.keys(done)) if (ArrayBuffer.isView(done[k])) { writeArr(imp.out + k + '.bin', done[k]); arrays[k] = done[k].constructor.name; }
        for (const k of Object.keys(done.climateDebugLayers)) { writeArr(imp.out + 'layer_' + k + '.bin', done.climateDebugLayers[k]); layers[k] = done.climateDebugLayers[k].constructor.name; }
        meta.climate = { keys: Object.keys(done), arrays, layers, timingKeys: Object.keys(done._climateTiming), withoutState,
                         progress: posted.filter((m) => m.type === 'progress').map((m) => [m.pct, m.label]) };
        // a second command reuses the cached wind and ocean
        posted.length = 0;
        self.onmessage({ data: { cmd: 'computeClimate', temperatureOffset: 10 } });
        const second = posted.find((m) => m.type === 'climateDone');
        meta.climate.secondWind = second._climateTiming.wind;
        meta.climate.secondProgress = posted.filter((m) => m.type === 'progress').map((m) => [m.pct, m.label]);
    }
    fs.writeFileSync(job.meta, JSON.stringify(meta));
}
main().catch((e) => { console.error(e.stack || e); process.exit(1); });
