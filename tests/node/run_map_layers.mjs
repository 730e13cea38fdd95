// Test driver for the layers and the centre meridian of the exportMap command of planet_heightmap_generation_amd/js/planet-worker.js:
// importHeightmap -> exportMap with a climate layer (no climate yet) -> computeClimate -> exportMap (color, every named layer and
// erosionDelta, around centerLon, png) -> an unknown layer -> `debug` by name -> exportMap without the new fields -> dispose; then the
// module's own exportMapBatch with layers on the small mesh.
//   node run_map_layers.mjs <dir>   (reads <dir>/layers_job.json and the image, writes <dir>/layers_result.json and the arrays)
import fs from 'fs';
import path from 'path';
import { fileURLToPath } from 'url';
import { Worker } from 'worker_threads';
import { MAP_LAYERS, MAP_TYPES, exportMap, exportMapBatch, layerFilename } from '../../planet_heightmap_generation_amd/js/map-export.js';

const here = path.dirname(fileURLToPath(import.meta.url));
const workerFile = path.join(here, '..', '..', 'planet_heightmap_generation_amd', 'js', 'planet-worker.js');
const dir = process.argv[2];
const job = JSON.parse(fs.readFileSync(path.join(dir, 'layers_job.json'), 'utf8'));
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
const ask = (msg) => new Promise((resolve) => { waiting = resolve; log = []; w.postMessage(msg); });
const typeName = (v) => (v === null ? 'null' : Array.isArray(v) ? 'Array' : (v && v.constructor ? v.constructor.name : typeof v));

function describe(tag, d) {
    const o = { type: d.type, message: d.message, keys: Object.keys(d), progress: log.slice() };
    if (d.type !== 'exportDone') return o;
    o.width = d.width; o.height = d.height;
    o.timingKeys = Object.keys(d._exportTiming);
    o.maps = d.maps.map((m) => ({ type: m.type, filename: m.filename, keys: Object.keys(m), rgba: typeName(m.rgba), png: m.png ? typeName(m.png) : null }));
    for (const m of d.maps) {
        writeArr(`${tag}_${m.type}.rgba`, m.rgba);
        if (m.png) writeArr(`${tag}_${m.type}.png`, m.png);
    }
    return o;
}

async function main() {
    const out = { layers: MAP_LAYERS, types: MAP_TYPES, filename: layerFilename('tempSummer', 7) };
    const d = await ask({ cmd: 'importHeightmap', N: job.N, jitter: job.jitter, grayscale: img, imageWidth: job.W, imageHeight: job.H, seed: job.seed, ...job.params });
    out.imported = { type: d.type, message: d.message };
    if (d.type === 'done') writeArr('erosionDelta.bin', d.debugLayers.erosionDelta);
    out.noWind = describe('nowind', await ask({ cmd: 'exportMap', type: 'color', layers: ['continentality'], width: job.width }));
    out.genericBeforeClimate = describe('generic', await ask({ cmd: 'exportMap', type: 'color', layers: ['erosionDelta'], width: 64 }));
    const c = await ask({ cmd: 'computeClimate' });
    out.climate = { type: c.type, message: c.message };
    out.all = describe('all', await ask({ cmd: 'exportMap', types: ['color'], layers: job.layers, centerLon: job.centerLon, width: job.width, png: true }));
    out.unknown = describe('unknown', await ask({ cmd: 'exportMap', type: 'color', layers: ['plates'], width: 64 }));
    out.debugByName = describe('debug', await ask({ cmd: 'exportMap', type: 'color', layers: ['debug'], width: 64 }));
    out.platesType = describe('platestype', await ask({ cmd: 'exportMap', type: 'plates', layers: ['tempSummer'], width: 64 }));
    out.badCenter = describe('badcenter', await ask({ cmd: 'exportMap', type: 'color', centerLon: 3.5, width: 64 }));
    out.old = describe('old', await ask({ cmd: 'exportMap', types: ['color', 'koppen'], width: job.width, png: true }));
    out.centerZero = describe('zero', await ask({ cmd: 'exportMap', types: ['color'], width: job.width, centerLon: 0 }));
    out.disposed = (await ask({ cmd: 'dispose' })).type;
    // the module's own exportMap / exportMapBatch with layers, on this thread, on the small mesh
    const n = job.small.numRegions;
    const whole = { numRegions: n, adjOffset: readArr(job.small.off, Int32Array), adjList: readArr(job.small.adj, Int32Array), triangles: readArr(job.small.tri, Int32Array),
                    halfedges: readArr(job.small.he, Int32Array) };
    const sxyz = readArr(job.small.xyz, Float32Array), se = readArr(job.small.e, Float32Array), sv = readArr(job.small.v, Float32Array);
    const batch = exportMapBatch(whole, sxyz, se, ['landmask'], 128, { layers: [{ name: 'slope', values: sv }, { name: 'precipWinter', values: sv }], centerLon: -2.5 });
    out.module = { batch: [batch.width, batch.height, batch.maps.map((m) => m.type)] };
    for (const m of batch.maps) writeArr(`module_${m.type}.rgba`, m.rgba);
    const one = exportMap(whole, sxyz, se, 'color', 128, { layers: [{ name: 'debug', values: sv }] });
    out.module.one = [Object.keys(one), one.maps.map((m) => m.type)];
    const threw = {};
    for (const [tag, layers] of [['noWind', ['windSpeedSummer']], ['unknown', ['plates']], ['debug', ['debug']]]) {
        try { exportMapBatch(whole, sxyz, se, ['color'], 128, { layers }); threw[tag] = null; } catch (e) { threw[tag] = e.message; }
    }
    out.module.threw = threw;
    fs.writeFileSync(path.join(dir, 'layers_result.json'), JSON.stringify(out));
    await w.terminate();
}
main().catch((e) => { console.error(e.stack || e); process.exit(1); });
