// Test driver for the exportGlobe command of planet_heightmap_generation_amd/js/planet-worker.js: importHeightmap -> exportGlobe of a
// climate layer (no climate yet) -> computeClimate -> exportGlobe of the default view, of one layer and of `plates`, each with both
// line sets, as GLB and as arrays -> the error answers -> an old exportMap command -> dispose; then the module's own buildMesh on the
// small mesh.
//   node run_globe.mjs <dir>   (reads <dir>/globe_job.json and the image, writes <dir>/globe_result.json and the arrays)
import fs from 'fs';
import path from 'path';
import { fileURLToPath } from 'url';
import { Worker } from 'worker_threads';
import { buildMesh, updateMeshColors, buildWireframe, updateSuperPlateBorders, computePlateColors, encodeGlb, globeFilename } from '../../planet_heightmap_generation_amd/js/globe-export.js';

const here = path.dirname(fileURLToPath(import.meta.url));
const workerFile = path.join(here, '..', '..', 'planet_heightmap_generation_amd', 'js', 'planet-worker.js');
const dir = process.argv[2];
const job = JSON.parse(fs.readFileSync(path.join(dir, 'globe_job.json'), 'utf8'));
function readArr(file, Type) {
    const buf = fs.readFileSync(path.join(dir, file));
    return new Type(buf.buffer.slice(buf.byteOffset, buf.byteOffset + buf.byteLength));
}
function writeArr(file, arr) { fs.writeFileSync(path.join(dir, file), Buffer.from(arr.buffer, arr.byteOffset, arr.byteLength)); }
const img = new Uint8Array(fs.readFileSync(path.join(dir, job.image)));
const sp = readArr(job.superPlates, Float32Array);

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
    if (d.type === 'exportDone') { for (const m of d.maps) writeArr(`${tag}_${m.type}.rgba`, m.rgba); o.maps = d.maps.map((m) => [m.type, m.filename]); return o; }
    if (d.type !== 'globeDone') return o;
    o.view = d.view; o.filename = d.filename; o.numSides = d.numSides; o.bounds = Array.from(d.bounds);
    o.kinds = {};
    for (const k of ['glb', 'position', 'color', 'wireframe', 'superPlateBorders']) if (d[k]) { o.kinds[k] = typeName(d[k]); writeArr(`${tag}.${k}`, d[k]); }
    return o;
}

async function main() {
    const out = { filename: globeFilename('koppen', 7) };
    const d = await ask({ cmd: 'importHeightmap', N: job.N, jitter: job.jitter, grayscale: img, imageWidth: job.W, imageHeight: job.H, seed: job.seed, ...job.params });
    out.imported = { type: d.type, message: d.message };
    out.noWind = describe('nowind', await ask({ cmd: 'exportGlobe', layer: 'continentality' }));
    const c = await ask({ cmd: 'computeClimate' });
    out.climate = { type: c.type, message: c.message };
    for (const [tag, extra] of [['default', {}], ['layer', { layer: job.layer }], ['plates', { plates: true }], ['koppen', { view: 'koppen' }]]) {
        out[tag + 'Glb'] = describe(tag + '_glb', await ask({ cmd: 'exportGlobe', ...extra, wireframe: true, superPlateBorders: sp, glb: true }));
    }
    out.arrays = describe('arrays', await ask({ cmd: 'exportGlobe', layer: job.layer, wireframe: true, superPlateBorders: sp }));
    out.bare = describe('bare', await ask({ cmd: 'exportGlobe' }));
    out.generic = describe('generic', await ask({ cmd: 'exportGlobe', layer: 'erosionDelta' }));
    out.unknownLayer = describe('unknownlayer', await ask({ cmd: 'exportGlobe', layer: 'stress' }));
    out.landmask = describe('landmask', await ask({ cmd: 'exportGlobe', view: 'landmask' }));
    out.noSuperPlates = describe('nosp', await ask({ cmd: 'exportGlobe', superPlateBorders: true }));
    out.oldMap = describe('oldmap', await ask({ cmd: 'exportMap', types: ['color', 'koppen'], width: job.width }));
    out.disposed = (await ask({ cmd: 'dispose' })).type;
    out.afterDispose = describe('gone', await ask({ cmd: 'exportGlobe' }));
    // the module's own functions, on this thread, on the small mesh
    const s = job.small, n = s.numRegions;
    const whole = { numRegions: n, adjOffset: readArr(s.off, Int32Array), adjList: readArr(s.adj, Int32Array), triangles: readArr(s.tri, Int32Array), halfedges: readArr(s.he, Int32Array) };
    const sxyz = readArr(s.xyz, Float32Array), se = readArr(s.e, Float32Array), ssp = readArr(s.sp, Float32Array), plate = readArr(s.plate, Int32Array);
    const m = buildMesh(whole, sxyz, se, 'heightmap');
    writeArr('module.position', m.position); writeArr('module.color', m.color); writeArr('module.bounds', m.bounds);
    writeArr('module.layer', updateMeshColors(whole, sxyz, se, 'precipWinter', { values: ssp }));
    writeArr('module.wireframe', buildWireframe(whole, sxyz, se));
    writeArr('module.borders', updateSuperPlateBorders(whole, sxyz, se, ssp));
    const colors = computePlateColors(s.seeds, new Set(s.ocean));
    writeArr('module.plates', updateMeshColors(whole, sxyz, se, 'plates', { plates: { r_plate: plate, plateSeeds: s.seeds, plateColors: colors } }));
    writeArr('module.glb', encodeGlb(m));
    const threw = {};
    for (const [tag, f] of [['landmask', () => buildMesh(whole, sxyz, se, 'landmask')], ['noWind', () => buildMesh(whole, sxyz, se, 'windSpeedSummer')],
                            ['noTable', () => buildMesh(whole, sxyz, se, 'plates', { plates: { r_plate: plate } })]]) {
        try { f(); threw[tag] = null; } catch (e) { threw[tag] = e.message; }
    }
    out.threw = threw;
    fs.writeFileSync(path.join(dir, 'globe_result.json'), JSON.stringify(out));
    await w.terminate();
}
main().catch((e) => { console.error(e.stack || e); process.exit(1); });
