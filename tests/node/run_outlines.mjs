// Test driver for the outlines under Node:
//   node run_outlines.mjs shim            the shim's outline entries without a device: how they are defined, and the checks that come
//       before the planet handle (prints JSON)
//   node run_outlines.mjs worker <dir>    exportOutlines with nothing retained -> importHeightmap -> exportOutlines of the coast in every
//       format, of the plates, of levels, of one class -> exportGlobe without and with `outlines` (GLB and arrays) -> the refusals ->
//       dispose (reads <dir>/outline_job.json, writes <dir>/outline_result.json and the arrays beside it)
import fs from 'fs';
import path from 'path';
import { fileURLToPath } from 'url';
import { Worker } from 'worker_threads';
import { createRequire } from 'module';

const here = path.dirname(fileURLToPath(import.meta.url));
const pkg = path.join(here, '..', '..', 'planet_heightmap_generation_amd');
const typeName = (v) => (v === null ? 'null' : Array.isArray(v) ? 'Array' : (v && v.constructor ? v.constructor.name : typeof v));

function shim() {
    const addon = createRequire(import.meta.url)(path.join(pkg, 'worogen.node'));
    const out = {};
    const thrown = (f) => { try { f(); return null; } catch (e) { return [e.constructor.name, e.message]; } };
    for (const k of ['outlineBuild', 'outlineDownload', 'outlinePositions', 'outlineLonLat']) {
        const d = Object.getOwnPropertyDescriptor(addon, k) || {};
        out[`export ${k}`] = { type: typeof addon[k], enumerable: !!d.enumerable, writable: !!d.writable, configurable: !!d.configurable, listed: Object.keys(addon).indexOf(k) >= 0 };
    }
    const tri = new Int32Array(6), he = new Int32Array(6);
    out['outlineBuild()'] = { thrown: thrown(() => addon.outlineBuild()) };
    out['outlineBuild: halfedges of another type'] = { thrown: thrown(() => addon.outlineBuild(null, tri, new Float32Array(6), 0)) };
    out['outlineBuild: halfedges of another length'] = { thrown: thrown(() => addon.outlineBuild(null, tri, new Int32Array(3), 0)) };
    out['outlineBuild: no planet'] = { thrown: thrown(() => addon.outlineBuild(null, tri, he, 0)) };
    out['outlineDownload()'] = { thrown: thrown(() => addon.outlineDownload()) };
    out['outlinePositions({})'] = { thrown: thrown(() => addon.outlinePositions({}, 3, 1.002, null)) };
    out['outlineLonLat(null)'] = { thrown: thrown(() => addon.outlineLonLat(null, 3)) };
    console.log(JSON.stringify(out));
}

async function worker(dir) {
    const writeArr = (file, arr) => fs.writeFileSync(path.join(dir, file), Buffer.from(arr.buffer, arr.byteOffset, arr.byteLength));
    const job = JSON.parse(fs.readFileSync(path.join(dir, 'outline_job.json'), 'utf8'));
    const img = new Uint8Array(fs.readFileSync(path.join(dir, job.image)));
    const w = new Worker(path.join(pkg, 'js', 'planet-worker.js'));
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
        if (d.type === 'outlinesDone') {
            for (const k of ['source', 'format', 'filename', 'boundarySides', 'rings', 'longestRing', 'rounds', 'launches']) o[k] = d[k];
            o.fields = {};
            for (const k of ['sides', 'ring_start', 'ring_class', 'ring_of_side', 'lonlat']) if (d[k]) { o.fields[k] = typeName(d[k]); writeArr(`${tag}_${k}.bin`, d[k]); }
            if (typeof d.text === 'string') fs.writeFileSync(path.join(dir, `${tag}.txt`), d.text);
        }
        if (d.type === 'globeDone') for (const k of ['glb', 'outlines', 'position']) if (d[k]) { o[k] = typeName(d[k]); writeArr(`${tag}_${k}.bin`, d[k]); }
        return o;
    }

    const out = {};
    out.nothingRetained = describe('none', await ask({ cmd: 'exportOutlines', source: 'coast' }));
    const d = await ask({ cmd: 'importHeightmap', N: job.N, jitter: job.jitter, grayscale: img, imageWidth: job.W, imageHeight: job.H, seed: job.seed, ...job.params });
    out.imported = { type: d.type, message: d.message };
    out.coast = describe('coast', await ask({ cmd: 'exportOutlines', source: 'coast' }));
    out.coastGeojson = describe('coastGeojson', await ask({ cmd: 'exportOutlines', source: 'coast', format: 'geojson' }));
    out.coastSvg = describe('coastSvg', await ask({ cmd: 'exportOutlines', source: 'coast', format: 'svg', width: job.width, centerLon: job.centerLon }));
    out.plates = describe('plates', await ask({ cmd: 'exportOutlines', source: 'plates' }));
    out.levels = describe('levels', await ask({ cmd: 'exportOutlines', source: 'levels', levels: job.levels, onlyClass: 1 }));
    out.globePlain = describe('globePlain', await ask({ cmd: 'exportGlobe', glb: true, wireframe: true }));
    out.globeOutlines = describe('globeOutlines', await ask({ cmd: 'exportGlobe', glb: true, wireframe: true, outlines: { source: 'coast' } }));
    out.globeArrays = describe('globeArrays', await ask({ cmd: 'exportGlobe', outlines: { source: 'coast', onlyClass: 1 } }));
    out.errors = {};
    out.errors.badSource = describe('e1', await ask({ cmd: 'exportOutlines', source: 'shore' }));
    out.errors.badFormat = describe('e2', await ask({ cmd: 'exportOutlines', source: 'coast', format: 'kml' }));
    out.errors.noKoppen = describe('e3', await ask({ cmd: 'exportOutlines', source: 'koppen' }));
    out.errors.noRivers = describe('e4', await ask({ cmd: 'exportOutlines', source: 'lakes' }));
    out.errors.descending = describe('e5', await ask({ cmd: 'exportOutlines', source: 'levels', levels: [0.5, 0.1] }));
    out.errors.onlyClass = describe('e6', await ask({ cmd: 'exportOutlines', source: 'coast', onlyClass: -2 }));
    out.errors.noSuperPlates = describe('e7', await ask({ cmd: 'exportOutlines', source: 'superPlates' }));
    out.errors.globeNoSource = describe('e8', await ask({ cmd: 'exportGlobe', outlines: {} }));
    out.afterErrors = describe('after', await ask({ cmd: 'exportOutlines', source: 'coast' }));
    out.disposed = (await ask({ cmd: 'dispose' })).type;
    out.afterDispose = describe('gone', await ask({ cmd: 'exportOutlines', source: 'coast' }));
    await w.terminate();
    fs.writeFileSync(path.join(dir, 'outline_result.json'), JSON.stringify(out));
}

if (process.argv[2] === 'shim') shim();
else worker(process.argv[3]).catch((e) => { console.error(e.stack || e); process.exit(1); });
