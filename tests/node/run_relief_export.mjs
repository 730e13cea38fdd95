// Test driver for the exportRelief command of planet_heightmap_generation_amd/js/planet-worker.js and for js/relief-export.js:
//   node run_relief_export.mjs png16 <dir>     encodePng16 of <dir>/gray.bin (png16_job.json: width, height) -> <dir>/gray.png, and its refusals
//   node run_relief_export.mjs worker <dir>    exportRelief with nothing retained -> importHeightmap -> exportRelief on the map and on the
//       cube (faces, column), png -> the error answers -> an exportMap right after -> reapply -> exportRelief again -> dispose; then the
//       module's own exportRelief / exportCubeRelief on the small mesh (reads <dir>/relief_job.json, writes <dir>/relief_result.json)
import fs from 'fs';
import path from 'path';
import { fileURLToPath } from 'url';
import { Worker } from 'worker_threads';
import { RELIEF_KINDS, encodePng16, exportCubeRelief, exportRelief, reliefFilename } from '../../planet_heightmap_generation_amd/js/relief-export.js';

const here = path.dirname(fileURLToPath(import.meta.url));
const workerFile = path.join(here, '..', '..', 'planet_heightmap_generation_amd', 'js', 'planet-worker.js');
const mode = process.argv[2], dir = process.argv[3];
function readArr(file, Type) {
    const buf = fs.readFileSync(path.join(dir, file));
    return new Type(buf.buffer.slice(buf.byteOffset, buf.byteOffset + buf.byteLength));
}
function writeArr(file, arr) { fs.writeFileSync(path.join(dir, file), Buffer.from(arr.buffer, arr.byteOffset, arr.byteLength)); }
const typeName = (v) => (v === null ? 'null' : Array.isArray(v) ? 'Array' : (v && v.constructor ? v.constructor.name : typeof v));
const message = (f) => { try { f(); return null; } catch (e) { return `${e.constructor.name}: ${e.message}`; } };

function png16() {
    const job = JSON.parse(fs.readFileSync(path.join(dir, 'png16_job.json'), 'utf8'));
    const gray = readArr('gray.bin', Uint16Array);
    const png = encodePng16(gray, job.width, job.height);
    writeArr('gray.png', png);
    const out = { type: typeName(png), ownBuffer: png.byteOffset === 0 && png.buffer.byteLength === png.length,
                  threw: { notU16: message(() => encodePng16(new Uint8Array(4), 2, 1)), length: message(() => encodePng16(gray, job.width + 1, job.height)),
                           zero: message(() => encodePng16(new Uint16Array(0), 0, 0)) } };
    fs.writeFileSync(path.join(dir, 'png16_result.json'), JSON.stringify(out));
}

async function worker() {
    const job = JSON.parse(fs.readFileSync(path.join(dir, 'relief_job.json'), 'utf8'));
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
        if (d.type === 'exportDone') {
            o.width = d.width; o.height = d.height;
            for (const m of d.maps) writeArr(`${tag}_${m.type}.rgba`, m.rgba);
            return o;
        }
        if (d.type !== 'exportReliefDone') return o;
        Object.assign(o, { projection: d.projection, width: d.width, height: d.height, faceSize: d.faceSize, covered: d.covered, uncovered: d.uncovered,
                           timingKeys: Object.keys(d._exportTiming) });
        const image = (kind, f, name) => {
            writeArr(`${tag}_${name}.bin`, f.data);
            if (f.png) writeArr(`${tag}_${name}.png`, f.png);
            return { kind, face: f.face, filename: f.filename, keys: Object.keys(f), data: typeName(f.data), length: f.data.length, png: f.png ? typeName(f.png) : null };
        };
        o.maps = d.maps.map((m) => (m.faces
            ? { kind: m.kind, keys: Object.keys(m), faces: m.faces.map((f) => image(m.kind, f, `${m.kind}_${f.face}`)),
                oneBuffer: m.faces.every((f, k) => f.data.buffer === m.faces[0].data.buffer && f.data.byteOffset === m.faces[0].data.byteOffset + k * f.data.byteLength) }
            : image(m.kind, m, m.kind)));
        return o;
    }

    const out = {};
    const S = job.faceSize, W = job.width, kinds = job.kinds;
    out.nothingRetained = describe('none', await ask({ cmd: 'exportRelief', kinds, width: W }));
    const d = await ask({ cmd: 'importHeightmap', N: job.N, jitter: job.jitter, grayscale: img, imageWidth: job.W, imageHeight: job.H, seed: job.seed, ...job.params });
    out.imported = { type: d.type, message: d.message };
    out.map = describe('map', await ask({ cmd: 'exportRelief', projection: 'map', kinds, width: W, centerLon: job.centerLon, strength: job.strength, flatOcean: true, png: true }));
    out.faces = describe('faces', await ask({ cmd: 'exportRelief', projection: 'cube', kinds, faceSize: S, strength: job.strength, png: true }));
    out.column = describe('column', await ask({ cmd: 'exportRelief', projection: 'cube', kinds: ['height16', 'normal'], faceSize: S, layout: 'column', png: true }));
    out.plain = describe('plain', await ask({ cmd: 'exportRelief', kinds: ['landHeight16'], width: 16 }));
    // the relief raster left an exportMap's region map: the colours need no raster of their own to be right, and the next one ends the relief
    out.flat = describe('flat', await ask({ cmd: 'exportMap', types: ['heightmap'], width: W }));
    out.errors = {};
    for (const [tag, msg] of Object.entries({
        noKinds: { kinds: [], width: W }, unknownKind: { kinds: ['heightmap'], width: W }, oddWidth: { kinds, width: 33 }, noWidth: { kinds },
        badProjection: { kinds, width: W, projection: 'cylinder' }, zeroFace: { kinds, projection: 'cube', faceSize: 0 }, largeFace: { kinds, projection: 'cube', faceSize: 16385 },
        badLayout: { kinds, projection: 'cube', faceSize: S, layout: 'cross' }, negativeStrength: { kinds: ['normal'], width: W, strength: -1 },
        badCenter: { kinds, width: W, centerLon: 4 } })) out.errors[tag] = describe(tag, await ask({ cmd: 'exportRelief', ...msg }));
    const r = await ask({ cmd: 'reapply', ...job.params2 });
    out.reapply = r.type;
    if (r.type === 'reapplyDone') writeArr('re_elevation.bin', r.r_elevation);
    out.afterReapply = describe('after', await ask({ cmd: 'exportRelief', kinds: ['height16', 'normal'], width: W }));
    out.disposed = (await ask({ cmd: 'dispose' })).type;
    out.afterDispose = describe('gone', await ask({ cmd: 'exportRelief', kinds, width: W }));
    await w.terminate();

    // the module's own exportRelief / exportCubeRelief, on this thread, on the small mesh
    const n = job.small.numRegions;
    const whole = { numRegions: n, adjOffset: readArr(job.small.off, Int32Array), adjList: readArr(job.small.adj, Int32Array),
                    triangles: readArr(job.small.tri, Int32Array), halfedges: readArr(job.small.he, Int32Array) };
    const sxyz = readArr(job.small.xyz, Float32Array), se = readArr(job.small.e, Float32Array);
    const flat = exportRelief(whole, sxyz, se, RELIEF_KINDS, 64, { centerLon: 0.5, strength: 3 });
    const cube = exportCubeRelief(whole, sxyz, se, ['landHeight16', 'normalObject'], 9, { flatOcean: true });
    for (const m of flat.maps) writeArr(`module_map_${m.kind}.bin`, m.data);
    for (const m of cube.maps) writeArr(`module_cube_${m.kind}.bin`, m.data);
    out.module = { kinds: RELIEF_KINDS, flat: [flat.width, flat.height, flat.maps.map((m) => [m.kind, typeName(m.data), m.data.length])],
                   cube: [cube.faceSize, cube.maps.map((m) => [m.kind, typeName(m.data), m.data.length, m.faces.map((f) => [f.face, f.data.length])])],
                   filenames: [reliefFilename('height16', 7), reliefFilename('landHeight16', 7, 'ny'), reliefFilename('normalObject', 7, 'column')],
                   threw: { kind: message(() => exportRelief(whole, sxyz, se, ['color'], 64)), width: message(() => exportRelief(whole, sxyz, se, ['normal'], 63)),
                            face: message(() => exportCubeRelief(whole, sxyz, se, ['normal'], 2.5)), elevation: message(() => exportRelief(whole, sxyz, se.subarray(1), ['normal'], 64)),
                            filename: message(() => reliefFilename('normal', 7, 'top')) } };
    fs.writeFileSync(path.join(dir, 'relief_result.json'), JSON.stringify(out));
}

(mode === 'png16' ? Promise.resolve().then(png16) : worker()).catch((e) => { console.error(e.stack || e); process.exit(1); });
