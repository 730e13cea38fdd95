// Golden-vector generator for the map export: runs the REFERENCE's own exportMapBatch, colour functions and gamma expression
// (scratch copy of the reference's js/, prepared by make_golden_map.py, which also writes the three / scene.js stubs it is run
// against) under Node 12.  No GPU is needed.  Test infrastructure.
//
//   node --harmony-optional-chaining --harmony-nullish run_map.mjs <refJsDir> <job.json>
import fs from 'fs';
import path from 'path';
import { pathToFileURL } from 'url';

const refDir = process.argv[2];
const job = JSON.parse(fs.readFileSync(process.argv[3], 'utf8'));

function readArr(file, Type) {
    const buf = fs.readFileSync(file);
    return new Type(buf.buffer.slice(buf.byteOffset, buf.byteOffset + buf.byteLength));
}
function writeArr(file, arr) { fs.writeFileSync(file, Buffer.from(arr.buffer, arr.byteOffset, arr.byteLength)); }

// the page the reference's modules expect to find
globalThis.__woRecorded = [];
globalThis.window = globalThis;
globalThis.navigator = { maxTouchPoints: 0 };
globalThis.location = { hash: '' };
globalThis.document = {
    createElement: () => ({
        width: 0, height: 0,
        getContext: () => ({ createImageData: (w, h) => ({ data: new Uint8ClampedArray(w * h * 4) }), putImageData: () => {} }),
        toBlob: (cb) => cb(null),
    }),
    getElementById: () => null,
};

const TYPES = ['color', 'heightmap', 'landheightmap', 'landmask', 'biome', 'koppen'];

async function main() {
    const PM = await import(pathToFileURL(path.join(refDir, 'planet-mesh.js')).href);
    const CM = await import(pathToFileURL(path.join(refDir, 'color-map.js')).href);
    const SM = await import(pathToFileURL(path.join(refDir, 'sphere-mesh.js')).href);
    const { state } = await import(pathToFileURL(path.join(refDir, 'state.js')).href);

    const triangles = readArr(job.triangles, Int32Array), halfedges = readArr(job.halfedges, Int32Array);
    const r_xyz = readArr(job.xyz, Float32Array), r_elevation = readArr(job.elevation, Float32Array), koppen = readArr(job.koppen, Uint8Array);
    const mesh = new SM.SphereMesh(triangles, halfedges, job.numRegions);
    const t_xyz = SM.generateTriangleCenters(mesh, r_xyz);
    const N = job.numRegions;

    // 1. the whole batch: positions once, one colour array per type
    state.curData = { mesh, r_xyz, t_xyz, r_elevation, debugLayers: { koppen }, seed: job.seed };
    __woRecorded.length = 0;
    const progress = [];
    await PM.exportMapBatch(TYPES.map((type) => ({ type, label: type })), job.width, (pct, label) => progress.push([pct, label]));
    const pos = __woRecorded.filter((r) => r.name === 'position'), col = __woRecorded.filter((r) => r.name === 'color');
    if (pos.length !== TYPES.length || col.length !== TYPES.length) throw new Error(`recorded ${pos.length} position and ${col.length} colour arrays`);
    const position = pos[0].array, triCount = position.length / 9;
    for (const p of pos) if (p.array !== position) throw new Error('the batch did not reuse its position array');
    const xy = new Float32Array(triCount * 6);
    for (let i = 0; i < triCount; i++)
        for (let c = 0; c < 3; c++) {
            xy[6 * i + 2 * c] = position[9 * i + 3 * c]; xy[6 * i + 2 * c + 1] = position[9 * i + 3 * c + 1];
            if (position[9 * i + 3 * c + 2] !== 0) throw new Error('z is not 0');
        }
    writeArr(job.out + 'position_xy.bin', xy);

    // 2. triRegions, which the batch keeps to itself: bit k of a triangle's region is its land-mask colour when r_elevation is
    //    bit k of the region id (one more tiny batch per bit)
    const triRegions = new Int32Array(triCount);
    for (let k = 0; (1 << k) <= N; k++) {
        const bitElev = new Float32Array(N);
        for (let r = 0; r < N; r++) bitElev[r] = ((r >> k) & 1) ? 1 : -1;
        state.curData = { mesh, r_xyz, t_xyz, r_elevation: bitElev, debugLayers: null, seed: job.seed };
        __woRecorded.length = 0;
        await PM.exportMapBatch([{ type: 'landmask', label: 'bit' }], 2, null);
        const c = __woRecorded.filter((r) => r.name === 'color')[0].array;
        if (c.length !== triCount * 9) throw new Error('triangle count changed');
        for (let i = 0; i < triCount; i++) if (c[9 * i] === 1) triRegions[i] |= (1 << k);
    }
    writeArr(job.out + 'triRegions.bin', triRegions);

    // 3. one colour per region per type, after checking that all of a region's triangles (and vertices) carry the same one
    for (let ti = 0; ti < TYPES.length; ti++) {
        const c = col[ti].array, out = new Float32Array(3 * N), seen = new Uint8Array(N);
        for (let i = 0; i < triCount; i++) {
            const r = triRegions[i];
            for (let v = 0; v < 3; v++)
                for (let ch = 0; ch < 3; ch++) {
                    const x = c[9 * i + 3 * v + ch];
                    if (seen[r] && !Object.is(out[3 * r + ch], x)) throw new Error(`region ${r} has two colours in ${TYPES[ti]}`);
                    out[3 * r + ch] = x;
                }
            seen[r] = 1;
        }
        if (seen.indexOf(0) >= 0) throw new Error('a region without triangles');
        writeArr(job.out + 'regionColor_' + TYPES[ti] + '.bin', out);
    }

    // 4. the gamma table (the reference's own expression, js/planet-mesh.js:1908-1910) and the background chain
    const lut = new Uint8Array(256);
    for (let k = 0; k < 256; k++) {
        const v = k / 255;
        lut[k] = (v <= 0.0031308
            ? v * 12.92
            : 1.055 * Math.pow(v, 1 / 2.4) - 0.055) * 255 + 0.5 | 0;
    }
    writeArr(job.out + 'lut.bin', lut);
    const srgbToLinear = (c) => (c < 0.04045) ? c * 0.0773993808 : Math.pow(c * 0.9478672986 + 0.0521327014, 2.4);     // three r160, math/ColorManagement.js
    const bgLinear = new Float32Array([0x1a, 0x1a, 0x2e].map((h) => srgbToLinear(h / 255)));
    writeArr(job.out + 'background_linear.bin', bgLinear);

    // 5. the colour sweep through the functions themselves
    const se = readArr(job.sweep_e, Float32Array), sk = readArr(job.sweep_k, Uint8Array);
    const fns = { color: CM.elevationToColor, heightmap: PM.heightmapColor, landheightmap: PM.landHeightmapColor, landmask: PM.landMaskColor };
    for (const [name, fn] of Object.entries(fns)) {
        const out = new Float32Array(3 * se.length);
        for (let i = 0; i < se.length; i++) out.set(fn(se[i]), 3 * i);
        writeArr(job.out + 'sweep_' + name + '.bin', out);
    }
    const ko = new Float32Array(3 * sk.length);
    for (let i = 0; i < sk.length; i++) ko.set(PM.koppenColor(sk[i]), 3 * i);
    writeArr(job.out + 'sweep_koppen.bin', ko);
    const bo = new Float32Array(3 * sk.length * se.length);                    // [k][e]
    for (let a = 0; a < sk.length; a++)
        for (let b = 0; b < se.length; b++) bo.set(CM.biomeColor(sk[a], se[b]), 3 * (a * se.length + b));
    writeArr(job.out + 'sweep_biome.bin', bo);
    // smoothBiomeColors, called directly: an isolated region keeps its raw colour
    const iso = PM.smoothBiomeColors({ numRegions: 3, adjOffset: new Int32Array([0, 2, 2, 3]), adjList: new Int32Array([1, 2, 0]) }, new Uint8Array([3, 0, 30]),
                                     new Float32Array([0.4, -0.2, 0.9]));
    writeArr(job.out + 'smooth_small.bin', iso);

    fs.writeFileSync(job.out + 'meta.json', JSON.stringify({ types: TYPES, triCount, progress: progress.slice(0, 4), filenames: null }));
}
main().catch((e) => { console.error(e.stack || e); process.exit(1); });
