// Golden-vector generator for the map view's layers and centre meridian: runs the REFERENCE's own buildMapMesh and its six layer
// colour functions (scratch copy of the reference's js/, prepared by make_golden_map_layers.py, which also writes the three /
// scene.js stubs it is run against) under Node 12.  No GPU is needed.  Test infrastructure.
//
//   node --harmony-optional-chaining --harmony-nullish run_map_layers.mjs <refJsDir> <job.json>
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
globalThis.window = globalThis;
globalThis.navigator = { maxTouchPoints: 0 };
globalThis.location = { hash: '' };
globalThis.document = {
    createElement: () => ({ width: 0, height: 0, getContext: () => ({ createImageData: (w, h) => ({ data: new Uint8ClampedArray(w * h * 4) }), putImageData: () => {} }), toBlob: (cb) => cb(null) }),
    getElementById: () => ({ checked: false }),
};

async function main() {
    const PM = await import(pathToFileURL(path.join(refDir, 'planet-mesh.js')).href);
    const SM = await import(pathToFileURL(path.join(refDir, 'sphere-mesh.js')).href);
    const { state } = await import(pathToFileURL(path.join(refDir, 'state.js')).href);

    const triangles = readArr(job.triangles, Int32Array), halfedges = readArr(job.halfedges, Int32Array);
    const r_xyz = readArr(job.xyz, Float32Array), r_elevation = readArr(job.elevation, Float32Array);
    const mesh = new SM.SphereMesh(triangles, halfedges, job.numRegions);
    const t_xyz = SM.generateTriangleCenters(mesh, r_xyz);
    const N = job.numRegions;
    const F = {};
    for (const [k, file] of Object.entries(job.fields)) F[k] = readArr(file, Float32Array);
    const R = {};
    for (const [k, file] of Object.entries(job.ranges)) R[k] = readArr(file, Float32Array);

    // what buildMapMesh reads: the climate layers by their debugLayer names, the range cases as further keys, the four ocean fields
    const debugLayers = {};
    for (const [k, a] of Object.entries(F)) if (!k.startsWith('r_ocean_')) debugLayers[k] = a;
    for (const [k, a] of Object.entries(R)) debugLayers['range_' + k] = a;
    state.curData = { mesh, r_xyz, t_xyz, r_elevation, debugLayers, seed: job.seed,
                      r_ocean_warmth_summer: F.r_ocean_warmth_summer, r_ocean_speed_summer: F.r_ocean_speed_summer,
                      r_ocean_warmth_winter: F.r_ocean_warmth_winter, r_ocean_speed_winter: F.r_ocean_speed_winter };
    state.mapMode = true;

    function build(centerLon, debugLayer) {
        state.mapCenterLon = centerLon;
        state.debugLayer = debugLayer;
        PM.buildMapMesh();
        const geo = state.mapMesh.geometry, position = geo.attributes.position.array, color = geo.attributes.color.array, faceToSide = state.mapFaceToSide;
        const triCount = position.length / 9;
        if (faceToSide.length !== triCount || color.length !== position.length) throw new Error('array lengths disagree');
        if (state.mapMesh._builtCenterLon !== centerLon) throw new Error('the mesh was not built around the centre asked for');
        return { position, color, faceToSide, triCount };
    }
    function xyOf(b) {
        const xy = new Float32Array(b.triCount * 6);
        for (let i = 0; i < b.triCount; i++)
            for (let c = 0; c < 3; c++) {
                xy[6 * i + 2 * c] = b.position[9 * i + 3 * c]; xy[6 * i + 2 * c + 1] = b.position[9 * i + 3 * c + 1];
                if (b.position[9 * i + 3 * c + 2] !== 0) throw new Error('z is not 0');
            }
        return xy;
    }
    function regionsOf(b) {
        const out = new Int32Array(b.triCount);
        for (let i = 0; i < b.triCount; i++) out[i] = mesh.s_begin_r(b.faceToSide[i]);
        return out;
    }
    // one colour per region, after checking that all of a region's triangles (and vertices) carry the same one
    function regionColors(b, what) {
        const out = new Float32Array(3 * N), seen = new Uint8Array(N);
        for (let i = 0; i < b.triCount; i++) {
            const r = mesh.s_begin_r(b.faceToSide[i]);
            for (let v = 0; v < 3; v++)
                for (let ch = 0; ch < 3; ch++) {
                    const x = b.color[9 * i + 3 * v + ch];
                    if (seen[r] && !Object.is(out[3 * r + ch], x)) throw new Error(`region ${r} has two colours in ${what}`);
                    out[3 * r + ch] = x;
                }
            seen[r] = 1;
        }
        if (seen.indexOf(0) >= 0) throw new Error('a region without triangles');
        return out;
    }

    // 1. positions at centre 0 and at every other centre
    const centers = [0, ...job.centers], triCounts = [];
    for (let k = 0; k < centers.length; k++) {
        const b = build(centers[k], '');
        writeArr(job.out + 'position_c' + k + '.bin', xyOf(b));
        writeArr(job.out + (k === 0 ? 'triRegions.bin' : 'triRegions_c' + k + '.bin'), regionsOf(b));
        triCounts.push(b.triCount);
    }

    // 2. the colour of every region in every climate layer, and in the five range cases of a generic layer, at centre 0
    for (const name of job.layers) writeArr(job.out + 'regionColor_' + name + '.bin', regionColors(build(0, name), name));
    for (const name of job.rangeCases) {
        writeArr(job.out + 'regionColor_range_' + name + '.bin', regionColors(build(0, 'range_' + name), name));
        const a = R[name];
        let lo = 0, hi = 0;                                  // the loop of js/planet-mesh.js:233-236 restated
        for (let r = 0; r < N; r++) { if (a[r] < lo) lo = a[r]; if (a[r] > hi) hi = a[r]; }
        writeArr(job.out + 'rangeMinMax_' + name + '.bin', new Float32Array([lo, hi]));
    }

    // 3. the six colour functions called directly
    const S = {};
    for (const [k, file] of Object.entries(job.sweeps)) S[k] = readArr(file, Float32Array);
    const one = { precipitation: PM.precipitationColor, rainShadow: PM.rainShadowColor, continentality: PM.continentalityColor, temperature: PM.temperatureColor };
    for (const [name, fn] of Object.entries(one)) {
        const x = S['sweep_in_' + name], out = new Float32Array(3 * x.length);
        for (let i = 0; i < x.length; i++) out.set(fn(x[i]), 3 * i);
        writeArr(job.out + 'sweep_' + name + '.bin', out);
    }
    {
        const v = S.sweep_debug_v, lo = S.sweep_debug_min, hi = S.sweep_debug_max, out = new Float32Array(3 * v.length);
        for (let i = 0; i < v.length; i++) out.set(PM.debugValueToColor(v[i], lo[i], hi[i]), 3 * i);
        writeArr(job.out + 'sweep_debug.bin', out);
    }
    {
        const v = S.sweep_in_debugSelf, out = new Float32Array(3 * v.length);
        let lo = 0, hi = 0;
        for (let r = 0; r < v.length; r++) { if (v[r] < lo) lo = v[r]; if (v[r] > hi) hi = v[r]; }
        for (let i = 0; i < v.length; i++) out.set(PM.debugValueToColor(v[i], lo, hi), 3 * i);
        writeArr(job.out + 'sweep_debugSelf.bin', out);
        writeArr(job.out + 'sweep_debugSelf_minmax.bin', new Float32Array([lo, hi]));
    }
    {
        const w = S.sweep_ocean_warmth, sp = S.sweep_ocean_speed, el = S.sweep_ocean_elevation, out = new Float32Array(3 * w.length);
        for (let i = 0; i < w.length; i++) out.set(PM.oceanCurrentColor(w[i], sp[i], el[i] <= 0), 3 * i);
        writeArr(job.out + 'sweep_ocean.bin', out);
    }

    fs.writeFileSync(job.out + 'meta.json', JSON.stringify({ centers, triCounts, layers: job.layers, rangeCases: job.rangeCases }));
}
main().catch((e) => { console.error(e.stack || e); process.exit(1); });
