// Golden-vector generator for the line overlays: runs the REFERENCE's own buildWindArrows, buildOceanCurrentArrows (with its ITCZ
// line) and rebuildGrids (scratch copy of the reference's js/, prepared by make_golden_overlays.py, which also writes the three /
// scene.js stubs it is run against and patches the copy so that the two builders leave their gridRegions in globalThis) under
// Node 12.  No GPU is needed.  Test infrastructure.
//
//   node --harmony-optional-chaining --harmony-nullish run_overlays.mjs <refJsDir> <job.json>
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

globalThis.window = globalThis;
globalThis.navigator = { maxTouchPoints: 0 };
globalThis.location = { hash: '' };
globalThis.document = {
    createElement: () => ({ width: 0, height: 0, getContext: () => ({ createImageData: (w, h) => ({ data: new Uint8ClampedArray(w * h * 4) }), putImageData: () => {} }), toBlob: (cb) => cb(null) }),
    getElementById: () => ({ checked: false }),
};
const log = console.log;
console.log = () => {};                                       // buildOceanCurrentArrows reports its count

// the group's line sets by name and by whether they carry colours (the arrows do, the ITCZ line does not)
function pick(group, name, colored) {
    const hit = group.children.filter((c) => c.name === name && !!c.geometry.getAttribute('color') === colored);
    if (hit.length > 1) throw new Error('two line sets named ' + name);
    return hit.length ? hit[0] : null;
}
const arr = (mesh, attr) => (mesh ? mesh.geometry.getAttribute(attr).array : new Float32Array(0));

async function main() {
    const PM = await import(pathToFileURL(path.join(refDir, 'planet-mesh.js')).href);
    const { state } = await import(pathToFileURL(path.join(refDir, 'state.js')).href);
    const meta = { calls: {}, opacity: {} };

    if (job.xyz) {
        const r_xyz = readArr(job.xyz, Float32Array);
        const N = r_xyz.length / 3;
        const cur = { mesh: { numRegions: N }, r_xyz, r_elevation: job.elevation ? readArr(job.elevation, Float32Array) : new Float32Array(N) };
        for (const [key, file] of Object.entries(job.fields || {})) cur[key] = readArr(file, Float32Array);
        state.curData = cur;
        state.mapMode = false;
        for (const c of job.calls) {
            state.mapCenterLon = c.centerLon;
            state.debugLayer = c.itcz ? (c.season === 'winter' ? 'pressureWinter' : 'pressureSummer') : '';
            globalThis.__gridRegions = null;
            state.windArrowGroup = null; state.oceanCurrentArrowGroup = null;      // the stub's groups cannot be traversed for disposal
            let group, names;
            if (c.fn === 'wind') { PM.buildWindArrows(c.season); group = state.windArrowGroup; names = ['windGlobe', 'windMap']; }
            else { PM.buildOceanCurrentArrows(c.season); group = state.oceanCurrentArrowGroup; names = ['oceanGlobe', 'oceanMap']; }
            if (!group || !globalThis.__gridRegions) throw new Error(c.prefix + ': the builder returned early');
            const g = pick(group, names[0], true), m = pick(group, names[1], true);
            writeArr(job.out + c.prefix + '_gridRegions.bin', globalThis.__gridRegions);
            writeArr(job.out + c.prefix + '_globe_position.bin', arr(g, 'position'));
            writeArr(job.out + c.prefix + '_globe_color.bin', arr(g, 'color'));
            writeArr(job.out + c.prefix + '_map_position.bin', arr(m, 'position'));
            writeArr(job.out + c.prefix + '_map_color.bin', arr(m, 'color'));
            meta.calls[c.prefix] = { count: arr(g, 'position').length / 18 };
            if (g) meta.opacity.arrows = g.material.opacity;
            if (c.itcz) {
                const ig = pick(group, names[0], false), im = pick(group, names[1], false);
                if (!ig || !im) throw new Error(c.prefix + ': no ITCZ line');
                writeArr(job.out + c.prefix + '_itcz_globe.bin', arr(ig, 'position'));
                writeArr(job.out + c.prefix + '_itcz_map.bin', arr(im, 'position'));
                meta.itczColor = ig.material.color;
            }
        }
        // what the loop computes per region, restated: the bin, d2 and whether d2 rounds up when it is stored
        if (job.probe) {
            const PI = Math.PI, DEG = PI / 180;
            const idx = new Int32Array(N).fill(-1), d2s = new Float64Array(N), up = new Uint8Array(N);
            for (let r = 0; r < N; r++) {
                const lat = Math.asin(Math.max(-1, Math.min(1, r_xyz[3 * r + 1])));
                const lon = Math.atan2(r_xyz[3 * r], r_xyz[3 * r + 2]);
                const li = Math.max(0, Math.min(59, Math.floor((lat + PI / 2) / (3 * DEG))));
                const lo = Math.max(0, Math.min(119, Math.floor((lon + PI) / (3 * DEG))));
                const dlat = lat - (-90 + li * 3 + 3 * 0.5) * DEG, dlon = lon - (-180 + lo * 3 + 3 * 0.5) * DEG;
                const d2 = dlat * dlat + dlon * dlon, i = li * 120 + lo;
                if (i === i) { idx[r] = i; d2s[r] = d2; up[r] = d2 < Math.fround(d2) ? 1 : 0; }
            }
            writeArr(job.out + 'probe_idx.bin', idx); writeArr(job.out + 'probe_d2.bin', d2s); writeArr(job.out + 'probe_up.bin', up);
        }
    }
    for (const g of job.grids || []) {
        state.gridSpacing = g.spacing; state.mapCenterLon = g.centerLon;
        PM.rebuildGrids();
        writeArr(job.out + g.prefix + '_globe.bin', state.globeGridMesh.geometry.getAttribute('position').array);
        writeArr(job.out + g.prefix + '_map.bin', state.mapGridMesh.geometry.getAttribute('position').array);
        meta.opacity.mapGrid = state.mapGridMesh.material.opacity;
        meta.opacity.globeGrid = state.globeGridMesh.material.uniforms.opacity.value;
    }
    fs.writeFileSync(job.out + 'meta.json', JSON.stringify(meta));
    log('run_overlays: ' + Object.keys(meta.calls).length + ' arrow calls, ' + (job.grids || []).length + ' grids');
}
main().catch((e) => { console.error(e.stack || e); process.exit(1); });
