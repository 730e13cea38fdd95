// Golden-vector generator for the editor's hit test and highlights: runs the REFERENCE's own findNearestRegion, getHitInfoGlobe and
// getHitInfoMap (js/edit-mode.js) and its buildMesh / updateMeshColors with their highlight functions (js/planet-mesh.js) on a scratch
// copy of the reference's js/, prepared by make_golden_editor.py, which also writes the three / scene.js stubs it is run against and
// patches edit-mode.js (in the scratch copy only) to export its private functions and to record the direction that reaches
// findNearestRegion.  Under Node 12; no GPU is needed.  Test infrastructure.
//
//   node --harmony-optional-chaining --harmony-nullish run_editor.mjs <refJsDir> <job.json>
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

const boxes = { chkPlates: false, chkWire: false };
globalThis.window = globalThis;
globalThis.navigator = { maxTouchPoints: 0 };
globalThis.location = { hash: '' };
globalThis.document = {
    createElement: () => ({ width: 0, height: 0, getContext: () => ({ createImageData: (w, h) => ({ data: new Uint8ClampedArray(w * h * 4) }), putImageData: () => {} }), toBlob: (cb) => cb(null) }),
    getElementById: (id) => ({ checked: !!boxes[id] }),
};

async function main() {
    const PM = await import(pathToFileURL(path.join(refDir, 'planet-mesh.js')).href);
    const SM = await import(pathToFileURL(path.join(refDir, 'sphere-mesh.js')).href);
    const EM = await import(pathToFileURL(path.join(refDir, 'edit-mode.js')).href);
    const { state } = await import(pathToFileURL(path.join(refDir, 'state.js')).href);

    const triangles = readArr(job.triangles, Int32Array), halfedges = readArr(job.halfedges, Int32Array);
    const N = job.numRegions;
    const mesh = new SM.SphereMesh(triangles, halfedges, N);
    const r_plate = readArr(job.r_plate, Int32Array);
    const event = { clientX: 0, clientY: 0 };

    // ---- 1. the hit test: per case its positions, and direction / ray / map queries ------------------------------------------------
    // every answer: the region or -1, and the direction findNearestRegion was called with (NaN when it was not reached)
    function answer(call, n, regions, dirs, at) {
        for (let i = 0; i < n; i++) {
            globalThis.__pickDirection = null;
            const hit = call(i);
            regions[at + i] = hit ? hit.region : -1;
            if (hit && hit.plate !== r_plate[hit.region]) throw new Error('plate of the hit');
            const d = globalThis.__pickDirection;
            for (let k = 0; k < 3; k++) dirs[3 * (at + i) + k] = d ? d[k] : NaN;
        }
    }
    for (const c of job.pickCases) {
        const r_xyz = readArr(c.xyz, Float32Array);
        state.curData = { mesh, r_xyz, r_plate };
        state.planetMesh = { matrixWorld: {} };
        state.mapMesh = {};
        const D = readArr(c.directions, Float64Array), nD = D.length / 3;
        const regions = new Int32Array(nD), dirs = new Float64Array(3 * nD);
        answer((i) => EM.__findNearestRegion(D[3 * i], D[3 * i + 1], D[3 * i + 2]), nD, regions, dirs, 0);
        for (let i = 0; i < D.length; i++) if (!Object.is(D[i], dirs[i])) throw new Error('a direct query was not recorded as given');
        writeArr(c.out + 'regions.bin', regions);
        if (c.rays) {
            const R = readArr(c.rays, Float64Array), nR = R.length / 6;
            const rr = new Int32Array(nR), rd = new Float64Array(3 * nR);
            state.mapMode = false;
            answer((i) => { globalThis.__jobRay = R.subarray(6 * i, 6 * i + 6); return EM.__getHitInfoGlobe(event); }, nR, rr, rd, 0);
            writeArr(c.out + 'ray_regions.bin', rr);
            writeArr(c.out + 'ray_directions.bin', rd);
        }
        for (const m of c.maps || []) {
            const P = readArr(m.points, Float64Array), nP = P.length / 2;
            const mr = new Int32Array(nP), md = new Float64Array(3 * nP);
            state.mapMode = true;
            state.mapCenterLon = m.centerLon;
            // a ray straight down onto the point: t = -o.z / d.z = 1 and o.x + t * d.x = wx exactly
            answer((i) => { globalThis.__jobRay = [P[2 * i], P[2 * i + 1], 1, 0, 0, -1]; return EM.__getHitInfoMap(event); }, nP, mr, md, 0);
            writeArr(m.out + 'regions.bin', mr);
            writeArr(m.out + 'directions.bin', md);
        }
    }
    if (!job.states) return;

    // ---- 2. the highlights: buildMesh / updateMeshColors under every state, in the colour view and in the plate view ----------------
    const r_xyz = readArr(job.xyz, Float32Array), r_elevation = readArr(job.elevation, Float32Array);
    const t_xyz = SM.generateTriangleCenters(mesh, r_xyz);
    const t_elevation = new Float32Array(mesh.numTriangles);
    for (let t = 0; t < mesh.numTriangles; t++) {
        const s0 = 3 * t;
        t_elevation[t] = (r_elevation[mesh.s_begin_r(s0)] + r_elevation[mesh.s_begin_r(s0 + 1)] + r_elevation[mesh.s_begin_r(s0 + 2)]) / 3;
    }
    const koppen = readArr(job.koppen, Uint8Array);
    const plateColors = readArr(job.plateColors, Float32Array);
    state.curData = { mesh, r_xyz, t_xyz, r_elevation, t_elevation, debugLayers: { koppen }, r_plate, seed: job.seed, plateIsOcean: new Set(job.plateIsOcean),
                      mountain_r: new Set(), coastline_r: new Set(), ocean_r: new Set(), r_stress: null };
    state.mapMode = false;
    state.mapMesh = null;
    state.debugLayer = '';
    state.plateColors = {};
    job.plateSeeds.forEach((seed, i) => { state.plateColors[seed] = { r: plateColors[3 * i], g: plateColors[3 * i + 1], b: plateColors[3 * i + 2] }; });

    const colours = () => state.planetMesh.geometry.getAttribute('color').array;
    // one triple per side: the three vertices of a side must agree
    function perSide(c) {
        const out = new Float32Array(mesh.numSides * 3);
        for (let s = 0; s < mesh.numSides; s++)
            for (let k = 0; k < 3; k++) {
                const v = c[9 * s + k];
                if (!Object.is(v, c[9 * s + 3 + k]) || !Object.is(v, c[9 * s + 6 + k])) throw new Error('side ' + s + ': its vertices disagree');
                out[3 * s + k] = v;
            }
        return out;
    }
    const same = (a, b) => { if (a.length !== b.length) return false; for (let i = 0; i < a.length; i++) if (!Object.is(a[i], b[i])) return false; return true; };
    for (const view of ['color', 'plates']) {
        boxes.chkPlates = view === 'plates';
        for (const st of [{ name: 'none', pending: [], hoveredPlate: -1, hoveredKoppen: -1 }].concat(job.states)) {
            state.pendingToggles = new Set(st.pending);
            state.hoveredPlate = st.hoveredPlate;
            state.hoveredKoppen = st.hoveredKoppen;
            state._pendingBackup = null;                      // as main.js:863 does before a rebuild
            state.planetMesh = null;
            PM.buildMesh();
            if (st.hoveredKoppen >= 0) PM.updateKoppenHoverHighlight();
            const built = perSide(colours());
            // the colours alone into the same mesh: the same words
            PM.updateMeshColors();
            if (st.hoveredKoppen >= 0) PM.updateKoppenHoverHighlight();
            if (!same(built, perSide(colours()))) throw new Error(view + ' / ' + st.name + ': updateMeshColors differs from buildMesh');
            writeArr(job.out + 'color_' + view + '_' + st.name + '.bin', built);
        }
    }
}
main().catch((e) => { console.error(e.stack || e); process.exit(1); });
