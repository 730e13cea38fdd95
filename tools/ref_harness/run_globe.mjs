// Golden-vector generator for the globe mesh: runs the REFERENCE's own buildMesh, updateMeshColors and updateSuperPlateBorders
// (scratch copy of the reference's js/, prepared by make_golden_globe.py, which also writes the three / scene.js stubs it is run
// against) under Node 12.  No GPU is needed.  Test infrastructure.
//
//   node --harmony-optional-chaining --harmony-nullish run_globe.mjs <refJsDir> <job.json>
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

// the page the reference's modules expect to find; the two check boxes buildMesh reads are set per run
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
    const { state } = await import(pathToFileURL(path.join(refDir, 'state.js')).href);

    const triangles = readArr(job.triangles, Int32Array), halfedges = readArr(job.halfedges, Int32Array);
    const r_xyz = readArr(job.xyz, Float32Array), r_elevation = readArr(job.elevation, Float32Array);
    const N = job.numRegions;
    const mesh = new SM.SphereMesh(triangles, halfedges, N);
    const t_xyz = SM.generateTriangleCenters(mesh, r_xyz);
    // t_elevation as the reference's worker makes it (js/planet-worker.js:33-35)
    const t_elevation = new Float32Array(mesh.numTriangles);
    for (let t = 0; t < mesh.numTriangles; t++) {
        const s0 = 3 * t;
        t_elevation[t] = (r_elevation[mesh.s_begin_r(s0)] + r_elevation[mesh.s_begin_r(s0 + 1)] + r_elevation[mesh.s_begin_r(s0 + 2)]) / 3;
    }
    const debugLayers = { superPlates: readArr(job.superPlates, Float32Array) };
    debugLayers[job.layer] = readArr(job.layerField, Float32Array);
    state.curData = { mesh, r_xyz, t_xyz, r_elevation, t_elevation, debugLayers, r_plate: new Int32Array(N), seed: job.seed,
                      mountain_r: new Set(), coastline_r: new Set(), ocean_r: new Set(), r_stress: null };
    state.mapMode = false;
    state.plateColors = {};

    // 1. the default view with the wireframe; the super-plate borders need the Show Plates box, which changes the colours, so they
    //    come from a run of their own
    boxes.chkWire = true; boxes.chkPlates = false; state.debugLayer = '';
    PM.buildMesh();
    const geo = state.planetMesh.geometry;
    const position = geo.getAttribute('position').array, color = geo.getAttribute('color').array;
    if (position.length !== mesh.numSides * 9 || color.length !== position.length) throw new Error('array lengths disagree');
    writeArr(job.out + 'position.bin', position);
    writeArr(job.out + 'color_default.bin', new Float32Array(color));
    writeArr(job.out + 'wireframe.bin', state.wireMesh.geometry.getAttribute('position').array);
    writeArr(job.out + 't_elevation.bin', t_elevation);

    // how many sides had their winding swapped: the vertex stored second is the displaced region, not the outer centre
    const V = 0.04, same = (a, b) => Object.is(Math.fround(a), b);
    let swapped = 0;
    const swappedSides = new Uint8Array(mesh.numSides);
    for (let s = 0; s < mesh.numSides; s++) {
        const ot = mesh.s_outer_t(s), br = mesh.s_begin_r(s), re = r_elevation[br], ote = t_elevation[ot];
        const rDisp = 1.0 + (re > 0 ? re * V : re * V * 0.3), otDisp = 1.0 + (ote > 0 ? ote * V : ote * V * 0.3);
        let isOuter = true, isRegion = true;
        for (let k = 0; k < 3; k++) {
            if (!same(t_xyz[3 * ot + k] * otDisp, position[9 * s + 3 + k])) isOuter = false;
            if (!same(r_xyz[3 * br + k] * rDisp, position[9 * s + 3 + k])) isRegion = false;
        }
        if (!isOuter && !isRegion) throw new Error('side ' + s + ': the second vertex is neither the outer centre nor the region');
        // both: the two vertices have the same bits (NaN or infinite ones), the arrays cannot tell; such a side is marked 2 and not counted
        if (isOuter && isRegion) swappedSides[s] = 2;
        else if (isRegion) { swapped++; swappedSides[s] = 1; }
    }
    writeArr(job.out + 'swappedSides.bin', swappedSides);

    // 2. updateMeshColors into the same mesh for one layer
    state.debugLayer = job.layer;
    PM.updateMeshColors();
    writeArr(job.out + 'color_layer.bin', new Float32Array(state.planetMesh.geometry.getAttribute('color').array));

    // 3. the super-plate borders, globe form
    boxes.chkPlates = true; state.debugLayer = '';
    PM.updateSuperPlateBorders();
    if (!state.superPlateBorderMesh) throw new Error('no border mesh');
    writeArr(job.out + 'borders.bin', state.superPlateBorderMesh.geometry.getAttribute('position').array);
    const lineOpacity = { wireframe: state.wireMesh.material.opacity, superPlateBorders: state.superPlateBorderMesh.material.opacity };

    // 4. the plate view: every plate without a colour takes the fallback
    PM.updateMeshColors();
    const pc = state.planetMesh.geometry.getAttribute('color').array;
    const fallback = [pc[0], pc[1], pc[2]];
    for (let i = 0; i < pc.length; i++) if (!Object.is(pc[i], fallback[i % 3])) throw new Error('the plate fallback is not one colour');

    fs.writeFileSync(job.out + 'meta.json', JSON.stringify({ numSides: mesh.numSides, swapped, lineOpacity, plateFallback: fallback, layer: job.layer }));
}
main().catch((e) => { console.error(e.stack || e); process.exit(1); });
