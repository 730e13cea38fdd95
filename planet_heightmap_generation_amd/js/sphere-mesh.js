// Counterpart of the reference's js/sphere-mesh.js on the native mesh producer (no Delaunator needed):
// buildSphere / SphereMesh / computeNeighborDist keep their names, argument order and result shapes
// (js/sphere-mesh.js:94-146,174-203).  `rngSeed` is the number the caller would have passed to makeRng().
import addon from './native.js';

export class SphereMesh {
    // csr: { adjOffset, adjList, adjTriList } when the caller already has them (the device builder), else they are built here
    constructor(triangles, halfedges, numRegions, csr = null) {
        this.triangles = triangles;
        this.halfedges = halfedges;
        this.numRegions = numRegions;
        this.numSides = triangles.length;
        this.numTriangles = (triangles.length / 3) | 0;
        if (!csr) csr = addon.meshCsr(numRegions, triangles, halfedges);
        this._adjOffset = csr.adjOffset;
        this._adjList = csr.adjList;
        this._adjTriList = csr.adjTriList;
        this.adjOffset = this._adjOffset;
        this.adjList = this._adjList;
    }
    _next(s)     { return (s % 3 === 2) ? s - 2 : s + 1; }
    s_begin_r(s) { return this.triangles[s]; }
    s_end_r(s)   { return this.triangles[this._next(s)]; }
    s_inner_t(s) { return (s / 3) | 0; }
    s_outer_t(s) { return (this.halfedges[s] / 3) | 0; }
    r_circulate_r(out, r) {
        const start = this._adjOffset[r], len = this._adjOffset[r + 1] - start;
        out.length = len;
        for (let i = 0; i < len; i++) out[i] = this._adjList[start + i];
        return out;
    }
    r_circulate_t(out, r) {
        const start = this._adjOffset[r], len = this._adjOffset[r + 1] - start;
        out.length = len;
        for (let i = 0; i < len; i++) out[i] = this._adjTriList[start + i];
        return out;
    }
}

// ctx (a context handle): the points are made on the device, one thread per point (the same floats)
export function generateFibonacciSphere(N, jitter, rngSeed, ctx = null) {
    return (ctx ? addon.fibSpherePointsDevice(ctx, N, jitter, rngSeed) : addon.fibSpherePoints(N, jitter, rngSeed)).subarray(0, 3 * N);
}

// buildSphere(N, jitter, makeRng(seed)) in the reference; here the seed itself is passed.  referenceClosure: number the closing
// pole fan the way the reference's addPoleToMesh does (js/sphere-mesh.js:55-88) — the same triangles, but the CSR rows around the
// pole then start at the reference's neighbour, which the order-defined host stages (generatePlates, the plate smoothing) can see.
// ctx (a context handle, native.js: defaultContext()): the device builder makes the whole product in one call, the same arrays as
// the host route, and the result carries neighborDist as well.  devicePoints (needs ctx): the points are generated on the device too,
// into the buffer the mesh stage reads, in the same call.
export function buildSphere(N, jitter, rngSeed, referenceClosure = false, ctx = null, devicePoints = false) {
    if (devicePoints) {
        if (!ctx) throw new TypeError('buildSphere: devicePoints needs a context');
        const d = addon.sphereMeshSeedDevice(ctx, N, jitter, rngSeed, referenceClosure ? 1 : 0);
        return { mesh: new SphereMesh(d.triangles, d.halfedges, N + 1, d), r_xyz: d.r_xyz, neighborDist: d.neighborDist };
    }
    const r_xyz = addon.fibSpherePoints(N, jitter, rngSeed);         // pole already appended at index N
    if (ctx) {
        const d = addon.sphereMeshDevice(ctx, r_xyz, referenceClosure ? 1 : 0);
        return { mesh: new SphereMesh(d.triangles, d.halfedges, N + 1, d), r_xyz, neighborDist: d.neighborDist };
    }
    const { triangles, halfedges } = addon.sphereDelaunay(r_xyz);
    if (referenceClosure) addon.sphereReferenceClosure(N + 1, triangles, halfedges);
    return { mesh: new SphereMesh(triangles, halfedges, N + 1), r_xyz };
}

export function computeNeighborDist(mesh, r_xyz) {
    return addon.neighborDist(mesh.adjOffset, mesh.adjList, r_xyz);
}

export function computeTriangleElevations(mesh, r_elevation) {       // js/planet-worker.js:29-37
    return addon.triangleElevations(mesh.triangles, r_elevation);
}

export function generateTriangleCenters(mesh, r_xyz) {                // js/sphere-mesh.js:206-219
    return addon.triangleCenters(mesh.triangles, r_xyz);
}
