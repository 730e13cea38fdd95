// N-API shim: the thin binding between the JavaScript host (planet_heightmap_generation_amd/js/*.js) and
// the C ABI of libworogen (include/worogen.h).  It only unwraps typed arrays into pointers, forwards the
// call and turns a non-zero status into a thrown JS Error carrying wo_last_error() — which is how the
// reference's worker expects failures to surface (try/catch around each handler, js/planet-worker.js:336-338).
// No computation happens here.  Built with plain g++ against /usr/include/node (N-API v8, Node >= 12).
#include <node_api.h>

#include <cstdint>
#include <cstring>
#include <initializer_list>
#include <string>
#include <vector>

#include "../../include/worogen.h"

namespace {

#define NAPI_OK(call)                                                          \
    do { if ((call) != napi_ok) { napi_throw_error(env, nullptr, "N-API call failed: " #call); return nullptr; } } while (0)

napi_value throw_wo(napi_env env, const char* what) {
    std::string msg = std::string(what) + ": " + wo_last_error();
    napi_throw_error(env, nullptr, msg.c_str());
    return nullptr;
}

struct Args {
    napi_env env; size_t argc = 16; napi_value argv[16];
    bool ok = true;
    Args(napi_env e, napi_callback_info info) : env(e) { ok = napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr) == napi_ok; }
    bool has(size_t i) const {
        if (i >= argc) return false;
        napi_valuetype t; napi_typeof(env, argv[i], &t);
        return t != napi_undefined && t != napi_null;
    }
    double num(size_t i) { double v = 0; if (i < argc) napi_get_value_double(env, argv[i], &v); return v; }
    int32_t i32(size_t i) { return (int32_t)num(i); }
    // typed array of the expected element type; returns nullptr (and throws) on mismatch
    void* ta(size_t i, napi_typedarray_type want, size_t* len) {
        bool is = false;
        if (i >= argc || napi_is_typedarray(env, argv[i], &is) != napi_ok || !is) { napi_throw_type_error(env, nullptr, "expected a typed array"); ok = false; return nullptr; }
        napi_typedarray_type t; size_t n; void* data; napi_value ab; size_t off;
        napi_get_typedarray_info(env, argv[i], &t, &n, &data, &ab, &off);
        if (t != want) { napi_throw_type_error(env, nullptr, "typed array has the wrong element type"); ok = false; return nullptr; }
        if (len) *len = n;
        return data;
    }
    void* ext(size_t i) { void* p = nullptr; if (i < argc) napi_get_value_external(env, argv[i], &p); return p; }
};

napi_value make_ta(napi_env env, napi_typedarray_type t, size_t n, size_t elem, void** data) {
    napi_value ab, ta;
    if (napi_create_arraybuffer(env, n * elem, data, &ab) != napi_ok) return nullptr;
    if (napi_create_typedarray(env, t, n, ab, 0, &ta) != napi_ok) return nullptr;
    return ta;
}

void set_prop(napi_env env, napi_value obj, const char* k, napi_value v) { napi_set_named_property(env, obj, k, v); }

// ---- host-side producers -------------------------------------------------------------------------
napi_value FibSpherePoints(napi_env env, napi_callback_info info) {            // (N, jitter, seed) -> Float32Array(3*(N+1))
    Args a(env, info);
    const int32_t N = a.i32(0);
    void* d; napi_value out = make_ta(env, napi_float32_array, 3 * (size_t)(N + 1), 4, &d);
    if (!out) return nullptr;
    if (wo_fib_sphere_points(N, a.num(1), a.num(2), (float*)d)) return throw_wo(env, "fibSpherePoints");
    return out;
}

napi_value SphereDelaunay(napi_env env, napi_callback_info info) {             // (xyz) -> {triangles, halfedges}
    Args a(env, info);
    size_t n; float* xyz = (float*)a.ta(0, napi_float32_array, &n); if (!a.ok) return nullptr;
    const int32_t V = (int32_t)(n / 3);
    const size_t ns = 3 * (size_t)(2 * V - 4);
    void *t, *h; napi_value ta = make_ta(env, napi_int32_array, ns, 4, &t), ha = make_ta(env, napi_int32_array, ns, 4, &h);
    if (wo_sphere_delaunay(V, xyz, (int32_t*)t, (int32_t*)h)) return throw_wo(env, "sphereDelaunay");
    napi_value o; napi_create_object(env, &o); set_prop(env, o, "triangles", ta); set_prop(env, o, "halfedges", ha);
    return o;
}

napi_value SphereReferenceClosure(napi_env env, napi_callback_info info) {     // (numRegions, triangles, halfedges): in place
    Args a(env, info);
    size_t ns, nh; int32_t* tri = (int32_t*)a.ta(1, napi_int32_array, &ns); if (!a.ok) return nullptr;
    int32_t* he = (int32_t*)a.ta(2, napi_int32_array, &nh); if (!a.ok) return nullptr;
    const int32_t V = a.i32(0);
    if (V < 4 || ns != nh || ns != 3 * (size_t)(2 * (int64_t)V - 4)) { napi_throw_range_error(env, nullptr, "sphereReferenceClosure: triangles and halfedges must have 3*(2*numRegions-4) entries"); return nullptr; }
    if (wo_sphere_reference_closure(V, tri, he)) return throw_wo(env, "sphereReferenceClosure");
    return nullptr;
}

napi_value MeshCsr(napi_env env, napi_callback_info info) {                    // (numRegions, triangles, halfedges)
    Args a(env, info);
    const int32_t V = a.i32(0);
    size_t ns, nh; int32_t* tri = (int32_t*)a.ta(1, napi_int32_array, &ns); int32_t* he = (int32_t*)a.ta(2, napi_int32_array, &nh);
    if (!a.ok) return nullptr;
    if (ns != nh || V < 0) { napi_throw_range_error(env, nullptr, "meshCsr: triangles and halfedges must have the same length"); return nullptr; }
    void *o1, *o2, *o3;
    napi_value off = make_ta(env, napi_int32_array, (size_t)V + 1, 4, &o1);
    std::vector<int32_t> adj(ns), adjt(ns);
    if (wo_mesh_csr(V, (int32_t)ns, tri, he, (int32_t*)o1, adj.data(), adjt.data())) return throw_wo(env, "meshCsr");
    const size_t E = (size_t)((int32_t*)o1)[V];
    napi_value al = make_ta(env, napi_int32_array, E, 4, &o2), at = make_ta(env, napi_int32_array, E, 4, &o3);
    std::memcpy(o2, adj.data(), E * 4); std::memcpy(o3, adjt.data(), E * 4);
    napi_value o; napi_create_object(env, &o);
    set_prop(env, o, "adjOffset", off); set_prop(env, o, "adjList", al); set_prop(env, o, "adjTriList", at);
    return o;
}

napi_value NeighborDist(napi_env env, napi_callback_info info) {               // (adjOffset, adjList, xyz)
    Args a(env, info);
    size_t no, na, nx; int32_t* off = (int32_t*)a.ta(0, napi_int32_array, &no); int32_t* adj = (int32_t*)a.ta(1, napi_int32_array, &na);
    float* xyz = (float*)a.ta(2, napi_float32_array, &nx); if (!a.ok) return nullptr;
    void* d; napi_value out = make_ta(env, napi_float32_array, na, 4, &d);
    if (wo_neighbor_dist((int32_t)no - 1, off, adj, xyz, (float*)d)) return throw_wo(env, "neighborDist");
    return out;
}

napi_value TriangleElevations(napi_env env, napi_callback_info info) {         // (triangles, r_elevation)
    Args a(env, info);
    size_t ns, ne; int32_t* tri = (int32_t*)a.ta(0, napi_int32_array, &ns); float* e = (float*)a.ta(1, napi_float32_array, &ne);
    if (!a.ok) return nullptr;
    void* d; napi_value out = make_ta(env, napi_float32_array, ns / 3, 4, &d);
    if (wo_triangle_elevations((int32_t)(ns / 3), tri, e, (float*)d)) return throw_wo(env, "triangleElevations");
    return out;
}

napi_value NoiseTables(napi_env env, napi_callback_info info) {                // (seed) -> {perm, pm12}
    Args a(env, info);
    void *p, *m; napi_value pa = make_ta(env, napi_uint8_array, 512, 1, &p), ma = make_ta(env, napi_uint8_array, 512, 1, &m);
    if (wo_noise_tables(a.num(0), (uint8_t*)p, (uint8_t*)m)) return throw_wo(env, "noiseTables");
    napi_value o; napi_create_object(env, &o); set_prop(env, o, "perm", pa); set_prop(env, o, "pm12", ma);
    return o;
}

// ---- handles ---------------------------------------------------------------------------------------
void FinalizeCtx(napi_env, void* data, void*) { wo_ctx_destroy((wo_ctx*)data); }
// wo_planet_destroy uses the planet's context (device, stream), and the order in which the garbage collector finalizes
// two externals is unspecified: the planet holds a strong reference to its context value and drops it only after the
// planet itself is gone.
// The external's data is a box, so that planetDestroy() can free the device memory NOW (a planet at 40 M cells holds several GB,
// and the external's tiny JS footprint gives the collector no reason to run) and leave a dead handle behind: the finalizer then
// only frees the box, and every entry point sees a null planet ("expected a live planet handle").
struct PlanetBox { wo_planet* p; };
void FinalizePlanet(napi_env env, void* data, void* hint) {
    PlanetBox* b = (PlanetBox*)data;
    if (b) { if (b->p) wo_planet_destroy(b->p); delete b; }
    if (hint) napi_delete_reference(env, (napi_ref)hint);
}
static wo_planet* planet_at(Args& a, size_t i) { PlanetBox* b = (PlanetBox*)a.ext(i); return b ? b->p : nullptr; }

napi_value DeviceCount(napi_env env, napi_callback_info) { napi_value v; napi_create_int32(env, wo_device_count(), &v); return v; }

napi_value CtxCreate(napi_env env, napi_callback_info info) {
    Args a(env, info);
    wo_ctx* c = wo_ctx_create(a.i32(0));
    if (!c) return throw_wo(env, "ctxCreate");
    napi_value v; NAPI_OK(napi_create_external(env, c, FinalizeCtx, nullptr, &v));
    return v;
}

napi_value SphereMeshDevice(napi_env env, napi_callback_info info) {           // (ctx, xyz, referenceClosure) -> {triangles, halfedges, adjOffset, adjList, adjTriList, neighborDist}
    Args a(env, info);
    wo_ctx* c = (wo_ctx*)a.ext(0);
    size_t n; float* xyz = (float*)a.ta(1, napi_float32_array, &n); if (!a.ok) return nullptr;
    if (!c) { napi_throw_type_error(env, nullptr, "sphereMeshDevice: expected a context handle"); return nullptr; }
    if (n % 3 != 0 || n < 12) { napi_throw_range_error(env, nullptr, "sphereMeshDevice: xyz must hold three floats for each of at least 4 points"); return nullptr; }
    const int32_t V = (int32_t)(n / 3);
    const size_t ns = 3 * (size_t)(2 * V - 4);
    void *t, *h, *o1, *o2, *o3, *o4;
    napi_value ta = make_ta(env, napi_int32_array, ns, 4, &t), ha = make_ta(env, napi_int32_array, ns, 4, &h);
    napi_value off = make_ta(env, napi_int32_array, (size_t)V + 1, 4, &o1);
    // the library writes the first adjOffset[V] entries of these three; on a closed triangulation that is all of them
    napi_value alBuf, atBuf, distBuf;
    if (!ta || !ha || !off || napi_create_arraybuffer(env, ns * 4, &o2, &alBuf) != napi_ok || napi_create_arraybuffer(env, ns * 4, &o3, &atBuf) != napi_ok ||
        napi_create_arraybuffer(env, ns * 4, &o4, &distBuf) != napi_ok) return nullptr;
    if (wo_sphere_mesh_device(c, V, xyz, a.has(2) && a.num(2) != 0 ? 1 : 0, (int32_t*)t, (int32_t*)h, (int32_t*)o1, (int32_t*)o2, (int32_t*)o3, (float*)o4))
        return throw_wo(env, "sphereMeshDevice");
    const size_t E = (size_t)((int32_t*)o1)[V];
    napi_value al, at, dist;
    NAPI_OK(napi_create_typedarray(env, napi_int32_array, E, alBuf, 0, &al));
    NAPI_OK(napi_create_typedarray(env, napi_int32_array, E, atBuf, 0, &at));
    NAPI_OK(napi_create_typedarray(env, napi_float32_array, E, distBuf, 0, &dist));
    napi_value o; napi_create_object(env, &o);
    set_prop(env, o, "triangles", ta); set_prop(env, o, "halfedges", ha); set_prop(env, o, "adjOffset", off); set_prop(env, o, "adjList", al);
    set_prop(env, o, "adjTriList", at); set_prop(env, o, "neighborDist", dist);
    return o;
}

napi_value FibSpherePointsDevice(napi_env env, napi_callback_info info) {       // (ctx, N, jitter, seed) -> Float32Array(3*(N+1))
    Args a(env, info);
    wo_ctx* c = (wo_ctx*)a.ext(0);
    const int32_t N = a.i32(1);
    if (!c) { napi_throw_type_error(env, nullptr, "fibSpherePointsDevice: expected a context handle"); return nullptr; }
    if (N < 1) { napi_throw_range_error(env, nullptr, "fibSpherePointsDevice: N must be at least 1"); return nullptr; }
    void* d; napi_value out = make_ta(env, napi_float32_array, 3 * ((size_t)N + 1), 4, &d);
    if (!out) return nullptr;
    if (wo_fib_sphere_points_device(c, N, a.num(2), a.num(3), (float*)d)) return throw_wo(env, "fibSpherePointsDevice");
    return out;
}

napi_value SphereMeshSeedDevice(napi_env env, napi_callback_info info) {       // (ctx, N, jitter, seed, referenceClosure) -> {r_xyz, triangles, halfedges, adjOffset, adjList, adjTriList, neighborDist}
    Args a(env, info);
    wo_ctx* c = (wo_ctx*)a.ext(0);
    const int32_t N = a.i32(1);
    if (!c) { napi_throw_type_error(env, nullptr, "sphereMeshSeedDevice: expected a context handle"); return nullptr; }
    if (N < 3) { napi_throw_range_error(env, nullptr, "sphereMeshSeedDevice: N + 1 must be at least 4 points"); return nullptr; }
    const int32_t V = N + 1;
    const size_t ns = 3 * (size_t)(2 * V - 4);
    void *x, *t, *h, *o1, *o2, *o3, *o4;
    napi_value xa = make_ta(env, napi_float32_array, 3 * (size_t)V, 4, &x);
    napi_value ta = make_ta(env, napi_int32_array, ns, 4, &t), ha = make_ta(env, napi_int32_array, ns, 4, &h);
    napi_value off = make_ta(env, napi_int32_array, (size_t)V + 1, 4, &o1);
    napi_value alBuf, atBuf, distBuf;
    if (!xa || !ta || !ha || !off || napi_create_arraybuffer(env, ns * 4, &o2, &alBuf) != napi_ok || napi_create_arraybuffer(env, ns * 4, &o3, &atBuf) != napi_ok ||
        napi_create_arraybuffer(env, ns * 4, &o4, &distBuf) != napi_ok) return nullptr;
    if (wo_sphere_mesh_seed_device(c, N, a.num(2), a.num(3), a.has(4) && a.num(4) != 0 ? 1 : 0, (float*)x, (int32_t*)t, (int32_t*)h, (int32_t*)o1, (int32_t*)o2,
                                   (int32_t*)o3, (float*)o4))
        return throw_wo(env, "sphereMeshSeedDevice");
    const size_t E = (size_t)((int32_t*)o1)[V];
    napi_value al, at, dist;
    NAPI_OK(napi_create_typedarray(env, napi_int32_array, E, alBuf, 0, &al));
    NAPI_OK(napi_create_typedarray(env, napi_int32_array, E, atBuf, 0, &at));
    NAPI_OK(napi_create_typedarray(env, napi_float32_array, E, distBuf, 0, &dist));
    napi_value o; napi_create_object(env, &o);
    set_prop(env, o, "r_xyz", xa); set_prop(env, o, "triangles", ta); set_prop(env, o, "halfedges", ha); set_prop(env, o, "adjOffset", off);
    set_prop(env, o, "adjList", al); set_prop(env, o, "adjTriList", at); set_prop(env, o, "neighborDist", dist);
    return o;
}

napi_value PlanetCreate(napi_env env, napi_callback_info info) {               // (ctx, numRegions, adjOffset, adjList, xyz, neighborDist|null)
    Args a(env, info);
    wo_ctx* c = (wo_ctx*)a.ext(0);
    const int32_t V = a.i32(1);
    size_t no, na, nx, nd = 0;
    int32_t* off = (int32_t*)a.ta(2, napi_int32_array, &no); int32_t* adj = (int32_t*)a.ta(3, napi_int32_array, &na);
    float* xyz = (float*)a.ta(4, napi_float32_array, &nx); if (!a.ok) return nullptr;
    float* dist = a.has(5) ? (float*)a.ta(5, napi_float32_array, &nd) : nullptr; if (!a.ok) return nullptr;
    if (no != (size_t)V + 1 || nx != 3 * (size_t)V || (dist && nd != na)) { napi_throw_range_error(env, nullptr, "planetCreate: array sizes do not match numRegions"); return nullptr; }
    if (!c) { napi_throw_type_error(env, nullptr, "planetCreate: expected a context handle"); return nullptr; }
    wo_planet* p = wo_planet_create(c, V, off, adj, xyz, dist);
    if (!p) return throw_wo(env, "planetCreate");
    napi_ref ctxRef = nullptr;
    if (napi_create_reference(env, a.argv[0], 1, &ctxRef) != napi_ok) { wo_planet_destroy(p); napi_throw_error(env, nullptr, "planetCreate: cannot reference the context"); return nullptr; }
    napi_value v;
    PlanetBox* box = new PlanetBox{p};
    if (napi_create_external(env, box, FinalizePlanet, ctxRef, &v) != napi_ok) { wo_planet_destroy(p); delete box; napi_delete_reference(env, ctxRef); napi_throw_error(env, nullptr, "planetCreate: cannot wrap the planet"); return nullptr; }
    return v;
}
napi_value PlanetDestroy(napi_env env, napi_callback_info info) {               // (planet): frees the device memory now; the handle stays, dead
    Args a(env, info);
    PlanetBox* b = (PlanetBox*)a.ext(0);
    if (b && b->p) { wo_planet_destroy(b->p); b->p = nullptr; }
    napi_value u; napi_get_undefined(env, &u); return u;
}

// A planet argument must be a live handle, and every per-region array handed over with it must have exactly
// mesh.numRegions entries: the C ABI copies numRegions elements in and out of the pointer it is given (the reference
// would merely index `undefined`; here a short array would be an out-of-bounds read and write in the V8 heap).
bool planet_ok(napi_env env, wo_planet* p) {
    if (p) return true;
    napi_throw_type_error(env, nullptr, "expected a planet handle");
    return false;
}
bool regions_ok(napi_env env, wo_planet* p, size_t len, const char* what) {
    if ((int64_t)len == (int64_t)wo_planet_num_regions(p)) return true;
    std::string msg = std::string(what) + " length must equal mesh.numRegions";
    napi_throw_range_error(env, nullptr, msg.c_str());
    return false;
}

// ---- terrain-post, JS call surface (arrays mutated in place, return undefined) --------------------------
#define PLANET_AND_ELEV()                                                                        \
    Args a(env, info); wo_planet* p = planet_at(a, 0);                                      \
    if (!planet_ok(env, p)) return nullptr;                                                      \
    size_t ne; float* e = (float*)a.ta(1, napi_float32_array, &ne); if (!a.ok) return nullptr;   \
    if (!regions_ok(env, p, ne, "r_elevation")) return nullptr;

napi_value WarpTerrain(napi_env env, napi_callback_info info) {                // (planet, elev, seed, strength, hotspot|null)
    PLANET_AND_ELEV();
    size_t nh = 0; float* hot = a.has(4) ? (float*)a.ta(4, napi_float32_array, &nh) : nullptr; if (!a.ok) return nullptr;
    if (hot && !regions_ok(env, p, nh, "r_hotspot")) return nullptr;
    if (wo_warp_terrain(p, e, a.num(2), a.num(3), hot)) return throw_wo(env, "warpTerrain");
    return nullptr;
}
napi_value SmoothElevation(napi_env env, napi_callback_info info) {            // (planet, elev, isOcean, iterations, strength)
    PLANET_AND_ELEV();
    size_t no; uint8_t* oc = (uint8_t*)a.ta(2, napi_uint8_array, &no); if (!a.ok) return nullptr;
    if (no != ne) { napi_throw_range_error(env, nullptr, "r_isOcean length mismatch"); return nullptr; }
    if (wo_smooth_elevation(p, e, oc, a.i32(3), a.num(4))) return throw_wo(env, "smoothElevation");
    return nullptr;
}
napi_value SharpenRidges(napi_env env, napi_callback_info info) {
    PLANET_AND_ELEV();
    size_t no; uint8_t* oc = (uint8_t*)a.ta(2, napi_uint8_array, &no); if (!a.ok) return nullptr;
    if (no != ne) { napi_throw_range_error(env, nullptr, "r_isOcean length mismatch"); return nullptr; }
    if (wo_sharpen_ridges(p, e, oc, a.i32(3), a.num(4))) return throw_wo(env, "sharpenRidges");
    return nullptr;
}
napi_value ApplySoilCreep(napi_env env, napi_callback_info info) {
    PLANET_AND_ELEV();
    size_t no; uint8_t* oc = (uint8_t*)a.ta(2, napi_uint8_array, &no); if (!a.ok) return nullptr;
    if (no != ne) { napi_throw_range_error(env, nullptr, "r_isOcean length mismatch"); return nullptr; }
    if (wo_soil_creep(p, e, oc, a.i32(3), a.num(4))) return throw_wo(env, "applySoilCreep");
    return nullptr;
}
napi_value ErodeComposite(napi_env env, napi_callback_info info) {             // (planet, elev, isOcean, h,K,m,dt, t,talus,kT, g,gs)
    PLANET_AND_ELEV();
    size_t no; uint8_t* oc = (uint8_t*)a.ta(2, napi_uint8_array, &no); if (!a.ok) return nullptr;
    if (no != ne) { napi_throw_range_error(env, nullptr, "r_isOcean length mismatch"); return nullptr; }
    if (wo_erode_composite(p, e, oc, a.i32(3), a.num(4), a.num(5), a.num(6), a.i32(7), a.num(8), a.num(9), a.i32(10), a.num(11)))
        return throw_wo(env, "erodeComposite");
    return nullptr;
}

// ---- resident variants ("reapply": the field stays in HBM) ---------------------------------------------
napi_value PlanetUpload(napi_env env, napi_callback_info info) {               // (planet, elev|null, isOcean|null)
    Args a(env, info); wo_planet* p = planet_at(a, 0);
    if (!planet_ok(env, p)) return nullptr;
    size_t n1 = 0, n2 = 0;
    float* e = a.has(1) ? (float*)a.ta(1, napi_float32_array, &n1) : nullptr; if (!a.ok) return nullptr;
    uint8_t* oc = a.has(2) ? (uint8_t*)a.ta(2, napi_uint8_array, &n2) : nullptr; if (!a.ok) return nullptr;
    if ((e && !regions_ok(env, p, n1, "r_elevation")) || (oc && !regions_ok(env, p, n2, "r_isOcean"))) return nullptr;
    if (wo_planet_upload(p, e, oc)) return throw_wo(env, "planetUpload");
    return nullptr;
}
napi_value PlanetDownload(napi_env env, napi_callback_info info) {             // (planet, elevOut)
    PLANET_AND_ELEV();
    if (wo_planet_download(p, e)) return throw_wo(env, "planetDownload");
    return nullptr;
}
napi_value PlanetDownloadOcean(napi_env env, napi_callback_info info) {        // (planet, isOceanOut)
    Args a(env, info); wo_planet* p = planet_at(a, 0);
    if (!planet_ok(env, p)) return nullptr;
    size_t n; uint8_t* oc = (uint8_t*)a.ta(1, napi_uint8_array, &n); if (!a.ok) return nullptr;
    if (!regions_ok(env, p, n, "r_isOcean")) return nullptr;
    if (wo_planet_download_ocean(p, oc)) return throw_wo(env, "planetDownloadOcean");
    return nullptr;
}
napi_value PlanetUploadHotspot(napi_env env, napi_callback_info info) {
    PLANET_AND_ELEV();
    if (wo_planet_upload_hotspot(p, e)) return throw_wo(env, "planetUploadHotspot");
    return nullptr;
}
#define SIMPLE_PLANET_CALL(NAME, EXPR)                                                     \
    napi_value NAME(napi_env env, napi_callback_info info) {                               \
        Args a(env, info); wo_planet* p = planet_at(a, 0);                            \
        if (!planet_ok(env, p)) return nullptr;                                            \
        if (EXPR) return throw_wo(env, #NAME);                                             \
        return nullptr;                                                                    \
    }
SIMPLE_PLANET_CALL(PlanetOceanFromElevation, wo_planet_ocean_from_elevation(p))
SIMPLE_PLANET_CALL(PlanetSync, wo_planet_sync(p))
SIMPLE_PLANET_CALL(PlanetSaveState, wo_planet_save_state(p))
SIMPLE_PLANET_CALL(PlanetRestoreState, wo_planet_restore_state(p))
SIMPLE_PLANET_CALL(PlanetSyntheticTerrain, wo_planet_synthetic_terrain(p, a.num(1)))
SIMPLE_PLANET_CALL(WarpTerrainResident, wo_warp_terrain_resident(p, a.num(1), a.num(2), a.i32(3)))
SIMPLE_PLANET_CALL(SmoothElevationResident, wo_smooth_elevation_resident(p, a.i32(1), a.num(2)))
SIMPLE_PLANET_CALL(SharpenRidgesResident, wo_sharpen_ridges_resident(p, a.i32(1), a.num(2)))
SIMPLE_PLANET_CALL(ApplySoilCreepResident, wo_soil_creep_resident(p, a.i32(1), a.num(2)))
SIMPLE_PLANET_CALL(ErodeCompositeResident, wo_erode_composite_resident(p, a.i32(1), a.num(2), a.num(3), a.num(4), a.i32(5), a.num(6), a.num(7), a.i32(8), a.num(9)))
SIMPLE_PLANET_CALL(TimerStart, wo_timer_start(p))

napi_value TimerStopMs(napi_env env, napi_callback_info info) {
    Args a(env, info); wo_planet* p = planet_at(a, 0);
    if (!planet_ok(env, p)) return nullptr;
    double ms = 0;
    if (wo_timer_stop_ms(p, &ms)) return throw_wo(env, "timerStopMs");
    napi_value v; napi_create_double(env, ms, &v); return v;
}

// [{stage, ms}] of the last erodeComposite — same shape as the reference's _postTiming entries
napi_value LastStageTiming(napi_env env, napi_callback_info info) {
    Args a(env, info); wo_planet* p = planet_at(a, 0);
    if (!planet_ok(env, p)) return nullptr;
    const char* names[64]; double ms[64]; int32_t n = 0;
    if (wo_last_stage_timing(p, 64, names, ms, &n)) return throw_wo(env, "lastStageTiming");
    napi_value arr; napi_create_array_with_length(env, n, &arr);
    for (int32_t i = 0; i < n; ++i) {
        napi_value o, s, v; napi_create_object(env, &o);
        napi_create_string_utf8(env, names[i], NAPI_AUTO_LENGTH, &s); napi_create_double(env, ms[i], &v);
        set_prop(env, o, "stage", s); set_prop(env, o, "ms", v);
        napi_set_element(env, arr, i, o);
    }
    return arr;
}

// lastErodeStats(planet) -> {name: number}: counters of the last erodeComposite (rounds, launches, the host flood's route)
napi_value LastErodeStats(napi_env env, napi_callback_info info) {
    Args a(env, info); wo_planet* p = planet_at(a, 0);
    if (!planet_ok(env, p)) return nullptr;
    const char* names[64]; double vals[64]; int32_t n = 0;
    if (wo_last_erode_stats(p, 64, names, vals, &n)) return throw_wo(env, "lastErodeStats");
    napi_value o; napi_create_object(env, &o);
    for (int32_t i = 0; i < n; ++i) { napi_value v; napi_create_double(env, vals[i], &v); napi_set_named_property(env, o, names[i], v); }
    return o;
}

// noisePoint(perm, pm12, kind, octaves, p0, p1, p2, x, y, z) -> number (host)
napi_value NoisePoint(napi_env env, napi_callback_info info) {
    Args a(env, info);
    size_t np_, nm;
    uint8_t* P = (uint8_t*)a.ta(0, napi_uint8_array, &np_); if (!a.ok) return nullptr;
    uint8_t* M = (uint8_t*)a.ta(1, napi_uint8_array, &nm); if (!a.ok) return nullptr;
    if (np_ != 512 || nm != 512) { napi_throw_range_error(env, nullptr, "noise tables must have 512 entries"); return nullptr; }
    double out = 0;
    if (wo_noise_point(P, M, a.i32(2), a.i32(3), a.num(4), a.num(5), a.num(6), a.num(7), a.num(8), a.num(9), &out)) return throw_wo(env, "noisePoint");
    napi_value v; napi_create_double(env, out, &v); return v;
}
napi_value NoiseEval(napi_env env, napi_callback_info info) {                  // (ctx, seed, kind, octaves, p0, p1, p2, xyz Float64Array) -> Float64Array
    Args a(env, info); wo_ctx* c = (wo_ctx*)a.ext(0);
    size_t n; double* xyz = (double*)a.ta(7, napi_float64_array, &n); if (!a.ok) return nullptr;
    void* d; napi_value out = make_ta(env, napi_float64_array, n / 3, 8, &d);
    if (wo_noise_eval(c, a.num(1), a.i32(2), a.i32(3), a.num(4), a.num(5), a.num(6), (int64_t)(n / 3), xyz, (double*)d)) return throw_wo(env, "noiseEval");
    return out;
}

// assignElevation(planet, r_plate, plates, plateSeeds, r_superPlate|null, superPlates|null, perm, pm12, noiseMag, seed, spread, wantDebug)
// plates = { numIds, hasVec:Uint8Array, pole:Float64Array, omega:Float64Array, isOcean:Uint8Array, density:Float64Array }
bool read_table(Args& a, napi_value obj, wo_plate_table* t) {
    napi_env env = a.env;
    auto get = [&](const char* k) { napi_value v; napi_get_named_property(env, obj, k, &v); return v; };
    double n = 0; napi_get_value_double(env, get("numIds"), &n);
    t->numIds = (int32_t)n;
    auto arr = [&](const char* k, napi_typedarray_type want, size_t need) -> void* {
        napi_value v = get(k); bool is = false; napi_is_typedarray(env, v, &is);
        if (!is) { napi_throw_type_error(env, nullptr, "plate table: expected typed arrays"); a.ok = false; return nullptr; }
        napi_typedarray_type ty; size_t len; void* data; napi_value ab; size_t off;
        napi_get_typedarray_info(env, v, &ty, &len, &data, &ab, &off);
        if (ty != want || len != need) { napi_throw_range_error(env, nullptr, "plate table: wrong array type or length"); a.ok = false; return nullptr; }
        return data;
    };
    const size_t m = (size_t)t->numIds;
    t->hasVec = (const uint8_t*)arr("hasVec", napi_uint8_array, m); if (!a.ok) return false;
    t->pole = (const double*)arr("pole", napi_float64_array, 3 * m); if (!a.ok) return false;
    t->omega = (const double*)arr("omega", napi_float64_array, m); if (!a.ok) return false;
    t->isOcean = (const uint8_t*)arr("isOcean", napi_uint8_array, m); if (!a.ok) return false;
    t->density = (const double*)arr("density", napi_float64_array, m); if (!a.ok) return false;
    return true;
}

napi_value AssignElevation(napi_env env, napi_callback_info info) {
    Args a(env, info); wo_planet* p = planet_at(a, 0);
    if (!planet_ok(env, p)) return nullptr;
    size_t n, ns, nsup = 0, np_, nm;
    int32_t* r_plate = (int32_t*)a.ta(1, napi_int32_array, &n); if (!a.ok) return nullptr;
    if (!regions_ok(env, p, n, "r_plate")) return nullptr;
    wo_plate_table T{}, TS{};
    if (!read_table(a, a.argv[2], &T)) return nullptr;
    int32_t* seeds = (int32_t*)a.ta(3, napi_int32_array, &ns); if (!a.ok) return nullptr;
    int32_t* r_super = a.has(4) ? (int32_t*)a.ta(4, napi_int32_array, &nsup) : nullptr; if (!a.ok) return nullptr;
    const bool hasSuper = r_super != nullptr && a.has(5);
    if (hasSuper && !read_table(a, a.argv[5], &TS)) return nullptr;
    if (hasSuper && nsup != n) { napi_throw_range_error(env, nullptr, "r_superPlate length mismatch"); return nullptr; }
    uint8_t* perm = (uint8_t*)a.ta(6, napi_uint8_array, &np_); uint8_t* pm12 = (uint8_t*)a.ta(7, napi_uint8_array, &nm); if (!a.ok) return nullptr;
    if (np_ != 512 || nm != 512) { napi_throw_range_error(env, nullptr, "noise tables must have 512 entries"); return nullptr; }
    bool wantDebug = true; if (a.argc > 11) napi_get_value_bool(env, a.argv[11], &wantDebug);
    void *e, *st, *dl = nullptr;
    napi_value ea = make_ta(env, napi_float32_array, n, 4, &e), sa = make_ta(env, napi_float32_array, n, 4, &st), da = nullptr;
    if (wantDebug) da = make_ta(env, napi_float32_array, 12 * n, 4, &dl);
    std::vector<int32_t> mo(n), co(n), oc(n); int32_t cnt[3] = {0, 0, 0};
    if (wo_assign_elevation(p, r_plate, &T, seeds, (int32_t)ns, hasSuper ? r_super : nullptr, hasSuper ? &TS : nullptr, perm, pm12,
                            a.num(8), a.num(9), a.num(10), (float*)e, (float*)st, (float*)dl, mo.data(), co.data(), oc.data(), cnt))
        return throw_wo(env, "assignElevation");
    napi_value o; napi_create_object(env, &o);
    set_prop(env, o, "r_elevation", ea); set_prop(env, o, "r_stress", sa);
    if (da) set_prop(env, o, "debugLayers", da);
    const char* names[3] = {"mountain", "coastline", "ocean"}; std::vector<int32_t>* v[3] = {&mo, &co, &oc};
    for (int k = 0; k < 3; ++k) { void* d; napi_value t = make_ta(env, napi_int32_array, (size_t)cnt[k], 4, &d); std::memcpy(d, v[k]->data(), (size_t)cnt[k] * 4); set_prop(env, o, names[k], t); }
    return o;
}

// buildSuperPlates(planet, r_plate, plates, plateSeeds) -> { r_superPlate:Int32Array, numSuperPlates, pole:Float64Array(3 n), omega:Float64Array(n),
//                                                            isOcean:Uint8Array(n), density:Float64Array(n) }   (plates as for assignElevation)
napi_value BuildSuperPlates(napi_env env, napi_callback_info info) {
    Args a(env, info); wo_planet* p = planet_at(a, 0);
    if (!planet_ok(env, p)) return nullptr;
    size_t n, ns;
    int32_t* r_plate = (int32_t*)a.ta(1, napi_int32_array, &n); if (!a.ok) return nullptr;
    if (!regions_ok(env, p, n, "r_plate")) return nullptr;
    wo_plate_table T{};
    if (!read_table(a, a.argv[2], &T)) return nullptr;
    int32_t* seeds = (int32_t*)a.ta(3, napi_int32_array, &ns); if (!a.ok) return nullptr;
    void* rs; napi_value ra = make_ta(env, napi_int32_array, n, 4, &rs);
    if (!ra) return nullptr;
    const size_t room = ns > 0 ? ns : 1;
    std::vector<double> pole(3 * room), omega(room), density(room); std::vector<uint8_t> isOcean(room);
    int32_t numSuper = 0;
    if (wo_build_super_plates(p, r_plate, &T, seeds, (int32_t)ns, (int32_t*)rs, &numSuper, pole.data(), omega.data(), isOcean.data(), density.data()))
        return throw_wo(env, "buildSuperPlates");
    const size_t m = (size_t)numSuper;
    void *dp, *dw, *dn, *di;
    napi_value pa = make_ta(env, napi_float64_array, 3 * m, 8, &dp), wa = make_ta(env, napi_float64_array, m, 8, &dw);
    napi_value na = make_ta(env, napi_float64_array, m, 8, &dn), ia = make_ta(env, napi_uint8_array, m, 1, &di);
    if (!pa || !wa || !na || !ia) return nullptr;
    std::memcpy(dp, pole.data(), 3 * m * 8); std::memcpy(dw, omega.data(), m * 8); std::memcpy(dn, density.data(), m * 8); std::memcpy(di, isOcean.data(), m);
    napi_value o, cnt; napi_create_object(env, &o); napi_create_int32(env, numSuper, &cnt);
    set_prop(env, o, "r_superPlate", ra); set_prop(env, o, "numSuperPlates", cnt);
    set_prop(env, o, "pole", pa); set_prop(env, o, "omega", wa); set_prop(env, o, "isOcean", ia); set_prop(env, o, "density", na);
    return o;
}

// smoothField(planet, field Float32Array (in place), passes)
napi_value SmoothField(napi_env env, napi_callback_info info) {
    PLANET_AND_ELEV();
    if (wo_smooth_field(p, e, a.i32(2))) return throw_wo(env, "smoothField");
    return nullptr;
}
// optional Float32Array / Uint8Array / Int32Array of numRegions entries (null / undefined -> nullptr)
static void* opt_regions(Args& a, size_t i, napi_typedarray_type t, wo_planet* p, const char* what, bool required) {
    if (!a.has(i)) { if (required) { napi_throw_type_error(a.env, nullptr, what); a.ok = false; } return nullptr; }
    size_t n; void* d = a.ta(i, t, &n); if (!a.ok) return nullptr;
    if (!regions_ok(a.env, p, n, what)) { a.ok = false; return nullptr; }
    return d;
}
// diffuseOceanWarmth(planet, r_oceanWarmth|null, r_isLand, r_plateContinentality|null, passes) -> Float32Array
napi_value DiffuseOceanWarmth(napi_env env, napi_callback_info info) {
    Args a(env, info); wo_planet* p = planet_at(a, 0);
    if (!planet_ok(env, p)) return nullptr;
    float* w = (float*)opt_regions(a, 1, napi_float32_array, p, "r_oceanWarmth", false); if (!a.ok) return nullptr;
    uint8_t* land = (uint8_t*)opt_regions(a, 2, napi_uint8_array, p, "r_isLand", true); if (!a.ok) return nullptr;
    float* c = (float*)opt_regions(a, 3, napi_float32_array, p, "r_plateContinentality", false); if (!a.ok) return nullptr;
    void* d; napi_value out = make_ta(env, napi_float32_array, (size_t)wo_planet_num_regions(p), 4, &d);
    if (wo_diffuse_ocean_warmth(p, w, land, c, a.i32(4), (float*)d)) return throw_wo(env, "diffuseOceanWarmth");
    return out;
}
// computeWindConvergence(planet, r_wind3dX, r_wind3dY, r_wind3dZ) -> Float32Array
napi_value WindConvergence(napi_env env, napi_callback_info info) {
    Args a(env, info); wo_planet* p = planet_at(a, 0);
    if (!planet_ok(env, p)) return nullptr;
    float* x = (float*)opt_regions(a, 1, napi_float32_array, p, "r_wind3dX", true); if (!a.ok) return nullptr;
    float* y = (float*)opt_regions(a, 2, napi_float32_array, p, "r_wind3dY", true); if (!a.ok) return nullptr;
    float* z = (float*)opt_regions(a, 3, napi_float32_array, p, "r_wind3dZ", true); if (!a.ok) return nullptr;
    void* d; napi_value out = make_ta(env, napi_float32_array, (size_t)wo_planet_num_regions(p), 4, &d);
    if (wo_wind_convergence(p, x, y, z, (float*)d)) return throw_wo(env, "computeWindConvergence");
    return out;
}
// advectMoisture(planet, r_heightKm, r_isLand, r_windE, r_windN, r_wind3dX, r_wind3dY, r_wind3dZ, r_oceanWarmth|null, r_coastDistLand, maxHops) -> Float32Array
napi_value AdvectMoisture(napi_env env, napi_callback_info info) {
    Args a(env, info); wo_planet* p = planet_at(a, 0);
    if (!planet_ok(env, p)) return nullptr;
    float* hk = (float*)opt_regions(a, 1, napi_float32_array, p, "r_heightKm", true); if (!a.ok) return nullptr;
    uint8_t* land = (uint8_t*)opt_regions(a, 2, napi_uint8_array, p, "r_isLand", true); if (!a.ok) return nullptr;
    float* we = (float*)opt_regions(a, 3, napi_float32_array, p, "r_windE", true); if (!a.ok) return nullptr;
    float* wn = (float*)opt_regions(a, 4, napi_float32_array, p, "r_windN", true); if (!a.ok) return nullptr;
    float* x = (float*)opt_regions(a, 5, napi_float32_array, p, "r_wind3dX", true); if (!a.ok) return nullptr;
    float* y = (float*)opt_regions(a, 6, napi_float32_array, p, "r_wind3dY", true); if (!a.ok) return nullptr;
    float* z = (float*)opt_regions(a, 7, napi_float32_array, p, "r_wind3dZ", true); if (!a.ok) return nullptr;
    float* w = (float*)opt_regions(a, 8, napi_float32_array, p, "r_oceanWarmth", false); if (!a.ok) return nullptr;
    int32_t* cd = (int32_t*)opt_regions(a, 9, napi_int32_array, p, "r_coastDistLand", true); if (!a.ok) return nullptr;
    void* d; napi_value out = make_ta(env, napi_float32_array, (size_t)wo_planet_num_regions(p), 4, &d);
    if (wo_advect_moisture(p, hk, land, we, wn, x, y, z, w, cd, a.i32(10), (float*)d)) return throw_wo(env, "advectMoisture");
    return out;
}
// computeWind(planet, r_elevation | null, r_plate, oceanPlates Int32Array, seed, axialTilt) -> the reference's result object
// (js/wind.js:649-683, without _windTiming); null elevation: the planet's resident field
napi_value ComputeWind(napi_env env, napi_callback_info info) {
    Args a(env, info); wo_planet* p = planet_at(a, 0);
    if (!planet_ok(env, p)) return nullptr;
    float* e = (float*)opt_regions(a, 1, napi_float32_array, p, "r_elevation", false); if (!a.ok) return nullptr;
    int32_t* plate = (int32_t*)opt_regions(a, 2, napi_int32_array, p, "computeWind: r_plate must be an Int32Array", true); if (!a.ok) return nullptr;
    size_t nOcean = 0; int32_t* ocean = (int32_t*)a.ta(3, napi_int32_array, &nOcean); if (!a.ok) return nullptr;
    const int32_t n = wo_planet_num_regions(p);
    if (wo_compute_wind(p, n, e, plate, nOcean ? ocean : nullptr, (int32_t)nOcean, a.num(4), a.num(5), nullptr)) return throw_wo(env, "computeWind");
    static const char* const f32[] = {"r_pressure_summer", "r_wind_east_summer", "r_wind_north_summer", "r_wind_speed_summer",
                                      "r_pressure_winter", "r_wind_east_winter", "r_wind_north_winter", "r_wind_speed_winter",
                                      "itczLons", "itczLatsSummer", "itczLatsWinter", "r_lat", "r_lon", "r_sinLat", "r_isLand",
                                      "r_continentality", "r_coastDistLand", "r_plateContinentality",
                                      "r_eastX", "r_eastY", "r_eastZ", "r_northX", "r_northY", "r_northZ"};
    napi_value o; napi_create_object(env, &o);
    for (const char* k : f32) {
        const bool itcz = k[0] == 'i', land = std::strcmp(k, "r_isLand") == 0, dist = std::strcmp(k, "r_coastDistLand") == 0;
        const size_t len = itcz ? 360 : (size_t)n, elem = land ? 1 : 4;
        void* d; napi_value v = make_ta(env, land ? napi_uint8_array : dist ? napi_int32_array : napi_float32_array, len, elem, &d);
        if (!v) return nullptr;
        if (wo_wind_download(p, k, d, (int64_t)(len * elem))) return throw_wo(env, "computeWind");
        set_prop(env, o, k, v);
    }
    return o;
}
// computeGradients(planet, r_pressure, r_eastX, r_eastY, r_eastZ, r_northX, r_northY, r_northZ, r_gradE, r_gradN): the last two are written
napi_value ComputeGradients(napi_env env, napi_callback_info info) {
    Args a(env, info); wo_planet* p = planet_at(a, 0);
    if (!planet_ok(env, p)) return nullptr;
    float* q[9];
    for (int i = 0; i < 9; ++i) { q[i] = (float*)opt_regions(a, (size_t)i + 1, napi_float32_array, p, "computeGradients: nine Float32Arrays of numRegions entries", true); if (!a.ok) return nullptr; }
    const size_t n = (size_t)wo_planet_num_regions(p);
    std::vector<float> east(3 * n), north(3 * n);
    for (int c = 0; c < 3; ++c) { std::memcpy(east.data() + c * n, q[1 + c], n * 4); std::memcpy(north.data() + c * n, q[4 + c], n * 4); }
    if (wo_compute_gradients(p, (int32_t)n, q[0], east.data(), north.data(), q[7], q[8])) return throw_wo(env, "computeGradients");
    return nullptr;
}
// windUpload(planet, key, typedArray): one field of the planet's wind block by its result key (the C ABI checks key and size)
static bool key_at(Args& a, size_t i, char (&key)[64]) {
    size_t n = 0;
    if (i < a.argc && napi_get_value_string_utf8(a.env, a.argv[i], key, sizeof(key), &n) == napi_ok) return true;
    napi_throw_type_error(a.env, nullptr, "expected a result key (string)");
    return false;
}
// <block>Download(planet, key) -> Float32Array: one field of the planet's ocean, precipitation or temperature block by the reference's result key
static napi_value block_download(napi_env env, napi_callback_info info, int (*fn)(wo_planet*, const char*, void*, int64_t), const char* name) {
    Args a(env, info); wo_planet* p = planet_at(a, 0);
    if (!planet_ok(env, p)) return nullptr;
    char key[64]; if (!key_at(a, 1, key)) return nullptr;
    const size_t n = (size_t)wo_planet_num_regions(p);
    void* d; napi_value out = make_ta(env, napi_float32_array, n, 4, &d);
    if (!out) return nullptr;
    if (fn(p, key, d, (int64_t)(n * 4))) return throw_wo(env, name);
    return out;
}
// <block>Upload(planet, key, Float32Array): one field of such a block by its result key (the C ABI checks key and size)
static napi_value block_upload(napi_env env, napi_callback_info info, int (*fn)(wo_planet*, const char*, const void*, int64_t), const char* name) {
    Args a(env, info); wo_planet* p = planet_at(a, 0);
    if (!planet_ok(env, p)) return nullptr;
    char key[64]; if (!key_at(a, 1, key)) return nullptr;
    size_t n = 0; float* data = (float*)a.ta(2, napi_float32_array, &n); if (!a.ok) return nullptr;
    if (fn(p, key, data, (int64_t)(n * 4))) return throw_wo(env, name);
    return nullptr;
}
// the scalars of a stage's call as number properties of o
struct Num { const char* k; double x; };
static void set_nums(napi_env env, napi_value o, std::initializer_list<Num> nums) {
    for (const Num& e : nums) { napi_value v; napi_create_double(env, e.x, &v); set_prop(env, o, e.k, v); }
}
napi_value WindUpload(napi_env env, napi_callback_info info) {
    Args a(env, info); wo_planet* p = planet_at(a, 0);
    if (!planet_ok(env, p)) return nullptr;
    char key[64]; if (!key_at(a, 1, key)) return nullptr;
    bool is = false;
    if (a.argc < 3 || napi_is_typedarray(env, a.argv[2], &is) != napi_ok || !is) { napi_throw_type_error(env, nullptr, "windUpload: expected a typed array"); return nullptr; }
    napi_typedarray_type t; size_t n; void* data; napi_value ab; size_t off;
    napi_get_typedarray_info(env, a.argv[2], &t, &n, &data, &ab, &off);
    const size_t elem = (t == napi_uint8_array || t == napi_int8_array || t == napi_uint8_clamped_array) ? 1 : (t == napi_float32_array || t == napi_int32_array || t == napi_uint32_array) ? 4 : 0;
    if (!elem) { napi_throw_type_error(env, nullptr, "windUpload: expected a Float32Array, Int32Array or Uint8Array"); return nullptr; }
    if (wo_wind_upload(p, key, data, (int64_t)(n * elem))) return throw_wo(env, "windUpload");
    return nullptr;
}
// computeOceanCurrents(planet) -> {circumpolarNH, circumpolarSH, coastThreshold, warmthRange, ...}: the stage on the planet's wind block;
// the results stay on the device (oceanDownload)
napi_value ComputeOceanCurrents(napi_env env, napi_callback_info info) {
    Args a(env, info); wo_planet* p = planet_at(a, 0);
    if (!planet_ok(env, p)) return nullptr;
    wo_ocean_info oi;
    if (wo_compute_ocean_currents(p, wo_planet_num_regions(p), &oi)) return throw_wo(env, "computeOceanCurrents");
    napi_value o, v; napi_create_object(env, &o);
    napi_get_boolean(env, oi.circumpolarNH != 0, &v); set_prop(env, o, "circumpolarNH", v);
    napi_get_boolean(env, oi.circumpolarSH != 0, &v); set_prop(env, o, "circumpolarSH", v);
    set_nums(env, o, {{"coastThreshold", (double)oi.coastThreshold}, {"warmthRange", (double)oi.warmthRange},
        {"currentSmoothPasses", (double)oi.currentSmoothPasses}, {"warmthSmoothPasses", (double)oi.warmthSmoothPasses}, {"oceanCellsSummer", (double)oi.oceanCells[0]},
        {"oceanCellsWinter", (double)oi.oceanCells[1]}, {"p95Summer", (double)oi.p95[0]}, {"p95Winter", (double)oi.p95[1]}});
    return o;
}
napi_value OceanDownload(napi_env env, napi_callback_info info) { return block_download(env, info, wo_ocean_download, "oceanDownload"); }
napi_value OceanUpload(napi_env env, napi_callback_info info) { return block_upload(env, info, wo_ocean_upload, "oceanUpload"); }
// computePrecipitation(planet, r_elevation | null, precipitationOffset, landCoverage) -> the scalars of the call: the stage on the planet's
// wind and ocean blocks; the results stay on the device (precipDownload)
napi_value ComputePrecipitation(napi_env env, napi_callback_info info) {
    Args a(env, info); wo_planet* p = planet_at(a, 0);
    if (!planet_ok(env, p)) return nullptr;
    float* e = (float*)opt_regions(a, 1, napi_float32_array, p, "r_elevation", false); if (!a.ok) return nullptr;
    wo_precip_info pi;
    if (wo_compute_precipitation(p, wo_planet_num_regions(p), e, a.num(2), a.num(3), &pi)) return throw_wo(env, "computePrecipitation");
    napi_value o; napi_create_object(env, &o);
    set_nums(env, o, {{"maxHops", (double)pi.maxHops}, {"elevSmoothPasses", (double)pi.elevSmoothPasses},
        {"convSmoothPasses", (double)pi.convSmoothPasses}, {"shadowHops", (double)pi.shadowHops}, {"windwardHops", (double)pi.windwardHops},
        {"rsSmoothPasses", (double)pi.rsSmoothPasses}, {"precipSmoothPasses", (double)pi.precipSmoothPasses}, {"wcPasses", (double)pi.wcPasses},
        {"leeCoastHops", (double)pi.leeCoastHops}, {"upCountSummer", (double)pi.listLengths[0]}, {"downCountSummer", (double)pi.listLengths[1]},
        {"upCountWinter", (double)pi.listLengths[2]}, {"downCountWinter", (double)pi.listLengths[3]}, {"depletionBase", pi.depletionBase},
        {"shadowDecay", pi.shadowDecay}, {"windwardDecay", pi.windwardDecay}, {"p95Summer", (double)pi.p95[0]}, {"p95Winter", (double)pi.p95[1]}});
    return o;
}
napi_value PrecipDownload(napi_env env, napi_callback_info info) { return block_download(env, info, wo_precip_download, "precipDownload"); }
napi_value PrecipUpload(napi_env env, napi_callback_info info) { return block_upload(env, info, wo_precip_upload, "precipUpload"); }
// computeTemperature(planet, r_elevation | null, temperatureOffset) -> the scalars of the call: the stage on the planet's wind, ocean and
// precipitation blocks; the results stay on the device (temperatureDownload)
napi_value ComputeTemperature(napi_env env, napi_callback_info info) {
    Args a(env, info); wo_planet* p = planet_at(a, 0);
    if (!planet_ok(env, p)) return nullptr;
    float* e = (float*)opt_regions(a, 1, napi_float32_array, p, "r_elevation", false); if (!a.ok) return nullptr;
    wo_temperature_info ti;
    if (wo_compute_temperature(p, wo_planet_num_regions(p), e, a.num(2), &ti)) return throw_wo(env, "computeTemperature");
    napi_value o; napi_create_object(env, &o);
    set_nums(env, o, {{"oceanWarmthPasses", (double)ti.oceanWarmthPasses}, {"smoothPasses", (double)ti.smoothPasses}, {"launches", (double)ti.launches}});
    return o;
}
napi_value TemperatureDownload(napi_env env, napi_callback_info info) { return block_download(env, info, wo_temperature_download, "temperatureDownload"); }
napi_value TemperatureUpload(napi_env env, napi_callback_info info) { return block_upload(env, info, wo_temperature_upload, "temperatureUpload"); }
// classifyKoppen(planet, r_elevation | null) -> Uint8Array of class ids: the classification on the planet's temperature and
// precipitation blocks; the ids also stay on the device
napi_value ClassifyKoppen(napi_env env, napi_callback_info info) {
    Args a(env, info); wo_planet* p = planet_at(a, 0);
    if (!planet_ok(env, p)) return nullptr;
    float* e = (float*)opt_regions(a, 1, napi_float32_array, p, "r_elevation", false); if (!a.ok) return nullptr;
    const size_t n = (size_t)wo_planet_num_regions(p);
    if (wo_classify_koppen(p, (int32_t)n, e)) return throw_wo(env, "classifyKoppen");
    void* d; napi_value out = make_ta(env, napi_uint8_array, n, 1, &d);
    if (!out) return nullptr;
    if (wo_koppen_download(p, (uint8_t*)d, (int64_t)n)) return throw_wo(env, "classifyKoppen");
    return out;
}
// landComponents(numRegions, adjOffset, adjList, r_isOcean) -> Int32Array (label = smallest id of the landmass, -1 for ocean)
napi_value LandComponents(napi_env env, napi_callback_info info) {
    Args a(env, info);
    size_t no, na, nc;
    int32_t* off = (int32_t*)a.ta(1, napi_int32_array, &no); if (!a.ok) return nullptr;
    int32_t* adj = (int32_t*)a.ta(2, napi_int32_array, &na); if (!a.ok) return nullptr;
    uint8_t* oc = (uint8_t*)a.ta(3, napi_uint8_array, &nc); if (!a.ok) return nullptr;
    const int32_t n = a.i32(0);
    if (n < 1 || (size_t)n + 1 != no || (size_t)n != nc) { napi_throw_range_error(env, nullptr, "mesh / r_isOcean length mismatch"); return nullptr; }
    void* d; napi_value out = make_ta(env, napi_int32_array, (size_t)n, 4, &d);
    if (wo_land_components(n, off, adj, oc, (int32_t*)d)) return throw_wo(env, "landComponents");
    return out;
}
// projectCoarsePlates(planet, coarseAdjOffset, coarseAdjList, coarse_xyz, coarse_r_plate, seed, numPlates|null) -> Int32Array
napi_value ProjectCoarsePlates(napi_env env, napi_callback_info info) {
    Args a(env, info); wo_planet* p = planet_at(a, 0);
    if (!planet_ok(env, p)) return nullptr;
    size_t no, na, nx, np_;
    int32_t* off = (int32_t*)a.ta(1, napi_int32_array, &no); if (!a.ok) return nullptr;
    int32_t* adj = (int32_t*)a.ta(2, napi_int32_array, &na); if (!a.ok) return nullptr;
    float* xyz = (float*)a.ta(3, napi_float32_array, &nx); if (!a.ok) return nullptr;
    int32_t* pl = (int32_t*)a.ta(4, napi_int32_array, &np_); if (!a.ok) return nullptr;
    if (no < 2 || nx != 3 * (no - 1) || np_ != no - 1) { napi_throw_range_error(env, nullptr, "coarse mesh arrays do not match"); return nullptr; }
    const int32_t n = wo_planet_num_regions(p);
    if (n < 1) return throw_wo(env, "projectCoarsePlates");
    void* d; napi_value out = make_ta(env, napi_int32_array, (size_t)n, 4, &d);
    if (wo_project_coarse_plates(p, (int32_t)(no - 1), off, adj, xyz, pl, a.num(5), a.has(6) ? a.i32(6) : -1, (int32_t*)d)) return throw_wo(env, "projectCoarsePlates");
    return out;
}
// smoothAndReconnectPlates(numRegions, adjOffset, adjList, r_plate (in place), plateSeeds Int32Array, numPasses)
napi_value SmoothAndReconnectPlates(napi_env env, napi_callback_info info) {
    Args a(env, info);
    size_t no, na, nr, ns;
    int32_t* off = (int32_t*)a.ta(1, napi_int32_array, &no); if (!a.ok) return nullptr;
    int32_t* adj = (int32_t*)a.ta(2, napi_int32_array, &na); if (!a.ok) return nullptr;
    int32_t* rp = (int32_t*)a.ta(3, napi_int32_array, &nr); if (!a.ok) return nullptr;
    int32_t* seeds = (int32_t*)a.ta(4, napi_int32_array, &ns); if (!a.ok) return nullptr;
    const int32_t n = a.i32(0);
    if ((size_t)n + 1 != no || (size_t)n != nr) { napi_throw_range_error(env, nullptr, "mesh / r_plate length mismatch"); return nullptr; }
    if (wo_smooth_reconnect_plates(n, off, adj, rp, seeds, (int32_t)ns, a.i32(5))) return throw_wo(env, "smoothAndReconnectPlates");
    return nullptr;
}

// generatePlates(adjOffset, adjList, r_xyz, numPlates, seed) -> { r_plate, plateSeeds Int32Array (Set order), pole Float64Array(3P), omega Float64Array(P), stats Float64Array }
napi_value GeneratePlates(napi_env env, napi_callback_info info) {
    Args a(env, info);
    size_t no, na, nx;
    int32_t* off = (int32_t*)a.ta(0, napi_int32_array, &no); if (!a.ok) return nullptr;
    int32_t* adj = (int32_t*)a.ta(1, napi_int32_array, &na); if (!a.ok) return nullptr;
    float* xyz = (float*)a.ta(2, napi_float32_array, &nx); if (!a.ok) return nullptr;
    const double np_ = a.num(3);
    if (no < 2 || nx != 3 * (no - 1) || (size_t)off[no - 1] != na) { napi_throw_range_error(env, nullptr, "generatePlates: mesh arrays and r_xyz do not match"); return nullptr; }
    if (!(np_ >= 1 && np_ <= 2147483647.0 && np_ == (double)(int64_t)np_)) { napi_throw_range_error(env, nullptr, "generatePlates: numPlates must be a positive integer"); return nullptr; }
    const int32_t N = (int32_t)(no - 1), numPlates = (int32_t)np_;
    const size_t cap = (size_t)(numPlates < N ? numPlates : N);
    void* rp; napi_value rpv = make_ta(env, napi_int32_array, (size_t)N, 4, &rp); if (!rpv) return nullptr;
    std::vector<int32_t> seeds(cap); std::vector<double> pole(3 * cap), omega(cap);
    int32_t P = 0; int64_t st[WO_PLATES_GEN_STATS];
    if (wo_generate_plates(N, off, adj, xyz, numPlates, a.num(4), (int32_t*)rp, seeds.data(), &P, pole.data(), omega.data(), st)) return throw_wo(env, "generatePlates");
    void *d1, *d2, *d3, *d4;
    napi_value sv = make_ta(env, napi_int32_array, (size_t)P, 4, &d1), pv = make_ta(env, napi_float64_array, 3 * (size_t)P, 8, &d2),
               ov = make_ta(env, napi_float64_array, (size_t)P, 8, &d3), tv = make_ta(env, napi_float64_array, WO_PLATES_GEN_STATS, 8, &d4);
    if (!sv || !pv || !ov || !tv) return nullptr;
    std::memcpy(d1, seeds.data(), (size_t)P * 4); std::memcpy(d2, pole.data(), 3 * (size_t)P * 8); std::memcpy(d3, omega.data(), (size_t)P * 8);
    for (int i = 0; i < WO_PLATES_GEN_STATS; ++i) ((double*)d4)[i] = (double)st[i];
    napi_value o; napi_create_object(env, &o);
    set_prop(env, o, "r_plate", rpv); set_prop(env, o, "plateSeeds", sv); set_prop(env, o, "pole", pv); set_prop(env, o, "omega", ov); set_prop(env, o, "stats", tv);
    return o;
}
// assignOceanLand(adjOffset, adjList, r_plate, plateSeeds Int32Array, r_xyz, seed, numContinents, continentSizeVariety, landCoverage)
//   -> { isOcean Uint8Array (one flag per seed), stats Float64Array }
napi_value AssignOceanLand(napi_env env, napi_callback_info info) {
    Args a(env, info);
    size_t no, na, nr, ns, nx;
    int32_t* off = (int32_t*)a.ta(0, napi_int32_array, &no); if (!a.ok) return nullptr;
    int32_t* adj = (int32_t*)a.ta(1, napi_int32_array, &na); if (!a.ok) return nullptr;
    int32_t* rp = (int32_t*)a.ta(2, napi_int32_array, &nr); if (!a.ok) return nullptr;
    int32_t* seeds = (int32_t*)a.ta(3, napi_int32_array, &ns); if (!a.ok) return nullptr;
    float* xyz = (float*)a.ta(4, napi_float32_array, &nx); if (!a.ok) return nullptr;
    if (no < 2 || nr != no - 1 || nx != 3 * (no - 1) || (size_t)off[no - 1] != na) { napi_throw_range_error(env, nullptr, "assignOceanLand: mesh arrays, r_plate and r_xyz do not match"); return nullptr; }
    if (ns < 1 || ns > nr) { napi_throw_range_error(env, nullptr, "assignOceanLand: plateSeeds must hold 1 .. numRegions ids"); return nullptr; }
    void *d1, *d2;
    napi_value fv = make_ta(env, napi_uint8_array, ns, 1, &d1), tv = make_ta(env, napi_float64_array, WO_PLATES_GEN_STATS, 8, &d2);
    if (!fv || !tv) return nullptr;
    int64_t st[WO_PLATES_GEN_STATS];
    if (wo_assign_ocean_land((int32_t)(no - 1), off, adj, rp, seeds, (int32_t)ns, xyz, a.num(5), a.i32(6), a.num(7), a.num(8), (uint8_t*)d1, st)) return throw_wo(env, "assignOceanLand");
    for (int i = 0; i < WO_PLATES_GEN_STATS; ++i) ((double*)d2)[i] = (double)st[i];
    napi_value o; napi_create_object(env, &o);
    set_prop(env, o, "isOcean", fv); set_prop(env, o, "stats", tv);
    return o;
}

// ---- heightmap import (include/worogen.h: wo_sample_heightmap / wo_synthetic_plates / wo_classify_regions / wo_triangle_centers) ----
// The image (Uint8Array or Uint8ClampedArray of imgW*imgH pixels) is checked before the planet handle is looked at.
napi_value SampleHeightmap(napi_env env, napi_callback_info info) {            // (planet, gray, imgW, imgH, download) -> Float32Array | undefined
    Args a(env, info);
    bool is = false; napi_typedarray_type t = napi_int8_array; size_t n = 0; void* data = nullptr; napi_value ab; size_t off;
    if (a.argc > 1 && napi_is_typedarray(env, a.argv[1], &is) == napi_ok && is) napi_get_typedarray_info(env, a.argv[1], &t, &n, &data, &ab, &off);
    if (!is || (t != napi_uint8_array && t != napi_uint8_clamped_array)) { napi_throw_type_error(env, nullptr, "sampleHeightmap: the image must be a Uint8Array or Uint8ClampedArray"); return nullptr; }
    const double W = a.num(2), H = a.num(3);
    if (!(W >= 1 && H >= 1 && W == (double)(int64_t)W && H == (double)(int64_t)H) || W * H > 2147483647.0) { napi_throw_range_error(env, nullptr, "sampleHeightmap: imgW and imgH must be positive integers with imgW*imgH < 2^31"); return nullptr; }
    if ((double)n != W * H) { napi_throw_range_error(env, nullptr, "sampleHeightmap: the image length must be imgW*imgH"); return nullptr; }
    wo_planet* p = planet_at(a, 0);
    if (!planet_ok(env, p)) return nullptr;
    bool download = false; if (a.argc > 4) napi_get_value_bool(env, a.argv[4], &download);
    void* d = nullptr; napi_value out = nullptr;
    if (download) { out = make_ta(env, napi_float32_array, (size_t)wo_planet_num_regions(p), 4, &d); if (!out) return nullptr; }
    if (wo_sample_heightmap(p, (const uint8_t*)data, (int32_t)W, (int32_t)H, (float*)d)) return throw_wo(env, "sampleHeightmap");
    return out;
}
napi_value SyntheticPlates(napi_env env, napi_callback_info info) {            // (planet) -> {r_plate, seeds Int32Array, seedIsOcean Uint8Array}
    Args a(env, info); wo_planet* p = planet_at(a, 0);
    if (!planet_ok(env, p)) return nullptr;
    const size_t n = (size_t)wo_planet_num_regions(p);
    void *rp, *sd, *so; napi_value vrp = make_ta(env, napi_int32_array, n, 4, &rp);
    std::vector<int32_t> seeds(n); std::vector<uint8_t> isOc(n); int32_t k = 0;
    if (!vrp) return nullptr;
    if (wo_synthetic_plates(p, (int32_t*)rp, seeds.data(), isOc.data(), &k)) return throw_wo(env, "syntheticPlates");
    napi_value vs = make_ta(env, napi_int32_array, (size_t)k, 4, &sd), vo = make_ta(env, napi_uint8_array, (size_t)k, 1, &so);
    if (!vs || !vo) return nullptr;
    if (k) { std::memcpy(sd, seeds.data(), (size_t)k * 4); std::memcpy(so, isOc.data(), (size_t)k); }
    napi_value o; napi_create_object(env, &o);
    set_prop(env, o, "r_plate", vrp); set_prop(env, o, "seeds", vs); set_prop(env, o, "seedIsOcean", vo);
    return o;
}
napi_value ClassifyRegions(napi_env env, napi_callback_info info) {            // (planet) -> {mountain_r, coastline_r, ocean_r} Int32Arrays
    Args a(env, info); wo_planet* p = planet_at(a, 0);
    if (!planet_ok(env, p)) return nullptr;
    const size_t n = (size_t)wo_planet_num_regions(p);
    std::vector<int32_t> l[3] = {std::vector<int32_t>(n), std::vector<int32_t>(n), std::vector<int32_t>(n)};
    int32_t counts[3] = {0, 0, 0};
    if (wo_classify_regions(p, l[0].data(), l[1].data(), l[2].data(), counts)) return throw_wo(env, "classifyRegions");
    napi_value o; napi_create_object(env, &o);
    const char* names[3] = {"mountain_r", "coastline_r", "ocean_r"};
    for (int j = 0; j < 3; ++j) {
        void* d; napi_value v = make_ta(env, napi_int32_array, (size_t)counts[j], 4, &d); if (!v) return nullptr;
        if (counts[j]) std::memcpy(d, l[j].data(), (size_t)counts[j] * 4);
        set_prop(env, o, names[j], v);
    }
    return o;
}
napi_value TriangleCenters(napi_env env, napi_callback_info info) {            // (triangles, r_xyz) -> Float32Array(numSides)
    Args a(env, info);
    size_t ns, nx; int32_t* tri = (int32_t*)a.ta(0, napi_int32_array, &ns); if (!a.ok) return nullptr;
    float* xyz = (float*)a.ta(1, napi_float32_array, &nx); if (!a.ok) return nullptr;
    for (size_t i = 0; i < ns; ++i) if (tri[i] < 0 || 3 * (size_t)tri[i] + 2 >= nx) { napi_throw_range_error(env, nullptr, "triangleCenters: corner out of range"); return nullptr; }
    void* d; napi_value out = make_ta(env, napi_float32_array, 3 * (ns / 3), 4, &d);
    if (!out) return nullptr;
    if (wo_triangle_centers((int32_t)(ns / 3), tri, xyz, (float*)d)) return throw_wo(env, "triangleCenters");
    return out;
}

// ---- map export (include/worogen.h: wo_map_raster / wo_map_color / wo_map_free / wo_map_raster_centered / wo_map_color_layer /
// wo_map_raster_cube / wo_map_dims) ----
// mapRaster(planet, triangles, halfedges, width, download) -> { width, height, covered, uncovered, regionMap: Int32Array | null }
napi_value MapRaster(napi_env env, napi_callback_info info) {
    Args a(env, info);
    size_t nt, nh;
    int32_t* tri = (int32_t*)a.ta(1, napi_int32_array, &nt); if (!a.ok) return nullptr;
    int32_t* he = (int32_t*)a.ta(2, napi_int32_array, &nh); if (!a.ok) return nullptr;
    if (nt != nh || nt == 0 || nt >= ((size_t)1 << 30)) { napi_throw_range_error(env, nullptr, "mapRaster: triangles and halfedges must have the same length, numSides"); return nullptr; }
    const double w = a.num(3);
    if (!(w >= 2 && w <= 32768 && w == (double)(int64_t)w && ((int64_t)w & 1) == 0)) { napi_throw_range_error(env, nullptr, "mapRaster: width must be an even integer from 2 to 32768"); return nullptr; }
    wo_planet* p = planet_at(a, 0);
    if (!planet_ok(env, p)) return nullptr;
    const int32_t W = (int32_t)w, H = W / 2;
    bool download = false; if (a.argc > 4) napi_get_value_bool(env, a.argv[4], &download);
    void* d = nullptr; napi_value map = nullptr;
    if (download) { map = make_ta(env, napi_int32_array, (size_t)W * (size_t)H, 4, &d); if (!map) return nullptr; }
    else napi_get_null(env, &map);
    int64_t counts[2] = {0, 0};
    if (wo_map_raster(p, (int32_t)nt, tri, he, W, (int32_t*)d, counts)) return throw_wo(env, "mapRaster");
    napi_value o; napi_create_object(env, &o);
    set_nums(env, o, {{"width", (double)W}, {"height", (double)H}, {"covered", (double)counts[0]}, {"uncovered", (double)counts[1]}});
    set_prop(env, o, "regionMap", map);
    return o;
}
// mapRasterCentered(planet, triangles, halfedges, width, centerLon, download) -> as mapRaster, around a centre meridian (radians)
napi_value MapRasterCentered(napi_env env, napi_callback_info info) {
    Args a(env, info);
    size_t nt, nh;
    int32_t* tri = (int32_t*)a.ta(1, napi_int32_array, &nt); if (!a.ok) return nullptr;
    int32_t* he = (int32_t*)a.ta(2, napi_int32_array, &nh); if (!a.ok) return nullptr;
    if (nt != nh || nt == 0 || nt >= ((size_t)1 << 30)) { napi_throw_range_error(env, nullptr, "mapRasterCentered: triangles and halfedges must have the same length, numSides"); return nullptr; }
    const double w = a.num(3);
    if (!(w >= 2 && w <= 32768 && w == (double)(int64_t)w && ((int64_t)w & 1) == 0)) { napi_throw_range_error(env, nullptr, "mapRasterCentered: width must be an even integer from 2 to 32768"); return nullptr; }
    wo_planet* p = planet_at(a, 0);
    if (!planet_ok(env, p)) return nullptr;
    const int32_t W = (int32_t)w, H = W / 2;
    const double centerLon = a.num(4);                                         // the library refuses what is not finite and within [-pi, pi]
    bool download = false; if (a.argc > 5) napi_get_value_bool(env, a.argv[5], &download);
    void* d = nullptr; napi_value map = nullptr;
    if (download) { map = make_ta(env, napi_int32_array, (size_t)W * (size_t)H, 4, &d); if (!map) return nullptr; }
    else napi_get_null(env, &map);
    int64_t counts[2] = {0, 0};
    if (wo_map_raster_centered(p, (int32_t)nt, tri, he, W, centerLon, (int32_t*)d, counts)) return throw_wo(env, "mapRasterCentered");
    napi_value o; napi_create_object(env, &o);
    set_nums(env, o, {{"width", (double)W}, {"height", (double)H}, {"covered", (double)counts[0]}, {"uncovered", (double)counts[1]}});
    set_prop(env, o, "regionMap", map);
    return o;
}
// The size of the RGBA of the planet's region map: of a width x width / 2 map when argument i gives a width, else of the resident map
// (wo_map_dims: the six stacked faces after mapRasterCube; the library says what is missing when there is none)
bool map_bytes(Args& a, size_t i, wo_planet* p, const char* fn, size_t* bytes) {
    if (a.has(i)) {
        const double w = a.num(i);
        if (!(w >= 2 && w <= 32768 && w == (double)(int64_t)w && ((int64_t)w & 1) == 0)) { napi_throw_range_error(a.env, nullptr, (std::string(fn) + ": width must be an even integer from 2 to 32768").c_str()); return false; }
        *bytes = (size_t)w * (size_t)(w / 2) * 4;
        return true;
    }
    int32_t dims[2] = {0, 0};
    if (wo_map_dims(p, dims)) { throw_wo(a.env, fn); return false; }
    *bytes = (size_t)dims[0] * (size_t)dims[1] * 4;
    return true;
}
// mapColor(planet, type 0..5, r_elevation | null, width?) -> Uint8ClampedArray(width * width / 2 * 4): the planet's region map coloured;
// without a width the result has the size of the resident map
napi_value MapColor(napi_env env, napi_callback_info info) {
    Args a(env, info); wo_planet* p = planet_at(a, 0);
    if (!planet_ok(env, p)) return nullptr;
    float* e = (float*)opt_regions(a, 2, napi_float32_array, p, "r_elevation", false); if (!a.ok) return nullptr;
    const double t = a.num(1);
    if (!(t >= 0 && t <= 5 && t == (double)(int64_t)t)) { napi_throw_range_error(env, nullptr, "mapColor: type must be an integer from 0 to 5"); return nullptr; }
    size_t bytes;
    if (!map_bytes(a, 3, p, "mapColor", &bytes)) return nullptr;
    void* d; napi_value out = make_ta(env, napi_uint8_clamped_array, bytes, 1, &d);
    if (!out) return nullptr;
    if (wo_map_color(p, (int32_t)t, e, (uint8_t*)d, (int64_t)bytes)) return throw_wo(env, "mapColor");
    return out;
}
// mapColorLayer(planet, layer 0..13, values | null, r_elevation | null, width?) -> Uint8ClampedArray(width * width / 2 * 4): the planet's
// region map coloured as a layer of the map view (WO_MAP_LAYER_*); values null: the layer's field of the planet's resident block
napi_value MapColorLayer(napi_env env, napi_callback_info info) {
    Args a(env, info); wo_planet* p = planet_at(a, 0);
    if (!planet_ok(env, p)) return nullptr;
    float* v = (float*)opt_regions(a, 2, napi_float32_array, p, "values", false); if (!a.ok) return nullptr;
    float* e = (float*)opt_regions(a, 3, napi_float32_array, p, "r_elevation", false); if (!a.ok) return nullptr;
    const double l = a.num(1);
    if (!(l >= 0 && l < WO_MAP_LAYER_COUNT && l == (double)(int64_t)l)) { napi_throw_range_error(env, nullptr, "mapColorLayer: layer must be an integer from 0 to 13"); return nullptr; }
    size_t bytes;
    if (!map_bytes(a, 4, p, "mapColorLayer", &bytes)) return nullptr;
    void* d; napi_value out = make_ta(env, napi_uint8_clamped_array, bytes, 1, &d);
    if (!out) return nullptr;
    if (wo_map_color_layer(p, (int32_t)l, v, e, (uint8_t*)d, (int64_t)bytes)) return throw_wo(env, "mapColorLayer");
    return out;
}
// mapRasterCube(planet, triangles, halfedges, faceSize, download) -> { faceSize, width, height, covered, uncovered, regionMap: Int32Array | null }:
// the six faces stacked, width = faceSize, height = 6 faceSize (include/worogen.h: wo_map_raster_cube)
napi_value MapRasterCube(napi_env env, napi_callback_info info) {
    Args a(env, info);
    size_t nt, nh;
    int32_t* tri = (int32_t*)a.ta(1, napi_int32_array, &nt); if (!a.ok) return nullptr;
    int32_t* he = (int32_t*)a.ta(2, napi_int32_array, &nh); if (!a.ok) return nullptr;
    if (nt != nh || nt == 0 || nt >= ((size_t)1 << 30)) { napi_throw_range_error(env, nullptr, "mapRasterCube: triangles and halfedges must have the same length, numSides"); return nullptr; }
    const double w = a.num(3);
    if (!(w >= 1 && w <= 16384 && w == (double)(int64_t)w)) { napi_throw_range_error(env, nullptr, "mapRasterCube: faceSize must be an integer from 1 to 16384"); return nullptr; }
    wo_planet* p = planet_at(a, 0);
    if (!planet_ok(env, p)) return nullptr;
    const int32_t S = (int32_t)w;
    bool download = false; if (a.argc > 4) napi_get_value_bool(env, a.argv[4], &download);
    void* d = nullptr; napi_value map = nullptr;
    if (download) { map = make_ta(env, napi_int32_array, 6 * (size_t)S * (size_t)S, 4, &d); if (!map) return nullptr; }
    else napi_get_null(env, &map);
    int64_t counts[2] = {0, 0};
    if (wo_map_raster_cube(p, (int32_t)nt, tri, he, S, (int32_t*)d, counts)) return throw_wo(env, "mapRasterCube");
    napi_value o; napi_create_object(env, &o);
    set_nums(env, o, {{"faceSize", (double)S}, {"width", (double)S}, {"height", 6.0 * (double)S}, {"covered", (double)counts[0]}, {"uncovered", (double)counts[1]}});
    set_prop(env, o, "regionMap", map);
    return o;
}
// mapDims(planet) -> { width, height } of the planet's resident region map, 0 and 0 without one
napi_value MapDims(napi_env env, napi_callback_info info) {
    Args a(env, info); wo_planet* p = planet_at(a, 0);
    if (!planet_ok(env, p)) return nullptr;
    int32_t dims[2] = {0, 0};
    if (wo_map_dims(p, dims)) return throw_wo(env, "mapDims");
    napi_value o; napi_create_object(env, &o);
    set_nums(env, o, {{"width", (double)dims[0]}, {"height", (double)dims[1]}});
    return o;
}
// reliefRaster(planet, triangles, halfedges, width, centerLon, r_elevation | null, download) -> { width, height, covered, uncovered,
// heights: Float32Array | null }: mapRasterCentered, and the height map beside its region map (include/worogen.h: wo_relief_raster)
napi_value ReliefRaster(napi_env env, napi_callback_info info) {
    Args a(env, info);
    size_t nt, nh;
    int32_t* tri = (int32_t*)a.ta(1, napi_int32_array, &nt); if (!a.ok) return nullptr;
    int32_t* he = (int32_t*)a.ta(2, napi_int32_array, &nh); if (!a.ok) return nullptr;
    if (nt != nh || nt == 0 || nt >= ((size_t)1 << 30)) { napi_throw_range_error(env, nullptr, "reliefRaster: triangles and halfedges must have the same length, numSides"); return nullptr; }
    const double w = a.num(3);
    if (!(w >= 2 && w <= 32768 && w == (double)(int64_t)w && ((int64_t)w & 1) == 0)) { napi_throw_range_error(env, nullptr, "reliefRaster: width must be an even integer from 2 to 32768"); return nullptr; }
    wo_planet* p = planet_at(a, 0);
    if (!planet_ok(env, p)) return nullptr;
    const int32_t W = (int32_t)w, H = W / 2;
    const double centerLon = a.num(4);                                         // the library refuses what is not finite and within [-pi, pi]
    float* e = (float*)opt_regions(a, 5, napi_float32_array, p, "r_elevation", false); if (!a.ok) return nullptr;
    bool download = false; if (a.argc > 6) napi_get_value_bool(env, a.argv[6], &download);
    void* d = nullptr; napi_value map = nullptr;
    if (download) { map = make_ta(env, napi_float32_array, (size_t)W * (size_t)H, 4, &d); if (!map) return nullptr; }
    else napi_get_null(env, &map);
    int64_t counts[2] = {0, 0};
    if (wo_relief_raster(p, (int32_t)nt, tri, he, W, centerLon, e, (float*)d, counts)) return throw_wo(env, "reliefRaster");
    napi_value o; napi_create_object(env, &o);
    set_nums(env, o, {{"width", (double)W}, {"height", (double)H}, {"covered", (double)counts[0]}, {"uncovered", (double)counts[1]}});
    set_prop(env, o, "heights", map);
    return o;
}
// reliefRasterCube(planet, triangles, halfedges, faceSize, r_elevation | null, download) -> { faceSize, width, height, covered, uncovered,
// heights: Float32Array | null }: mapRasterCube, and the height map of the six stacked faces (wo_relief_raster_cube)
napi_value ReliefRasterCube(napi_env env, napi_callback_info info) {
    Args a(env, info);
    size_t nt, nh;
    int32_t* tri = (int32_t*)a.ta(1, napi_int32_array, &nt); if (!a.ok) return nullptr;
    int32_t* he = (int32_t*)a.ta(2, napi_int32_array, &nh); if (!a.ok) return nullptr;
    if (nt != nh || nt == 0 || nt >= ((size_t)1 << 30)) { napi_throw_range_error(env, nullptr, "reliefRasterCube: triangles and halfedges must have the same length, numSides"); return nullptr; }
    const double w = a.num(3);
    if (!(w >= 1 && w <= 16384 && w == (double)(int64_t)w)) { napi_throw_range_error(env, nullptr, "reliefRasterCube: faceSize must be an integer from 1 to 16384"); return nullptr; }
    wo_planet* p = planet_at(a, 0);
    if (!planet_ok(env, p)) return nullptr;
    const int32_t S = (int32_t)w;
    float* e = (float*)opt_regions(a, 4, napi_float32_array, p, "r_elevation", false); if (!a.ok) return nullptr;
    bool download = false; if (a.argc > 5) napi_get_value_bool(env, a.argv[5], &download);
    void* d = nullptr; napi_value map = nullptr;
    if (download) { map = make_ta(env, napi_float32_array, 6 * (size_t)S * (size_t)S, 4, &d); if (!map) return nullptr; }
    else napi_get_null(env, &map);
    int64_t counts[2] = {0, 0};
    if (wo_relief_raster_cube(p, (int32_t)nt, tri, he, S, e, (float*)d, counts)) return throw_wo(env, "reliefRasterCube");
    napi_value o; napi_create_object(env, &o);
    set_nums(env, o, {{"faceSize", (double)S}, {"width", (double)S}, {"height", 6.0 * (double)S}, {"covered", (double)counts[0]}, {"uncovered", (double)counts[1]}});
    set_prop(env, o, "heights", map);
    return o;
}
// the pixels of the planet's resident map (wo_map_dims; 0 without one: the library then says what is missing)
bool relief_pixels(napi_env env, wo_planet* p, const char* fn, size_t* pixels) {
    int32_t dims[2] = {0, 0};
    if (wo_map_dims(p, dims)) { throw_wo(env, fn); return false; }
    *pixels = (size_t)dims[0] * (size_t)dims[1];
    return true;
}
// reliefHeights(planet) -> Float32Array: the resident height map (NaN: nothing covers the pixel)
napi_value ReliefHeights(napi_env env, napi_callback_info info) {
    Args a(env, info); wo_planet* p = planet_at(a, 0);
    if (!planet_ok(env, p)) return nullptr;
    size_t n;
    if (!relief_pixels(env, p, "reliefHeights", &n)) return nullptr;
    void* d; napi_value out = make_ta(env, napi_float32_array, n, 4, &d);
    if (!out) return nullptr;
    if (wo_relief_download(p, (float*)d, (int64_t)n * 4)) return throw_wo(env, "reliefHeights");
    return out;
}
// reliefHeight16(planet, kind 0..1) -> Uint16Array: the height map in 16 bits, linear (WO_RELIEF_HEIGHT, WO_RELIEF_LAND_HEIGHT)
napi_value ReliefHeight16(napi_env env, napi_callback_info info) {
    Args a(env, info); wo_planet* p = planet_at(a, 0);
    if (!planet_ok(env, p)) return nullptr;
    const double k = a.num(1);
    if (!(k >= 0 && k <= 1 && k == (double)(int64_t)k)) { napi_throw_range_error(env, nullptr, "reliefHeight16: kind must be 0 or 1"); return nullptr; }
    size_t n;
    if (!relief_pixels(env, p, "reliefHeight16", &n)) return nullptr;
    void* d; napi_value out = make_ta(env, napi_uint16_array, n, 2, &d);
    if (!out) return nullptr;
    if (wo_relief_height16(p, (int32_t)k, (uint16_t*)d, (int64_t)n * 2)) return throw_wo(env, "reliefHeight16");
    return out;
}
// reliefNormals(planet, space 0..1, strength, flags) -> Uint8ClampedArray: RGBA8 normals of the displaced surface (WO_RELIEF_NORMAL_*,
// WO_RELIEF_FLAT_OCEAN); the library refuses a strength that is not finite and >= 0
napi_value ReliefNormals(napi_env env, napi_callback_info info) {
    Args a(env, info); wo_planet* p = planet_at(a, 0);
    if (!planet_ok(env, p)) return nullptr;
    const double s = a.num(1), strength = a.num(2), flags = a.num(3);
    if (!(s >= 0 && s <= 1 && s == (double)(int64_t)s)) { napi_throw_range_error(env, nullptr, "reliefNormals: space must be 0 or 1"); return nullptr; }
    if (!(flags >= 0 && flags <= 1 && flags == (double)(int64_t)flags)) { napi_throw_range_error(env, nullptr, "reliefNormals: flags must be 0 or 1"); return nullptr; }
    size_t n;
    if (!relief_pixels(env, p, "reliefNormals", &n)) return nullptr;
    void* d; napi_value out = make_ta(env, napi_uint8_clamped_array, n * 4, 1, &d);
    if (!out) return nullptr;
    if (wo_relief_normals(p, (int32_t)s, strength, (int32_t)flags, (uint8_t*)d, (int64_t)n * 4)) return throw_wo(env, "reliefNormals");
    return out;
}

// ---- rivers and lakes (include/worogen.h: wo_compute_rivers and what reads its block) ------------------------------------------
// computeRivers(planet, r_elevation | null, source 0 precip | 1 uniform | 2 values, values | null) -> { landCells, pits, spilledBasins,
// endorheicBasins, lakeCells, rounds, launches }; the five fields stay on the planet
napi_value ComputeRivers(napi_env env, napi_callback_info info) {
    Args a(env, info); wo_planet* p = planet_at(a, 0);
    if (!planet_ok(env, p)) return nullptr;
    float* e = (float*)opt_regions(a, 1, napi_float32_array, p, "r_elevation", false); if (!a.ok) return nullptr;
    const double s = a.num(2);
    if (!(s >= 0 && s <= 2 && s == (double)(int64_t)s)) { napi_throw_range_error(env, nullptr, "computeRivers: source must be 0, 1 or 2"); return nullptr; }
    float* v = (float*)opt_regions(a, 3, napi_float32_array, p, "runoff values", false); if (!a.ok) return nullptr;
    wo_rivers_info I{};
    if (wo_compute_rivers(p, wo_planet_num_regions(p), e, (int32_t)s, v, &I)) return throw_wo(env, "computeRivers");
    napi_value o; napi_create_object(env, &o);
    set_nums(env, o, {{"landCells", (double)I.landCells}, {"pits", (double)I.pits}, {"spilledBasins", (double)I.spilledBasins}, {"endorheicBasins", (double)I.endorheicBasins},
                      {"lakeCells", (double)I.lakeCells}, {"rounds", (double)I.rounds}, {"launches", (double)I.launches}});
    return o;
}
// riversDownload(planet, key) -> Int32Array (r_river_receiver, r_river_basin), Float32Array (r_lake_level, r_river_flow) or
// BigUint64Array (r_river_discharge)
napi_value RiversDownload(napi_env env, napi_callback_info info) {
    Args a(env, info); wo_planet* p = planet_at(a, 0);
    if (!planet_ok(env, p)) return nullptr;
    char key[64]; if (!key_at(a, 1, key)) return nullptr;
    const size_t n = (size_t)wo_planet_num_regions(p);
    const bool i32 = !std::strcmp(key, "r_river_receiver") || !std::strcmp(key, "r_river_basin"), u64 = !std::strcmp(key, "r_river_discharge");
    const size_t elem = u64 ? 8 : 4;
    void* d; napi_value out = make_ta(env, u64 ? napi_biguint64_array : i32 ? napi_int32_array : napi_float32_array, n, elem, &d);
    if (!out) return nullptr;
    if (wo_rivers_download(p, key, d, (int64_t)(n * elem))) return throw_wo(env, "riversDownload");
    return out;
}
// riverLines(planet, minFlow, r_elevation | null) -> { segments: Float32Array(count * 6), flows: Float32Array(count), count }
napi_value RiverLines(napi_env env, napi_callback_info info) {
    Args a(env, info); wo_planet* p = planet_at(a, 0);
    if (!planet_ok(env, p)) return nullptr;
    float* e = (float*)opt_regions(a, 2, napi_float32_array, p, "r_elevation", false); if (!a.ok) return nullptr;
    const size_t n = (size_t)wo_planet_num_regions(p);
    std::vector<float> seg(6 * n + 6), flows(n + 1);
    int64_t count = 0;
    if (wo_river_lines(p, a.num(1), e, seg.data(), flows.data(), (int64_t)n, &count)) return throw_wo(env, "riverLines");
    void *ds, *df;
    napi_value s = make_ta(env, napi_float32_array, (size_t)count * 6, 4, &ds); if (!s) return nullptr;
    napi_value f = make_ta(env, napi_float32_array, (size_t)count, 4, &df); if (!f) return nullptr;
    std::memcpy(ds, seg.data(), (size_t)count * 24);
    std::memcpy(df, flows.data(), (size_t)count * 4);
    napi_value o; napi_create_object(env, &o);
    set_prop(env, o, "segments", s); set_prop(env, o, "flows", f);
    set_nums(env, o, {{"count", (double)count}});
    return o;
}
// mapColorRivers(planet, type 0..5, r_elevation | null, minFlow, width?) -> as mapColor, the rivers under minFlow and the lakes painted
napi_value MapColorRivers(napi_env env, napi_callback_info info) {
    Args a(env, info); wo_planet* p = planet_at(a, 0);
    if (!planet_ok(env, p)) return nullptr;
    float* e = (float*)opt_regions(a, 2, napi_float32_array, p, "r_elevation", false); if (!a.ok) return nullptr;
    const double t = a.num(1);
    if (!(t >= 0 && t <= 5 && t == (double)(int64_t)t)) { napi_throw_range_error(env, nullptr, "mapColorRivers: type must be an integer from 0 to 5"); return nullptr; }
    size_t bytes;
    if (!map_bytes(a, 4, p, "mapColorRivers", &bytes)) return nullptr;
    void* d; napi_value out = make_ta(env, napi_uint8_clamped_array, bytes, 1, &d);
    if (!out) return nullptr;
    if (wo_map_color_rivers(p, (int32_t)t, e, a.num(3), (uint8_t*)d, (int64_t)bytes)) return throw_wo(env, "mapColorRivers");
    return out;
}
napi_value MapFree(napi_env env, napi_callback_info info) {                    // (planet)
    Args a(env, info); wo_planet* p = planet_at(a, 0);
    if (!planet_ok(env, p)) return nullptr;
    if (wo_map_free(p)) return throw_wo(env, "mapFree");
    return nullptr;
}

// ---- globe mesh (include/worogen.h: wo_globe_mesh / wo_globe_mesh_plates / wo_globe_lines) --------------------------------
// the sides of a mesh at arguments 1 and 2
bool globe_sides(Args& a, const char* fn, int32_t** tri, int32_t** he, size_t* ns) {
    size_t nh;
    *tri = (int32_t*)a.ta(1, napi_int32_array, ns); if (!a.ok) return false;
    *he = (int32_t*)a.ta(2, napi_int32_array, &nh); if (!a.ok) return false;
    if (*ns != nh || *ns == 0 || *ns >= ((size_t)1 << 30)) { napi_throw_range_error(a.env, nullptr, (std::string(fn) + ": triangles and halfedges must have the same length, numSides").c_str()); return false; }
    return true;
}
// the two outputs asked for by the booleans at arguments i and i + 1 (undefined: true), nine floats per side each
bool globe_outputs(Args& a, size_t i, size_t ns, napi_value* pos, void** dp, napi_value* col, void** dc) {
    bool wp = true, wc = true;
    if (a.has(i)) napi_get_value_bool(a.env, a.argv[i], &wp);
    if (a.has(i + 1)) napi_get_value_bool(a.env, a.argv[i + 1], &wc);
    *dp = *dc = nullptr;
    napi_get_null(a.env, pos); napi_get_null(a.env, col);
    if (wp && !(*pos = make_ta(a.env, napi_float32_array, ns * 9, 4, dp))) { napi_throw_range_error(a.env, nullptr, ("the position array of " + std::to_string(ns * 36) + " bytes does not fit into one ArrayBuffer").c_str()); return false; }
    if (wc && !(*col = make_ta(a.env, napi_float32_array, ns * 9, 4, dc))) { napi_throw_range_error(a.env, nullptr, ("the colour array of " + std::to_string(ns * 36) + " bytes does not fit into one ArrayBuffer").c_str()); return false; }
    return true;
}
napi_value globe_result(napi_env env, napi_value pos, napi_value col, const float bounds[6], bool havePositions) {
    napi_value o; napi_create_object(env, &o);
    set_prop(env, o, "position", pos); set_prop(env, o, "color", col);
    napi_value b; napi_get_null(env, &b);
    if (havePositions) { void* d; b = make_ta(env, napi_float32_array, 6, 4, &d); std::memcpy(d, bounds, 24); }
    set_prop(env, o, "bounds", b);
    return o;
}
// globeMesh(planet, triangles, halfedges, source 0 | 1, id, values | null, r_elevation | null, positions = true, colors = true)
//   -> { position: Float32Array(numSides * 9) | null, color: the same | null, bounds: Float32Array(6) | null }
napi_value GlobeMesh(napi_env env, napi_callback_info info) {
    Args a(env, info);
    int32_t *tri, *he; size_t ns;
    if (!globe_sides(a, "globeMesh", &tri, &he, &ns)) return nullptr;
    wo_planet* p = planet_at(a, 0);
    if (!planet_ok(env, p)) return nullptr;
    float* v = (float*)opt_regions(a, 5, napi_float32_array, p, "values", false); if (!a.ok) return nullptr;
    float* e = (float*)opt_regions(a, 6, napi_float32_array, p, "r_elevation", false); if (!a.ok) return nullptr;
    napi_value pos, col; void *dp, *dc;
    if (!globe_outputs(a, 7, ns, &pos, &dp, &col, &dc)) return nullptr;
    float bounds[6] = {0, 0, 0, 0, 0, 0};
    if (wo_globe_mesh(p, (int32_t)ns, tri, he, a.i32(3), a.i32(4), v, e, (float*)dp, (float*)dc, (int64_t)ns * 9, bounds)) return throw_wo(env, "globeMesh");
    return globe_result(env, pos, col, bounds, dp != nullptr);
}
// globeMeshPlates(planet, triangles, halfedges, r_plate, plateSeeds Int32Array, plateColors Float32Array(3 per seed), r_elevation | null,
//                 positions = true, colors = true) -> as globeMesh
napi_value GlobeMeshPlates(napi_env env, napi_callback_info info) {
    Args a(env, info);
    int32_t *tri, *he; size_t ns;
    if (!globe_sides(a, "globeMeshPlates", &tri, &he, &ns)) return nullptr;
    wo_planet* p = planet_at(a, 0);
    if (!planet_ok(env, p)) return nullptr;
    int32_t* plate = (int32_t*)opt_regions(a, 3, napi_int32_array, p, "r_plate", false); if (!a.ok) return nullptr;
    size_t nSeeds = 0, nColors = 0; int32_t* seeds = nullptr; float* colors = nullptr;
    if (a.has(4)) { seeds = (int32_t*)a.ta(4, napi_int32_array, &nSeeds); if (!a.ok) return nullptr; }
    if (a.has(5)) { colors = (float*)a.ta(5, napi_float32_array, &nColors); if (!a.ok) return nullptr; }
    if (seeds && colors && nColors != 3 * nSeeds) { napi_throw_range_error(env, nullptr, "globeMeshPlates: plateColors must hold three floats per plate seed"); return nullptr; }
    float* e = (float*)opt_regions(a, 6, napi_float32_array, p, "r_elevation", false); if (!a.ok) return nullptr;
    napi_value pos, col; void *dp, *dc;
    if (!globe_outputs(a, 7, ns, &pos, &dp, &col, &dc)) return nullptr;
    float bounds[6] = {0, 0, 0, 0, 0, 0};
    if (wo_globe_mesh_plates(p, (int32_t)ns, tri, he, plate, (int32_t)nSeeds, seeds, colors, e, (float*)dp, (float*)dc, (int64_t)ns * 9, bounds)) return throw_wo(env, "globeMeshPlates");
    return globe_result(env, pos, col, bounds, dp != nullptr);
}
// globeLines(planet, triangles, halfedges, kind 0 | 1, r_elevation | null, superPlates | null) -> Float32Array(segments * 6)
napi_value GlobeLines(napi_env env, napi_callback_info info) {
    Args a(env, info);
    int32_t *tri, *he; size_t ns;
    if (!globe_sides(a, "globeLines", &tri, &he, &ns)) return nullptr;
    wo_planet* p = planet_at(a, 0);
    if (!planet_ok(env, p)) return nullptr;
    float* e = (float*)opt_regions(a, 4, napi_float32_array, p, "r_elevation", false); if (!a.ok) return nullptr;
    float* sp = (float*)opt_regions(a, 5, napi_float32_array, p, "superPlates", false); if (!a.ok) return nullptr;
    const size_t room = ns / 2;
    std::vector<float> seg(6 * room + 6);
    int64_t count = 0;
    if (wo_globe_lines(p, (int32_t)ns, tri, he, a.i32(3), e, sp, seg.data(), (int64_t)room, &count)) return throw_wo(env, "globeLines");
    void* d; napi_value out = make_ta(env, napi_float32_array, (size_t)count * 6, 4, &d);
    if (!out) return nullptr;
    std::memcpy(d, seg.data(), (size_t)count * 24);
    return out;
}

// ---- arrow overlays (include/worogen.h: wo_overlay_bins / wo_overlay_arrows) ----------------------------------------------
// overlayBins(planet, skipLand, r_elevation | null) -> Int32Array(7200): per 3 x 3 degree cell the region closest to its centre, -1 for none
napi_value OverlayBins(napi_env env, napi_callback_info info) {
    Args a(env, info); wo_planet* p = planet_at(a, 0);
    if (!planet_ok(env, p)) return nullptr;
    bool skip = false;
    if (a.has(1)) napi_get_value_bool(env, a.argv[1], &skip);
    float* e = (float*)opt_regions(a, 2, napi_float32_array, p, "r_elevation", false); if (!a.ok) return nullptr;
    void* d; napi_value out = make_ta(env, napi_int32_array, WO_OVERLAY_BINS, 4, &d);
    if (!out) return nullptr;
    if (wo_overlay_bins(p, skip ? 1 : 0, e, (int32_t*)d)) return throw_wo(env, "overlayBins");
    return out;
}
// overlayArrows(planet, kind 0 wind | 1 ocean, season 0 summer | 1 winter, centerLon, r_elevation | null)
//   -> { globe: { position, color }, map: { position, color }, count }: Float32Array(count * 18) each
napi_value OverlayArrows(napi_env env, napi_callback_info info) {
    Args a(env, info); wo_planet* p = planet_at(a, 0);
    if (!planet_ok(env, p)) return nullptr;
    float* e = (float*)opt_regions(a, 4, napi_float32_array, p, "r_elevation", false); if (!a.ok) return nullptr;
    const size_t room = (size_t)WO_OVERLAY_BINS * 18;
    std::vector<float> buf(4 * room);
    int64_t count = 0;
    if (wo_overlay_arrows(p, a.i32(1), a.i32(2), a.has(3) ? a.num(3) : 0.0, e, buf.data(), buf.data() + room, buf.data() + 2 * room, buf.data() + 3 * room, WO_OVERLAY_BINS, &count))
        return throw_wo(env, "overlayArrows");
    napi_value o, forms[2], c;
    napi_create_object(env, &o);
    static const char* const names[4] = {"position", "color", "position", "color"};
    for (int k = 0; k < 4; ++k) {
        if (k % 2 == 0) napi_create_object(env, &forms[k / 2]);
        void* d; napi_value ta = make_ta(env, napi_float32_array, (size_t)count * 18, 4, &d);
        if (!ta) return nullptr;
        std::memcpy(d, buf.data() + k * room, (size_t)count * 72);
        set_prop(env, forms[k / 2], names[k], ta);
    }
    set_prop(env, o, "globe", forms[0]); set_prop(env, o, "map", forms[1]);
    napi_create_int32(env, (int32_t)count, &c); set_prop(env, o, "count", c);
    return o;
}

// ---- the editor: hit test and highlights (include/worogen.h: wo_pick_* / wo_highlight_*) ---------------------------------------------
static napi_value pick_result(napi_env env, const char* first, napi_value a, const char* second, napi_value b) {
    napi_value o; napi_create_object(env, &o);
    set_prop(env, o, first, a); set_prop(env, o, second, b);
    return o;
}
// pickRegions(planet, directions Float64Array(3 per query)) -> { regions: Int32Array, dots: Float64Array }
napi_value PickRegions(napi_env env, napi_callback_info info) {
    Args a(env, info); wo_planet* p = planet_at(a, 0);
    if (!planet_ok(env, p)) return nullptr;
    size_t n = 0; double* dirs = (double*)a.ta(1, napi_float64_array, &n); if (!a.ok) return nullptr;
    if (n % 3) { napi_throw_range_error(env, nullptr, "pickRegions: directions must hold three doubles per query"); return nullptr; }
    if (n / 3 > (size_t)WO_PICK_MAX_QUERIES) { napi_throw_range_error(env, nullptr, "pickRegions: more than 65536 queries in one call"); return nullptr; }
    void *dr, *dd;
    napi_value regions = make_ta(env, napi_int32_array, n / 3, 4, &dr), dots = make_ta(env, napi_float64_array, n / 3, 8, &dd);
    if (!regions || !dots) return nullptr;
    double none[3] = {0, 0, 0}; int32_t noRegion = 0;        // an empty typed array may have no storage
    if (wo_pick_regions(p, (int32_t)(n / 3), n ? dirs : none, n ? (int32_t*)dr : &noRegion, n ? (double*)dd : nullptr)) return throw_wo(env, "pickRegions");
    return pick_result(env, "regions", regions, "dots", dots);
}
static napi_value pick_directions(napi_env env, napi_callback_info info, bool map) {
    Args a(env, info);
    const char* name = map ? "pickDirectionsMap" : "pickDirectionsGlobe";
    const size_t per = map ? 2 : 6;
    size_t n = 0; double* in = (double*)a.ta(0, napi_float64_array, &n); if (!a.ok) return nullptr;
    if (n % per || n / per > (size_t)WO_PICK_MAX_QUERIES) { napi_throw_range_error(env, nullptr, map ? "pickDirectionsMap: points must hold two doubles per query, at most 65536 queries" : "pickDirectionsGlobe: rays must hold six doubles per query, at most 65536 queries"); return nullptr; }
    const size_t q = n / per;
    void *dd, *dv;
    napi_value dirs = make_ta(env, napi_float64_array, 3 * q, 8, &dd), valid = make_ta(env, napi_uint8_array, q, 1, &dv);
    if (!dirs || !valid) return nullptr;
    if (q) {
        const int rc = map ? wo_pick_directions_map((int32_t)q, in, a.has(1) ? a.num(1) : 0.0, (double*)dd, (uint8_t*)dv) : wo_pick_directions_globe((int32_t)q, in, (double*)dd, (uint8_t*)dv);
        if (rc) return throw_wo(env, name);
    }
    return pick_result(env, "directions", dirs, "valid", valid);
}
// pickDirectionsGlobe(rays Float64Array(origin xyz, direction xyz per query)) -> { directions: Float64Array(3 per query), valid: Uint8Array }
napi_value PickDirectionsGlobe(napi_env env, napi_callback_info info) { return pick_directions(env, info, false); }
// pickDirectionsMap(points Float64Array(wx, wy per query), centerLon = 0) -> as pickDirectionsGlobe
napi_value PickDirectionsMap(napi_env env, napi_callback_info info) { return pick_directions(env, info, true); }
// highlightSet(planet, r_plate Int32Array, pendingPlates Int32Array, pendingIsOcean Uint8Array, hoveredPlate, hoveredKoppen)
//   -> { pendingOcean, pendingLand, hoveredPlate, hoveredKoppen }: the regions per tint
napi_value HighlightSet(napi_env env, napi_callback_info info) {
    Args a(env, info); wo_planet* p = planet_at(a, 0);
    if (!planet_ok(env, p)) return nullptr;
    int32_t* plate = (int32_t*)opt_regions(a, 1, napi_int32_array, p, "highlightSet: r_plate (an Int32Array of numRegions entries)", true); if (!a.ok) return nullptr;
    size_t nPending = 0, nOcean = 0;
    int32_t* pending = (int32_t*)a.ta(2, napi_int32_array, &nPending); if (!a.ok) return nullptr;
    uint8_t* isOcean = (uint8_t*)a.ta(3, napi_uint8_array, &nOcean); if (!a.ok) return nullptr;
    if (nPending != nOcean) { napi_throw_range_error(env, nullptr, "highlightSet: pendingIsOcean must hold one byte per pending plate"); return nullptr; }
    int64_t counts[4] = {0, 0, 0, 0};
    if (wo_highlight_set(p, plate, (int32_t)nPending, nPending ? pending : nullptr, nPending ? isOcean : nullptr, a.has(4) ? a.i32(4) : -1, a.has(5) ? a.i32(5) : -1, counts))
        return throw_wo(env, "highlightSet");
    napi_value o; napi_create_object(env, &o);
    set_nums(env, o, {{"pendingOcean", (double)counts[0]}, {"pendingLand", (double)counts[1]}, {"hoveredPlate", (double)counts[2]}, {"hoveredKoppen", (double)counts[3]}});
    return o;
}
// highlightClear(planet)
napi_value HighlightClear(napi_env env, napi_callback_info info) {
    Args a(env, info); wo_planet* p = planet_at(a, 0);
    if (!planet_ok(env, p)) return nullptr;
    if (wo_highlight_clear(p)) return throw_wo(env, "highlightClear");
    return nullptr;
}

// ---- multi-GPU exchange over RCCL (include/worogen.h: wo_comm_*; one worker thread per GPU holds one communicator) -------
void FinalizeComm(napi_env, void* data, void*) { wo_comm_destroy((wo_comm*)data); }
napi_value CommUniqueId(napi_env env, napi_callback_info) {                   // () -> Uint8Array(128): rank 0 makes it, the host posts it to every worker
    void* d; napi_value out = make_ta(env, napi_uint8_array, WO_COMM_ID_BYTES, 1, &d);
    if (wo_comm_unique_id((uint8_t*)d)) return throw_wo(env, "commUniqueId");
    return out;
}
napi_value CommCreate(napi_env env, napi_callback_info info) {                 // (ctx, id Uint8Array(128), nranks, rank) -> comm handle (collective)
    Args a(env, info);
    wo_ctx* c = (wo_ctx*)a.ext(0);
    size_t n; uint8_t* id = (uint8_t*)a.ta(1, napi_uint8_array, &n); if (!a.ok) return nullptr;
    if (!c || n != WO_COMM_ID_BYTES) { napi_throw_type_error(env, nullptr, "commCreate: expected (ctx, Uint8Array(128), nranks, rank)"); return nullptr; }
    wo_comm* cm = nullptr;
    if (wo_comm_create(c, id, a.i32(2), a.i32(3), &cm)) return throw_wo(env, "commCreate");
    napi_value v; NAPI_OK(napi_create_external(env, cm, FinalizeComm, nullptr, &v));
    return v;
}
napi_value PlanetSetHalo(napi_env env, napi_callback_info info) {              // (planet, sendIdx Int32Array, recvIdx Int32Array)
    Args a(env, info); wo_planet* p = planet_at(a, 0);
    if (!planet_ok(env, p)) return nullptr;
    size_t ns, nr; int32_t* s = (int32_t*)a.ta(1, napi_int32_array, &ns); if (!a.ok) return nullptr;
    int32_t* r = (int32_t*)a.ta(2, napi_int32_array, &nr); if (!a.ok) return nullptr;
    if (wo_planet_set_halo(p, s, (int32_t)ns, r, (int32_t)nr)) return throw_wo(env, "planetSetHalo");
    return nullptr;
}
napi_value PlanetExchangeAllgather(napi_env env, napi_callback_info info) {    // (planet, comm, counts Int32Array(nranks))
    Args a(env, info); wo_planet* p = planet_at(a, 0); wo_comm* cm = (wo_comm*)a.ext(1);
    if (!planet_ok(env, p)) return nullptr;
    size_t n; int32_t* counts = (int32_t*)a.ta(2, napi_int32_array, &n); if (!a.ok) return nullptr;
    if (!cm || (int)n != wo_comm_size(cm)) { napi_throw_range_error(env, nullptr, "planetExchangeAllgather: one count per rank"); return nullptr; }
    if (wo_planet_exchange_allgather(p, cm, counts)) return throw_wo(env, "planetExchangeAllgather");
    return nullptr;
}
napi_value PlanetExchangeNeighbors(napi_env env, napi_callback_info info) {    // (planet, comm, nToPrev, nFromPrev)
    Args a(env, info); wo_planet* p = planet_at(a, 0); wo_comm* cm = (wo_comm*)a.ext(1);
    if (!planet_ok(env, p)) return nullptr;
    if (!cm) { napi_throw_type_error(env, nullptr, "planetExchangeNeighbors: expected a communicator handle"); return nullptr; }
    if (wo_planet_exchange_neighbors(p, cm, a.i32(2), a.i32(3))) return throw_wo(env, "planetExchangeNeighbors");
    return nullptr;
}

napi_value PlanetSetFloodExchange(napi_env env, napi_callback_info info) {    // (planet, trueOcean Uint8Array | null, comm, counts Int32Array(nranks), cellsByRank Int32Array)
    Args a(env, info); wo_planet* p = planet_at(a, 0);
    if (!planet_ok(env, p)) return nullptr;
    napi_valuetype t; napi_typeof(env, a.argv[1], &t);
    if (t == napi_null || t == napi_undefined) {               // exchange off
        if (wo_planet_set_flood_exchange(p, nullptr, nullptr, nullptr)) return throw_wo(env, "planetSetFloodExchange");
        return nullptr;
    }
    size_t nOc, nCounts, nCells;
    uint8_t* oc = (uint8_t*)a.ta(1, napi_uint8_array, &nOc); if (!a.ok) return nullptr;
    wo_comm* cm = (wo_comm*)a.ext(2);
    int32_t* counts = (int32_t*)a.ta(3, napi_int32_array, &nCounts); if (!a.ok) return nullptr;
    int32_t* cells = (int32_t*)a.ta(4, napi_int32_array, &nCells); if (!a.ok) return nullptr;
    if ((int32_t)nOc != wo_planet_num_regions(p)) { napi_throw_range_error(env, nullptr, "planetSetFloodExchange: r_isOcean length must equal mesh.numRegions"); return nullptr; }
    if (!cm || (int)nCounts != wo_comm_size(cm)) { napi_throw_range_error(env, nullptr, "planetSetFloodExchange: one count per rank"); return nullptr; }
    int64_t total = 0; for (size_t j = 0; j < nCounts; ++j) total += counts[j];
    if (total != (int64_t)nCells) { napi_throw_range_error(env, nullptr, "planetSetFloodExchange: cellsByRank must hold every rank's cells, in rank order"); return nullptr; }
    if (wo_planet_set_flood_exchange_comm(p, oc, cm, counts, cells)) return throw_wo(env, "planetSetFloodExchange");
    return nullptr;
}

napi_value Init(napi_env env, napi_value exports) {
    struct { const char* name; napi_callback fn; } fns[] = {
        {"fibSpherePoints", FibSpherePoints}, {"sphereDelaunay", SphereDelaunay}, {"meshCsr", MeshCsr}, {"sphereReferenceClosure", SphereReferenceClosure},
        {"generatePlates", GeneratePlates}, {"assignOceanLand", AssignOceanLand}, {"neighborDist", NeighborDist},
        {"triangleElevations", TriangleElevations}, {"noiseTables", NoiseTables}, {"noiseEval", NoiseEval}, {"noisePoint", NoisePoint},
        {"deviceCount", DeviceCount}, {"ctxCreate", CtxCreate}, {"sphereMeshDevice", SphereMeshDevice}, {"fibSpherePointsDevice", FibSpherePointsDevice},
        {"sphereMeshSeedDevice", SphereMeshSeedDevice}, {"planetCreate", PlanetCreate}, {"planetDestroy", PlanetDestroy},
        {"warpTerrain", WarpTerrain}, {"smoothElevation", SmoothElevation}, {"erodeComposite", ErodeComposite},
        {"sharpenRidges", SharpenRidges}, {"applySoilCreep", ApplySoilCreep},
        {"planetUpload", PlanetUpload}, {"planetDownload", PlanetDownload}, {"planetDownloadOcean", PlanetDownloadOcean},
        {"planetUploadHotspot", PlanetUploadHotspot}, {"planetOceanFromElevation", PlanetOceanFromElevation}, {"planetSync", PlanetSync},
        {"planetSaveState", PlanetSaveState}, {"planetRestoreState", PlanetRestoreState}, {"planetSyntheticTerrain", PlanetSyntheticTerrain},
        {"warpTerrainResident", WarpTerrainResident}, {"smoothElevationResident", SmoothElevationResident},
        {"erodeCompositeResident", ErodeCompositeResident}, {"sharpenRidgesResident", SharpenRidgesResident},
        {"applySoilCreepResident", ApplySoilCreepResident}, {"timerStart", TimerStart}, {"timerStopMs", TimerStopMs},
        {"lastStageTiming", LastStageTiming}, {"lastErodeStats", LastErodeStats}, {"assignElevation", AssignElevation}, {"buildSuperPlates", BuildSuperPlates},
        {"projectCoarsePlates", ProjectCoarsePlates}, {"smoothField", SmoothField}, {"smoothAndReconnectPlates", SmoothAndReconnectPlates},
        {"diffuseOceanWarmth", DiffuseOceanWarmth}, {"computeWindConvergence", WindConvergence}, {"advectMoisture", AdvectMoisture},
        {"landComponents", LandComponents}, {"sampleHeightmap", SampleHeightmap}, {"syntheticPlates", SyntheticPlates},
        {"classifyRegions", ClassifyRegions}, {"triangleCenters", TriangleCenters}, {"computeWind", ComputeWind}, {"computeGradients", ComputeGradients},
        {"windUpload", WindUpload}, {"computeOceanCurrents", ComputeOceanCurrents}, {"oceanDownload", OceanDownload},
        {"oceanUpload", OceanUpload}, {"computePrecipitation", ComputePrecipitation}, {"precipDownload", PrecipDownload},
        {"precipUpload", PrecipUpload}, {"computeTemperature", ComputeTemperature}, {"temperatureDownload", TemperatureDownload},
        {"temperatureUpload", TemperatureUpload}, {"classifyKoppen", ClassifyKoppen},
        {"mapRaster", MapRaster}, {"mapColor", MapColor}, {"mapFree", MapFree}, {"mapRasterCentered", MapRasterCentered}, {"mapColorLayer", MapColorLayer},
        {"mapRasterCube", MapRasterCube}, {"mapDims", MapDims},
        {"reliefRaster", ReliefRaster}, {"reliefRasterCube", ReliefRasterCube}, {"reliefHeights", ReliefHeights}, {"reliefHeight16", ReliefHeight16},
        {"reliefNormals", ReliefNormals},
        {"computeRivers", ComputeRivers}, {"riversDownload", RiversDownload}, {"riverLines", RiverLines}, {"mapColorRivers", MapColorRivers},
        {"globeMesh", GlobeMesh}, {"globeMeshPlates", GlobeMeshPlates}, {"globeLines", GlobeLines},
        {"overlayBins", OverlayBins}, {"overlayArrows", OverlayArrows},
        {"pickRegions", PickRegions}, {"pickDirectionsGlobe", PickDirectionsGlobe}, {"pickDirectionsMap", PickDirectionsMap},
        {"highlightSet", HighlightSet}, {"highlightClear", HighlightClear},
        {"commUniqueId", CommUniqueId}, {"commCreate", CommCreate}, {"planetSetHalo", PlanetSetHalo},
        {"planetExchangeAllgather", PlanetExchangeAllgather}, {"planetExchangeNeighbors", PlanetExchangeNeighbors}, {"planetSetFloodExchange", PlanetSetFloodExchange},
    };
    for (auto& f : fns) {
        napi_value v;
        if (napi_create_function(env, f.name, NAPI_AUTO_LENGTH, f.fn, nullptr, &v) != napi_ok) return nullptr;
        napi_set_named_property(env, exports, f.name, v);
    }
    napi_value ver; napi_create_int32(env, wo_abi_version(), &ver); napi_set_named_property(env, exports, "abiVersion", ver);
    return exports;
}

}  // namespace

NAPI_MODULE(NODE_GYP_MODULE_NAME, Init)
