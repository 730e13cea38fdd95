// The terrain passes on the planet's resident field and their entry points: coast flags, the Jacobi passes (smoothElevation,
// sharpenRidges, soil creep: js/terrain-post.js), warpTerrain, the synthetic terrain, and the noise functions on caller-owned points.
#include <hip/hip_runtime.h>

#include "../../include/worogen.h"
#include "common_kernels.h"
#include "device.h"
#include "erode_block.h"
#include "mirror.h"
#include "noise.h"

namespace wo {

// ---------------------------------------------------------------- fields / Jacobi ---------------
__global__ __launch_bounds__(WO_BLOCK) void k_coast(Fields F, uint8_t* coast) {
    WO_XCD_CELLS(r, F.N) coast[r] = coast_flag(F, r);
}
__global__ __launch_bounds__(WO_BLOCK) void k_smooth(Fields F, const float* in, float* out, double strength) {
    WO_XCD_CELLS(r, F.N) out[r] = smooth_cell(F, in, r, strength);
}
__global__ __launch_bounds__(WO_BLOCK) void k_sharpen(Fields F, const float* in, const float* orig, float* out, double strength) {
    WO_XCD_CELLS(r, F.N) out[r] = sharpen_cell(F, in, orig, r, strength);
}
__global__ __launch_bounds__(WO_BLOCK) void k_creep(Fields F, const float* in, float* out, double strength) {
    WO_XCD_CELLS(r, F.N) out[r] = creep_cell(F, in, r, strength);
}

// ---------------------------------------------------------------- noise -------------------------
__global__ __launch_bounds__(WO_BLOCK) void k_noise_eval(const uint8_t* tables, int32_t kind, int32_t octaves, double p0,
                                                          double p1, double p2, int64_t n, const double* xyz, double* out) {
    __shared__ uint8_t sP[512], sM[512];
    load_tables(tables, sP, sM);
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const double x = xyz[3 * i], y = xyz[3 * i + 1], z = xyz[3 * i + 2];
        double v;
        if (kind == 0) v = noise3d(sP, sM, x, y, z);
        else if (kind == 1) v = fbm(sP, sM, x, y, z, octaves, p0);
        else v = ridged_fbm(sP, sM, x, y, z, octaves, p0, p1, p2);
        out[i] = v;
    }
}

// SURVEY 8(d) synthetic terrain: e = 0.9*fbm(1.5p,5) - 0.12 + 0.25*ridged(3p,4)*max(0,fbm(1.5p,5))
__global__ __launch_bounds__(WO_BLOCK) void k_synthetic(const uint8_t* tables, const float* xyz, float* e, uint8_t* ocean, int32_t N) {
    __shared__ uint8_t sP[512], sM[512];
    load_tables(tables, sP, sM);
    WO_GRID_STRIDE(r, N) {
        const double x = xyz[3 * r], y = xyz[3 * r + 1], z = xyz[3 * r + 2];
        const double f = fbm(sP, sM, x * 1.5, y * 1.5, z * 1.5, 5);
        const double rg = ridged_fbm(sP, sM, x * 3, y * 3, z * 3, 4);
        const float v = (float)(0.9 * f - 0.12 + 0.25 * rg * (f > 0 ? f : 0));
        e[r] = v;
        ocean[r] = (v <= 0.0f) ? 1 : 0;
    }
}

__global__ __launch_bounds__(WO_BLOCK) void k_warp(Fields F, const uint8_t* tables, const float* in, float* out, double maxAmp,
                                                    double warpBias, const float* hot) {
    __shared__ uint8_t sP[512], sM[512];
    load_tables(tables, sP, sM);
    WO_XCD_CELLS(r, F.N) {
        const int32_t src = warp_source_cell(F, sP, sM, r, maxAmp);
        out[r] = warp_blend(in[r], in[src], warpBias, hot != nullptr, hot ? hot[r] : 0.0f);
    }
}

void coast_flags(wo_planet* p) {
    launch(p, FAM_COAST, k_coast, xcd_grid(p->N), WO_BLOCK, fields(p), p->d_coast);
}

static void jacobi(wo_planet* p, int kind, int32_t iterations, double strength) {
    if (iterations <= 0) return;
    MirrorScope mir(p);                     // Jacobi passes read rows and neighbour values only: any naming of the cells gives the same field
    if (iterations >= 2) mir.enter();       // (moving the field in and out costs about one pass)
    coast_flags(p);
    const int gridN = xcd_grid(p->N);
    hipStream_t s = p->ctx->stream;
    if (kind == 1) WO_HIP(hipMemcpyAsync(p->d_orig, p->d_e, (size_t)p->N * sizeof(float), hipMemcpyDeviceToDevice, s));
    for (int32_t it = 0; it < iterations; ++it) {
        Fields F = fields(p);
        if (kind == 0) launch(p, FAM_SMOOTH, k_smooth, gridN, WO_BLOCK, F, (const float*)p->d_e, p->d_e2, strength);
        else if (kind == 1) launch(p, FAM_SHARPEN, k_sharpen, gridN, WO_BLOCK, F, (const float*)p->d_e, (const float*)p->d_orig, p->d_e2, strength);
        else launch(p, FAM_CREEP, k_creep, gridN, WO_BLOCK, F, (const float*)p->d_e, p->d_e2, strength);
        swap_elev(p);
    }
    mir.finish();
}

void upload_tables(wo_planet* p, double seed) {
    uint8_t t[1024];
    noise_tables(seed, t, t + 512);
    WO_HIP(hipMemcpyAsync(p->d_tables, t, 1024, hipMemcpyHostToDevice, p->ctx->stream));
    WO_HIP(hipStreamSynchronize(p->ctx->stream));     // t is a stack buffer
}

static void warp(wo_planet* p, double seed, double strength, bool useHot) {
    if (!(strength > 0)) return;          // js/terrain-post.js:234
    upload_tables(p, seed + 9999);
    const double maxAmp = 0.12 * strength, bias = 0.25 + 0.5 * strength;
    // the greedy walk reads rows and positions of cells along its path, nothing that depends on a cell's name: it runs on the
    // patch-major mirror as well (10 M cells: 15 -> 5 ms)
    MirrorScope mir(p);
    mir.enter();
    const float* hot = useHot ? (const float*)p->d_hot : (const float*)nullptr;
    if (mir.on && useHot) {
        auto& M = p->mirror;
        if (!M.hot) M.hot = M.mem.dev<float>(p->N);
        mirror_gather_f32(p, p->d_hot, M.hot);
        hot = M.hot;
    }
    launch(p, FAM_WARP, k_warp, xcd_grid(p->N), WO_BLOCK, fields(p), (const uint8_t*)p->d_tables, (const float*)p->d_e, p->d_e2,
           maxAmp, bias, hot);
    swap_elev(p);
    mir.finish();
}

// A pass on host arrays: upload, body, download (the entry points of the JS call surface, here and in erode.hip)
int with_host_field(wo_planet* p, const char* fn, float* e, const uint8_t* oc, bool needOcean, void (*body)(wo_planet*, void*), void* arg) {
    if (!check_planet(p, fn)) return 1;
    if (!e || (needOcean && !oc)) { set_error(std::string(fn) + ": null pointer"); return 1; }
    WO_TRY
    int rc = wo_planet_upload(p, e, oc);
    if (rc) return rc;
    body(p, arg);
    return wo_planet_download(p, e);
    WO_CATCH(fn)
}

}  // namespace wo

using namespace wo;

extern "C" {

int wo_warp_terrain_resident(wo_planet* p, double seed, double strength, int32_t useHotspot) {
    if (!check_planet(p, "wo_warp_terrain_resident")) return 1;
    if (useHotspot && !p->hot_valid) { set_error("wo_warp_terrain_resident: no hotspot field uploaded"); return 1; }
    WO_TRY
    warp(p, seed, strength, useHotspot != 0);
    return 0;
    WO_CATCH("wo_warp_terrain_resident")
}

int wo_smooth_elevation_resident(wo_planet* p, int32_t iterations, double strength) {
    if (!check_planet(p, "wo_smooth_elevation_resident")) return 1;
    WO_TRY jacobi(p, 0, iterations, strength); return 0; WO_CATCH("wo_smooth_elevation_resident")
}
int wo_sharpen_ridges_resident(wo_planet* p, int32_t iterations, double strength) {
    if (!check_planet(p, "wo_sharpen_ridges_resident")) return 1;
    WO_TRY jacobi(p, 1, iterations, strength); return 0; WO_CATCH("wo_sharpen_ridges_resident")
}
int wo_soil_creep_resident(wo_planet* p, int32_t iterations, double strength) {
    if (!check_planet(p, "wo_soil_creep_resident")) return 1;
    WO_TRY jacobi(p, 2, iterations, strength); return 0; WO_CATCH("wo_soil_creep_resident")
}

int wo_planet_synthetic_terrain(wo_planet* p, double seed) {
    if (!check_planet(p, "wo_planet_synthetic_terrain")) return 1;
    WO_TRY
    upload_tables(p, seed);
    launch(p, FAM_SYNTH, k_synthetic, blocks_for(p->N), WO_BLOCK, (const uint8_t*)p->d_tables, (const float*)p->d_xyz, p->d_e, p->d_ocean, p->N);
    ocean_changed(p);
    return 0;
    WO_CATCH("wo_planet_synthetic_terrain")
}

// ---- JS call surface: host arrays in, mutated in place ----
struct JacArgs { int kind; int32_t it; double s; };
struct WarpArgs { double seed, strength; bool hot; };

int wo_warp_terrain(wo_planet* p, float* r_elevation, double seed, double strength, const float* r_hotspot) {
    if (p && r_hotspot) { int rc = wo_planet_upload_hotspot(p, r_hotspot); if (rc) return rc; }
    WarpArgs a{seed, strength, r_hotspot != nullptr};
    return with_host_field(p, "wo_warp_terrain", r_elevation, nullptr, false,
                           [](wo_planet* q, void* v) { auto* w = (WarpArgs*)v; warp(q, w->seed, w->strength, w->hot); }, &a);
}
// the three Jacobi passes on host arrays (kind 0: smoothElevation, 1: sharpenRidges, 2: soil creep)
static int jacobi_host_field(wo_planet* p, const char* fn, int kind, float* e, const uint8_t* oc, int32_t it, double s) {
    JacArgs a{kind, it, s};
    return with_host_field(p, fn, e, oc, true, [](wo_planet* q, void* v) { auto* j = (JacArgs*)v; jacobi(q, j->kind, j->it, j->s); }, &a);
}
int wo_smooth_elevation(wo_planet* p, float* e, const uint8_t* oc, int32_t it, double s) { return jacobi_host_field(p, "wo_smooth_elevation", 0, e, oc, it, s); }
int wo_sharpen_ridges(wo_planet* p, float* e, const uint8_t* oc, int32_t it, double s) { return jacobi_host_field(p, "wo_sharpen_ridges", 1, e, oc, it, s); }
int wo_soil_creep(wo_planet* p, float* e, const uint8_t* oc, int32_t it, double s) { return jacobi_host_field(p, "wo_soil_creep", 2, e, oc, it, s); }

int wo_noise_eval(wo_ctx* ctx, double seed, int32_t kind, int32_t octaves, double p0, double p1, double p2, int64_t n,
                  const double* xyz, double* out) {
    if (!ctx || !xyz || !out || n < 0 || kind < 0 || kind > 2) { set_error("wo_noise_eval: bad arguments"); return 1; }
    if (n == 0) return 0;
    WO_TRY
    WO_HIP(hipSetDevice(ctx->device));
    uint8_t t[1024];
    noise_tables(seed, t, t + 512);
    hipStream_t s = ctx->stream;
    DeviceArena B;
    double* d_in = B.dev<double>(3 * (size_t)n); double* d_out = B.dev<double>((size_t)n); uint8_t* d_t = B.dev<uint8_t>(1024);
    WO_HIP(hipMemcpyAsync(d_t, t, 1024, hipMemcpyHostToDevice, s));
    WO_HIP(hipMemcpyAsync(d_in, xyz, 3 * (size_t)n * 8, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_noise_eval, dim3(blocks_for(n, 4096)), dim3(WO_BLOCK), 0, s, (const uint8_t*)d_t, kind, octaves, p0, p1, p2, n,
                       (const double*)d_in, d_out);
    WO_HIP(hipMemcpyAsync(out, d_out, (size_t)n * 8, hipMemcpyDeviceToHost, s));
    WO_HIP(hipStreamSynchronize(s));
    return 0;
    WO_CATCH("wo_noise_eval")
}

}  // extern "C"
