// The climate sweeps on the planet's mesh: smoothField (js/climate-util.js), diffuseOceanWarmth (js/temperature.js),
// computeWindConvergence and advectMoisture (js/precipitation.js).  Each sweep has a form on device-resident fields, which wind.hip,
// temp.hip and precip.hip call, and an entry point on caller-owned host arrays around it.
#include <hip/hip_runtime.h>

#include <cmath>

#include "../../include/worogen.h"
#include "climate_ops.h"
#include "common_kernels.h"
#include "device.h"
#include "erode_block.h"

namespace wo {

// ---------------------------------------------------------------- climate-util smoothField ------
__global__ __launch_bounds__(WO_BLOCK) void k_smooth_field(Fields F, const float* src, float* dst) {
    WO_XCD_CELLS(r, F.N) dst[r] = smooth_field_cell(F, src, r);
}

// ---------------------------------------------------------------- climate sweeps (js/temperature.js, js/precipitation.js) ----
__global__ __launch_bounds__(WO_BLOCK) void k_warmth_seed(const float* warmth, const uint8_t* isLand, float* out, int32_t N) {
    WO_GRID_STRIDE(r, N) out[r] = warmth_seed_cell(warmth, isLand, r);
}
__global__ __launch_bounds__(WO_BLOCK) void k_warmth_diffuse(Fields F, ClimateMesh M, const float* src, const float* cont, float* dst) {
    WO_XCD_CELLS(r, F.N) dst[r] = warmth_diffuse_cell(M, src, cont, r);
}
__global__ __launch_bounds__(WO_BLOCK) void k_wind_convergence(Fields F, ClimateMesh M, const float* wx, const float* wy, const float* wz, float* out) {
    WO_XCD_CELLS(r, F.N) out[r] = wind_convergence_cell(M, wx, wy, wz, r);
}
__global__ __launch_bounds__(WO_BLOCK) void k_moisture_seed(Fields F, ClimateMesh M, const uint8_t* isLand, const float* wx, const float* wy, const float* wz,
                                                             const float* warmth, const int32_t* coastDist, float* out) {
    WO_XCD_CELLS(r, F.N) out[r] = moisture_seed_cell(M, isLand, wx, wy, wz, warmth, coastDist, r);
}
__global__ __launch_bounds__(WO_BLOCK) void k_moisture_advect(Fields F, ClimateMesh M, const float* src, const float* heightKm, const uint8_t* isLand,
                                                               const float* windE, const float* windN, const float* wx, const float* wy, const float* wz,
                                                               int32_t maxHops, double depletionBase, float* dst) {
    WO_XCD_CELLS(r, F.N) dst[r] = moisture_advect_cell(M, src, heightKm, isLand, windE, windN, wx, wy, wz, maxHops, depletionBase, r);
}

ClimateMesh climate_mesh(const wo_planet* p) { ClimateMesh M; M.N = p->N; M.off = p->d_off; M.adj = p->d_adj; M.xyz = p->d_xyz; return M; }

}  // namespace wo

using namespace wo;

// smoothField (js/climate-util.js:5-25) on a device-resident field, no host round trip: `passes` Jacobi passes from a into b and
// back; returns the buffer that holds the result (wind.hip)
float* wo::smooth_field_resident(wo_planet* p, float* a, float* b, int32_t passes) {
    Fields F = fields(p);
    for (int32_t pass = 0; pass < passes; ++pass) {
        launch(p, FAM_SMOOTH_FIELD, k_smooth_field, xcd_grid(p->N), WO_BLOCK, F, (const float*)a, b);
        std::swap(a, b);
    }
    return a;
}

// diffuseOceanWarmth (js/temperature.js:19-54) of one season on device-resident fields (temp.hip, the split form of its diffusion)
float* wo::diffuse_warmth_resident(wo_planet* p, const float* warmth, const uint8_t* isLand, const float* plateCont, int32_t passes, float* a, float* b) {
    const Fields F = fields(p); const ClimateMesh M = climate_mesh(p);
    launch(p, FAM_CLIMATE, k_warmth_seed, blocks_for(p->N, 4096), WO_BLOCK, warmth, isLand, a, p->N);
    for (int32_t pass = 0; pass < passes; ++pass) { launch(p, FAM_CLIMATE, k_warmth_diffuse, xcd_grid(p->N), WO_BLOCK, F, M, (const float*)a, plateCont, b); std::swap(a, b); }
    return a;
}

// computeWindConvergence and advectMoisture (js/precipitation.js:19-52, :59-182) on device-resident fields (precip.hip); the
// advection returns the buffer that holds the result
void wo::wind_convergence_resident(wo_planet* p, const float* wx, const float* wy, const float* wz, float* out) {
    launch(p, FAM_CLIMATE, k_wind_convergence, xcd_grid(p->N), WO_BLOCK, fields(p), climate_mesh(p), wx, wy, wz, out);
}
float* wo::advect_moisture_resident(wo_planet* p, const float* heightKm, const uint8_t* isLand, const float* windE, const float* windN, const float* wx, const float* wy,
                                    const float* wz, const float* warmth, const int32_t* coastDist, int32_t maxHops, double depletionBase, float* a, float* b) {
    const Fields F = fields(p); const ClimateMesh M = climate_mesh(p);
    launch(p, FAM_CLIMATE, k_moisture_seed, xcd_grid(p->N), WO_BLOCK, F, M, isLand, wx, wy, wz, warmth, coastDist, a);
    for (int32_t it = 0; it < maxHops; ++it) {
        launch(p, FAM_CLIMATE, k_moisture_advect, xcd_grid(p->N), WO_BLOCK, F, M, (const float*)a, heightKm, isLand, windE, windN, wx, wy, wz, maxHops, depletionBase, b);
        std::swap(a, b);
    }
    return a;
}

extern "C" {

// smoothField (js/climate-util.js:5-25) on a caller-owned field; the planet's resident elevation is not touched
int wo_smooth_field(wo_planet* p, float* field, int32_t passes) {
    if (!check_planet(p, "wo_smooth_field")) return 1;
    if (!field) { set_error("wo_smooth_field: null field"); return 1; }
    if (passes <= 0) return 0;
    WO_TRY
    hipStream_t s = p->ctx->stream;
    const size_t bytes = (size_t)p->N * sizeof(float);
    DeviceArena B;
    float* a = B.dev<float>(p->N); float* b = B.dev<float>(p->N);
    WO_HIP(hipMemcpyAsync(a, field, bytes, hipMemcpyHostToDevice, s));
    WO_HIP(hipMemcpyAsync(field, smooth_field_resident(p, a, b, passes), bytes, hipMemcpyDeviceToHost, s));
    WO_HIP(hipStreamSynchronize(s));
    return 0;
    WO_CATCH("wo_smooth_field")
}

// ---- climate sweeps on caller-owned fields (js/temperature.js:19-66, js/precipitation.js:18-52, :59-195) ----
int wo_diffuse_ocean_warmth(wo_planet* p, const float* r_oceanWarmth, const uint8_t* r_isLand, const float* r_plateContinentality,
                            int32_t passes, float* out) {
    if (!check_planet(p, "wo_diffuse_ocean_warmth")) return 1;
    if (!r_isLand || !out) { set_error("wo_diffuse_ocean_warmth: null pointer"); return 1; }
    WO_TRY
    hipStream_t s = p->ctx->stream; const size_t N = (size_t)p->N;
    DeviceArena B;
    const float* w = up(B, r_oceanWarmth, N, s); const uint8_t* land = up(B, r_isLand, N, s); const float* cont = up(B, r_plateContinentality, N, s);
    float* a = B.dev<float>(N); float* b = B.dev<float>(N);
    WO_HIP(hipMemcpyAsync(out, diffuse_warmth_resident(p, w, land, cont, passes, a, b), N * sizeof(float), hipMemcpyDeviceToHost, s));
    WO_HIP(hipStreamSynchronize(s));
    return 0;
    WO_CATCH("wo_diffuse_ocean_warmth")
}

int wo_wind_convergence(wo_planet* p, const float* r_wind3dX, const float* r_wind3dY, const float* r_wind3dZ, float* out) {
    if (!check_planet(p, "wo_wind_convergence")) return 1;
    if (!r_wind3dX || !r_wind3dY || !r_wind3dZ || !out) { set_error("wo_wind_convergence: null pointer"); return 1; }
    WO_TRY
    hipStream_t s = p->ctx->stream; const size_t N = (size_t)p->N;
    DeviceArena B;
    const float* wx = up(B, r_wind3dX, N, s); const float* wy = up(B, r_wind3dY, N, s); const float* wz = up(B, r_wind3dZ, N, s);
    float* o = B.dev<float>(N);
    wind_convergence_resident(p, wx, wy, wz, o);
    WO_HIP(hipMemcpyAsync(out, o, N * sizeof(float), hipMemcpyDeviceToHost, s));
    WO_HIP(hipStreamSynchronize(s));
    return 0;
    WO_CATCH("wo_wind_convergence")
}

int wo_advect_moisture(wo_planet* p, const float* r_heightKm, const uint8_t* r_isLand, const float* r_windE, const float* r_windN,
                       const float* r_wind3dX, const float* r_wind3dY, const float* r_wind3dZ, const float* r_oceanWarmth,
                       const int32_t* r_coastDistLand, int32_t maxHops, float* out) {
    if (!check_planet(p, "wo_advect_moisture")) return 1;
    if (!r_heightKm || !r_isLand || !r_windE || !r_windN || !r_wind3dX || !r_wind3dY || !r_wind3dZ || !r_coastDistLand || !out) { set_error("wo_advect_moisture: null pointer"); return 1; }
    if (maxHops < 1) { set_error("wo_advect_moisture: maxHops must be >= 1"); return 1; }
    WO_TRY
    hipStream_t s = p->ctx->stream; const size_t N = (size_t)p->N;
    DeviceArena B;
    const float* hk = up(B, r_heightKm, N, s); const uint8_t* land = up(B, r_isLand, N, s); const float* we = up(B, r_windE, N, s); const float* wn = up(B, r_windN, N, s);
    const float* wx = up(B, r_wind3dX, N, s); const float* wy = up(B, r_wind3dY, N, s); const float* wz = up(B, r_wind3dZ, N, s);
    const float* w = up(B, r_oceanWarmth, N, s); const int32_t* cd = up(B, r_coastDistLand, N, s);
    float* a = B.dev<float>(N); float* b = B.dev<float>(N);
    const double depletionBase = 1 - std::pow(0.78, 1.0 / maxHops);                  // js/precipitation.js:123
    WO_HIP(hipMemcpyAsync(out, advect_moisture_resident(p, hk, land, we, wn, wx, wy, wz, w, cd, maxHops, depletionBase, a, b), N * sizeof(float), hipMemcpyDeviceToHost, s));
    WO_HIP(hipStreamSynchronize(s));
    return 0;
    WO_CATCH("wo_advect_moisture")
}

}  // extern "C"
