// Seasonal temperature and the Koppen classification on the device (js/temperature.js:69-237, js/koppen.js:67-288), on the
// planet's resident mesh and stream.  The per-cell bodies and the contract are in temp_ops.h.  computeTemperature reads the
// planet's wind block (wind_block.h: latitude, longitude, the land mask, both continentalities, the ITCZ arrays), the speed and
// warmth fields of its ocean block (ocean_block.h), r_precip_* of its precipitation block (precip_block.h) and the elevation, and
// leaves r_temperature_summer / _winter in the planet's temperature block (8 bytes per cell).  classifyKoppen reads the
// elevation, the temperature block and r_precip_* and leaves one class id per cell in the planet's Koppen block (1 byte per cell).
//
// Launches per call of wo_compute_temperature: oceanWarmthPasses + 3 (7 at 64 cells, 10 at 10 001, 73 at 1 000 001):
//   k_temp_seed [1]                      the seed of diffuseOceanWarmth, both seasons as one float2 per cell
//   k_temp_diffuse x oceanWarmthPasses   one pass on both seasons: row offsets, neighbour ids and plateContinentality are read
//                                        once, a neighbour's pair comes with one 8-byte load; ping-pong between two pair buffers
//   k_temp_cell [1]                      the per-cell loop, both seasons per thread (one ITCZ lookup per season from LDS)
//   k_temp_smooth [1]                    the smoothField pass with the normalisation at its store, both seasons
// and one of wo_classify_koppen: k_koppen [1].  Under WO_TEST_HOOKS=temp_split_diffuse the diffusion runs season by season with the
// single-field kernels of kernels_impl.h (k_warmth_seed, k_warmth_diffuse: 2 + 2 x oceanWarmthPasses launches, then k_temp_join);
// the same bits.  Temporaries live in an arena on the call's stack; no host round trip: the stream is waited for once, at the end.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstring>
#include <memory>
#include <string>

#include "../../include/worogen.h"
#include "device.h"
#include "ocean_block.h"
#include "precip_block.h"
#include "temp_ops.h"
#include "wind_block.h"

namespace Tm = wo::temp;

// the temperature block and the Koppen block of a planet
struct wo_temp_block {
    wo::DeviceArena mem;                                      // owns the two fields
    bool valid = false;                                       // a whole result of wo_compute_temperature
    uint32_t have = 0;                                        // bit f: out[f] was set, by wo_compute_temperature or by wo_temperature_upload
    float* out[2] = {nullptr, nullptr};                       // r_temperature_summer, r_temperature_winter
    wo_temperature_info info{};
};
struct wo_koppen_block {
    wo::DeviceArena mem;
    bool valid = false;
    uint8_t* cls = nullptr;
};

namespace wo {

using Tm::G2;

struct TempArgs {
    const float *lat, *lon, *elev, *cont, *plateCont;
    const uint8_t* isLand;
    const float *precip[2], *warmth[2], *speed[2];
    const G2* coastal;
    float* out[2];
};

__global__ __launch_bounds__(WO_BLOCK) void k_temp_seed(const float* __restrict__ warmS, const float* __restrict__ warmW, const uint8_t* __restrict__ isLand,
                                                        G2* __restrict__ out, int32_t N) {
    const int32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r < N) out[r] = G2{{warmth_seed_cell(warmS, isLand, r), warmth_seed_cell(warmW, isLand, r)}};
}

__global__ __launch_bounds__(WO_BLOCK) void k_temp_diffuse(int32_t tile, const int32_t* __restrict__ off, const int32_t* __restrict__ adj,
                                                           const float* __restrict__ plateCont, const G2* __restrict__ src, G2* __restrict__ dst, int32_t N) {
    const int32_t r = ocean_xcd_cell(tile);
    if (r < N) dst[r] = Tm::warmth_diffuse_pair_cell(off, adj, src, plateCont, r);
}

// the split form's two fields back into pairs
__global__ __launch_bounds__(WO_BLOCK) void k_temp_join(const float* __restrict__ a, const float* __restrict__ b, G2* __restrict__ out, int32_t N) {
    const int32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r < N) out[r] = G2{{a[r], b[r]}};
}

__global__ __launch_bounds__(WO_BLOCK) void k_temp_cell(TempArgs A, const float* __restrict__ itcz, double temperatureOffset, int32_t N) {
    __shared__ float sItcz[2 * W::ITCZ_SAMPLES];
    for (int i = threadIdx.x; i < 2 * W::ITCZ_SAMPLES; i += blockDim.x) sItcz[i] = itcz[i];
    __syncthreads();
    const int32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= N) return;
    const Tm::CellIn I{A.lat[r], A.lon[r], A.elev[r], A.cont[r], A.plateCont[r], A.isLand[r] != 0};
    const double T_annual = Tm::annual_curve(I.lat);
    const G2 cw = A.coastal[r];
    for (int s = 0; s < 2; ++s)
        A.out[s][r] = Tm::temperature_cell(I, s == 0, sItcz + s * W::ITCZ_SAMPLES, A.precip[s][r], A.warmth[s][r], A.speed[s][r], cw.v[s], T_annual, temperatureOffset,
                                           Tm::NoCensus());
}

__global__ __launch_bounds__(WO_BLOCK) void k_temp_smooth(Fields F, const float* __restrict__ srcS, const float* __restrict__ srcW, float* __restrict__ outS,
                                                          float* __restrict__ outW) {
    const int32_t r = ocean_xcd_cell(F.xcdTile);
    if (r >= F.N) return;
    outS[r] = Tm::smooth_normalise_cell(F, srcS, r);
    outW[r] = Tm::smooth_normalise_cell(F, srcW, r);
}

__global__ __launch_bounds__(WO_BLOCK) void k_koppen(const float* __restrict__ elev, const float* __restrict__ tS, const float* __restrict__ tW,
                                                     const float* __restrict__ pS, const float* __restrict__ pW, uint8_t* __restrict__ out, int32_t N) {
    const int32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r < N) out[r] = Tm::koppen_cell(elev[r], tS[r], tW[r], pS[r], pW[r], Tm::NoCensus());
}

void temp_free(wo_planet* p) {
    delete p->temp; p->temp = nullptr;
    delete p->koppen; p->koppen = nullptr;
}

static void temp_alloc(wo_planet* p) {
    if (p->temp) return;
    std::unique_ptr<wo_temp_block> block(new wo_temp_block());          // the planet gets the block once it is complete
    for (auto& o : block->out) o = block->mem.dev<float>((size_t)p->N);
    p->temp = block.release();
}

static void koppen_alloc(wo_planet* p) {
    if (p->koppen) return;
    std::unique_ptr<wo_koppen_block> block(new wo_koppen_block());
    block->cls = block->mem.dev<uint8_t>((size_t)p->N);
    p->koppen = block.release();
}

// the elevation a stage reads: the caller's, uploaded into the call's arena, or the resident field
static const float* stage_elevation(wo_planet* p, DeviceArena& T, const float* r_elevation) {
    return r_elevation ? up(T, r_elevation, (size_t)p->N, p->ctx->stream) : p->d_e;
}

static void temp_run(wo_planet* p, const float* r_elevation, double temperatureOffset) {
    auto* B = p->temp;
    auto* Wb = p->wind;
    auto* Ob = p->ocean;
    auto* Pb = p->precip;
    const int32_t N = p->N, g = blocks_for(N), tile = xcd_tile(N), xg = xcd_grid(N);
    const size_t n = (size_t)N;
    hipStream_t s = p->ctx->stream;
    B->valid = false; B->have = 0;
    const int32_t passes = Tm::warmth_passes(N);
    DeviceArena T;                                            // the temporaries of this call
    float* itcz = T.dev<float>((size_t)2 * W::ITCZ_SAMPLES);
    WO_HIP(hipMemcpyAsync(itcz, Wb->itcz[1], sizeof(float) * 2 * W::ITCZ_SAMPLES, hipMemcpyHostToDevice, s));      // itczLatsSummer and itczLatsWinter lie one after the other; the wind block outlives the copy
    const float* e = stage_elevation(p, T, r_elevation);
    const float* warm[2] = {Ob->out[3], Ob->out[7]};
    const float* speed[2] = {Ob->out[2], Ob->out[6]};
    // diffuseOceanWarmth of both seasons
    G2* pair[2] = {T.dev<G2>(n), T.dev<G2>(n)};
    const G2* coastal;
    int32_t launches;
    if (p->opt.tempSplitDiffuse) {
        float *a = T.dev<float>(n), *b = T.dev<float>(n), *c = T.dev<float>(n), *d = T.dev<float>(n);
        const float* rS = diffuse_warmth_resident(p, warm[0], Wb->isLand, Wb->plateCont, passes, a, b);
        const float* rW = diffuse_warmth_resident(p, warm[1], Wb->isLand, Wb->plateCont, passes, c, d);
        launch(p, FAM_CLIMATE, k_temp_join, g, WO_BLOCK, rS, rW, pair[0], N);
        coastal = pair[0];
        launches = 2 * (1 + passes) + 1;
    } else {
        launch(p, FAM_CLIMATE, k_temp_seed, g, WO_BLOCK, warm[0], warm[1], (const uint8_t*)Wb->isLand, pair[0], N);
        int cur = 0;
        for (int32_t pass = 0; pass < passes; ++pass, cur ^= 1)
            launch(p, FAM_CLIMATE, k_temp_diffuse, xg, WO_BLOCK, tile, (const int32_t*)p->d_off, (const int32_t*)p->d_adj, (const float*)Wb->plateCont, (const G2*)pair[cur],
                   pair[cur ^ 1], N);
        coastal = pair[cur];
        launches = 1 + passes;
    }
    // the per-cell loop, then the smoothing pass with the normalisation
    float* raw[2] = {T.dev<float>(n), T.dev<float>(n)};
    const TempArgs A{Wb->lat, Wb->lon, e, Wb->cont, Wb->plateCont, Wb->isLand, {Pb->out[0], Pb->out[1]}, {warm[0], warm[1]}, {speed[0], speed[1]}, coastal, {raw[0], raw[1]}};
    launch(p, FAM_CLIMATE, k_temp_cell, g, WO_BLOCK, A, (const float*)itcz, temperatureOffset, N);
    launch(p, FAM_CLIMATE, k_temp_smooth, xg, WO_BLOCK, p->fields(), (const float*)raw[0], (const float*)raw[1], B->out[0], B->out[1]);
    WO_HIP(hipStreamSynchronize(s));                          // before T frees the temporaries
    B->info = wo_temperature_info{passes, Tm::SMOOTH_PASSES, launches + 2, 0};
    B->valid = true; B->have = 3u;
}

}  // namespace wo

using namespace wo;

// the reference's result keys (js/temperature.js:232)
static const char* const kTempFields[2] = {"r_temperature_summer", "r_temperature_winter"};
// the fields of the wind, ocean and precipitation blocks the stages read
static constexpr uint32_t kWindNeeded = (7u << WF_ITCZ0) | (1u << WF_LAT) | (1u << WF_LON) | (1u << WF_ISLAND) | (1u << WF_CONT) | (1u << WF_PLATECONT);
static constexpr uint32_t kOceanNeeded = (1u << 2) | (1u << 3) | (1u << 6) | (1u << 7);      // r_ocean_speed_* and r_ocean_warmth_* of both seasons
static constexpr uint32_t kPrecipNeeded = 3u;                                              // r_precip_summer, r_precip_winter

static int temp_field_index(const char* name) {
    for (int i = 0; i < 2; ++i) if (std::strcmp(name, kTempFields[i]) == 0) return i;
    return -1;
}
static bool precip_ready(const wo_planet* p) { return p->precip && (p->precip->valid || (p->precip->have & kPrecipNeeded) == kPrecipNeeded); }

extern "C" {

int wo_compute_temperature(wo_planet* p, int32_t numRegions, const float* r_elevation, double temperatureOffset, wo_temperature_info* info) {
    if (!check_planet(p, "wo_compute_temperature")) return 1;
    if (numRegions != p->N) { set_error("wo_compute_temperature: numRegions is " + std::to_string(numRegions) + ", the planet has " + std::to_string(p->N)); return 1; }
    if (!(temperatureOffset == temperatureOffset)) { set_error("wo_compute_temperature: temperatureOffset is NaN"); return 1; }
    auto* Wb = p->wind;
    if (!Wb || !(Wb->valid || (Wb->have & kWindNeeded) == kWindNeeded)) {
        set_error("wo_compute_temperature: no wind result on this planet (call wo_compute_wind first, or wo_wind_upload r_lat r_lon r_isLand r_continentality "
                  "r_plateContinentality and the three ITCZ arrays)");
        return 1;
    }
    auto* Ob = p->ocean;
    if (!Ob || !(Ob->valid || (Ob->have & kOceanNeeded) == kOceanNeeded)) {
        set_error("wo_compute_temperature: no ocean result on this planet (call wo_compute_ocean_currents first, or wo_ocean_upload r_ocean_warmth_* and r_ocean_speed_* of both seasons)");
        return 1;
    }
    if (!precip_ready(p)) {
        set_error("wo_compute_temperature: no precipitation result on this planet (call wo_compute_precipitation first, or wo_precip_upload r_precip_summer r_precip_winter)");
        return 1;
    }
    WO_TRY
        temp_alloc(p);
        temp_run(p, r_elevation, temperatureOffset);
        if (info) *info = p->temp->info;
        return 0;
    WO_CATCH("wo_compute_temperature")
}

int wo_temperature_download(wo_planet* p, const char* field, void* out, int64_t outBytes) {
    if (!check_planet(p, "wo_temperature_download")) return 1;
    if (!field || !out) { set_error("wo_temperature_download: null pointer"); return 1; }
    auto* B = p->temp;
    if (!B || !(B->valid || B->have)) { set_error("wo_temperature_download: no temperature result on this planet (call wo_compute_temperature first)"); return 1; }
    const int f = temp_field_index(field);
    if (f < 0) { set_error(std::string("wo_temperature_download: unknown field '") + field + "'"); return 1; }
    if (!B->valid && !((B->have >> f) & 1u)) { set_error(std::string("wo_temperature_download: no temperature result on this planet: ") + field + " was never set (call wo_compute_temperature first)"); return 1; }
    WO_TRY
        const size_t bytes = (size_t)p->N * 4;
        if (outBytes < (int64_t)bytes) { set_error(std::string("wo_temperature_download: ") + field + " needs " + std::to_string(bytes) + " bytes, out has " + std::to_string(outBytes)); return 1; }
        WO_HIP(hipMemcpyAsync(out, B->out[f], bytes, hipMemcpyDeviceToHost, p->ctx->stream));
        WO_HIP(hipStreamSynchronize(p->ctx->stream));
        return 0;
    WO_CATCH("wo_temperature_download")
}

int wo_temperature_upload(wo_planet* p, const char* field, const void* data, int64_t bytes) {
    if (!check_planet(p, "wo_temperature_upload")) return 1;
    if (!field || !data) { set_error("wo_temperature_upload: null pointer"); return 1; }
    const int f = temp_field_index(field);
    if (f < 0) { set_error(std::string("wo_temperature_upload: unknown field '") + field + "'"); return 1; }
    WO_TRY
        const size_t want = (size_t)p->N * 4;
        if (bytes != (int64_t)want) { set_error(std::string("wo_temperature_upload: ") + field + " takes " + std::to_string(want) + " bytes, data has " + std::to_string(bytes)); return 1; }
        temp_alloc(p);
        auto* B = p->temp;
        WO_HIP(hipMemcpyAsync(B->out[f], data, want, hipMemcpyHostToDevice, p->ctx->stream));
        WO_HIP(hipStreamSynchronize(p->ctx->stream));         // `data` is the caller's, and pageable
        B->valid = false; B->have |= 1u << f;
        return 0;
    WO_CATCH("wo_temperature_upload")
}

int wo_classify_koppen(wo_planet* p, int32_t numRegions, const float* r_elevation) {
    if (!check_planet(p, "wo_classify_koppen")) return 1;
    if (numRegions != p->N) { set_error("wo_classify_koppen: numRegions is " + std::to_string(numRegions) + ", the planet has " + std::to_string(p->N)); return 1; }
    auto* Tb = p->temp;
    if (!Tb || !(Tb->valid || Tb->have == 3u)) {
        set_error("wo_classify_koppen: no temperature result on this planet (call wo_compute_temperature first, or wo_temperature_upload r_temperature_summer r_temperature_winter)");
        return 1;
    }
    if (!precip_ready(p)) {
        set_error("wo_classify_koppen: no precipitation result on this planet (call wo_compute_precipitation first, or wo_precip_upload r_precip_summer r_precip_winter)");
        return 1;
    }
    WO_TRY
        koppen_alloc(p);
        auto* K = p->koppen;
        K->valid = false;
        DeviceArena T;
        const float* e = stage_elevation(p, T, r_elevation);
        launch(p, FAM_CLIMATE, k_koppen, blocks_for(p->N), WO_BLOCK, e, (const float*)Tb->out[0], (const float*)Tb->out[1], (const float*)p->precip->out[0],
               (const float*)p->precip->out[1], K->cls, p->N);
        WO_HIP(hipStreamSynchronize(p->ctx->stream));         // before T frees the uploaded elevation
        K->valid = true;
        return 0;
    WO_CATCH("wo_classify_koppen")
}

int wo_koppen_download(wo_planet* p, uint8_t* out, int64_t outBytes) {
    if (!check_planet(p, "wo_koppen_download")) return 1;
    if (!out) { set_error("wo_koppen_download: null pointer"); return 1; }
    auto* K = p->koppen;
    if (!K || !K->valid) { set_error("wo_koppen_download: no Koppen result on this planet (call wo_classify_koppen first)"); return 1; }
    WO_TRY
        if (outBytes < (int64_t)p->N) { set_error("wo_koppen_download: r_koppen needs " + std::to_string(p->N) + " bytes, out has " + std::to_string(outBytes)); return 1; }
        WO_HIP(hipMemcpyAsync(out, K->cls, (size_t)p->N, hipMemcpyDeviceToHost, p->ctx->stream));
        WO_HIP(hipStreamSynchronize(p->ctx->stream));
        return 0;
    WO_CATCH("wo_koppen_download")
}

}  // extern "C"
