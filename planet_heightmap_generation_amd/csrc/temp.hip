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
// single-field kernels of climate_sweeps.hip (k_warmth_seed, k_warmth_diffuse: 2 + 2 x oceanWarmthPasses launches, then k_temp_join);
// the same bits.  Temporaries live in an arena on the call's stack; no host round trip: the stream is waited for once, at the end.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstring>
#include <memory>
#include <string>

#include "../../include/worogen.h"
#include "device.h"
#include "erode_block.h"
#include "ocean_block.h"
#include "precip_block.h"
#include "temp_ops.h"
#include "wind_block.h"

namespace Tm = wo::temp;

namespace wo {
// the fields of the temperature block by the reference's result keys (js/temperature.js:232)
enum TempField : int { TF_SUMMER = 0, TF_WINTER, TF_COUNT };
}  // namespace wo

// the temperature block and the Koppen block of a planet
struct wo_temp_block : wo::StageBlock {                       // have: bit f is out[f]
    float* out[wo::TF_COUNT] = {nullptr, nullptr};            // TempField
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
    float* out[TF_COUNT];
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

const uint8_t* koppen_classes(const wo_planet* p) { return (p->koppen && p->koppen->valid) ? p->koppen->cls : nullptr; }

static void temp_alloc(wo_planet* p) {
    if (p->temp) return;
    std::unique_ptr<wo_temp_block> block(new wo_temp_block());          // the planet gets the block once it is complete
    for (auto& o : block->out) o = block->mem.dev<float>((size_t)p->N);
    p->temp = block.release();
}

static const char* const kTempFields[TF_COUNT] = {"r_temperature_summer", "r_temperature_winter"};
static StageBlock* temp_of(const wo_planet* p) { return p->temp; }
static const BlockDesc kTempBlock{"temperature", "wo_compute_temperature", kTempFields, TF_COUNT, temp_of, temp_alloc, out_slot<wo_temp_block>};
const BlockDesc& temp_desc() { return kTempBlock; }

static void koppen_alloc(wo_planet* p) {
    if (p->koppen) return;
    std::unique_ptr<wo_koppen_block> block(new wo_koppen_block());
    block->cls = block->mem.dev<uint8_t>((size_t)p->N);
    p->koppen = block.release();
}

static void temp_run(wo_planet* p, const float* r_elevation, double temperatureOffset) {
    auto* B = p->temp;
    auto* Wb = p->wind;
    auto* Ob = p->ocean;
    auto* Pb = p->precip;
    const int32_t N = p->N, g = blocks_for(N), tile = xcd_tile(N), xg = xcd_grid(N);
    const size_t n = (size_t)N;
    hipStream_t s = p->ctx->stream;
    B->have = 0;
    const int32_t passes = Tm::warmth_passes(N);
    DeviceArena T;                                            // the temporaries of this call
    float* itcz = T.dev<float>((size_t)2 * W::ITCZ_SAMPLES);
    stage_itcz(p, itcz);
    const float* e = stage_elevation(p, T, r_elevation);
    const float* warm[2] = {Ob->out[ocean_field(0, OF_WARMTH)], Ob->out[ocean_field(1, OF_WARMTH)]};
    const float* speed[2] = {Ob->out[ocean_field(0, OF_SPEED)], Ob->out[ocean_field(1, OF_SPEED)]};
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
    const TempArgs A{Wb->lat, Wb->lon, e, Wb->cont, Wb->plateCont, Wb->isLand, {Pb->out[PF_PRECIP0], Pb->out[PF_PRECIP0 + 1]}, {warm[0], warm[1]}, {speed[0], speed[1]}, coastal, {raw[0], raw[1]}};
    launch(p, FAM_CLIMATE, k_temp_cell, g, WO_BLOCK, A, (const float*)itcz, temperatureOffset, N);
    launch(p, FAM_CLIMATE, k_temp_smooth, xg, WO_BLOCK, fields(p), (const float*)raw[0], (const float*)raw[1], B->out[TF_SUMMER], B->out[TF_WINTER]);
    WO_HIP(hipStreamSynchronize(s));                          // before T frees the temporaries
    B->info = wo_temperature_info{passes, Tm::SMOOTH_PASSES, launches + 2, 0};
    B->have = kTempBlock.all();
}

}  // namespace wo

using namespace wo;

// the fields of the wind, ocean and precipitation blocks the stages read
static constexpr uint32_t kWindForTemp = WF_ITCZ_ALL | bit(WF_LAT) | bit(WF_LON) | bit(WF_ISLAND) | bit(WF_CONT) | bit(WF_PLATECONT);
static constexpr uint32_t kOceanForTemp = ocean_both(OF_SPEED) | ocean_both(OF_WARMTH);      // r_ocean_speed_* and r_ocean_warmth_* of both seasons
static bool precip_ready(const wo_planet* p, const char* fn) { return block_require(p, fn, precip_desc(), PF_PRECIP_BOTH, "wo_precip_upload r_precip_summer r_precip_winter"); }

extern "C" {

int wo_compute_temperature(wo_planet* p, int32_t numRegions, const float* r_elevation, double temperatureOffset, wo_temperature_info* info) {
    if (!check_planet(p, "wo_compute_temperature")) return 1;
    if (numRegions != p->N) { set_error("wo_compute_temperature: numRegions is " + std::to_string(numRegions) + ", the planet has " + std::to_string(p->N)); return 1; }
    if (!(temperatureOffset == temperatureOffset)) { set_error("wo_compute_temperature: temperatureOffset is NaN"); return 1; }
    if (!block_require(p, "wo_compute_temperature", wind_desc(), kWindForTemp, "wo_wind_upload r_lat r_lon r_isLand r_continentality r_plateContinentality and the three ITCZ arrays")) return 1;
    if (!block_require(p, "wo_compute_temperature", ocean_desc(), kOceanForTemp, "wo_ocean_upload r_ocean_warmth_* and r_ocean_speed_* of both seasons")) return 1;
    if (!precip_ready(p, "wo_compute_temperature")) return 1;
    WO_TRY
        temp_alloc(p);
        temp_run(p, r_elevation, temperatureOffset);
        if (info) *info = p->temp->info;
        return 0;
    WO_CATCH("wo_compute_temperature")
}

int wo_temperature_download(wo_planet* p, const char* field, void* out, int64_t outBytes) {
    return block_download(p, "wo_temperature_download", kTempBlock, field, out, outBytes);
}
int wo_temperature_upload(wo_planet* p, const char* field, const void* data, int64_t bytes) { return block_upload(p, "wo_temperature_upload", kTempBlock, field, data, bytes); }

int wo_classify_koppen(wo_planet* p, int32_t numRegions, const float* r_elevation) {
    if (!check_planet(p, "wo_classify_koppen")) return 1;
    if (numRegions != p->N) { set_error("wo_classify_koppen: numRegions is " + std::to_string(numRegions) + ", the planet has " + std::to_string(p->N)); return 1; }
    if (!block_require(p, "wo_classify_koppen", kTempBlock, kTempBlock.all(), "wo_temperature_upload r_temperature_summer r_temperature_winter")) return 1;
    if (!precip_ready(p, "wo_classify_koppen")) return 1;
    auto* Tb = p->temp;
    WO_TRY
        koppen_alloc(p);
        auto* K = p->koppen;
        K->valid = false;
        DeviceArena T;
        const float* e = stage_elevation(p, T, r_elevation);
        launch(p, FAM_CLIMATE, k_koppen, blocks_for(p->N), WO_BLOCK, e, (const float*)Tb->out[TF_SUMMER], (const float*)Tb->out[TF_WINTER], (const float*)p->precip->out[PF_PRECIP0],
               (const float*)p->precip->out[PF_PRECIP0 + 1], K->cls, p->N);
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
