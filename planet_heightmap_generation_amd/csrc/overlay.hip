// The arrow overlays on the device (the reference's buildWindArrows and buildOceanCurrentArrows, js/planet-mesh.js:1289-1465,
// :1545-1720): per 3 x 3 degree bin the region closest to its centre, and for the bins that are kept the arrow the reference draws,
// on the globe and on the map.  The bodies and the contract are in overlay_ops.h; everything runs on the planet's resident
// positions, elevation, wind block and ocean block, on its stream.
//
// Launches of wo_overlay_bins / wo_overlay_arrows:
//   k_overlay_bins [1]      one lane per region in the planet's own index order: the bin and d2 in double (fdlibm's asin and atan2),
//                           the 64-bit key of overlay_ops.h, one atomicMin into the bin's word.  The atomic returns nothing, so a
//                           lane does not wait for it.  The test hook overlay_precheck=1 reads the word first (a relaxed load) and
//                           leaves the atomic out when its own key is not below it; a stale read can only be too high, which costs
//                           an atomic and never a result: the same minimum, the same bits, but every lane then waits for a load
//                           from L2, and the form measured three times slower (the A/B of DESIGN section 8.12).
//   k_overlay_winners [1]   the keys as region ids (wo_overlay_bins only)
//   k_overlay_arrows [1]    one workgroup walks the 7200 bins in ascending order, 256 at a time: block_ops.h's block_place gives every
//                           kept bin its place, and its lane writes the four runs of 18 floats there
// Memory (device_mem.h): everything is a temporary of the call, in an arena on its stack.
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/worogen.h"
#include "block_ops.h"
#include "device.h"
#include "ocean_block.h"
#include "overlay_ops.h"
#include "stage_block.h"
#include "wind_block.h"

namespace V = wo::overlay;

static_assert(V::KIND_WIND == WO_OVERLAY_WIND && V::KIND_OCEAN == WO_OVERLAY_OCEAN, "the kinds of overlay_ops.h are those of worogen.h");
static_assert(V::BINS == WO_OVERLAY_BINS, "the bin count of overlay_ops.h is that of worogen.h");

namespace wo {

// keys: BINS words, filled with EMPTY_KEY; e is read with skipLand only
template <bool PRECHECK>
__global__ __launch_bounds__(WO_BLOCK) void k_overlay_bins(const float* __restrict__ xyz, const float* __restrict__ e, int32_t skipLand, int32_t N, unsigned long long* __restrict__ keys) {
    const int32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= N) return;
    if (skipLand && !V::takes_part(true, e[r])) return;
    const V::Bin b = V::bin_of(xyz[3 * (int64_t)r], xyz[3 * (int64_t)r + 1], xyz[3 * (int64_t)r + 2]);
    if (b.idx < 0 || b.idx >= V::BINS) return;
    const unsigned long long key = V::key_of(b.d2, r);
    if (key == V::EMPTY_KEY) return;
    if (PRECHECK && key >= __hip_atomic_load(keys + b.idx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return;
    atomicMin(keys + b.idx, key);
}

__global__ __launch_bounds__(WO_BLOCK) void k_overlay_winners(const unsigned long long* __restrict__ keys, int32_t* __restrict__ out) {
    const int32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < V::BINS) out[i] = V::winner_of_key(keys[i]);
}

// One workgroup.  a, b: the vector's two fields; speed, warmth: the ocean form's (nullptr for the wind).  Each output holds BINS arrows or is nullptr.
__global__ __launch_bounds__(WO_BLOCK) void k_overlay_arrows(int32_t kind, const unsigned long long* __restrict__ keys, const float* __restrict__ xyz, const float* __restrict__ a,
                                                             const float* __restrict__ b, const float* __restrict__ speed, const float* __restrict__ warmth, double centerLon,
                                                             float* __restrict__ globePos, float* __restrict__ globeCol, float* __restrict__ mapPos, float* __restrict__ mapCol,
                                                             int32_t* __restrict__ total) {
    __shared__ int32_t waveCount[BLOCK_WAVES];
    int32_t base = 0;
    for (int32_t first = 0; first < V::BINS; first += WO_BLOCK) {
        const int32_t i = first + (int32_t)threadIdx.x;
        const int32_t r = i < V::BINS ? V::winner_of_key(keys[i]) : -1;
        V::Source src{0.0f, 0.0f, 0.0f, 0.0f};
        bool keep = false;
        if (r >= 0) {
            src.a = a[r]; src.b = b[r];
            if (kind == V::KIND_OCEAN) { src.speed = speed[r]; src.warmth = warmth[r]; }
            keep = !V::is_slow(kind, V::speed_of(kind, src));
        }
        const BlockPlace at = block_place(keep, waveCount);
        if (keep) {
            const float p[3] = {xyz[3 * (int64_t)r], xyz[3 * (int64_t)r + 1], xyz[3 * (int64_t)r + 2]};
            const int64_t o = (int64_t)(base + at.place) * V::ARROW_FLOATS;      // base + place < BINS: at most one arrow per bin
            V::arrow(kind, p, src, centerLon, globePos ? globePos + o : nullptr, globeCol ? globeCol + o : nullptr, mapPos ? mapPos + o : nullptr, mapCol ? mapCol + o : nullptr);
        }
        base += at.total;
        __syncthreads();                                      // waveCount is free again
    }
    if (threadIdx.x == 0) *total = base;
}

// the keys of every bin into a fresh buffer of T
static unsigned long long* overlay_keys(wo_planet* p, DeviceArena& T, bool skipLand, const float* e) {
    hipStream_t s = p->ctx->stream;
    unsigned long long* keys = T.dev<unsigned long long>((size_t)V::BINS);
    WO_HIP(hipMemsetAsync(keys, 0xFF, (size_t)V::BINS * 8, s));
    auto* kernel = p->opt.overlayPrecheck ? k_overlay_bins<true> : k_overlay_bins<false>;
    launch(p, FAM_OVERLAY_BINS, kernel, blocks_for(p->N, 1 << 23), WO_BLOCK, (const float*)p->d_xyz, e, (int32_t)skipLand, p->N, keys);
    return keys;
}

}  // namespace wo

using namespace wo;

extern "C" {

int wo_overlay_bins(wo_planet* p, int32_t skipLand, const float* r_elevation, int32_t* gridRegionsOut) {
    const char* fn = "wo_overlay_bins";
    const std::string F = "wo_overlay_bins: ";
    if (!check_planet(p, fn)) return 1;
    if (!gridRegionsOut) { set_error(F + "null pointer"); return 1; }
    if (skipLand != 0 && skipLand != 1) { set_error(F + "skipLand is " + std::to_string(skipLand) + ", it must be 0 or 1"); return 1; }
    WO_TRY
        hipStream_t s = p->ctx->stream;
        DeviceArena T;                                        // the temporaries of this call
        const float* e = skipLand ? stage_elevation(p, T, r_elevation) : nullptr;
        const unsigned long long* keys = overlay_keys(p, T, skipLand != 0, e);
        int32_t* winners = T.dev<int32_t>((size_t)V::BINS);
        launch(p, FAM_OVERLAY_ARROWS, k_overlay_winners, blocks_for(V::BINS), WO_BLOCK, keys, winners);
        WO_HIP(hipMemcpyAsync(gridRegionsOut, winners, (size_t)V::BINS * 4, hipMemcpyDeviceToHost, s));
        WO_HIP(hipStreamSynchronize(s));                      // before T frees the temporaries
        return 0;
    WO_CATCH("wo_overlay_bins")
}

int wo_overlay_arrows(wo_planet* p, int32_t kind, int32_t season, double centerLon, const float* r_elevation, float* globePos, float* globeCol, float* mapPos, float* mapCol,
                      int64_t capacityArrows, int64_t* count) {
    const char* fn = "wo_overlay_arrows";
    const std::string F = "wo_overlay_arrows: ";
    if (!check_planet(p, fn)) return 1;
    if (!count) { set_error(F + "null pointer"); return 1; }
    if (kind != V::KIND_WIND && kind != V::KIND_OCEAN) { set_error(F + "unknown arrow kind " + std::to_string(kind)); return 1; }
    if (season != 0 && season != 1) { set_error(F + "unknown season " + std::to_string(season) + " (0 is summer, 1 is winter)"); return 1; }
    const bool ocean = kind == V::KIND_OCEAN, any = globePos || globeCol || mapPos || mapCol;
    if (any && capacityArrows < V::BINS) { set_error(F + "the grid can give " + std::to_string(V::BINS) + " arrows, capacityArrows is " + std::to_string(capacityArrows)); return 1; }
    static const char* const windKeys[2][2] = {{"r_wind_east_summer", "r_wind_north_summer"}, {"r_wind_east_winter", "r_wind_north_winter"}};
    static const char* const oceanKeys[2][4] = {{"r_ocean_current_east_summer", "r_ocean_current_north_summer", "r_ocean_speed_summer", "r_ocean_warmth_summer"},
                                                {"r_ocean_current_east_winter", "r_ocean_current_north_winter", "r_ocean_speed_winter", "r_ocean_warmth_winter"}};
    static const char* const hints[2][2] = {{"wo_wind_upload r_wind_east_summer r_wind_north_summer", "wo_wind_upload r_wind_east_winter r_wind_north_winter"},
                                            {"wo_ocean_upload r_ocean_current_east_summer r_ocean_current_north_summer r_ocean_speed_summer r_ocean_warmth_summer",
                                             "wo_ocean_upload r_ocean_current_east_winter r_ocean_current_north_winter r_ocean_speed_winter r_ocean_warmth_winter"}};
    const BlockDesc& D = ocean ? ocean_desc() : wind_desc();
    const int fields = ocean ? 4 : 2;
    int f[4] = {-1, -1, -1, -1};
    uint32_t needed = 0;
    for (int k = 0; k < fields; ++k) { f[k] = D.index(ocean ? oceanKeys[season][k] : windKeys[season][k]); needed |= bit(f[k]); }
    if (!block_require(p, fn, D, needed, hints[ocean][season])) return 1;
    WO_TRY
        const size_t N = (size_t)p->N;
        hipStream_t s = p->ctx->stream;
        DeviceArena T;                                        // the temporaries of this call
        const float* e = ocean ? stage_elevation(p, T, r_elevation) : nullptr;
        const float* src[4] = {nullptr, nullptr, nullptr, nullptr};
        for (int k = 0; k < fields; ++k) src[k] = (const float*)D.slot(D.get(p), f[k], N).ptr;
        const unsigned long long* keys = overlay_keys(p, T, ocean, e);
        const size_t room = (size_t)V::BINS * V::ARROW_FLOATS;
        float* host[4] = {globePos, globeCol, mapPos, mapCol};
        float* dev[4] = {nullptr, nullptr, nullptr, nullptr};
        for (int k = 0; k < 4; ++k) if (host[k]) dev[k] = T.dev<float>(room);
        int32_t* d_total = T.dev<int32_t>(1);
        int32_t* h_total = T.pinned<int32_t>(1);
        launch(p, FAM_OVERLAY_ARROWS, k_overlay_arrows, 1, WO_BLOCK, kind, keys, (const float*)p->d_xyz, src[0], src[1], src[2], src[3], centerLon, dev[0], dev[1], dev[2], dev[3], d_total);
        WO_HIP(hipMemcpyAsync(h_total, d_total, 4, hipMemcpyDeviceToHost, s));
        WO_HIP(hipStreamSynchronize(s));
        const int64_t n = *h_total;
        if (n > 0 && any) {
            for (int k = 0; k < 4; ++k) if (host[k]) WO_HIP(hipMemcpyAsync(host[k], dev[k], (size_t)n * V::ARROW_FLOATS * 4, hipMemcpyDeviceToHost, s));
            WO_HIP(hipStreamSynchronize(s));                  // before T frees the temporaries
        }
        *count = n;
        return 0;
    WO_CATCH("wo_overlay_arrows")
}

}  // extern "C"
