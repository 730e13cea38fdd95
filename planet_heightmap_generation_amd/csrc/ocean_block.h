// The ocean block of a planet: results and scratch of wo_compute_ocean_currents (ocean.hip).  The precipitation stage (precip.hip)
// reads its two warmth fields and shares its histogram-and-pick selection of a percentile, so the block, the control words and
// the two selection kernels live here.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "../../include/worogen.h"
#include "device.h"
#include "ocean_ops.h"
#include "stage_block.h"

namespace O = wo::ocean;
namespace W = wo::wind;

namespace wo {
// what the kernels of a call share; cleared at its start.  The head (up to p95) comes back to the host at its end.
struct OceanCtl {
    int32_t counts[3];                                        // rotating frontier lengths
    uint32_t oceanCells[2];                                   // ocean speeds > 0 per season
    uint32_t circ[2];                                         // circumpolarNH, circumpolarSH
    float p95[2];
    uint32_t bins[2 * O::CIRC_BINS];
    W::SelState sel[2];
    uint32_t hist[2][W::SEL_PASSES][W::SEL_BINS];             // season, pass: no pass clears another's counters
};
constexpr size_t OCEAN_CTL_HEAD = offsetof(OceanCtl, bins);
}  // namespace wo

// the ocean block of a planet
struct wo_ocean_block : wo::StageBlock {                      // have: bit f is out[f]
    float* out[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};   // OceanField: per season east, north, speed, warmth
    uint8_t* isOcean = nullptr;
    void* group[2] = {nullptr, nullptr};                      // 16 bytes per cell each: frontiers (2 N entries), float4 currents, float2 warmths
    float* itcz = nullptr;                                    // 2 x 360: itczLatsSummer, itczLatsWinter
    wo::OceanCtl* ctl = nullptr;
    wo::OceanCtl* h_ctl = nullptr;                            // pinned: the head of ctl
    wo_ocean_info info{};
};
namespace wo {

// the fields of the block by the reference's result keys, in the order it sets them (js/ocean.js:374-377): summer's four, then winter's
enum OceanField : int { OF_EAST = 0, OF_NORTH, OF_SPEED, OF_WARMTH, OF_STRIDE, OF_COUNT = 2 * OF_STRIDE };
constexpr int ocean_field(int season, int f) { return OF_STRIDE * season + f; }
constexpr uint32_t ocean_both(int f) { return bit(ocean_field(0, f)) | bit(ocean_field(1, f)); }      // field f of both seasons
const BlockDesc& ocean_desc();                                // ocean.hip: the block's descriptor

// ocean.hip: allocates the planet's ocean block if there is none
void ocean_alloc(wo_planet* p);

// the cell of a thread under the XCD-aware tiling of the index-order passes (common_kernels.h: WO_XCD_CELLS); grid: xcd_grid(N)
__device__ inline int32_t ocean_xcd_cell(int32_t tile) {
    const int32_t xi = (int32_t)(blockIdx.x >> 3);
    return (((xi / tile) * 8 + (int32_t)(blockIdx.x & 7u)) * tile + (xi % tile)) * (int32_t)blockDim.x + (int32_t)threadIdx.x;
}

__device__ inline uint32_t sel_count(const OceanCtl* c, int season) { return c->oceanCells[season]; }

// The percentile of two fields at once (summer, winter) by a three-digit histogram select (wind_ops.h: sel_*).  Ctl brings
// sel[2], hist[2][SEL_PASSES][SEL_BINS], p95[2] and sel_count(ctl, season), the number of values that take part.
// Histogram of one digit over the values that agree with the digits already chosen; even workgroups take summer, odd ones
// winter.  mask != nullptr: only cells with mask[r] set and a value > 0 take part (the ocean speeds); nullptr: every cell.
template <class Ctl>
__global__ __launch_bounds__(WO_BLOCK) void k_ocean_sel_hist(const float* __restrict__ spS, const float* __restrict__ spW, const uint8_t* __restrict__ mask, int32_t N,
                                                             int32_t pass, Ctl* ctl) {
    __shared__ uint32_t s[W::SEL_BINS];
    const int season = blockIdx.x & 1;
    const float* __restrict__ v = season ? spW : spS;
    for (int i = threadIdx.x; i < W::SEL_BINS; i += blockDim.x) s[i] = 0;
    __syncthreads();
    const uint32_t prefix = ctl->sel[season].prefix;
    for (int32_t r = (blockIdx.x >> 1) * blockDim.x + threadIdx.x; r < N; r += (gridDim.x >> 1) * blockDim.x) {
        const float x = v[r];
        if (mask && !(mask[r] && x > 0.0f)) continue;
        const uint32_t key = W::sel_key(x);
        if (W::sel_matches(key, prefix, pass)) atomicAdd(&s[W::sel_digit(key, pass)], 1u);
    }
    __syncthreads();
    uint32_t* hist = ctl->hist[season][pass];
    for (int i = threadIdx.x; i < W::SEL_BINS; i += blockDim.x) if (s[i]) atomicAdd(&hist[i], s[i]);
}
// one wave per season chooses the digit (wind_ops.h: sel_pick, the counters scanned by the 64 lanes); pass 0 takes the rank
// from the count, the last pass leaves the percentile
template <class Ctl>
__global__ __launch_bounds__(64) void k_ocean_sel_pick(Ctl* ctl, int32_t pass) {
    const int season = blockIdx.x, lane = threadIdx.x;
    const uint32_t* hist = ctl->hist[season][pass];
    const uint32_t count = sel_count(ctl, season);
    W::SelState S = ctl->sel[season];
    if (pass == 0) { S.prefix = 0u; S.k = O::percentile_rank(count); }
    const int bins = pass == 2 ? 1024 : W::SEL_BINS, per = bins / 64, lo = lane * per;
    uint32_t sum = 0;
    for (int d = lo; d < lo + per; ++d) sum += hist[d];
    uint32_t incl = sum;
    for (int o = 1; o < 64; o <<= 1) { const uint32_t up = __shfl_up(incl, o); if (lane >= o) incl += up; }
    const unsigned long long over = __ballot(incl > S.k);
    const int owner = over ? __ffsll((long long)over) - 1 : 63;   // the lane whose counters hold the rank (none: the last digit, as sel_pick's loop ends)
    if (lane == owner) {
        uint32_t k = S.k - (incl - sum);
        int d = lo;
        for (; d < bins - 1; ++d) { if (k < hist[d]) break; k -= hist[d]; }
        S.prefix |= (uint32_t)d << W::sel_shift(pass);
        S.k = k;
        ctl->sel[season] = S;
        if (pass == W::SEL_PASSES - 1) ctl->p95[season] = O::p95_of(count, S.prefix);
    }
}
}  // namespace wo
