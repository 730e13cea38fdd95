// The precipitation block of a planet: the results of wo_compute_precipitation (precip.hip).  The temperature stage and the Koppen
// classification (temp.hip) read its two precipitation fields, so the block and its control words live here.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "../../include/worogen.h"
#include "device.h"
#include "ocean_block.h"

namespace wo {
// what the kernels of a call share; cleared at its start.  The head (up to sel) comes back to the host at its end.
struct PrecipCtl {
    uint32_t lists[4];                                        // members of the upwind, downwind lists of summer, then of winter
    uint32_t cells[2];                                        // values that enter the percentile: N, N
    float p95[2];                                             // maxPrecip
    W::SelState sel[2];
    uint32_t hist[2][W::SEL_PASSES][W::SEL_BINS];
};
constexpr size_t PRECIP_CTL_HEAD = offsetof(PrecipCtl, sel);
__device__ inline uint32_t sel_count(const PrecipCtl* c, int season) { return c->cells[season]; }
}  // namespace wo

// the precipitation block of a planet
struct wo_precip_block : wo::StageBlock {                     // have: bit f is out[f]
    float* out[4] = {nullptr, nullptr, nullptr, nullptr};     // PrecipField
    float* itcz = nullptr;                                    // 2 x 360: itczLatsSummer, itczLatsWinter
    wo::PrecipCtl* ctl = nullptr;
    wo::PrecipCtl* h_ctl = nullptr;                           // pinned: the head of ctl
    wo_precip_info info{};
};

namespace wo {
// the fields of the block by the reference's result keys (js/precipitation.js:640-641, :678); + season
enum PrecipField : int { PF_PRECIP0 = 0, PF_SHADOW0 = 2, PF_COUNT = 4 };
constexpr uint32_t PF_PRECIP_BOTH = bit(PF_PRECIP0) | bit(PF_PRECIP0 + 1);      // r_precip_summer, r_precip_winter
const BlockDesc& precip_desc();                               // precip.hip: the block's descriptor
}  // namespace wo
