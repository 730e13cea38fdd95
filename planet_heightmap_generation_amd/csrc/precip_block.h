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
struct wo_precip_block {
    wo::DeviceArena mem;                                      // owns every device and pinned buffer of the block
    bool valid = false;                                       // a whole result of wo_compute_precipitation
    uint32_t have = 0;                                        // bit f: out[f] was set, by wo_compute_precipitation or by wo_precip_upload
    float* out[4] = {nullptr, nullptr, nullptr, nullptr};     // r_precip_summer, r_precip_winter, r_rainshadow_summer, r_rainshadow_winter
    float* itcz = nullptr;                                    // 2 x 360: itczLatsSummer, itczLatsWinter
    wo::PrecipCtl* ctl = nullptr;
    wo::PrecipCtl* h_ctl = nullptr;                           // pinned: the head of ctl
    wo_precip_info info{};
};
