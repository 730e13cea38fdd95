// The wind block of a planet: results and scratch of wo_compute_wind (wind.hip).  The ocean-current stage (ocean.hip) reads
// its results and borrows its scratch, so the block and its field keys live here.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "device.h"
#include "stage_block.h"
#include "wind_ops.h"

struct wo_wind_block : wo::StageBlock {                       // have: bit f is field f of WindField
    // results (device): the eight season arrays, then the per-cell geography
    float* season[2][4] = {{nullptr, nullptr, nullptr, nullptr}, {nullptr, nullptr, nullptr, nullptr}};   // pressure, east, north, speed
    float *lat = nullptr, *lon = nullptr, *sinLat = nullptr, *cosLat = nullptr;
    uint8_t* isLand = nullptr;
    float *cont = nullptr, *plateCont = nullptr;
    int32_t* coastDist = nullptr;
    float* frame[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    float itcz[3][wo::wind::ITCZ_SAMPLES];                    // host: itczLons, itczLatsSummer, itczLatsWinter
    // scratch
    float *e = nullptr, *tmpA = nullptr, *tmpB = nullptr, *gradE = nullptr, *gradN = nullptr;
    int32_t *label = nullptr, *compSize = nullptr, *plateDist = nullptr, *plate = nullptr, *oceanIds = nullptr; int64_t oceanIdCap = 0; int32_t nOceanIds = 0;   // ascending ocean plate ids: capacity, count in use
    uint8_t* plateOcean = nullptr;
    uint32_t* keys[2] = {nullptr, nullptr}; int32_t* vals[2] = {nullptr, nullptr}; uint32_t* sortScratch = nullptr; int sortFlip = 0;
    int32_t* binOffset = nullptr;
    int32_t* frontier[2] = {nullptr, nullptr}; int32_t* counts = nullptr;      // 3 rotating frontier lengths
    unsigned long long* mainKey = nullptr;
    wo::wind::SampleSpec* specs = nullptr; wo::wind::SampleAcc* acc = nullptr; wo::wind::Spline* splines = nullptr;
    uint32_t* selHist = nullptr; wo::wind::SelState* selState = nullptr; float* maxSpeed = nullptr;
    // pinned host
    wo::wind::SampleAcc* h_acc = nullptr; int32_t* h_count = nullptr;
    int32_t bfsLevels[2] = {0, 0};
};

namespace wo {

// the fields of the block by the reference's result keys, in the order it sets them (js/wind.js:649-683)
enum WindField : int { WF_SEASON0 = 0, WF_ITCZ0 = 8, WF_LAT = 11, WF_LON, WF_SINLAT, WF_ISLAND, WF_CONT, WF_COASTDIST, WF_PLATECONT, WF_FRAME0, WF_COUNT = WF_FRAME0 + 6 };
// a season's four fields: WF_SEASON0 + WS_STRIDE * season + one of these
enum WindSeasonField : int { WS_PRESSURE = 0, WS_EAST, WS_NORTH, WS_SPEED, WS_STRIDE };
constexpr uint32_t wind_both(int f) { return bit(WF_SEASON0 + f) | bit(WF_SEASON0 + WS_STRIDE + f); }      // field f of both seasons
constexpr uint32_t WF_ITCZ_ALL = 7u << WF_ITCZ0;              // itczLons, itczLatsSummer, itczLatsWinter
const BlockDesc& wind_desc();                                 // wind.hip: the block's descriptor

// wind.hip: allocates the planet's wind block if there is none
void wind_alloc(wo_planet* p);
// wind.hip: computeGradients (js/wind.js:306-339) of a device-resident field
void gradient_resident(wo_planet* p, const float* field, const wind::Frames& T, float* gradE, float* gradN);

}  // namespace wo
