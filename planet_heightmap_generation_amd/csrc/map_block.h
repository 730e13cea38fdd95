// The map block of a planet and the two raster launches that the equirectangular export (map.hip) and the cube-map export (cube.hip)
// share: both leave a W x H region map in the same block, so that the colouring, the download and wo_map_free serve either.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "device.h"

struct wo_map_block {
    wo::DeviceArena mem;
    int32_t* region = nullptr;                                // W x H region ids, row 0 first; -1: nothing covers the pixel
    int32_t W = 0, H = 0;                                     // equirectangular: H = W / 2; cube map: the six faces stacked, H = 6 W
    double centerLon = 0.0;                                   // the centre meridian of the raster (wo_map_raster, wo_map_raster_cube: 0)
    bool valid = false;
};

namespace wo {

// map.hip: the planet's map block at W x H, marked invalid until the raster completes: the one it has when both sizes agree, else a
// new one (the old map goes first; the planet gets the new block once it is complete)
WO_LOCAL wo_map_block* map_block_for(wo_planet* p, int32_t W, int32_t H);

// map.hip: the side map (u32 per pixel) := no side
__global__ void k_map_fill(uint32_t* __restrict__ sideMap, int64_t pixels);
// map.hip: side -> region (triangles[s], or -1) and counts[0] += covered pixels
__global__ void k_map_resolve(const uint32_t* __restrict__ sideMap, const int32_t* __restrict__ triangles, int32_t* __restrict__ region, int64_t pixels, unsigned long long* counts);

}  // namespace wo
