// The map block of a planet and the two raster launches that the equirectangular export (map.hip) and the cube-map export (cube.hip)
// share: both leave a W x H region map in the same block, so that the colouring, the download and wo_map_free serve either.  The
// relief export (relief.hip) runs the same two rasters and adds a height map of the same shape to the block.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "device.h"
#include "map_ops.h"

struct wo_map_block {
    wo::DeviceArena mem;
    int32_t* region = nullptr;                                // W x H region ids, row 0 first; -1: nothing covers the pixel
    int32_t W = 0, H = 0;                                     // equirectangular: H = W / 2; cube map: the six faces stacked, H = 6 W
    double centerLon = 0.0;                                   // the centre meridian of the raster (wo_map_raster, wo_map_raster_cube: 0)
    bool valid = false;
    // the relief: W x H interpolated elevations (f32; NaN: nothing covers the pixel), allocated by the block's first relief raster;
    // valid only while the region map is the one that raster left
    float* height = nullptr;
    bool heightValid = false, heightCube = false;
};

namespace wo {

// map.hip: the planet's map block at W x H, marked invalid until the raster completes: the one it has when both sizes agree, else a
// new one (the old map goes first; the planet gets the new block once it is complete)
WO_LOCAL wo_map_block* map_block_for(wo_planet* p, int32_t W, int32_t H);

// map.hip: the side map (u32 per pixel) := no side
__global__ void k_map_fill(uint32_t* __restrict__ sideMap, int64_t pixels);
// map.hip: side -> region (triangles[s], or -1) and counts[0] += covered pixels
__global__ void k_map_resolve(const uint32_t* __restrict__ sideMap, const int32_t* __restrict__ triangles, int32_t* __restrict__ region, int64_t pixels, unsigned long long* counts);

// A relief raster's request to the two rasters below: the elevation to interpolate (the caller's host pointer, NULL: the resident
// field) and where the height map goes on the host (may be NULL)
struct ReliefRequest { const float* r_elevation; float* heightOut; };

// map.hip, cube.hip: the bodies of wo_map_raster / wo_map_raster_centered and of wo_map_raster_cube under the entry point's name;
// with a request, the height pass of relief.hip runs after k_map_resolve, while the side map and the vertex tables still live
WO_LOCAL int map_raster(wo_planet* p, const char* fn, int32_t numSides, const int32_t* triangles, const int32_t* halfedges, int32_t width, bool centered, double centerLon,
                        int32_t* regionMapOut, int64_t counts[2], const ReliefRequest* relief);
WO_LOCAL int cube_raster(wo_planet* p, const char* fn, int32_t numSides, const int32_t* triangles, const int32_t* halfedges, int32_t faceSize, int32_t* regionMapOut,
                         int64_t counts[2], const ReliefRequest* relief);

// relief.hip: the height pass into B->height on the planet's stream (T: the raster's arena, for the triangle elevations and the
// caller's field); the raster marks the height map valid once the stream has been waited for
WO_LOCAL void relief_heights_map(wo_planet* p, DeviceArena& T, wo_map_block* B, const ReliefRequest& q, const int32_t* d_tri, const int32_t* d_he, int32_t numTriangles,
                                 const map::LonLat* t_ll, const map::LonLat* r_ll, const uint32_t* sideMap);
WO_LOCAL void relief_heights_cube(wo_planet* p, DeviceArena& T, wo_map_block* B, const ReliefRequest& q, const int32_t* d_tri, const int32_t* d_he, int32_t numTriangles,
                                  const float* t_xyz, const uint32_t* sideMap);

}  // namespace wo
