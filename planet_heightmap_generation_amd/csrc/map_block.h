// The map block of a planet and the one raster (raster.hip) that the equirectangular export (map.hip), the cube-map export
// (cube.hip) and the globe view (view.hip) run: all leave a W x H region map in the same block, so that the colouring, the download
// and wo_map_free serve any of them.  The relief export (relief.hip) is the same raster with a request, which adds a height map of
// the same shape to the block; the globe view adds a depth map and, with a shading request, a Lambert map.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <functional>

#include "device.h"

struct wo_map_block {
    wo::DeviceArena mem;
    int32_t* region = nullptr;                                // W x H region ids, row 0 first; -1: nothing covers the pixel
    int32_t W = 0, H = 0;                                     // equirectangular: H = W / 2; cube map: the six faces stacked, H = 6 W; view: any
    double centerLon = 0.0;                                   // the centre meridian of the raster (wo_map_raster, wo_map_raster_cube: 0)
    bool valid = false;
    // the relief: W x H interpolated elevations (f32; NaN: nothing covers the pixel), allocated by the block's first relief raster;
    // valid only while the region map is the one that raster left
    float* height = nullptr;
    bool heightValid = false, heightCube = false;
    // the globe view: W x H depths (f32; NaN: nothing covers the pixel) and Lambert terms (f32), allocated by the block's first view
    // raster and its first shaded one; `view`, the background word and, with lambertValid, the two shading weights hold only while
    // the region map is the one a view raster left: a map or cube raster clears them
    float *depth = nullptr, *lambert = nullptr;
    bool view = false, lambertValid = false;
    uint32_t background = 0;
    double ambient = 0.0, diffuse = 0.0;
};

namespace wo {

// map.hip: the planet's map block at W x H, marked invalid until the raster completes: the one it has when both sizes agree, else a
// new one (the old map goes first; the planet gets the new block once it is complete)
WO_LOCAL wo_map_block* map_block_for(wo_planet* p, int32_t W, int32_t H);

// A relief raster's request to the raster below: the elevation to interpolate (the caller's host pointer, NULL: the resident field)
// and where the height map goes on the host (may be NULL)
struct ReliefRequest { const float* r_elevation; float* heightOut; };

// What tells one raster from another, next to its projection P (map::Projection, cube::Projection): the block's shape and centre
// meridian, whether a height map left in the block is a cube's, the profiling families of the four shared launches, and the
// projection's vertex tables: `tables` allocates them in the call's arena and returns the projection, `launchTables` launches their
// kernels (in a family of its own) from the uploaded triangles.  Two steps, because every allocation of a raster comes before its
// first launch: the stream does not wait for the allocator between two launches.
template <class P> struct RasterKind {
    int32_t W, H;
    double centerLon;
    bool heightCube;
    int famFill, famSides, famBigBoxes, famResolve;
    std::function<P(DeviceArena& T)> tables;
    std::function<void(const int32_t* d_tri)> launchTables;
    // a projection whose word is no side index resolves its side map itself (into B->region and the covered count d_counts[0], in
    // famResolve); whatever it allocates, it allocates in `tables`
    std::function<void(const P& proj, const typename P::Word* sideMap, const int32_t* d_tri, const int32_t* d_he, wo_map_block* B, unsigned long long* d_counts)> resolve = nullptr;
};

// raster.hip: the body of every raster entry point, under the entry point's name, after the checks of its own arguments: the checks
// of the sides, the uploads, the tables, fill, sides, big boxes and resolve into the block, the counts.  With a request, the height
// pass runs after the resolve, while the side map and the tables still live (map and cube only).  Instantiated for the three
// projections.
template <class P>
WO_LOCAL int raster(wo_planet* p, const char* fn, int32_t numSides, const int32_t* triangles, const int32_t* halfedges, const RasterKind<P>& kind, int32_t* regionMapOut,
                    int64_t counts[2], const ReliefRequest* relief);

// relief.hip: the height pass into B->height on the planet's stream (T: the raster's arena, for the triangle elevations and the
// caller's field); the raster marks the height map valid once the stream has been waited for.  Instantiated for the two projections.
template <class P>
WO_LOCAL void relief_heights(wo_planet* p, DeviceArena& T, wo_map_block* B, const ReliefRequest& q, const P& proj, const int32_t* d_tri, const int32_t* d_he, int32_t numTriangles,
                             const uint32_t* sideMap);

// view.hip: the shade pass of a view block with a valid Lambert map over rgba (W x H words on the device), on the planet's stream
WO_LOCAL void view_shade(wo_planet* p, const wo_map_block* B, uint32_t* rgba);

}  // namespace wo
