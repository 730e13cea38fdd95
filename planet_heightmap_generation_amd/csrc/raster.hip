// The raster of the mesh's sides into a region map, once for every projection: the equirectangular map (map.hip, map::Projection of
// map_ops.h), the six gnomonic faces of the cube map (cube.hip, cube::Projection of cube_ops.h) and the globe seen through a camera
// (view.hip, view::Projection of view_ops.h).  A projection says how a side becomes at most PIECES triangles, where a pixel lies and
// which word (P::Word) a side leaves under a minimum at a pixel it covers: its index for the map and the cube (u32), a (depth, side)
// key for the camera (u64), which has several sides per pixel.  The loop, the list, the driver and the contract of the coverage
// (map_ops.h) are the same.  Everything runs on the planet's stream.
//
// Launches of a raster (no host round trip between them; the stream is waited for once, at the end), in the caller's families:
//   the tables [1-2]          the caller's own kernels: what the projection reads per vertex
//   k_map_fill [1]            the side map (one word per pixel) := no side
//   k_raster_sides [1]        forward rasterisation, one lane per side: each piece's triangle and clipped box; a box of at most
//                             SMALL_BOX pixels is walked by the lane itself, atomicMin of the side's word into the side map; a larger
//                             one (the pole fan, the triangles at region N, the seam: thousands of pixels wide) is appended to a list
//                             as side * 4 + piece (numSides < 2^30: sides_ok)
//   k_raster_big_boxes [1]    one workgroup per list entry at a time, its threads stride over the box; the grid is fixed and strides
//                             over the list, whose length never comes back to the host
//   k_map_resolve [1]         side -> region (triangles[s], or -1) into the planet's region map, and the covered / uncovered counts
//                             (block_ops.h: block_add_to_global); the camera's own (view.hip: k_view_resolve) also writes depth and Lambert
//   the height pass [2]       with a relief request only (relief.hip: relief_heights), while the side map and the tables still live
// The lowest word wins, so the map does not depend on the order in which lanes, workgroups or launches arrive.
// Memory (device_mem.h): the region map lives in the planet's map block (map_block.h); triangles, half-edges, the tables, the side
// map and the list are temporaries of the call, in an arena on its stack.
#include <hip/hip_runtime.h>

#include "block_ops.h"
#include "cube_ops.h"
#include "device.h"
#include "map_block.h"
#include "map_ops.h"
#include "view_colors.h"
#include "view_ops.h"

#include <type_traits>

namespace M = wo::map;

namespace wo {

constexpr int BIG_GRID = 4096;                                // workgroups of k_raster_big_boxes

template <class Word>
__global__ __launch_bounds__(WO_BLOCK) void k_map_fill(Word* __restrict__ sideMap, int64_t pixels) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < pixels; i += (int64_t)gridDim.x * blockDim.x) sideMap[i] = ~(Word)0;      // NO_SIDE, view::NO_KEY
}

// pixel (i, j) of face f takes min(side s's word) if triangle t covers its centre; the caller's box lies within the map or the face
template <class P>
__device__ inline void raster_cover_pixel(const P& proj, const typename P::Side& v, const M::Tri& t, double area2, int32_t f, int32_t i, int32_t j, uint32_t s,
                                          typename P::Word* sideMap) {
    double xc, yc;
    proj.center(i, j, xc, yc);
    if (M::tri_covers(t, area2, xc, yc)) atomicMin(sideMap + proj.index(f, i, j), proj.word(v, t, area2, xc, yc, s));
}

template <class P>
__global__ __launch_bounds__(WO_BLOCK) void k_raster_sides(const P proj, const int32_t* __restrict__ triangles, const int32_t* __restrict__ halfedges, int32_t numSides,
                                                           typename P::Word* sideMap, uint32_t* __restrict__ bigList, uint32_t* bigCount) {
    for (int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; s < numSides; s += (int64_t)gridDim.x * blockDim.x) {
        typename P::Side v;
        const int n = proj.vertices(triangles, halfedges, s, v);
        for (int k = 0; k < n; ++k) {
            M::Tri t;
            double area2;
            M::Box b;
            int32_t f;
            if (!proj.piece(v, k, t, area2, b, f)) continue;
            if (M::box_pixels(b) > M::SMALL_BOX) {                  // at most one entry per side and piece: the list's size
                bigList[atomicAdd(bigCount, 1u)] = (uint32_t)s * 4u + (uint32_t)k;
                continue;
            }
            for (int32_t j = b.j0; j <= b.j1; ++j)
                for (int32_t i = b.i0; i <= b.i1; ++i) raster_cover_pixel(proj, v, t, area2, f, i, j, (uint32_t)s, sideMap);
        }
    }
}

template <class P>
__global__ __launch_bounds__(WO_BLOCK) void k_raster_big_boxes(const P proj, const int32_t* __restrict__ triangles, const int32_t* __restrict__ halfedges, typename P::Word* sideMap,
                                                               const uint32_t* __restrict__ bigList, const uint32_t* __restrict__ bigCount) {
    const uint32_t count = *bigCount;
    for (uint32_t e = blockIdx.x; e < count; e += gridDim.x) {
        const uint32_t code = bigList[e], s = code >> 2;
        typename P::Side v;
        proj.vertices(triangles, halfedges, s, v);
        M::Tri t;
        double area2;
        M::Box b;
        int32_t f;
        if (!proj.piece(v, (int)(code & 3u), t, area2, b, f)) continue;
        const int64_t bw = b.i1 - b.i0 + 1, n = M::box_pixels(b);
        for (int64_t q = threadIdx.x; q < n; q += blockDim.x) raster_cover_pixel(proj, v, t, area2, f, b.i0 + (int32_t)(q % bw), b.j0 + (int32_t)(q / bw), s, sideMap);
    }
}

// counts[0] += covered pixels
__global__ __launch_bounds__(WO_BLOCK) void k_map_resolve(const uint32_t* __restrict__ sideMap, const int32_t* __restrict__ triangles, int32_t* __restrict__ region,
                                                          int64_t pixels, unsigned long long* counts) {
    __shared__ unsigned long long blockCovered[1];
    if (threadIdx.x == 0) blockCovered[0] = 0;
    __syncthreads();
    unsigned long long covered[1] = {0};
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < pixels; i += (int64_t)gridDim.x * blockDim.x) {
        const uint32_t s = sideMap[i];
        region[i] = s == M::NO_SIDE ? -1 : triangles[s];
        covered[0] += s != M::NO_SIDE;
    }
    block_add_to_global<1>(covered, blockCovered, counts);
}

template <class P>
int raster(wo_planet* p, const char* fn, int32_t numSides, const int32_t* triangles, const int32_t* halfedges, const RasterKind<P>& kind, int32_t* regionMapOut, int64_t counts[2],
           const ReliefRequest* relief) {
    if (!sides_ok(fn, p, numSides, triangles, halfedges)) return 1;
    WO_TRY
        const int32_t numTriangles = numSides / 3;
        const int64_t pixels = (int64_t)kind.W * kind.H;
        hipStream_t s = p->ctx->stream;
        auto* B = map_block_for(p, kind.W, kind.H);
        B->centerLon = kind.centerLon;
        DeviceArena T;                                        // the temporaries of this call
        const int32_t* d_tri = up(T, triangles, (size_t)numSides, s);
        const int32_t* d_he = up(T, halfedges, (size_t)numSides, s);
        using Word = typename P::Word;
        const P proj = kind.tables(T);
        Word* sideMap = T.dev<Word>((size_t)pixels);
        uint32_t* bigList = T.dev<uint32_t>((size_t)P::PIECES * (size_t)numSides);
        unsigned long long* d_counts = T.dev<unsigned long long>(2);      // [0] covered pixels, [1] (as u32) the length of bigList
        unsigned long long* h_counts = T.pinned<unsigned long long>(2);
        uint32_t* bigCount = reinterpret_cast<uint32_t*>(d_counts + 1);
        WO_HIP(hipMemsetAsync(d_counts, 0, 16, s));
        kind.launchTables(d_tri);
        launch(p, kind.famFill, k_map_fill<Word>, blocks_for(pixels, 1 << 14), WO_BLOCK, sideMap, pixels);
        launch(p, kind.famSides, k_raster_sides<P>, blocks_for(numSides), WO_BLOCK, proj, d_tri, d_he, numSides, sideMap, bigList, bigCount);
        launch(p, kind.famBigBoxes, k_raster_big_boxes<P>, BIG_GRID, WO_BLOCK, proj, d_tri, d_he, sideMap, (const uint32_t*)bigList, (const uint32_t*)bigCount);
        if constexpr (std::is_same_v<Word, uint32_t>) {
            launch(p, kind.famResolve, k_map_resolve, blocks_for(pixels, 1 << 14), WO_BLOCK, (const uint32_t*)sideMap, d_tri, B->region, pixels, d_counts);
            if (relief) relief_heights(p, T, B, *relief, proj, d_tri, d_he, numTriangles, (const uint32_t*)sideMap);
        } else {
            kind.resolve(proj, (const Word*)sideMap, d_tri, d_he, B, d_counts);      // the projection's own, in famResolve
        }
        WO_HIP(hipMemcpyAsync(h_counts, d_counts, 16, hipMemcpyDeviceToHost, s));
        if (regionMapOut) WO_HIP(hipMemcpyAsync(regionMapOut, B->region, (size_t)pixels * 4, hipMemcpyDeviceToHost, s));
        WO_HIP(hipStreamSynchronize(s));                      // before T frees the temporaries
        B->valid = true;
        B->heightValid = relief != nullptr;
        B->heightCube = kind.heightCube;
        if (counts) { counts[0] = (int64_t)h_counts[0]; counts[1] = pixels - (int64_t)h_counts[0]; }
        return 0;
    WO_CATCH(fn)
}

template int raster(wo_planet*, const char*, int32_t, const int32_t*, const int32_t*, const RasterKind<map::Projection>&, int32_t*, int64_t*, const ReliefRequest*);
template int raster(wo_planet*, const char*, int32_t, const int32_t*, const int32_t*, const RasterKind<cube::Projection>&, int32_t*, int64_t*, const ReliefRequest*);
template int raster(wo_planet*, const char*, int32_t, const int32_t*, const int32_t*, const RasterKind<view::Projection>&, int32_t*, int64_t*, const ReliefRequest*);

}  // namespace wo
