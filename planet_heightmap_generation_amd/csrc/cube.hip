// Cube-map export on the device: the raster of the mesh's sides into the six gnomonic faces of a cube, stacked into one S x 6S
// region map in the planet's map block (map_block.h), where wo_map_color, wo_map_color_layer, wo_map_download, wo_map_free and the
// editor's tints serve it as they serve the equirectangular map.  The per-vertex, per-side and per-pixel bodies and the contract are
// in cube_ops.h; everything runs on the planet's resident positions, on its stream.
//
// Launches of wo_map_raster_cube (no host round trip between them; the stream is waited for once, at the end):
//   k_cube_centers [1]        the centre of every triangle as three f32 (12 bytes; the region positions are the resident d_xyz)
//   k_map_fill [1]            the side map (u32 per pixel) := no side                                                  (map.hip)
//   k_cube_sides [1]          forward rasterisation, one lane per side: for each axis the face in front of which the side's first
//                             vertex lies, the "all ma > 0" test, the projection and the clipped box; a box of at most SMALL_BOX
//                             pixels is walked by the lane itself, atomicMin of the side index into the side map; a larger one is
//                             appended to a list as (side, axis)
//   k_cube_big_boxes [1]      one workgroup per list entry at a time, its threads stride over the box; the grid is fixed and strides
//                             over the list, whose length never comes back to the host
//   k_map_resolve [1]         side -> region (triangles[s], or -1) into the planet's region map, and the covered count   (map.hip)
// The lowest covering side index wins, so the map does not depend on the order in which lanes, workgroups or launches arrive.
// wo_relief_raster_cube (relief.hip) is the same call with a request: after k_map_resolve, while the side map and the centres still
// live, relief_heights_cube adds its height pass.
// Memory (device_mem.h): triangles, half-edges, the centres, the side map and the list are temporaries of the call, in an arena on
// its stack.
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/worogen.h"
#include "cube_ops.h"
#include "device.h"
#include "map_block.h"
#include "view_colors.h"

namespace M = wo::map;
namespace Q = wo::cube;

namespace wo {

constexpr int CUBE_BIG_GRID = 4096;                           // workgroups of k_cube_big_boxes

__global__ __launch_bounds__(WO_BLOCK) void k_cube_centers(const int32_t* __restrict__ triangles, const float* __restrict__ xyz, float* __restrict__ t_xyz, int32_t numTriangles) {
    const int32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= numTriangles) return;
    float c[3];
    M::triangle_center(triangles, xyz, t, c);
    t_xyz[3 * (int64_t)t] = c[0]; t_xyz[3 * (int64_t)t + 1] = c[1]; t_xyz[3 * (int64_t)t + 2] = c[2];
}

// pixel (i, j) of face f takes min(side index) if triangle t covers its centre; the caller's box lies within the face
__device__ inline void cube_cover_pixel(const M::Tri& t, double area2, int32_t S, int32_t f, int32_t i, int32_t j, uint32_t s, uint32_t* sideMap) {
    if (M::tri_covers(t, area2, Q::pixel_c(i, S), Q::pixel_c(j, S))) atomicMin(sideMap + Q::pixel_index(f, i, j, S), s);
}

// the triangle and the box of side vertices v on the face of axis k; false: nothing to draw there
__device__ inline bool cube_side_axis(const float v[3][3], int32_t k, int32_t S, int32_t& f, M::Tri& t, double& area2, M::Box& b) {
    f = Q::face_of_axis(k, v[0][k]);
    if (!Q::side_on_face(v, f, t)) return false;
    area2 = M::tri_area2(t);
    return Q::tri_box(t, area2, S, b);
}

__global__ __launch_bounds__(WO_BLOCK) void k_cube_sides(const int32_t* __restrict__ triangles, const int32_t* __restrict__ halfedges, const float* __restrict__ t_xyz,
                                                         const float* __restrict__ r_xyz, int32_t numSides, int32_t S, uint32_t* sideMap, uint32_t* __restrict__ bigList,
                                                         uint32_t* bigCount) {
    for (int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; s < numSides; s += (int64_t)gridDim.x * blockDim.x) {
        float v[3][3];
        Q::side_vertices(triangles, halfedges, t_xyz, r_xyz, s, v);
        for (int32_t k = 0; k < 3; ++k) {                           // ma > 0 holds on at most one face per axis: that of the first vertex
            int32_t f;
            M::Tri t;
            double area2;
            M::Box b;
            if (!cube_side_axis(v, k, S, f, t, area2, b)) continue;
            if (M::box_pixels(b) > M::SMALL_BOX) {                  // at most one entry per side and axis, 3 * numSides: the list's size
                bigList[atomicAdd(bigCount, 1u)] = (uint32_t)s * 4u + (uint32_t)k;      // numSides < 2^30 (sides_ok)
                continue;
            }
            for (int32_t j = b.j0; j <= b.j1; ++j)
                for (int32_t i = b.i0; i <= b.i1; ++i) cube_cover_pixel(t, area2, S, f, i, j, (uint32_t)s, sideMap);
        }
    }
}

__global__ __launch_bounds__(WO_BLOCK) void k_cube_big_boxes(const int32_t* __restrict__ triangles, const int32_t* __restrict__ halfedges, const float* __restrict__ t_xyz,
                                                             const float* __restrict__ r_xyz, int32_t S, uint32_t* sideMap, const uint32_t* __restrict__ bigList,
                                                             const uint32_t* __restrict__ bigCount) {
    const uint32_t count = *bigCount;
    for (uint32_t e = blockIdx.x; e < count; e += gridDim.x) {
        const uint32_t code = bigList[e], s = code >> 2;
        float v[3][3];
        Q::side_vertices(triangles, halfedges, t_xyz, r_xyz, s, v);
        int32_t f;
        M::Tri t;
        double area2;
        M::Box b;
        if (!cube_side_axis(v, (int32_t)(code & 3u), S, f, t, area2, b)) continue;
        const int64_t bw = b.i1 - b.i0 + 1, n = M::box_pixels(b);
        for (int64_t q = threadIdx.x; q < n; q += blockDim.x) cube_cover_pixel(t, area2, S, f, b.i0 + (int32_t)(q % bw), b.j0 + (int32_t)(q / bw), s, sideMap);
    }
}

}  // namespace wo

using namespace wo;

// wo_map_raster_cube and, with a request, wo_relief_raster_cube
int wo::cube_raster(wo_planet* p, const char* fn, int32_t numSides, const int32_t* triangles, const int32_t* halfedges, int32_t faceSize, int32_t* regionMapOut, int64_t counts[2],
                    const ReliefRequest* relief) {
    const std::string F = std::string(fn) + ": ";
    if (!check_planet(p, fn)) return 1;
    if (!Q::face_size_ok(faceSize)) { set_error(F + "faceSize is " + std::to_string(faceSize) + ", it must be from 1 to 16384"); return 1; }
    if (!sides_ok(fn, p, numSides, triangles, halfedges)) return 1;
    WO_TRY
        const int32_t S = faceSize, numTriangles = numSides / 3;
        const int64_t pixels = (int64_t)Q::FACE_COUNT * S * S;
        hipStream_t s = p->ctx->stream;
        auto* B = map_block_for(p, S, Q::FACE_COUNT * S);
        B->centerLon = 0.0;
        DeviceArena T;                                        // the temporaries of this call
        const int32_t* d_tri = up(T, triangles, (size_t)numSides, s);
        const int32_t* d_he = up(T, halfedges, (size_t)numSides, s);
        float* t_xyz = T.dev<float>(3 * (size_t)numTriangles);
        uint32_t* sideMap = T.dev<uint32_t>((size_t)pixels);
        uint32_t* bigList = T.dev<uint32_t>(3 * (size_t)numSides);
        unsigned long long* d_counts = T.dev<unsigned long long>(2);      // [0] covered pixels, [1] (as u32) the length of bigList
        unsigned long long* h_counts = T.pinned<unsigned long long>(2);
        uint32_t* bigCount = reinterpret_cast<uint32_t*>(d_counts + 1);
        WO_HIP(hipMemsetAsync(d_counts, 0, 16, s));
        launch(p, FAM_CUBE_CENTERS, k_cube_centers, blocks_for(numTriangles), WO_BLOCK, d_tri, (const float*)p->d_xyz, t_xyz, numTriangles);
        launch(p, FAM_CUBE_FILL, k_map_fill, blocks_for(pixels, 1 << 14), WO_BLOCK, sideMap, pixels);
        launch(p, FAM_CUBE_SIDES, k_cube_sides, blocks_for(numSides), WO_BLOCK, d_tri, d_he, (const float*)t_xyz, (const float*)p->d_xyz, numSides, S, sideMap, bigList, bigCount);
        launch(p, FAM_CUBE_BIG_BOXES, k_cube_big_boxes, CUBE_BIG_GRID, WO_BLOCK, d_tri, d_he, (const float*)t_xyz, (const float*)p->d_xyz, S, sideMap, (const uint32_t*)bigList,
               (const uint32_t*)bigCount);
        launch(p, FAM_CUBE_RESOLVE, k_map_resolve, blocks_for(pixels, 1 << 14), WO_BLOCK, (const uint32_t*)sideMap, d_tri, B->region, pixels, d_counts);
        if (relief) relief_heights_cube(p, T, B, *relief, d_tri, d_he, numTriangles, t_xyz, sideMap);
        WO_HIP(hipMemcpyAsync(h_counts, d_counts, 16, hipMemcpyDeviceToHost, s));
        if (regionMapOut) WO_HIP(hipMemcpyAsync(regionMapOut, B->region, (size_t)pixels * 4, hipMemcpyDeviceToHost, s));
        WO_HIP(hipStreamSynchronize(s));                      // before T frees the temporaries
        B->valid = true;
        B->heightValid = relief != nullptr;
        B->heightCube = true;
        if (counts) { counts[0] = (int64_t)h_counts[0]; counts[1] = pixels - (int64_t)h_counts[0]; }
        return 0;
    WO_CATCH(fn)
}

extern "C" {

int wo_map_raster_cube(wo_planet* p, int32_t numSides, const int32_t* triangles, const int32_t* halfedges, int32_t faceSize, int32_t* regionMapOut, int64_t counts[2]) {
    return cube_raster(p, "wo_map_raster_cube", numSides, triangles, halfedges, faceSize, regionMapOut, counts, nullptr);
}

}  // extern "C"
