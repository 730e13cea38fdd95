// Cube-map export on the device: the raster of the mesh's sides into the six gnomonic faces of a cube, stacked into one S x 6S
// region map in the planet's map block (map_block.h), where wo_map_color, wo_map_color_layer, wo_map_download, wo_map_free and the
// editor's tints serve it as they serve the equirectangular map.  The per-vertex, per-side and per-pixel bodies and the contract are
// in cube_ops.h; everything runs on the planet's resident positions, on its stream.
//
// wo_map_raster_cube is the raster of raster.hip (its launches are listed there) under cube::Projection, in the cube_* families,
// with one table:
//   k_cube_centers [1]        the centre of every triangle as three f32 (12 bytes; the region positions are the resident d_xyz)
// wo_relief_raster_cube is the same call with a request: after k_map_resolve, while the side map and the centres still live,
// relief_heights (relief.hip) adds its height pass.
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/worogen.h"
#include "cube_ops.h"
#include "device.h"
#include "map_block.h"

namespace M = wo::map;
namespace Q = wo::cube;

namespace wo {

__global__ __launch_bounds__(WO_BLOCK) void k_cube_centers(const int32_t* __restrict__ triangles, const float* __restrict__ xyz, float* __restrict__ t_xyz, int32_t numTriangles) {
    const int32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= numTriangles) return;
    float c[3];
    M::triangle_center(triangles, xyz, t, c);
    t_xyz[3 * (int64_t)t] = c[0]; t_xyz[3 * (int64_t)t + 1] = c[1]; t_xyz[3 * (int64_t)t + 2] = c[2];
}

}  // namespace wo

using namespace wo;

// wo_map_raster_cube and, with a request, wo_relief_raster_cube: the check of the face size, and the raster of raster.hip with the
// cube's table and families
static int faces_raster(wo_planet* p, const char* fn, int32_t numSides, const int32_t* triangles, const int32_t* halfedges, int32_t faceSize, int32_t* regionMapOut,
                        int64_t counts[2], const ReliefRequest* relief) {
    if (!check_planet(p, fn)) return 1;
    if (!Q::face_size_ok(faceSize)) { set_error(std::string(fn) + ": faceSize is " + std::to_string(faceSize) + ", it must be from 1 to 16384"); return 1; }
    const int32_t S = faceSize, numTriangles = numSides / 3;
    float* t_xyz = nullptr;
    const auto tables = [&](DeviceArena& T) {
        t_xyz = T.dev<float>(3 * (size_t)numTriangles);
        return Q::Projection{t_xyz, (const float*)p->d_xyz, S};
    };
    const auto launchTables = [&](const int32_t* d_tri) {
        launch(p, FAM_CUBE_CENTERS, k_cube_centers, blocks_for(numTriangles), WO_BLOCK, d_tri, (const float*)p->d_xyz, t_xyz, numTriangles);
    };
    return raster<Q::Projection>(p, fn, numSides, triangles, halfedges,
                                 {S, Q::FACE_COUNT * S, 0.0, true, FAM_CUBE_FILL, FAM_CUBE_SIDES, FAM_CUBE_BIG_BOXES, FAM_CUBE_RESOLVE, tables, launchTables}, regionMapOut, counts,
                                 relief);
}

extern "C" {

int wo_map_raster_cube(wo_planet* p, int32_t numSides, const int32_t* triangles, const int32_t* halfedges, int32_t faceSize, int32_t* regionMapOut, int64_t counts[2]) {
    return faces_raster(p, "wo_map_raster_cube", numSides, triangles, halfedges, faceSize, regionMapOut, counts, nullptr);
}

int wo_relief_raster_cube(wo_planet* p, int32_t numSides, const int32_t* triangles, const int32_t* halfedges, int32_t faceSize, const float* r_elevation, float* heightOut,
                          int64_t counts[2]) {
    const ReliefRequest q{r_elevation, heightOut};
    return faces_raster(p, "wo_relief_raster_cube", numSides, triangles, halfedges, faceSize, nullptr, counts, &q);
}

}  // extern "C"
