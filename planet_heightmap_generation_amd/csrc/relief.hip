// Relief export on the device: a smooth height per pixel of the equirectangular map or of the cube map, its 16-bit encoding and the
// normals of the displaced surface.  The per-pixel bodies and the contract are in relief_ops.h.
//
// wo_relief_raster (map.hip) and wo_relief_raster_cube (cube.hip) run the raster of raster.hip launch for launch, so the region map
// and its counts are those of wo_map_raster_centered and wo_map_raster_cube; after k_map_resolve, while the side map and the
// projection's tables still live, relief_heights adds
//   k_relief_tri_elevation [1]   the elevation of every triangle centre (globe::triangle_elevation), 4 bytes per triangle
//   k_relief_heights<P> [1]      one pixel per thread: the side from the side map, its triangle rebuilt with the very functions the
//                                raster used, the interpolated elevation into the block's height map (f32 per pixel).  Bound by its
//                                gathers, as k_raster_sides is: three vertex records and three elevations per pixel.
// wo_relief_height16: k_relief_height16 [1], the height map to u16, four pixels per thread.
// wo_relief_normals: k_relief_tables [1] for the map (cos / sin of every row's latitude and every column's longitude), then
//   k_relief_normals_map or k_relief_normals_cube [1], a stencil over the height map: five height loads per pixel, a 4-byte store.
// Memory (device_mem.h): the height map lives in the planet's map block (map_block.h), allocated by the block's first relief raster
// and dropped with the block; the triangle elevations, an uploaded field, the tables and the outputs are temporaries of the call.
// All pixel and byte offsets are 64-bit.
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/worogen.h"
#include "device.h"
#include "map_block.h"
#include "relief_ops.h"
#include "stage_block.h"

static_assert(wo::relief::KIND_HEIGHT == WO_RELIEF_HEIGHT && wo::relief::KIND_LAND_HEIGHT == WO_RELIEF_LAND_HEIGHT, "the kinds of relief_ops.h are those of worogen.h");
static_assert(wo::relief::SPACE_TANGENT == WO_RELIEF_NORMAL_TANGENT && wo::relief::SPACE_OBJECT == WO_RELIEF_NORMAL_OBJECT, "the spaces of relief_ops.h are those of worogen.h");
static_assert(wo::relief::FLAG_FLAT_OCEAN == WO_RELIEF_FLAT_OCEAN, "the flags of relief_ops.h are those of worogen.h");

namespace M = wo::map;
namespace Q = wo::cube;
namespace R = wo::relief;

namespace wo {

__global__ __launch_bounds__(WO_BLOCK) void k_relief_tri_elevation(const int32_t* __restrict__ triangles, const float* __restrict__ r_elevation, float* __restrict__ t_elevation,
                                                                   int32_t numTriangles) {
    const int32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < numTriangles) t_elevation[t] = globe::triangle_elevation(triangles, r_elevation, t);
}

template <class P>
__global__ __launch_bounds__(WO_BLOCK) void k_relief_heights(const P proj, const uint32_t* __restrict__ sideMap, const int32_t* __restrict__ triangles,
                                                             const int32_t* __restrict__ halfedges, const float* __restrict__ t_elevation, const float* __restrict__ r_elevation,
                                                             float* __restrict__ heights) {
    const int64_t pixels = proj.pixels();
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < pixels; q += (int64_t)gridDim.x * blockDim.x) {
        const uint32_t s = sideMap[q];
        heights[q] = s == M::NO_SIDE ? R::quiet_nan() : R::pixel_height(proj, triangles, halfedges, t_elevation, r_elevation, s, q);
    }
}

// four pixels per thread: one 16-byte load, one 8-byte store
__global__ __launch_bounds__(WO_BLOCK) void k_relief_height16(const float* __restrict__ heights, int32_t kind, uint16_t* __restrict__ out, int64_t pixels) {
    const int64_t groups = (pixels + 3) / 4;
    for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < groups; g += (int64_t)gridDim.x * blockDim.x) {
        const int64_t i = 4 * g;
        if (i + 3 < pixels) {
            const float4 h = *reinterpret_cast<const float4*>(heights + i);
            uint2 o;
            o.x = (uint32_t)R::height16(kind, h.x) | ((uint32_t)R::height16(kind, h.y) << 16);
            o.y = (uint32_t)R::height16(kind, h.z) | ((uint32_t)R::height16(kind, h.w) << 16);
            *reinterpret_cast<uint2*>(out + i) = o;
        } else {
            for (int64_t k = i; k < pixels; ++k) out[k] = R::height16(kind, heights[k]);
        }
    }
}

// rows[j], j < H, and cols[i], i < W
__global__ __launch_bounds__(WO_BLOCK) void k_relief_tables(R::RowDir* __restrict__ rows, R::ColDir* __restrict__ cols, int32_t W, int32_t H, double centerLon) {
    const int32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k < H) rows[k] = R::map_row(k, H);
    else if (k < H + W) cols[k - H] = R::map_col(k - H, W, centerLon);
}

__global__ __launch_bounds__(WO_BLOCK) void k_relief_normals_map(const float* __restrict__ heights, const R::RowDir* __restrict__ rows, const R::ColDir* __restrict__ cols, int32_t W,
                                                                 int32_t H, int32_t space, double strength, int32_t flags, uint32_t* __restrict__ out) {
    const int64_t pixels = (int64_t)W * H;
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < pixels; q += (int64_t)gridDim.x * blockDim.x)
        out[q] = R::map_pixel_normal(heights, rows, cols, W, H, (int32_t)(q % W), (int32_t)(q / W), space, strength, flags);
}

__global__ __launch_bounds__(WO_BLOCK) void k_relief_normals_cube(const float* __restrict__ heights, int32_t S, int32_t space, double strength, int32_t flags,
                                                                  uint32_t* __restrict__ out) {
    const int64_t face = (int64_t)S * S, pixels = Q::FACE_COUNT * face;
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < pixels; q += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = q % face;
        out[q] = R::cube_pixel_normal(heights, S, (int32_t)(q / face), (int32_t)(r % S), (int32_t)(r / S), space, strength, flags);
    }
}

template <class P>
void relief_heights(wo_planet* p, DeviceArena& T, wo_map_block* B, const ReliefRequest& q, const P& proj, const int32_t* d_tri, const int32_t* d_he, int32_t numTriangles,
                    const uint32_t* sideMap) {
    if (!B->height) B->height = B->mem.dev<float>((size_t)B->W * (size_t)B->H);
    const float* r_elevation = stage_elevation(p, T, q.r_elevation);
    float* t_elevation = T.dev<float>((size_t)numTriangles);
    launch(p, FAM_RELIEF_TRI_ELEVATION, k_relief_tri_elevation, blocks_for(numTriangles), WO_BLOCK, d_tri, r_elevation, t_elevation, numTriangles);
    launch(p, FAM_RELIEF_HEIGHTS, k_relief_heights<P>, blocks_for((int64_t)B->W * B->H, 1 << 16), WO_BLOCK, proj, sideMap, d_tri, d_he, (const float*)t_elevation, r_elevation,
           B->height);
    if (q.heightOut) WO_HIP(hipMemcpyAsync(q.heightOut, B->height, (size_t)B->W * (size_t)B->H * 4, hipMemcpyDeviceToHost, p->ctx->stream));
}

template void relief_heights(wo_planet*, DeviceArena&, wo_map_block*, const ReliefRequest&, const M::Projection&, const int32_t*, const int32_t*, int32_t, const uint32_t*);
template void relief_heights(wo_planet*, DeviceArena&, wo_map_block*, const ReliefRequest&, const Q::Projection&, const int32_t*, const int32_t*, int32_t, const uint32_t*);

}  // namespace wo

using namespace wo;

// the block with a valid height map, or nullptr with the error set; outBytes must be pixels * bytesPerPixel
static wo_map_block* relief_block(wo_planet* p, const char* fn, const void* out, int64_t outBytes, int64_t bytesPerPixel) {
    const std::string F = std::string(fn) + ": ";
    if (!out) { set_error(F + "null pointer"); return nullptr; }
    auto* B = p->map;
    if (!B || !B->valid || !B->heightValid) { set_error(F + "no relief raster on this planet (call wo_relief_raster or wo_relief_raster_cube first)"); return nullptr; }
    const int64_t bytes = (int64_t)B->W * B->H * bytesPerPixel;
    if (outBytes != bytes) { set_error(F + "a " + std::to_string(B->W) + " x " + std::to_string(B->H) + " map takes " + std::to_string(bytes) + " bytes, out has " + std::to_string(outBytes)); return nullptr; }
    return B;
}

extern "C" {

int wo_relief_download(wo_planet* p, float* out, int64_t outBytes) {
    const char* fn = "wo_relief_download";
    if (!check_planet(p, fn)) return 1;
    auto* B = relief_block(p, fn, out, outBytes, 4);
    if (!B) return 1;
    WO_TRY
        WO_HIP(hipMemcpyAsync(out, B->height, (size_t)outBytes, hipMemcpyDeviceToHost, p->ctx->stream));
        WO_HIP(hipStreamSynchronize(p->ctx->stream));
        return 0;
    WO_CATCH(fn)
}

int wo_relief_height16(wo_planet* p, int32_t kind, uint16_t* out, int64_t outBytes) {
    const char* fn = "wo_relief_height16";
    if (!check_planet(p, fn)) return 1;
    if (!R::kind_ok(kind)) { set_error(std::string(fn) + ": unknown kind " + std::to_string(kind)); return 1; }
    auto* B = relief_block(p, fn, out, outBytes, 2);
    if (!B) return 1;
    WO_TRY
        const int64_t pixels = (int64_t)B->W * B->H;
        hipStream_t s = p->ctx->stream;
        DeviceArena T;                                        // the temporaries of this call
        uint16_t* d_out = T.dev<uint16_t>((size_t)pixels);
        launch(p, FAM_RELIEF_HEIGHT16, k_relief_height16, blocks_for((pixels + 3) / 4, 1 << 14), WO_BLOCK, (const float*)B->height, kind, d_out, pixels);
        WO_HIP(hipMemcpyAsync(out, d_out, (size_t)outBytes, hipMemcpyDeviceToHost, s));
        WO_HIP(hipStreamSynchronize(s));                      // before T frees the temporaries
        return 0;
    WO_CATCH(fn)
}

int wo_relief_normals(wo_planet* p, int32_t space, double strength, int32_t flags, uint8_t* rgbaOut, int64_t outBytes) {
    const char* fn = "wo_relief_normals";
    const std::string F = std::string(fn) + ": ";
    if (!check_planet(p, fn)) return 1;
    if (!R::space_ok(space)) { set_error(F + "unknown space " + std::to_string(space)); return 1; }
    if (!R::strength_ok(strength)) { set_error(F + "strength is " + std::to_string(strength) + ", it must be finite and not negative"); return 1; }
    if (!R::flags_ok(flags)) { set_error(F + "unknown flags " + std::to_string(flags)); return 1; }
    auto* B = relief_block(p, fn, rgbaOut, outBytes, 4);
    if (!B) return 1;
    WO_TRY
        const int64_t pixels = (int64_t)B->W * B->H;
        hipStream_t s = p->ctx->stream;
        DeviceArena T;                                        // the temporaries of this call
        uint32_t* d_out = T.dev<uint32_t>((size_t)pixels);
        if (B->heightCube) {
            launch(p, FAM_RELIEF_NORMALS, k_relief_normals_cube, blocks_for(pixels, 1 << 16), WO_BLOCK, (const float*)B->height, B->W, space, strength, flags, d_out);
        } else {
            R::RowDir* rows = T.dev<R::RowDir>((size_t)B->H);
            R::ColDir* cols = T.dev<R::ColDir>((size_t)B->W);
            launch(p, FAM_RELIEF_TABLES, k_relief_tables, blocks_for((int64_t)B->W + B->H), WO_BLOCK, rows, cols, B->W, B->H, B->centerLon);
            launch(p, FAM_RELIEF_NORMALS, k_relief_normals_map, blocks_for(pixels, 1 << 16), WO_BLOCK, (const float*)B->height, (const R::RowDir*)rows, (const R::ColDir*)cols, B->W, B->H,
                   space, strength, flags, d_out);
        }
        WO_HIP(hipMemcpyAsync(rgbaOut, d_out, (size_t)outBytes, hipMemcpyDeviceToHost, s));
        WO_HIP(hipStreamSynchronize(s));                      // before T frees the temporaries
        return 0;
    WO_CATCH(fn)
}

}  // extern "C"
