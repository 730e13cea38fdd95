// Equirectangular map export on the device (the reference's exportMap / exportMapBatch, js/planet-mesh.js:1752-2180): the raster
// of the mesh's map triangles into a region map, and the colouring of that map into RGBA8 in the reference's six kinds.  The
// per-vertex, per-side, per-pixel and per-region bodies and the contract are in map_ops.h; everything runs on the planet's
// resident positions, elevation and Koppen block, on its stream.
//
// Launches of wo_map_raster (no host round trip between them; the stream is waited for once, at the end):
//   k_map_region_lonlat [1]   longitude and latitude of every region, one thread each
//   k_map_center_lonlat [1]   the same of every triangle centre: 3 N evaluations of atan2 / asin in all, not 18 N
//   k_map_fill [1]            the side map (u32 per pixel) := no side
//   k_map_sides [1]           forward rasterisation, one lane per side: the side's one or two triangles; a pixel box of at most
//                             SMALL_BOX pixels is walked by the lane itself, atomicMin of the side index into the side map; a
//                             larger one (the pole fan, the triangles at region N, the seam: thousands of pixels wide) is appended
//                             to a list
//   k_map_big_boxes [1]       one workgroup per listed triangle at a time, its threads stride over the box; the grid is fixed and
//                             strides over the list, whose length never comes back to the host
//   k_map_resolve [1]         side -> region (triangles[s], or -1) into the planet's region map, and the covered / uncovered counts
//                             (block_ops.h: block_add_to_global)
// The lowest covering side index wins, so the map does not depend on the order in which lanes, workgroups or launches arrive.
// Launches of wo_map_color and wo_map_color_layer: the region colours of view_colors.hip, one packed RGBA per region [1-2], then
// k_map_pixels [1] (region map -> RGBA8, four pixels per thread).
// wo_map_raster_centered is the same raster around a centre meridian (the map view's, map_layer_ops.h): the two table kernels take
// centerLon (k_map_region_lonlat_centered, k_map_center_lonlat_centered), every other launch is wo_map_raster's.
// wo_relief_raster (relief.hip) is wo_map_raster_centered with a request: after k_map_resolve, while the side map and the two tables
// still live, relief_heights_map adds its height pass; the launches above are the same and so are the region map and the counts.
// Memory (device_mem.h): the region map lives in a block with an arena of its own on the planet (map_block.h; int32 per pixel; a
// raster at another width or height, wo_map_raster_cube's included, replaces it, wo_map_free and wo_planet_destroy drop it);
// triangles, half-edges, both longitude / latitude tables, the side map, the list and the colour tables are temporaries of the call,
// in an arena on its stack.
#include <hip/hip_runtime.h>

#include <memory>
#include <string>

#include "../../include/worogen.h"
#include "block_ops.h"
#include "device.h"
#include "map_block.h"
#include "map_layer_ops.h"
#include "map_ops.h"
#include "rivers_block.h"
#include "stage_block.h"
#include "view_colors.h"

static_assert(wo::map::LAYER_COUNT == WO_MAP_LAYER_COUNT && wo::map::LAYER_WINDSPEED_WINTER == WO_MAP_LAYER_WINDSPEED_WINTER, "the layers of map_layer_ops.h are those of worogen.h");

namespace M = wo::map;

namespace wo {

constexpr int MAP_BIG_GRID = 4096;                            // workgroups of k_map_big_boxes

__global__ __launch_bounds__(WO_BLOCK) void k_map_region_lonlat(const float* __restrict__ xyz, M::LonLat* __restrict__ out, int32_t N) {
    const int32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r < N) out[r] = M::lonlat_of(xyz[3 * (int64_t)r], xyz[3 * (int64_t)r + 1], xyz[3 * (int64_t)r + 2]);
}

__global__ __launch_bounds__(WO_BLOCK) void k_map_center_lonlat(const int32_t* __restrict__ triangles, const float* __restrict__ xyz, M::LonLat* __restrict__ out,
                                                                int32_t numTriangles) {
    const int32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < numTriangles) out[t] = M::lonlat_of_center(triangles, xyz, t);
}

// the same two tables around a centre meridian
__global__ __launch_bounds__(WO_BLOCK) void k_map_region_lonlat_centered(const float* __restrict__ xyz, M::LonLat* __restrict__ out, int32_t N, double centerLon) {
    const int32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r < N) out[r] = M::lonlat_of_centered(xyz[3 * (int64_t)r], xyz[3 * (int64_t)r + 1], xyz[3 * (int64_t)r + 2], centerLon);
}
__global__ __launch_bounds__(WO_BLOCK) void k_map_center_lonlat_centered(const int32_t* __restrict__ triangles, const float* __restrict__ xyz, M::LonLat* __restrict__ out,
                                                                         int32_t numTriangles, double centerLon) {
    const int32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < numTriangles) out[t] = M::lonlat_of_center_centered(triangles, xyz, t, centerLon);
}

__global__ __launch_bounds__(WO_BLOCK) void k_map_fill(uint32_t* __restrict__ sideMap, int64_t pixels) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < pixels; i += (int64_t)gridDim.x * blockDim.x) sideMap[i] = M::NO_SIDE;
}

// the pixels of box b that triangle t covers take min(side index)
__device__ inline void map_cover_pixel(const M::Tri& t, double area2, int32_t W, int32_t H, int32_t i, int32_t j, uint32_t s, uint32_t* sideMap) {
    if (M::tri_covers(t, area2, M::pixel_xc(i, W), M::pixel_yc(j, H))) atomicMin(sideMap + ((int64_t)j * W + i), s);
}

__global__ __launch_bounds__(WO_BLOCK) void k_map_sides(const int32_t* __restrict__ triangles, const int32_t* __restrict__ halfedges, const M::LonLat* __restrict__ t_ll,
                                                        const M::LonLat* __restrict__ r_ll, int32_t numSides, int32_t W, int32_t H, uint32_t* sideMap,
                                                        uint32_t* __restrict__ bigList, uint32_t* bigCount) {
    for (int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; s < numSides; s += (int64_t)gridDim.x * blockDim.x) {
        M::LonLat v[3];
        M::side_vertices(triangles, halfedges, t_ll, r_ll, s, v);
        M::Tri tri[2];
        const int n = M::side_triangles(v, tri);
        for (int k = 0; k < n; ++k) {
            const double area2 = M::tri_area2(tri[k]);
            M::Box b;
            if (!M::tri_box(tri[k], area2, W, H, b)) continue;
            if (M::box_pixels(b) > M::SMALL_BOX) {                  // at most 2 * numSides entries: the list's size
                bigList[atomicAdd(bigCount, 1u)] = (uint32_t)s * 2u + (uint32_t)k;
                continue;
            }
            for (int32_t j = b.j0; j <= b.j1; ++j)
                for (int32_t i = b.i0; i <= b.i1; ++i) map_cover_pixel(tri[k], area2, W, H, i, j, (uint32_t)s, sideMap);
        }
    }
}

__global__ __launch_bounds__(WO_BLOCK) void k_map_big_boxes(const int32_t* __restrict__ triangles, const int32_t* __restrict__ halfedges, const M::LonLat* __restrict__ t_ll,
                                                            const M::LonLat* __restrict__ r_ll, int32_t W, int32_t H, uint32_t* sideMap,
                                                            const uint32_t* __restrict__ bigList, const uint32_t* __restrict__ bigCount) {
    const uint32_t count = *bigCount;
    for (uint32_t e = blockIdx.x; e < count; e += gridDim.x) {
        const uint32_t code = bigList[e], s = code >> 1;
        M::LonLat v[3];
        M::side_vertices(triangles, halfedges, t_ll, r_ll, s, v);
        M::Tri tri[2];
        M::side_triangles(v, tri);
        const M::Tri& t = tri[code & 1u];
        const double area2 = M::tri_area2(t);
        M::Box b;
        if (!M::tri_box(t, area2, W, H, b)) continue;
        const int64_t bw = b.i1 - b.i0 + 1, n = M::box_pixels(b);
        for (int64_t q = threadIdx.x; q < n; q += blockDim.x)
            map_cover_pixel(t, area2, W, H, b.i0 + (int32_t)(q % bw), b.j0 + (int32_t)(q / bw), s, sideMap);
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

// four pixels per thread: one 16-byte load of region ids, four gathers from the colour table, one 16-byte store
__global__ __launch_bounds__(WO_BLOCK) void k_map_pixels(const int32_t* __restrict__ region, const uint32_t* __restrict__ regionRgba, uint32_t background,
                                                         uint32_t* __restrict__ out, int64_t pixels) {
    const int64_t groups = (pixels + 3) / 4;
    for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < groups; g += (int64_t)gridDim.x * blockDim.x) {
        const int64_t i = 4 * g;
        if (i + 3 < pixels) {
            const int4 r = *reinterpret_cast<const int4*>(region + i);
            uint4 c;
            c.x = r.x < 0 ? background : regionRgba[r.x];
            c.y = r.y < 0 ? background : regionRgba[r.y];
            c.z = r.z < 0 ? background : regionRgba[r.z];
            c.w = r.w < 0 ? background : regionRgba[r.w];
            *reinterpret_cast<uint4*>(out + i) = c;
        } else {
            for (int64_t k = i; k < pixels; ++k) out[k] = region[k] < 0 ? background : regionRgba[region[k]];
        }
    }
}

void map_free(wo_planet* p) { delete p->map; p->map = nullptr; }

wo_map_block* map_block_for(wo_planet* p, int32_t W, int32_t H) {
    if (!p->map || p->map->W != W || p->map->H != H) {        // a cube block of face size 64 is no 64 x 32 map
        map_free(p);
        std::unique_ptr<wo_map_block> block(new wo_map_block());
        block->region = block->mem.dev<int32_t>((size_t)W * (size_t)H);
        block->W = W; block->H = H;
        p->map = block.release();
    }
    p->map->valid = p->map->heightValid = false;             // any raster, through any entry point, ends the relief of the last
    return p->map;
}

static bool map_width_ok(int32_t width) { return width >= 2 && width <= 32768 && (width & 1) == 0; }

}  // namespace wo

using namespace wo;

// wo_map_raster (centered == false: its own two table kernels), wo_map_raster_centered and, with a request, wo_relief_raster
int wo::map_raster(wo_planet* p, const char* fn, int32_t numSides, const int32_t* triangles, const int32_t* halfedges, int32_t width, bool centered, double centerLon,
                   int32_t* regionMapOut, int64_t counts[2], const ReliefRequest* relief) {
    const std::string F = std::string(fn) + ": ";
    if (!check_planet(p, fn)) return 1;
    if (!map_width_ok(width)) { set_error(F + "width is " + std::to_string(width) + ", it must be even and from 2 to 32768"); return 1; }
    if (centered && !M::center_lon_ok(centerLon)) { set_error(F + "centerLon is " + std::to_string(centerLon) + ", it must be finite and from -pi to pi"); return 1; }
    if (!sides_ok(fn, p, numSides, triangles, halfedges)) return 1;
    WO_TRY
        const int32_t W = width, H = width / 2, N = p->N, numTriangles = numSides / 3;
        const int64_t pixels = (int64_t)W * H;
        hipStream_t s = p->ctx->stream;
        auto* B = map_block_for(p, W, H);
        B->centerLon = centered ? centerLon : 0.0;
        DeviceArena T;                                        // the temporaries of this call
        const int32_t* d_tri = up(T, triangles, (size_t)numSides, s);
        const int32_t* d_he = up(T, halfedges, (size_t)numSides, s);
        M::LonLat* r_ll = T.dev<M::LonLat>((size_t)N);
        M::LonLat* t_ll = T.dev<M::LonLat>((size_t)numTriangles);
        uint32_t* sideMap = T.dev<uint32_t>((size_t)pixels);
        uint32_t* bigList = T.dev<uint32_t>(2 * (size_t)numSides);
        unsigned long long* d_counts = T.dev<unsigned long long>(2);      // [0] covered pixels, [1] (as u32) the length of bigList
        unsigned long long* h_counts = T.pinned<unsigned long long>(2);
        uint32_t* bigCount = reinterpret_cast<uint32_t*>(d_counts + 1);
        WO_HIP(hipMemsetAsync(d_counts, 0, 16, s));
        if (centered) {
            launch(p, FAM_MAP_LONLAT, k_map_region_lonlat_centered, blocks_for(N), WO_BLOCK, (const float*)p->d_xyz, r_ll, N, centerLon);
            launch(p, FAM_MAP_LONLAT, k_map_center_lonlat_centered, blocks_for(numTriangles), WO_BLOCK, d_tri, (const float*)p->d_xyz, t_ll, numTriangles, centerLon);
        } else {
            launch(p, FAM_MAP_LONLAT, k_map_region_lonlat, blocks_for(N), WO_BLOCK, (const float*)p->d_xyz, r_ll, N);
            launch(p, FAM_MAP_LONLAT, k_map_center_lonlat, blocks_for(numTriangles), WO_BLOCK, d_tri, (const float*)p->d_xyz, t_ll, numTriangles);
        }
        launch(p, FAM_MAP_FILL, k_map_fill, blocks_for(pixels, 1 << 14), WO_BLOCK, sideMap, pixels);
        launch(p, FAM_MAP_SIDES, k_map_sides, blocks_for(numSides), WO_BLOCK, d_tri, d_he, (const M::LonLat*)t_ll, (const M::LonLat*)r_ll, numSides, W, H, sideMap, bigList, bigCount);
        launch(p, FAM_MAP_BIG_BOXES, k_map_big_boxes, MAP_BIG_GRID, WO_BLOCK, d_tri, d_he, (const M::LonLat*)t_ll, (const M::LonLat*)r_ll, W, H, sideMap, (const uint32_t*)bigList,
               (const uint32_t*)bigCount);
        launch(p, FAM_MAP_RESOLVE, k_map_resolve, blocks_for(pixels, 1 << 14), WO_BLOCK, (const uint32_t*)sideMap, d_tri, B->region, pixels, d_counts);
        if (relief) relief_heights_map(p, T, B, *relief, d_tri, d_he, numTriangles, t_ll, r_ll, sideMap);
        WO_HIP(hipMemcpyAsync(h_counts, d_counts, 16, hipMemcpyDeviceToHost, s));
        if (regionMapOut) WO_HIP(hipMemcpyAsync(regionMapOut, B->region, (size_t)pixels * 4, hipMemcpyDeviceToHost, s));
        WO_HIP(hipStreamSynchronize(s));                      // before T frees the temporaries
        B->valid = true;
        B->heightValid = relief != nullptr;
        B->heightCube = false;
        if (counts) { counts[0] = (int64_t)h_counts[0]; counts[1] = pixels - (int64_t)h_counts[0]; }
        return 0;
    WO_CATCH(fn)
}

// wo_map_color and wo_map_color_layer: the request's checks around those of the region map (`rasters`: the calls that give one, as the
// message names them), one packed colour per region, then the pixels; backgroundType: the map type whose background the uncovered
// pixels take; riverMinQ (wo_map_color_rivers: a map type and a rivers block, which the caller checked): the river cells under that
// threshold and the lakes take the river tint (rivers.hip) before the pixels are written
static int map_paint(wo_planet* p, const char* fn, const char* rasters, const ViewRequest& q, ViewFamilies families, int32_t backgroundType, uint8_t* rgbaOut, int64_t outBytes,
                     const uint64_t* riverMinQ = nullptr) {
    const std::string F = std::string(fn) + ": ";
    if (!check_planet(p, fn)) return 1;
    if (!rgbaOut) { set_error(F + "null pointer"); return 1; }
    ViewPlan plan;
    const bool ok = view_resolve(fn, p, q, plan, [&] {
        auto* B = p->map;
        if (!B || !B->valid) { set_error(F + "no region map on this planet (call " + rasters + " first)"); return false; }
        const int64_t bytes = (int64_t)B->W * B->H * 4;
        if (outBytes != bytes) { set_error(F + "a " + std::to_string(B->W) + " x " + std::to_string(B->H) + " map takes " + std::to_string(bytes) + " bytes, rgbaOut has " + std::to_string(outBytes)); return false; }
        return true;
    });
    if (!ok) return 1;
    WO_TRY
        auto* B = p->map;
        const int32_t N = p->N;
        const int64_t pixels = (int64_t)B->W * B->H;
        hipStream_t s = p->ctx->stream;
        uint8_t lut[256];
        M::gamma_lut(lut);
        DeviceArena T;                                        // the temporaries of this call
        const uint8_t* d_lut = up(T, (const uint8_t*)lut, 256, s);
        const float* e = q.source == VIEW_TYPE || M::layer_is_ocean_current(q.id) ? stage_elevation(p, T, q.r_elevation) : nullptr;
        uint32_t* regionRgba = T.dev<uint32_t>((size_t)N);
        uint32_t* out = T.dev<uint32_t>((size_t)pixels);
        view_region_colors(p, T, plan, e, ViewSink{nullptr, regionRgba, d_lut}, families);
        if (riverMinQ) rivers_tint_regions(p, e, *riverMinQ, regionRgba);
        launch(p, FAM_MAP_PIXELS, k_map_pixels, blocks_for((pixels + 3) / 4, 1 << 14), WO_BLOCK, (const int32_t*)B->region, (const uint32_t*)regionRgba, M::background_rgba(backgroundType, lut), out,
               pixels);
        WO_HIP(hipMemcpyAsync(rgbaOut, out, (size_t)pixels * 4, hipMemcpyDeviceToHost, s));
        WO_HIP(hipStreamSynchronize(s));                      // before T frees the temporaries; lut is this frame's
        return 0;
    WO_CATCH(fn)
}

extern "C" {

int wo_map_raster(wo_planet* p, int32_t numSides, const int32_t* triangles, const int32_t* halfedges, int32_t width, int32_t* regionMapOut, int64_t counts[2]) {
    return map_raster(p, "wo_map_raster", numSides, triangles, halfedges, width, false, 0.0, regionMapOut, counts, nullptr);
}

int wo_map_raster_centered(wo_planet* p, int32_t numSides, const int32_t* triangles, const int32_t* halfedges, int32_t width, double centerLon, int32_t* regionMapOut,
                           int64_t counts[2]) {
    return map_raster(p, "wo_map_raster_centered", numSides, triangles, halfedges, width, true, centerLon, regionMapOut, counts, nullptr);
}

int wo_map_color(wo_planet* p, int32_t type, const float* r_elevation, uint8_t* rgbaOut, int64_t outBytes) {
    ViewRequest q;
    q.source = VIEW_TYPE; q.id = type; q.r_elevation = r_elevation;
    return map_paint(p, "wo_map_color", "wo_map_raster", q, {FAM_MAP_REGION_COLORS, FAM_MAP_RANGE}, type, rgbaOut, outBytes);
}

int wo_map_color_rivers(wo_planet* p, int32_t type, const float* r_elevation, double minFlow, uint8_t* rgbaOut, int64_t outBytes) {
    const char* fn = "wo_map_color_rivers";
    if (!check_planet(p, fn)) return 1;
    if (!(minFlow - minFlow == 0.0)) { set_error(std::string(fn) + ": minFlow is " + std::to_string(minFlow) + ", it must be finite"); return 1; }
    if (!block_require(p, fn, rivers_desc(), rivers_desc().all(), nullptr)) return 1;
    ViewRequest q;
    q.source = VIEW_TYPE; q.id = type; q.r_elevation = r_elevation;
    const uint64_t minQ = rivers::min_q(minFlow);
    return map_paint(p, fn, "wo_map_raster", q, {FAM_MAP_REGION_COLORS, FAM_MAP_RANGE}, type, rgbaOut, outBytes, &minQ);
}

int wo_map_color_layer(wo_planet* p, int32_t layer, const float* values, const float* r_elevation, uint8_t* rgbaOut, int64_t outBytes) {
    ViewRequest q;
    q.source = VIEW_LAYER; q.id = layer; q.values = values; q.r_elevation = r_elevation;
    return map_paint(p, "wo_map_color_layer", "wo_map_raster or wo_map_raster_centered", q, {FAM_MAP_LAYER_COLORS, FAM_MAP_RANGE}, M::TYPE_COLOR, rgbaOut, outBytes);
}

int wo_map_download(wo_planet* p, int32_t* out, int64_t outBytes) {
    if (!check_planet(p, "wo_map_download")) return 1;
    if (!out) { set_error("wo_map_download: null pointer"); return 1; }
    auto* B = p->map;
    if (!B || !B->valid) { set_error("wo_map_download: no region map on this planet (call wo_map_raster first)"); return 1; }
    const int64_t bytes = (int64_t)B->W * B->H * 4;
    if (outBytes != bytes) { set_error("wo_map_download: a " + std::to_string(B->W) + " x " + std::to_string(B->H) + " map takes " + std::to_string(bytes) + " bytes, out has " + std::to_string(outBytes)); return 1; }
    WO_TRY
        WO_HIP(hipMemcpyAsync(out, B->region, (size_t)bytes, hipMemcpyDeviceToHost, p->ctx->stream));
        WO_HIP(hipStreamSynchronize(p->ctx->stream));
        return 0;
    WO_CATCH("wo_map_download")
}

int wo_map_dims(wo_planet* p, int32_t dims[2]) {
    if (!check_planet(p, "wo_map_dims")) return 1;
    if (!dims) { set_error("wo_map_dims: null pointer"); return 1; }
    auto* B = p->map;
    dims[0] = (B && B->valid) ? B->W : 0;
    dims[1] = (B && B->valid) ? B->H : 0;
    return 0;
}

int wo_map_free(wo_planet* p) {
    if (!check_planet(p, "wo_map_free")) return 1;
    map_free(p);
    return 0;
}

}  // extern "C"
