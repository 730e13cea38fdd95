// Equirectangular map export on the device (the reference's exportMap / exportMapBatch, js/planet-mesh.js:1752-2180): the raster
// of the mesh's map triangles into a region map, and the colouring of that map into RGBA8 in the reference's six kinds.  The
// per-vertex, per-side, per-pixel and per-region bodies and the contract are in map_ops.h; everything runs on the planet's
// resident positions, elevation and Koppen block, on its stream.
//
// wo_map_raster is the raster of raster.hip (its launches are listed there) under map::Projection, in the map_* families, with the
// map's two tables:
//   k_map_region_lonlat [1]   longitude and latitude of every region, one thread each
//   k_map_center_lonlat [1]   the same of every triangle centre: 3 N evaluations of atan2 / asin in all, not 18 N
// wo_map_raster_centered is the same raster around a centre meridian (the map view's, map_layer_ops.h): the two table kernels are
// the <true> instances, which take centerLon through lonlat_of_centered; every other launch is wo_map_raster's.
// wo_relief_raster is wo_map_raster_centered with a request: after k_map_resolve, while the side map and the two tables still live,
// relief_heights (relief.hip) adds its height pass; the launches above are the same and so are the region map and the counts.
// Launches of wo_map_color and wo_map_color_layer: the region colours of view_colors.hip, one packed RGBA per region [1-2], then
// k_map_pixels [1] (region map -> RGBA8, four pixels per thread).  On the block of a globe view (view.hip) the uncovered pixels take
// the view's background word and, after a shaded raster, k_view_shade [1] follows; a map or cube block paints as it always did.
// Memory (device_mem.h): the region map lives in a block with an arena of its own on the planet (map_block.h; int32 per pixel; a
// raster at another width or height, wo_map_raster_cube's included, replaces it, wo_map_free and wo_planet_destroy drop it); the
// colour tables are temporaries of the call, in an arena on its stack.
#include <hip/hip_runtime.h>

#include <memory>
#include <string>

#include "../../include/worogen.h"
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

// the two tables; Centered: around a centre meridian (centerLon is not read otherwise)
template <bool Centered>
__global__ __launch_bounds__(WO_BLOCK) void k_map_region_lonlat(const float* __restrict__ xyz, M::LonLat* __restrict__ out, int32_t N, double centerLon) {
    const int32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= N) return;
    const float x = xyz[3 * (int64_t)r], y = xyz[3 * (int64_t)r + 1], z = xyz[3 * (int64_t)r + 2];
    if constexpr (Centered) out[r] = M::lonlat_of_centered(x, y, z, centerLon);
    else out[r] = M::lonlat_of(x, y, z);
}

template <bool Centered>
__global__ __launch_bounds__(WO_BLOCK) void k_map_center_lonlat(const int32_t* __restrict__ triangles, const float* __restrict__ xyz, M::LonLat* __restrict__ out,
                                                                int32_t numTriangles, double centerLon) {
    const int32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= numTriangles) return;
    if constexpr (Centered) out[t] = M::lonlat_of_center_centered(triangles, xyz, t, centerLon);
    else out[t] = M::lonlat_of_center(triangles, xyz, t);
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
    p->map->valid = p->map->heightValid = p->map->view = p->map->lambertValid = false;      // any raster, through any entry point, ends the relief and the view of the last
    return p->map;
}

static bool map_width_ok(int32_t width) { return width >= 2 && width <= 32768 && (width & 1) == 0; }

}  // namespace wo

using namespace wo;

// wo_map_raster (centered == false: the plain table kernels), wo_map_raster_centered and, with a request, wo_relief_raster: the checks
// of the width and the centre, and the raster of raster.hip with the map's tables and families
static int map_raster(wo_planet* p, const char* fn, int32_t numSides, const int32_t* triangles, const int32_t* halfedges, int32_t width, bool centered, double centerLon,
                      int32_t* regionMapOut, int64_t counts[2], const ReliefRequest* relief) {
    const std::string F = std::string(fn) + ": ";
    if (!check_planet(p, fn)) return 1;
    if (!map_width_ok(width)) { set_error(F + "width is " + std::to_string(width) + ", it must be even and from 2 to 32768"); return 1; }
    if (centered && !M::center_lon_ok(centerLon)) { set_error(F + "centerLon is " + std::to_string(centerLon) + ", it must be finite and from -pi to pi"); return 1; }
    const int32_t W = width, H = width / 2, N = p->N, numTriangles = numSides / 3;
    M::LonLat *r_ll = nullptr, *t_ll = nullptr;
    const auto tables = [&](DeviceArena& T) {
        r_ll = T.dev<M::LonLat>((size_t)N);
        t_ll = T.dev<M::LonLat>((size_t)numTriangles);
        return M::Projection{t_ll, r_ll, W, H};
    };
    const auto launchTables = [&](const int32_t* d_tri) {
        launch(p, FAM_MAP_LONLAT, centered ? k_map_region_lonlat<true> : k_map_region_lonlat<false>, blocks_for(N), WO_BLOCK, (const float*)p->d_xyz, r_ll, N, centerLon);
        launch(p, FAM_MAP_LONLAT, centered ? k_map_center_lonlat<true> : k_map_center_lonlat<false>, blocks_for(numTriangles), WO_BLOCK, d_tri, (const float*)p->d_xyz, t_ll,
               numTriangles, centerLon);
    };
    return raster<M::Projection>(p, fn, numSides, triangles, halfedges,
                                 {W, H, centered ? centerLon : 0.0, false, FAM_MAP_FILL, FAM_MAP_SIDES, FAM_MAP_BIG_BOXES, FAM_MAP_RESOLVE, tables, launchTables}, regionMapOut, counts,
                                 relief);
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
        launch(p, FAM_MAP_PIXELS, k_map_pixels, blocks_for((pixels + 3) / 4, 1 << 14), WO_BLOCK, (const int32_t*)B->region, (const uint32_t*)regionRgba,
               B->view ? B->background : M::background_rgba(backgroundType, lut), out, pixels);
        if (B->view && B->lambertValid) view_shade(p, B, out);
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

int wo_relief_raster(wo_planet* p, int32_t numSides, const int32_t* triangles, const int32_t* halfedges, int32_t width, double centerLon, const float* r_elevation,
                     float* heightOut, int64_t counts[2]) {
    const ReliefRequest q{r_elevation, heightOut};
    return map_raster(p, "wo_relief_raster", numSides, triangles, halfedges, width, true, centerLon, nullptr, counts, &q);
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
