// The globe view on the device: the displaced globe mesh seen through a perspective or orthographic camera, rastered with a depth
// per pixel into a region map in the planet's map block (map_block.h), where wo_map_color, wo_map_color_rivers, wo_map_color_layer,
// wo_map_download, wo_map_dims, wo_map_free and the editor's tints serve it as they serve a map, and shaded by one Lambert term per
// facet.  The per-vertex, per-side and per-pixel bodies and the contract are in view_ops.h; everything runs on the planet's
// resident positions and on its elevation or the caller's, on its stream.
//
// wo_view_raster is the raster of raster.hip (its launches are listed there) under view::Projection, whose per-pixel word is the
// 64-bit (depth, side) key, in the view_* families, with one table and its own resolve:
//   k_globe_centers [1]       globe.hip's: the centre and the elevation of every triangle as one 16-byte record
//   k_view_resolve [1]        key -> region (triangles[side], or -1) into the block's region map, the depth into its depth map, with
//                             a shading request the Lambert term of the winning side into its Lambert map (the side's nine floats
//                             rebuilt with the functions the raster used), and the covered count
// Launches that a view block adds to wo_map_color and its siblings (map.hip: map_paint): k_view_shade [1] after k_map_pixels, four
//   pixels per thread, only after a shaded raster.
// Memory (device_mem.h): the depth and Lambert maps live in the map block, allocated by its first view raster and its first shaded
// one and dropped with the block; the centre records, an uploaded elevation and the key map are temporaries of the raster's arena.
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/worogen.h"
#include "block_ops.h"
#include "device.h"
#include "map_block.h"
#include "stage_block.h"
#include "view_ops.h"

static_assert(wo::view::DEFAULT_BACKGROUND == WO_VIEW_BACKGROUND, "the background of view_ops.h is that of worogen.h");

namespace G = wo::globe;
namespace V = wo::view;

namespace wo {

struct ViewLight { double d[3]; };

// counts[0] += covered pixels; lambert may be nullptr (no shading request: light is not read)
__global__ __launch_bounds__(WO_BLOCK) void k_view_resolve(const V::Projection proj, const unsigned long long* __restrict__ keyMap, const int32_t* __restrict__ triangles,
                                                           const int32_t* __restrict__ halfedges, const ViewLight light, int32_t* __restrict__ region, float* __restrict__ depth,
                                                           float* __restrict__ lambert, int64_t pixels, unsigned long long* counts) {
    __shared__ unsigned long long blockCovered[1];
    if (threadIdx.x == 0) blockCovered[0] = 0;
    __syncthreads();
    unsigned long long covered[1] = {0};
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < pixels; i += (int64_t)gridDim.x * blockDim.x) {
        const V::Pixel px = V::pixel_of(proj, triangles, halfedges, keyMap[i], lambert != nullptr, light.d[0], light.d[1], light.d[2]);
        region[i] = px.region;
        depth[i] = px.depth;
        if (lambert) lambert[i] = px.lambert;
        covered[0] += px.region >= 0;
    }
    block_add_to_global<1>(covered, blockCovered, counts);
}

// four pixels per thread: 16-byte loads of the regions, the Lambert terms and the colours, one 16-byte store
__global__ __launch_bounds__(WO_BLOCK) void k_view_shade(const int32_t* __restrict__ region, const float* __restrict__ lambert, double ambient, double diffuse,
                                                         uint32_t* __restrict__ rgba, int64_t pixels) {
    const int64_t groups = (pixels + 3) / 4;
    for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < groups; g += (int64_t)gridDim.x * blockDim.x) {
        const int64_t i = 4 * g;
        if (i + 3 < pixels) {
            const int4 r = *reinterpret_cast<const int4*>(region + i);
            const float4 l = *reinterpret_cast<const float4*>(lambert + i);
            uint4 c = *reinterpret_cast<const uint4*>(rgba + i);
            if (r.x >= 0) c.x = V::shade_rgba(c.x, l.x, ambient, diffuse);
            if (r.y >= 0) c.y = V::shade_rgba(c.y, l.y, ambient, diffuse);
            if (r.z >= 0) c.z = V::shade_rgba(c.z, l.z, ambient, diffuse);
            if (r.w >= 0) c.w = V::shade_rgba(c.w, l.w, ambient, diffuse);
            *reinterpret_cast<uint4*>(rgba + i) = c;
        } else {
            for (int64_t k = i; k < pixels; ++k)
                if (region[k] >= 0) rgba[k] = V::shade_rgba(rgba[k], lambert[k], ambient, diffuse);
        }
    }
}

void view_shade(wo_planet* p, const wo_map_block* B, uint32_t* rgba) {
    const int64_t pixels = (int64_t)B->W * B->H;
    launch(p, FAM_VIEW_SHADE, k_view_shade, blocks_for((pixels + 3) / 4, 1 << 14), WO_BLOCK, (const int32_t*)B->region, (const float*)B->lambert, B->ambient, B->diffuse, rgba, pixels);
}

}  // namespace wo

using namespace wo;

static bool finite_nonneg(double v) { return v >= 0.0 && v - v == 0.0; }

// the depth map of a view block, or the Lambert map of a shaded one, to the host
static int view_download(wo_planet* p, const char* fn, bool lambert, float* out, int64_t outBytes) {
    const std::string F = std::string(fn) + ": ";
    if (!check_planet(p, fn)) return 1;
    if (!out) { set_error(F + "null pointer"); return 1; }
    auto* B = p->map;
    if (!B || !B->valid || !B->view) { set_error(F + "no view raster on this planet (call wo_view_raster first)"); return 1; }
    if (lambert && !B->lambertValid) { set_error(F + "no shaded view raster on this planet (call wo_view_raster with shade set first)"); return 1; }
    const int64_t bytes = (int64_t)B->W * B->H * 4;
    if (outBytes != bytes) { set_error(F + "a " + std::to_string(B->W) + " x " + std::to_string(B->H) + " view takes " + std::to_string(bytes) + " bytes, out has " + std::to_string(outBytes)); return 1; }
    WO_TRY
        WO_HIP(hipMemcpyAsync(out, lambert ? B->lambert : B->depth, (size_t)bytes, hipMemcpyDeviceToHost, p->ctx->stream));
        WO_HIP(hipStreamSynchronize(p->ctx->stream));
        return 0;
    WO_CATCH(fn)
}

extern "C" {

int wo_view_raster(wo_planet* p, int32_t numSides, const int32_t* triangles, const int32_t* halfedges, int32_t width, int32_t height, const wo_view_request* request,
                   int32_t* regionMapOut, float* depthOut, int64_t counts[2]) {
    const char* fn = "wo_view_raster";
    const std::string F = std::string(fn) + ": ";
    if (!check_planet(p, fn)) return 1;
    if (!request) { set_error(F + "null pointer (request)"); return 1; }
    const wo_view_request& q = *request;
    if (!V::size_ok(width)) { set_error(F + "width is " + std::to_string(width) + ", it must be from 1 to 16384"); return 1; }
    if (!V::size_ok(height)) { set_error(F + "height is " + std::to_string(height) + ", it must be from 1 to 16384"); return 1; }
    V::Camera cam;
    const int bad = V::camera_make(q.eye, q.fovY, q.halfHeight, cam);
    if (bad == V::CAMERA_BAD_EYE) { set_error(F + "eye is (" + std::to_string(q.eye[0]) + ", " + std::to_string(q.eye[1]) + ", " + std::to_string(q.eye[2]) + "), it must be finite and not the origin"); return 1; }
    if (bad == V::CAMERA_BAD_FOV) { set_error(F + "fovY is " + std::to_string(q.fovY) + ", it must be 0 (orthographic) or above 0 and below 180 degrees"); return 1; }
    if (bad == V::CAMERA_BAD_HALF_HEIGHT) { set_error(F + "halfHeight is " + std::to_string(q.halfHeight) + ", an orthographic view (fovY 0) takes a finite one above 0"); return 1; }
    if (!finite_nonneg(q.exaggeration)) { set_error(F + "exaggeration is " + std::to_string(q.exaggeration) + ", it must be finite and >= 0"); return 1; }
    ViewLight light{{0.0, 0.0, 0.0}};
    if (q.shade) {
        if (!V::unit3(q.light, light.d)) { set_error(F + "light is (" + std::to_string(q.light[0]) + ", " + std::to_string(q.light[1]) + ", " + std::to_string(q.light[2]) + "), it must be finite and not zero"); return 1; }
        if (!finite_nonneg(q.ambient) || !finite_nonneg(q.diffuse)) { set_error(F + "ambient is " + std::to_string(q.ambient) + " and diffuse is " + std::to_string(q.diffuse) + ", they must be finite and >= 0"); return 1; }
    }
    const int32_t W = width, H = height, numTriangles = numSides / 3;
    const int64_t pixels = (int64_t)W * H;
    const bool shade = q.shade != 0;
    G::Center* centers = nullptr;
    const float* e = nullptr;
    const auto tables = [&](DeviceArena& T) {
        auto* B = p->map;                                     // the raster's block: every allocation comes before the first launch
        if (!B->depth) B->depth = B->mem.dev<float>((size_t)pixels);
        if (shade && !B->lambert) B->lambert = B->mem.dev<float>((size_t)pixels);
        e = stage_elevation(p, T, q.r_elevation);
        centers = T.dev<G::Center>((size_t)numTriangles);
        return V::Projection{centers, (const float*)p->d_xyz, e, cam, G::V * q.exaggeration, W, H};
    };
    const auto launchTables = [&](const int32_t* d_tri) { globe_centers(p, FAM_VIEW_TABLES, d_tri, e, centers, numTriangles); };
    const auto resolve = [&](const V::Projection& proj, const unsigned long long* keyMap, const int32_t* d_tri, const int32_t* d_he, wo_map_block* B, unsigned long long* d_counts) {
        launch(p, FAM_VIEW_RESOLVE, k_view_resolve, blocks_for(pixels, 1 << 14), WO_BLOCK, proj, keyMap, d_tri, d_he, light, B->region, B->depth, shade ? B->lambert : (float*)nullptr, pixels,
               d_counts);
        if (depthOut) WO_HIP(hipMemcpyAsync(depthOut, B->depth, (size_t)pixels * 4, hipMemcpyDeviceToHost, p->ctx->stream));
    };
    const int rc = raster<V::Projection>(p, fn, numSides, triangles, halfedges,
                                         {W, H, 0.0, false, FAM_VIEW_FILL, FAM_VIEW_SIDES, FAM_VIEW_BIG_BOXES, FAM_VIEW_RESOLVE, tables, launchTables, resolve}, regionMapOut, counts, nullptr);
    if (rc != 0) return rc;
    auto* B = p->map;                                         // the stream has been waited for
    B->view = true;
    B->lambertValid = shade;
    B->background = q.backgroundRgba;
    B->ambient = q.ambient; B->diffuse = q.diffuse;
    return 0;
}

int wo_view_depth_download(wo_planet* p, float* out, int64_t outBytes) { return view_download(p, "wo_view_depth_download", false, out, outBytes); }

int wo_view_lambert_download(wo_planet* p, float* out, int64_t outBytes) { return view_download(p, "wo_view_lambert_download", true, out, outBytes); }

}  // extern "C"
