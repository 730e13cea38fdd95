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
// The lowest covering side index wins, so the map does not depend on the order in which lanes, workgroups or launches arrive.
// Launches of wo_map_color: k_map_region_colors [1] (one packed RGBA per region; `biome`: k_map_biome_raw [1] and
// k_map_biome_smooth [1] instead), k_map_pixels [1] (region map -> RGBA8, four pixels per thread).
// wo_map_raster_centered is the same raster around a centre meridian (the map view's, map_layer_ops.h): the two table kernels take
// centerLon (k_map_region_lonlat_centered, k_map_center_lonlat_centered), every other launch is wo_map_raster's.
// Launches of wo_map_color_layer: k_map_range [1] for the layers coloured over their range (the bounds as two uint32 words in
// device memory: a wave64 shuffle reduction, then at most one atomicMax per workgroup and bound), k_map_layer_colors [1] (one packed RGBA per
// region; it reads the bounds from device memory, no host round trip in between), k_map_pixels [1].
// Memory (device_mem.h): the region map lives in a block with an arena of its own on the planet (int32 per pixel; a raster at
// another width replaces it, wo_map_free and wo_planet_destroy drop it); triangles, half-edges, both longitude / latitude tables,
// the side map, the list and the colour tables are temporaries of the call, in an arena on its stack.
#include <hip/hip_runtime.h>

#include <atomic>
#include <memory>
#include <string>

#include "../../include/worogen.h"
#include "device.h"
#include "map_layer_ops.h"
#include "map_ops.h"
#include "map_shared.h"
#include "ocean_block.h"
#include "pick_ops.h"
#include "precip_block.h"
#include "stage_block.h"
#include "wind_block.h"

static_assert(wo::map::LAYER_COUNT == WO_MAP_LAYER_COUNT && wo::map::LAYER_WINDSPEED_WINTER == WO_MAP_LAYER_WINDSPEED_WINTER, "the layers of map_layer_ops.h are those of worogen.h");

namespace M = wo::map;

// the map block of a planet
struct wo_map_block {
    wo::DeviceArena mem;
    int32_t* region = nullptr;                                // W x H region ids, row 0 north; -1: nothing covers the pixel
    int32_t W = 0, H = 0;
    double centerLon = 0.0;                                   // the centre meridian of the raster (wo_map_raster: 0)
    bool valid = false;
};

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
    __shared__ unsigned long long blockCovered;
    if (threadIdx.x == 0) blockCovered = 0;
    __syncthreads();
    unsigned long long covered = 0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < pixels; i += (int64_t)gridDim.x * blockDim.x) {
        const uint32_t s = sideMap[i];
        region[i] = s == M::NO_SIDE ? -1 : triangles[s];
        covered += s != M::NO_SIDE;
    }
    for (int d = 32; d > 0; d >>= 1) covered += __shfl_down(covered, d, 64);
    if ((threadIdx.x & 63) == 0 && covered) atomicAdd(&blockCovered, covered);
    __syncthreads();
    if (threadIdx.x == 0 && blockCovered) atomicAdd(counts, blockCovered);
}

// the editor's tints (pick_ops.h) on a region's f32 colour, before the quantiser and the gamma table; cls: the highlight state's class
// bytes, nullptr without a state
__device__ inline M::Rgb map_tinted(const M::Rgb& c, const uint8_t* __restrict__ cls, int32_t r) { return cls && cls[r] ? wo::pick::tint(c, cls[r]) : c; }

__global__ __launch_bounds__(WO_BLOCK) void k_map_region_colors(int32_t type, const float* __restrict__ e, const uint8_t* __restrict__ koppen, const uint8_t* __restrict__ lut,
                                                                const uint8_t* __restrict__ cls, uint32_t* __restrict__ rgba, int32_t N) {
    const int32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r < N) rgba[r] = M::pack_rgba(map_tinted(M::region_color(type, e[r], koppen ? (int32_t)koppen[r] : 0), cls, r), lut);
}
__global__ __launch_bounds__(WO_BLOCK) void k_map_biome_raw(const float* __restrict__ e, const uint8_t* __restrict__ koppen, float* __restrict__ raw, int32_t N) {
    const int32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= N) return;
    const M::Rgb c = M::region_color(M::TYPE_BIOME, e[r], (int32_t)koppen[r]);
    raw[3 * (int64_t)r] = c.r; raw[3 * (int64_t)r + 1] = c.g; raw[3 * (int64_t)r + 2] = c.b;
}
__global__ __launch_bounds__(WO_BLOCK) void k_map_biome_smooth(const float* __restrict__ raw, const int32_t* __restrict__ off, const int32_t* __restrict__ adj,
                                                               const uint8_t* __restrict__ lut, const uint8_t* __restrict__ cls, uint32_t* __restrict__ rgba, int32_t N) {
    const int32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r < N) rgba[r] = M::pack_rgba(map_tinted(M::biome_smooth(raw, off, adj, r), cls, r), lut);
}

// The range of a layer's values (map_layer_ops.h: RangeBits): range[0], range[1] were cleared; every bound is a maximum over uint32
// words.  Sixteen bytes per load where v is aligned for it, four loads in flight per thread, the last N % 4 values one by one.  A
// workgroup whose bound does not exceed what the word already holds (a relaxed read: the word only grows) skips its atomic, so the
// atomics on the two words do not queue behind one another.
__global__ __launch_bounds__(WO_BLOCK) void k_map_range(const float* __restrict__ v, int32_t N, uint32_t* __restrict__ range) {
    __shared__ uint32_t blockLo, blockHi;
    if (threadIdx.x == 0) { blockLo = 0u; blockHi = 0u; }
    __syncthreads();
    M::RangeBits r{0u, 0u};
    const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (int64_t)gridDim.x * blockDim.x;
    const int64_t groups = (reinterpret_cast<uintptr_t>(v) & 15u) ? 0 : (int64_t)N / 4;
    const float4* __restrict__ v4 = reinterpret_cast<const float4*>(v);
    int64_t g = tid;
    for (; g + 3 * stride < groups; g += 4 * stride) {
        const float4 q0 = v4[g], q1 = v4[g + stride], q2 = v4[g + 2 * stride], q3 = v4[g + 3 * stride];
        M::range_take(r, q0.x); M::range_take(r, q0.y); M::range_take(r, q0.z); M::range_take(r, q0.w);
        M::range_take(r, q1.x); M::range_take(r, q1.y); M::range_take(r, q1.z); M::range_take(r, q1.w);
        M::range_take(r, q2.x); M::range_take(r, q2.y); M::range_take(r, q2.z); M::range_take(r, q2.w);
        M::range_take(r, q3.x); M::range_take(r, q3.y); M::range_take(r, q3.z); M::range_take(r, q3.w);
    }
    for (; g < groups; g += stride) {
        const float4 q = v4[g];
        M::range_take(r, q.x); M::range_take(r, q.y); M::range_take(r, q.z); M::range_take(r, q.w);
    }
    for (int64_t i = 4 * groups + tid; i < N; i += stride) M::range_take(r, v[i]);
    for (int d = 32; d > 0; d >>= 1) {
        r.lo = max(r.lo, (uint32_t)__shfl_down(r.lo, d, 64));
        r.hi = max(r.hi, (uint32_t)__shfl_down(r.hi, d, 64));
    }
    if ((threadIdx.x & 63) == 0) {
        if (r.lo) atomicMax(&blockLo, r.lo);
        if (r.hi) atomicMax(&blockHi, r.hi);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        if (blockLo > __hip_atomic_load(range, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(range, blockLo);
        if (blockHi > __hip_atomic_load(range + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(range + 1, blockHi);
    }
}

// b and e are read by the ocean-current layers only, range by the layers coloured over their range
__global__ __launch_bounds__(WO_BLOCK) void k_map_layer_colors(int32_t layer, const float* __restrict__ a, const float* __restrict__ b, const float* __restrict__ e,
                                                               const uint32_t* __restrict__ range, const uint8_t* __restrict__ lut, const uint8_t* __restrict__ cls, uint32_t* __restrict__ rgba,
                                                               int32_t N) {
    const int32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= N) return;
    const bool current = M::layer_is_ocean_current(layer);
    const M::RangeBits R = M::layer_needs_range(layer) ? M::RangeBits{range[0], range[1]} : M::RangeBits{0u, 0u};
    rgba[r] = M::pack_rgba(map_tinted(M::layer_color(layer, a[r], current ? b[r] : 0.0f, current ? e[r] : 0.0f, R), cls, r), lut);
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

// map_shared.h: the two launches the globe mesh shares with the map
void map_launch_range(wo_planet* p, int fam, const float* v, int32_t N, uint32_t* range) {
    launch(p, fam, k_map_range, blocks_for(((int64_t)N + 15) / 16, 1024), WO_BLOCK, v, N, range);      // 16 values per thread and turn
}
void map_launch_biome_raw(wo_planet* p, int fam, const float* e, const uint8_t* koppen, float* raw, int32_t N) {
    launch(p, fam, k_map_biome_raw, blocks_for(N), WO_BLOCK, e, koppen, raw, N);
}

static bool map_width_ok(int32_t width) { return width >= 2 && width <= 32768 && (width & 1) == 0; }

// numSides % 3 == 0 was checked; every corner a region of the planet, every half-edge a side of the mesh
bool map_topology_ok(int32_t N, int32_t numSides, const int32_t* triangles, const int32_t* halfedges, std::string& err) {
    std::atomic<int64_t> badCorner{-1}, badEdge{-1};
    parallel_ranges(numSides, [&](int64_t b, int64_t e, int) {
        for (int64_t s = b; s < e; ++s) {
            if ((uint32_t)triangles[s] >= (uint32_t)N) badCorner.store(s);
            if ((uint32_t)halfedges[s] >= (uint32_t)numSides) badEdge.store(s);
        }
    });
    if (badEdge.load() >= 0) { err = "half-edge out of range: halfedges[" + std::to_string(badEdge.load()) + "] = " + std::to_string(halfedges[badEdge.load()]) + ", the mesh has " + std::to_string(numSides) + " sides"; return false; }
    if (badCorner.load() >= 0) { err = "corner out of range: triangles[" + std::to_string(badCorner.load()) + "] = " + std::to_string(triangles[badCorner.load()]) + ", the planet has " + std::to_string(N) + " regions"; return false; }
    return true;
}

}  // namespace wo

using namespace wo;

// wo_map_raster (centered == false: its own two table kernels) and wo_map_raster_centered
static int map_raster(wo_planet* p, const char* fn, int32_t numSides, const int32_t* triangles, const int32_t* halfedges, int32_t width, bool centered, double centerLon,
                      int32_t* regionMapOut, int64_t counts[2]) {
    const std::string F = std::string(fn) + ": ";
    if (!check_planet(p, fn)) return 1;
    if (!triangles || !halfedges) { set_error(F + "null pointer"); return 1; }
    if (!map_width_ok(width)) { set_error(F + "width is " + std::to_string(width) + ", it must be even and from 2 to 32768"); return 1; }
    if (numSides < 3 || numSides % 3 != 0 || numSides >= (1 << 30)) { set_error(F + "numSides is " + std::to_string(numSides) + ", it must be a multiple of 3 from 3 to 2^30 - 3"); return 1; }
    if (centered && !M::center_lon_ok(centerLon)) { set_error(F + "centerLon is " + std::to_string(centerLon) + ", it must be finite and from -pi to pi"); return 1; }
    std::string err;
    if (!map_topology_ok(p->N, numSides, triangles, halfedges, err)) { set_error(F + err); return 1; }
    WO_TRY
        const int32_t W = width, H = width / 2, N = p->N, numTriangles = numSides / 3;
        const int64_t pixels = (int64_t)W * H;
        hipStream_t s = p->ctx->stream;
        if (!p->map || p->map->W != W) {                     // the old map goes first; the planet gets the new block once it is complete
            map_free(p);
            std::unique_ptr<wo_map_block> block(new wo_map_block());
            block->region = block->mem.dev<int32_t>((size_t)pixels);
            block->W = W; block->H = H;
            p->map = block.release();
        }
        auto* B = p->map;
        B->valid = false;
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
        WO_HIP(hipMemcpyAsync(h_counts, d_counts, 16, hipMemcpyDeviceToHost, s));
        if (regionMapOut) WO_HIP(hipMemcpyAsync(regionMapOut, B->region, (size_t)pixels * 4, hipMemcpyDeviceToHost, s));
        WO_HIP(hipStreamSynchronize(s));                      // before T frees the temporaries
        B->valid = true;
        if (counts) { counts[0] = (int64_t)h_counts[0]; counts[1] = pixels - (int64_t)h_counts[0]; }
        return 0;
    WO_CATCH(fn)
}

// where a named layer's values live: the block, and the reference's result key of the field (two for the ocean-current layers)
LayerSource wo::layer_source(int32_t layer) {
    switch (layer) {
        case M::LAYER_CONTINENTALITY: return {&wind_desc(), "r_continentality", nullptr, "wo_wind_upload r_continentality"};
        case M::LAYER_TEMP_SUMMER: return {&temp_desc(), "r_temperature_summer", nullptr, "wo_temperature_upload r_temperature_summer"};
        case M::LAYER_TEMP_WINTER: return {&temp_desc(), "r_temperature_winter", nullptr, "wo_temperature_upload r_temperature_winter"};
        case M::LAYER_PRECIP_SUMMER: return {&precip_desc(), "r_precip_summer", nullptr, "wo_precip_upload r_precip_summer"};
        case M::LAYER_PRECIP_WINTER: return {&precip_desc(), "r_precip_winter", nullptr, "wo_precip_upload r_precip_winter"};
        case M::LAYER_RAINSHADOW_SUMMER: return {&precip_desc(), "r_rainshadow_summer", nullptr, "wo_precip_upload r_rainshadow_summer"};
        case M::LAYER_RAINSHADOW_WINTER: return {&precip_desc(), "r_rainshadow_winter", nullptr, "wo_precip_upload r_rainshadow_winter"};
        case M::LAYER_OCEANCURRENT_SUMMER: return {&ocean_desc(), "r_ocean_warmth_summer", "r_ocean_speed_summer", "wo_ocean_upload r_ocean_warmth_summer r_ocean_speed_summer"};
        case M::LAYER_OCEANCURRENT_WINTER: return {&ocean_desc(), "r_ocean_warmth_winter", "r_ocean_speed_winter", "wo_ocean_upload r_ocean_warmth_winter r_ocean_speed_winter"};
        case M::LAYER_PRESSURE_SUMMER: return {&wind_desc(), "r_pressure_summer", nullptr, "wo_wind_upload r_pressure_summer"};
        case M::LAYER_PRESSURE_WINTER: return {&wind_desc(), "r_pressure_winter", nullptr, "wo_wind_upload r_pressure_winter"};
        case M::LAYER_WINDSPEED_SUMMER: return {&wind_desc(), "r_wind_speed_summer", nullptr, "wo_wind_upload r_wind_speed_summer"};
        case M::LAYER_WINDSPEED_WINTER: return {&wind_desc(), "r_wind_speed_winter", nullptr, "wo_wind_upload r_wind_speed_winter"};
        default: return {nullptr, nullptr, nullptr, nullptr};
    }
}

extern "C" {

int wo_map_raster(wo_planet* p, int32_t numSides, const int32_t* triangles, const int32_t* halfedges, int32_t width, int32_t* regionMapOut, int64_t counts[2]) {
    return map_raster(p, "wo_map_raster", numSides, triangles, halfedges, width, false, 0.0, regionMapOut, counts);
}

int wo_map_raster_centered(wo_planet* p, int32_t numSides, const int32_t* triangles, const int32_t* halfedges, int32_t width, double centerLon, int32_t* regionMapOut,
                           int64_t counts[2]) {
    return map_raster(p, "wo_map_raster_centered", numSides, triangles, halfedges, width, true, centerLon, regionMapOut, counts);
}

int wo_map_color(wo_planet* p, int32_t type, const float* r_elevation, uint8_t* rgbaOut, int64_t outBytes) {
    if (!check_planet(p, "wo_map_color")) return 1;
    if (!rgbaOut) { set_error("wo_map_color: null pointer"); return 1; }
    if (type < 0 || type >= M::TYPE_COUNT) { set_error("wo_map_color: unknown map type " + std::to_string(type)); return 1; }
    auto* B = p->map;
    if (!B || !B->valid) { set_error("wo_map_color: no region map on this planet (call wo_map_raster first)"); return 1; }
    const int64_t pixels = (int64_t)B->W * B->H;
    if (outBytes != pixels * 4) { set_error("wo_map_color: a " + std::to_string(B->W) + " x " + std::to_string(B->H) + " map takes " + std::to_string(pixels * 4) + " bytes, rgbaOut has " + std::to_string(outBytes)); return 1; }
    const uint8_t* koppen = M::type_needs_koppen(type) ? koppen_classes(p) : nullptr;
    if (M::type_needs_koppen(type) && !koppen) { set_error("wo_map_color: no Koppen result on this planet (call wo_classify_koppen first)"); return 1; }
    WO_TRY
        const int32_t N = p->N, g = blocks_for(N);
        hipStream_t s = p->ctx->stream;
        uint8_t lut[256];
        M::gamma_lut(lut);
        DeviceArena T;                                        // the temporaries of this call
        const uint8_t* d_lut = up(T, (const uint8_t*)lut, 256, s);
        const float* e = stage_elevation(p, T, r_elevation);
        uint32_t* regionRgba = T.dev<uint32_t>((size_t)N);
        uint32_t* out = T.dev<uint32_t>((size_t)pixels);
        if (type == M::TYPE_BIOME) {
            float* raw = T.dev<float>(3 * (size_t)N);
            map_launch_biome_raw(p, FAM_MAP_REGION_COLORS, e, koppen, raw, N);
            launch(p, FAM_MAP_REGION_COLORS, k_map_biome_smooth, g, WO_BLOCK, (const float*)raw, (const int32_t*)p->d_off, (const int32_t*)p->d_adj, d_lut, highlight_classes(p),
                   regionRgba, N);
        } else {
            launch(p, FAM_MAP_REGION_COLORS, k_map_region_colors, g, WO_BLOCK, type, e, koppen, d_lut, highlight_classes(p), regionRgba, N);
        }
        launch(p, FAM_MAP_PIXELS, k_map_pixels, blocks_for((pixels + 3) / 4, 1 << 14), WO_BLOCK, (const int32_t*)B->region, (const uint32_t*)regionRgba, M::background_rgba(type, lut), out,
               pixels);
        WO_HIP(hipMemcpyAsync(rgbaOut, out, (size_t)pixels * 4, hipMemcpyDeviceToHost, s));
        WO_HIP(hipStreamSynchronize(s));                      // before T frees the temporaries; lut is this frame's
        return 0;
    WO_CATCH("wo_map_color")
}

int wo_map_color_layer(wo_planet* p, int32_t layer, const float* values, const float* r_elevation, uint8_t* rgbaOut, int64_t outBytes) {
    const char* fn = "wo_map_color_layer";
    if (!check_planet(p, fn)) return 1;
    if (!rgbaOut) { set_error("wo_map_color_layer: null pointer"); return 1; }
    if (layer < 0 || layer >= M::LAYER_COUNT) { set_error("wo_map_color_layer: unknown map layer " + std::to_string(layer)); return 1; }
    auto* B = p->map;
    if (!B || !B->valid) { set_error("wo_map_color_layer: no region map on this planet (call wo_map_raster or wo_map_raster_centered first)"); return 1; }
    const int64_t pixels = (int64_t)B->W * B->H;
    if (outBytes != pixels * 4) { set_error("wo_map_color_layer: a " + std::to_string(B->W) + " x " + std::to_string(B->H) + " map takes " + std::to_string(pixels * 4) + " bytes, rgbaOut has " + std::to_string(outBytes)); return 1; }
    const bool current = M::layer_is_ocean_current(layer);
    if (layer == M::LAYER_DEBUG && !values) { set_error("wo_map_color_layer: WO_MAP_LAYER_DEBUG takes its values from the caller, values is NULL"); return 1; }
    if (current && values) { set_error("wo_map_color_layer: an ocean-current layer reads two fields, values must be NULL (wo_ocean_upload sets the warmth and the speed)"); return 1; }
    const LayerSource S = layer_source(layer);
    int fa = -1, fb = -1;
    if (!values) {                                            // the resident field(s)
        fa = S.block->index(S.a);
        fb = S.b ? S.block->index(S.b) : -1;
        if (!block_require(p, fn, *S.block, bit(fa) | (fb >= 0 ? bit(fb) : 0u), S.hint)) return 1;
    }
    WO_TRY
        const int32_t N = p->N, g = blocks_for(N);
        hipStream_t s = p->ctx->stream;
        uint8_t lut[256];
        M::gamma_lut(lut);
        DeviceArena T;                                        // the temporaries of this call
        const uint8_t* d_lut = up(T, (const uint8_t*)lut, 256, s);
        const float* a = values ? up(T, values, (size_t)N, s) : (const float*)S.block->slot(S.block->get(p), fa, (size_t)N).ptr;
        const float* b = fb >= 0 ? (const float*)S.block->slot(S.block->get(p), fb, (size_t)N).ptr : nullptr;
        const float* e = current ? stage_elevation(p, T, r_elevation) : nullptr;
        uint32_t* range = T.dev<uint32_t>(2);
        uint32_t* regionRgba = T.dev<uint32_t>((size_t)N);
        uint32_t* out = T.dev<uint32_t>((size_t)pixels);
        if (M::layer_needs_range(layer)) {
            WO_HIP(hipMemsetAsync(range, 0, 8, s));
            map_launch_range(p, FAM_MAP_RANGE, a, N, range);
        }
        launch(p, FAM_MAP_LAYER_COLORS, k_map_layer_colors, g, WO_BLOCK, layer, a, b, e, (const uint32_t*)range, d_lut, highlight_classes(p), regionRgba, N);
        launch(p, FAM_MAP_PIXELS, k_map_pixels, blocks_for((pixels + 3) / 4, 1 << 14), WO_BLOCK, (const int32_t*)B->region, (const uint32_t*)regionRgba, M::background_rgba(M::TYPE_COLOR, lut),
               out, pixels);
        WO_HIP(hipMemcpyAsync(rgbaOut, out, (size_t)pixels * 4, hipMemcpyDeviceToHost, s));
        WO_HIP(hipStreamSynchronize(s));                      // before T frees the temporaries; lut is this frame's
        return 0;
    WO_CATCH("wo_map_color_layer")
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

int wo_map_free(wo_planet* p) {
    if (!check_planet(p, "wo_map_free")) return 1;
    map_free(p);
    return 0;
}

}  // extern "C"
