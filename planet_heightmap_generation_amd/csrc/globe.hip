// The globe mesh on the device (the reference's buildMesh, updateMeshColors and updateSuperPlateBorders, js/planet-mesh.js:620-836,
// :840-957, :533-576): the displaced Voronoi-fan triangles of every side with one colour per region, the Voronoi wireframe and the
// super-plate borders.  The bodies and the contract are in globe_ops.h; everything runs on the planet's resident positions,
// elevation, Koppen block and climate blocks, on its stream.
//
// Launches of wo_globe_mesh / wo_globe_mesh_plates (no host round trip between them; the stream is waited for once, at the end):
//   k_globe_centers [1]        t_xyz and t_elevation of every triangle as one 16-byte record: 2 N records instead of 18 N sums
//   region colours [1-3]       one f32 triple per region: k_globe_type_colors, k_globe_layer_colors (after k_map_range over the
//                              layers coloured over their range), k_map_biome_raw + k_globe_biome_smooth, or k_globe_plate_slots +
//                              k_globe_plate_colors
//   k_globe_mesh [1]           one lane per side: two centre records, the region's position and elevation, the colour; nine floats
//                              of positions and nine of colours per side.  A workgroup's 256 sides are 9216 contiguous bytes of each
//                              output: the lanes put their nine floats into LDS (stride 9, no bank conflict) and the workgroup
//                              stores them 16 bytes per lane and instruction.  The bounds of the stored positions are reduced here:
//                              a wave64 shuffle, one LDS atomic per wave and word, at most one global atomic per workgroup and word
//                              after a relaxed read.  Either output may be absent: without positions it is updateMeshColors.
// Launches of wo_globe_lines, an order-preserving compaction: k_globe_centers [1], k_globe_line_count [1] (per workgroup, ballot
//   and popcount), k_globe_line_scan [1] (one workgroup scans the workgroup counts in place and leaves the total),
//   k_globe_line_write [1] (every lane's place is its workgroup's offset + its wave's + the popcount of the ballot below it).
//   The segment count is waited for before the segments are copied, so that nothing is written behind them.
// The editor's highlight state (wo_highlight_set / wo_highlight_clear; the bodies in pick_ops.h): one class byte per region, kept in a
//   block of its own.  k_highlight_kinds [1] scatters the pending plates' kinds over a cleared table of one byte per region id,
//   k_highlight_classes [1] gives every region its byte and counts the regions per bit (ballot and popcount per wave, one LDS atomic
//   per wave and bit, one global integer atomic per workgroup and bit).  While the state is set, k_highlight_tint [1] runs over the
//   region colours of wo_globe_mesh / wo_globe_mesh_plates before the mesh kernel reads them; a region whose byte is 0 is not
//   written.
// Memory (device_mem.h): everything is a temporary of the call, in an arena on its stack, but the class bytes, which the highlight
// block owns.
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "../../include/worogen.h"
#include "device.h"
#include "globe_ops.h"
#include "map_shared.h"
#include "pick_ops.h"

namespace G = wo::globe;
namespace M = wo::map;
namespace P = wo::pick;

static_assert(G::SOURCE_TYPE == WO_GLOBE_SOURCE_TYPE && G::SOURCE_LAYER == WO_GLOBE_SOURCE_LAYER, "the sources of globe_ops.h are those of worogen.h");
static_assert(G::LINES_WIREFRAME == WO_GLOBE_LINES_WIREFRAME && G::LINES_SUPER_PLATE_BORDERS == WO_GLOBE_LINES_SUPER_PLATE_BORDERS, "the line kinds of globe_ops.h are those of worogen.h");
static_assert(sizeof(G::Center) == 16, "one 16-byte load per centre");

struct wo_highlight_block {
    wo::DeviceArena mem;                 // owns cls
    uint8_t* cls = nullptr;              // one class byte per region (pick_ops.h: CLS_*)
};

namespace wo {

constexpr int GLOBE_WAVES = WO_BLOCK / 64;

void highlight_free(wo_planet* p) { delete p->highlight; p->highlight = nullptr; }
const uint8_t* highlight_classes(const wo_planet* p) { return p->highlight ? p->highlight->cls : nullptr; }

// kind was cleared; the entry point checked that every plate is a region id and that none is listed twice
__global__ __launch_bounds__(WO_BLOCK) void k_highlight_kinds(const int32_t* __restrict__ plates, const uint8_t* __restrict__ isOcean, int32_t n, uint8_t* __restrict__ kind) {
    const int32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) kind[plates[i]] = isOcean[i] ? P::CLS_PENDING_OCEAN : P::CLS_PENDING_LAND;
}
// counts (four words, cleared): the regions per bit.  The grid covers N exactly.
__global__ __launch_bounds__(WO_BLOCK) void k_highlight_classes(const int32_t* __restrict__ r_plate, const uint8_t* __restrict__ kind, int32_t hoveredPlate,
                                                                const uint8_t* __restrict__ koppen, int32_t hoveredKoppen, uint8_t* __restrict__ cls, int32_t N,
                                                                unsigned long long* __restrict__ counts) {
    __shared__ uint32_t blockCount[4];
    if (threadIdx.x < 4) blockCount[threadIdx.x] = 0u;
    __syncthreads();
    const int32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    uint8_t c = 0;
    if (r < N) { c = P::class_of(r_plate[r], N, kind, hoveredPlate, koppen, r, hoveredKoppen); cls[r] = c; }
    for (int b = 0; b < 4; ++b) {
        const unsigned long long mask = __ballot((c >> b) & 1);
        if ((threadIdx.x & 63) == 0 && mask) atomicAdd(&blockCount[b], (uint32_t)__popcll(mask));
    }
    __syncthreads();
    if (threadIdx.x < 4 && blockCount[threadIdx.x]) atomicAdd(counts + threadIdx.x, (unsigned long long)blockCount[threadIdx.x]);
}
__global__ __launch_bounds__(WO_BLOCK) void k_highlight_tint(const uint8_t* __restrict__ cls, float* __restrict__ rgb, int32_t N) {
    const int32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= N) return;
    const uint8_t c = cls[r];
    if (!c) return;
    const int64_t o = 3 * (int64_t)r;
    const M::Rgb t = P::tint(M::Rgb{rgb[o], rgb[o + 1], rgb[o + 2]}, c);
    rgb[o] = t.r; rgb[o + 1] = t.g; rgb[o + 2] = t.b;
}

__global__ __launch_bounds__(WO_BLOCK) void k_globe_centers(const int32_t* __restrict__ triangles, const float* __restrict__ xyz, const float* __restrict__ e,
                                                            G::Center* __restrict__ out, int32_t numTriangles) {
    const int32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < numTriangles) out[t] = G::center_of(triangles, xyz, e, t);
}

__device__ inline void globe_store_rgb(float* __restrict__ rgb, int32_t r, const M::Rgb& c) {
    rgb[3 * (int64_t)r] = c.r; rgb[3 * (int64_t)r + 1] = c.g; rgb[3 * (int64_t)r + 2] = c.b;
}

__global__ __launch_bounds__(WO_BLOCK) void k_globe_type_colors(int32_t type, const float* __restrict__ e, const uint8_t* __restrict__ koppen, float* __restrict__ rgb, int32_t N) {
    const int32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r < N) globe_store_rgb(rgb, r, M::region_color(type, e[r], koppen ? (int32_t)koppen[r] : 0));
}
__global__ __launch_bounds__(WO_BLOCK) void k_globe_biome_smooth(const float* __restrict__ raw, const int32_t* __restrict__ off, const int32_t* __restrict__ adj,
                                                                 float* __restrict__ rgb, int32_t N) {
    const int32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r < N) globe_store_rgb(rgb, r, M::biome_smooth(raw, off, adj, r));
}
// b and e are read by the ocean-current layers only, range by the layers coloured over their range
__global__ __launch_bounds__(WO_BLOCK) void k_globe_layer_colors(int32_t layer, const float* __restrict__ a, const float* __restrict__ b, const float* __restrict__ e,
                                                                 const uint32_t* __restrict__ range, float* __restrict__ rgb, int32_t N) {
    const int32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= N) return;
    const bool current = M::layer_is_ocean_current(layer);
    const M::RangeBits R = M::layer_needs_range(layer) ? M::RangeBits{range[0], range[1]} : M::RangeBits{0u, 0u};
    globe_store_rgb(rgb, r, M::layer_color(layer, a[r], current ? b[r] : 0.0f, current ? e[r] : 0.0f, R));
}
// slot[seed] = the last row of the table with that seed (the reference's object keeps the last assignment); slot was filled with -1
__global__ __launch_bounds__(WO_BLOCK) void k_globe_plate_slots(const int32_t* __restrict__ seeds, int32_t numPlates, int32_t* slot) {
    const int32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < numPlates) atomicMax(slot + seeds[i], i);             // the entry point checked 0 <= seeds[i] < N
}
__global__ __launch_bounds__(WO_BLOCK) void k_globe_plate_colors(const int32_t* __restrict__ r_plate, const int32_t* __restrict__ slot, const float* __restrict__ plateColors,
                                                                 float* __restrict__ rgb, int32_t N) {
    const int32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r < N) globe_store_rgb(rgb, r, G::plate_color(r_plate[r], N, slot, plateColors));
}

// the workgroup's `floats` floats of `stage` to out, 16 bytes per lane and turn; out is 16-byte aligned (a workgroup's share is 9216 bytes)
__device__ inline void globe_flush(const float* stage, float* __restrict__ out, int32_t floats) {
    const int32_t quads = floats / 4;
    const float4* s4 = reinterpret_cast<const float4*>(stage);
    float4* o4 = reinterpret_cast<float4*>(out);
    for (int32_t q = threadIdx.x; q < quads; q += WO_BLOCK) o4[q] = s4[q];
    for (int32_t i = 4 * quads + threadIdx.x; i < floats; i += WO_BLOCK) out[i] = stage[i];
}

// pos or col may be nullptr; bounds (six words, cleared) is reduced only with pos.  The grid covers numSides exactly: one workgroup per 256 sides.
template <bool STAGED>
__global__ __launch_bounds__(WO_BLOCK) void k_globe_mesh(const int32_t* __restrict__ triangles, const int32_t* __restrict__ halfedges, const G::Center* __restrict__ centers,
                                                         const float* __restrict__ xyz, const float* __restrict__ e, const float* __restrict__ rgb, int32_t numSides,
                                                         float* __restrict__ pos, float* __restrict__ col, uint32_t* __restrict__ bounds) {
    __shared__ __attribute__((aligned(16))) float stage[STAGED ? WO_BLOCK * 9 : 4];
    __shared__ uint32_t blockB[6];
    const int64_t first = (int64_t)blockIdx.x * WO_BLOCK, s = first + threadIdx.x;
    const bool active = s < numSides;
    const int32_t mine = (int32_t)((numSides - first < WO_BLOCK ? numSides - first : WO_BLOCK) * 9);      // floats of this workgroup
    if (threadIdx.x < 6) blockB[threadIdx.x] = 0u;
    const int32_t br = active ? triangles[s] : 0;
    if (pos) {
        float P[9];
        G::BoundsBits b{{0u, 0u, 0u, 0u, 0u, 0u}};
        if (active) {
            const G::Center a = centers[s / 3], c = centers[halfedges[s] / 3];
            const float r[3] = {xyz[3 * (int64_t)br], xyz[3 * (int64_t)br + 1], xyz[3 * (int64_t)br + 2]};
            G::side_positions(a, c, r, e[br], P);
            for (int k = 0; k < 9; ++k) G::bounds_take(b, k % 3, P[k]);
            if (STAGED) { for (int k = 0; k < 9; ++k) stage[threadIdx.x * 9 + k] = P[k]; }
            else { for (int k = 0; k < 9; ++k) pos[9 * s + k] = P[k]; }
        }
        for (int w = 0; w < 6; ++w)
            for (int d = 32; d > 0; d >>= 1) b.w[w] = max(b.w[w], (uint32_t)__shfl_down(b.w[w], d, 64));
        __syncthreads();                                      // blockB is cleared, stage is written
        if ((threadIdx.x & 63) == 0)
            for (int w = 0; w < 6; ++w) if (b.w[w]) atomicMax(&blockB[w], b.w[w]);
        if (STAGED) globe_flush(stage, pos + first * 9, mine);
        __syncthreads();                                      // blockB is complete, stage is free again
        if (threadIdx.x < 6 && blockB[threadIdx.x] > __hip_atomic_load(bounds + threadIdx.x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
            atomicMax(bounds + threadIdx.x, blockB[threadIdx.x]);
    }
    if (col) {
        if (active) {
            const float cr = rgb[3 * (int64_t)br], cg = rgb[3 * (int64_t)br + 1], cb = rgb[3 * (int64_t)br + 2];
            for (int j = 0; j < 3; ++j) {
                if (STAGED) { stage[threadIdx.x * 9 + 3 * j] = cr; stage[threadIdx.x * 9 + 3 * j + 1] = cg; stage[threadIdx.x * 9 + 3 * j + 2] = cb; }
                else { col[9 * s + 3 * j] = cr; col[9 * s + 3 * j + 1] = cg; col[9 * s + 3 * j + 2] = cb; }
            }
        }
        if (STAGED) {
            __syncthreads();
            globe_flush(stage, col + first * 9, mine);
        }
    }
}

// ---- lines: an order-preserving compaction ------------------------------------------------------------------------------------
__global__ __launch_bounds__(WO_BLOCK) void k_globe_line_count(int32_t kind, const int32_t* __restrict__ triangles, const int32_t* __restrict__ halfedges, const float* __restrict__ sp,
                                                               int32_t numSides, int32_t* __restrict__ blockCount) {
    __shared__ int32_t waveCount[GLOBE_WAVES];
    const int64_t s = (int64_t)blockIdx.x * WO_BLOCK + threadIdx.x;
    const bool take = s < numSides && G::side_has_segment(kind, triangles, halfedges, sp, s);
    const unsigned long long mask = __ballot(take);
    if ((threadIdx.x & 63) == 0) waveCount[threadIdx.x >> 6] = (int32_t)__popcll(mask);
    __syncthreads();
    if (threadIdx.x == 0) {
        int32_t n = 0;
        for (int w = 0; w < GLOBE_WAVES; ++w) n += waveCount[w];
        blockCount[blockIdx.x] = n;
    }
}

// One workgroup: counts[0 .. n) become their exclusive prefix sums, *total their sum.  Every thread owns a run of consecutive counts.
__global__ __launch_bounds__(WO_BLOCK) void k_globe_line_scan(int32_t* __restrict__ counts, int32_t n, int32_t* __restrict__ total) {
    __shared__ int32_t part[WO_BLOCK];
    const int32_t per = (n + WO_BLOCK - 1) / WO_BLOCK;
    const int32_t b = min(n, (int32_t)threadIdx.x * per), e = min(n, b + per);
    int32_t sum = 0;
    for (int32_t i = b; i < e; ++i) sum += counts[i];
    part[threadIdx.x] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        int32_t run = 0;
        for (int t = 0; t < WO_BLOCK; ++t) { const int32_t c = part[t]; part[t] = run; run += c; }
        *total = run;
    }
    __syncthreads();
    int32_t run = part[threadIdx.x];
    for (int32_t i = b; i < e; ++i) { const int32_t c = counts[i]; counts[i] = run; run += c; }
}

// capacity segments fit into out; a segment whose place lies behind it is dropped (the entry point asks for numSides / 2, which holds them all)
__global__ __launch_bounds__(WO_BLOCK) void k_globe_line_write(int32_t kind, const int32_t* __restrict__ triangles, const int32_t* __restrict__ halfedges, const float* __restrict__ sp,
                                                               const G::Center* __restrict__ centers, int32_t numSides, const int32_t* __restrict__ blockOffset,
                                                               float* __restrict__ out, int64_t capacity) {
    __shared__ int32_t waveCount[GLOBE_WAVES];
    const int64_t s = (int64_t)blockIdx.x * WO_BLOCK + threadIdx.x;
    const bool take = s < numSides && G::side_has_segment(kind, triangles, halfedges, sp, s);
    const unsigned long long mask = __ballot(take);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) waveCount[wave] = (int32_t)__popcll(mask);
    __syncthreads();
    if (!take) return;
    int64_t at = blockOffset[blockIdx.x];
    for (int w = 0; w < wave; ++w) at += waveCount[w];
    at += __popcll(mask & ((1ull << lane) - 1ull));
    if (at >= capacity) return;
    float seg[6];
    G::line_segment(centers[s / 3], centers[halfedges[s] / 3], G::line_base(kind), seg);
    float2* o = reinterpret_cast<float2*>(out + 6 * at);      // 24 bytes per segment: 8-byte aligned
    o[0] = make_float2(seg[0], seg[1]); o[1] = make_float2(seg[2], seg[3]); o[2] = make_float2(seg[4], seg[5]);
}

static bool globe_sides_ok(const char* fn, wo_planet* p, int32_t numSides, const int32_t* triangles, const int32_t* halfedges) {
    const std::string F = std::string(fn) + ": ";
    if (!triangles || !halfedges) { set_error(F + "null pointer"); return false; }
    if (numSides < 3 || numSides % 3 != 0 || numSides >= (1 << 30)) { set_error(F + "numSides is " + std::to_string(numSides) + ", it must be a multiple of 3 from 3 to 2^30 - 3"); return false; }
    std::string err;
    if (!map_topology_ok(p->N, numSides, triangles, halfedges, err)) { set_error(F + err); return false; }
    return true;
}

// what both mesh entry points check of their outputs
static bool globe_outputs_ok(const char* fn, int32_t numSides, const float* positionsOut, const float* colorsOut, int64_t outFloats) {
    const std::string F = std::string(fn) + ": ";
    if (!positionsOut && !colorsOut) { set_error(F + "positionsOut and colorsOut are both NULL, there is nothing to build"); return false; }
    if (outFloats != (int64_t)numSides * 9) { set_error(F + "a mesh of " + std::to_string(numSides) + " sides takes " + std::to_string((int64_t)numSides * 9) + " floats per array, outFloats is " + std::to_string(outFloats)); return false; }
    return true;
}

// the editor's tints over the region colours, when a highlight state is set
static void globe_tint(wo_planet* p, float* rgb) {
    if (rgb && highlight_classes(p)) launch(p, FAM_HIGHLIGHT, k_highlight_tint, blocks_for(p->N), WO_BLOCK, highlight_classes(p), rgb, p->N);
}

// the tables, the mesh kernel and the copies; rgb holds the region colours (nullptr without colorsOut)
static void globe_mesh_run(wo_planet* p, DeviceArena& T, int32_t numSides, const int32_t* triangles, const int32_t* halfedges, const float* e, const float* rgb,
                           float* positionsOut, float* colorsOut, float bounds[6]) {
    hipStream_t s = p->ctx->stream;
    const size_t floats = (size_t)numSides * 9;
    const int32_t* d_tri = up(T, triangles, (size_t)numSides, s);
    const int32_t* d_he = positionsOut ? up(T, halfedges, (size_t)numSides, s) : nullptr;
    G::Center* centers = nullptr;
    float *pos = nullptr, *col = nullptr;
    uint32_t* d_bounds = T.dev<uint32_t>(6);
    uint32_t* h_bounds = T.pinned<uint32_t>(6);
    if (positionsOut) {
        centers = T.dev<G::Center>((size_t)numSides / 3);
        pos = T.dev<float>(floats);
        WO_HIP(hipMemsetAsync(d_bounds, 0, 24, s));
        launch(p, FAM_GLOBE_TABLES, k_globe_centers, blocks_for(numSides / 3), WO_BLOCK, d_tri, (const float*)p->d_xyz, e, centers, numSides / 3);
    }
    if (colorsOut) col = T.dev<float>(floats);
    auto* kernel = p->opt.globeDirectStores ? k_globe_mesh<false> : k_globe_mesh<true>;
    launch(p, FAM_GLOBE_MESH, kernel, blocks_for(numSides, 1 << 23), WO_BLOCK, d_tri, d_he, (const G::Center*)centers, (const float*)p->d_xyz, e, rgb, numSides, pos, col, d_bounds);
    if (positionsOut) {
        WO_HIP(hipMemcpyAsync(h_bounds, d_bounds, 24, hipMemcpyDeviceToHost, s));
        WO_HIP(hipMemcpyAsync(positionsOut, pos, floats * 4, hipMemcpyDeviceToHost, s));
    }
    if (colorsOut) WO_HIP(hipMemcpyAsync(colorsOut, col, floats * 4, hipMemcpyDeviceToHost, s));
    WO_HIP(hipStreamSynchronize(s));                          // before T frees the temporaries
    if (positionsOut && bounds) G::bounds_decode(h_bounds, bounds);
}

}  // namespace wo

using namespace wo;

extern "C" {

int wo_globe_mesh(wo_planet* p, int32_t numSides, const int32_t* triangles, const int32_t* halfedges, int32_t source, int32_t id, const float* values,
                  const float* r_elevation, float* positionsOut, float* colorsOut, int64_t outFloats, float bounds[6]) {
    const char* fn = "wo_globe_mesh";
    const std::string F = "wo_globe_mesh: ";
    if (!check_planet(p, fn)) return 1;
    if (!globe_outputs_ok(fn, numSides, positionsOut, colorsOut, outFloats)) return 1;
    if (source != G::SOURCE_TYPE && source != G::SOURCE_LAYER) { set_error(F + "unknown colour source " + std::to_string(source)); return 1; }
    const bool layered = source == G::SOURCE_LAYER;
    if (!layered && (id < 0 || id >= M::TYPE_COUNT)) { set_error(F + "unknown map type " + std::to_string(id)); return 1; }
    if (!layered && id == M::TYPE_LANDMASK) { set_error(F + "map type " + std::to_string(id) + " (landmask) is no view of the globe: buildMesh has no such branch"); return 1; }
    if (layered && (id < 0 || id >= M::LAYER_COUNT)) { set_error(F + "unknown map layer " + std::to_string(id)); return 1; }
    if (!globe_sides_ok(fn, p, numSides, triangles, halfedges)) return 1;
    const uint8_t* koppen = nullptr;
    LayerSource S{nullptr, nullptr, nullptr, nullptr};
    int fa = -1, fb = -1;
    const bool current = layered && M::layer_is_ocean_current(id);
    if (colorsOut && !layered) {
        if (values) { set_error(F + "a map type reads the elevation, values must be NULL"); return 1; }
        if (M::type_needs_koppen(id) && !(koppen = koppen_classes(p))) { set_error(F + "no Koppen result on this planet (call wo_classify_koppen first)"); return 1; }
    }
    if (colorsOut && layered) {
        if (id == M::LAYER_DEBUG && !values) { set_error(F + "WO_MAP_LAYER_DEBUG takes its values from the caller, values is NULL"); return 1; }
        if (current && values) { set_error(F + "an ocean-current layer reads two fields, values must be NULL (wo_ocean_upload sets the warmth and the speed)"); return 1; }
        S = layer_source(id);
        if (!values) {                                        // the resident field(s)
            fa = S.block->index(S.a);
            fb = S.b ? S.block->index(S.b) : -1;
            if (!block_require(p, fn, *S.block, bit(fa) | (fb >= 0 ? bit(fb) : 0u), S.hint)) return 1;
        }
    }
    WO_TRY
        const int32_t N = p->N, g = blocks_for(N);
        hipStream_t s = p->ctx->stream;
        DeviceArena T;                                        // the temporaries of this call
        const float* e = stage_elevation(p, T, r_elevation);
        float* rgb = nullptr;
        if (colorsOut) {
            rgb = T.dev<float>(3 * (size_t)N);
            if (!layered && id == M::TYPE_BIOME) {
                float* raw = T.dev<float>(3 * (size_t)N);
                map_launch_biome_raw(p, FAM_GLOBE_REGION_COLORS, e, koppen, raw, N);
                launch(p, FAM_GLOBE_REGION_COLORS, k_globe_biome_smooth, g, WO_BLOCK, (const float*)raw, (const int32_t*)p->d_off, (const int32_t*)p->d_adj, rgb, N);
            } else if (!layered) {
                launch(p, FAM_GLOBE_REGION_COLORS, k_globe_type_colors, g, WO_BLOCK, id, e, koppen, rgb, N);
            } else {
                const float* a = values ? up(T, values, (size_t)N, s) : (const float*)S.block->slot(S.block->get(p), fa, (size_t)N).ptr;
                const float* b = fb >= 0 ? (const float*)S.block->slot(S.block->get(p), fb, (size_t)N).ptr : nullptr;
                uint32_t* range = T.dev<uint32_t>(2);
                if (M::layer_needs_range(id)) {
                    WO_HIP(hipMemsetAsync(range, 0, 8, s));
                    map_launch_range(p, FAM_GLOBE_RANGE, a, N, range);
                }
                launch(p, FAM_GLOBE_REGION_COLORS, k_globe_layer_colors, g, WO_BLOCK, id, a, b, e, (const uint32_t*)range, rgb, N);
            }
        }
        globe_tint(p, rgb);
        globe_mesh_run(p, T, numSides, triangles, halfedges, e, rgb, positionsOut, colorsOut, bounds);
        return 0;
    WO_CATCH("wo_globe_mesh")
}

int wo_globe_mesh_plates(wo_planet* p, int32_t numSides, const int32_t* triangles, const int32_t* halfedges, const int32_t* r_plate, int32_t numPlates,
                         const int32_t* plateSeeds, const float* plateColors, const float* r_elevation, float* positionsOut, float* colorsOut, int64_t outFloats,
                         float bounds[6]) {
    const char* fn = "wo_globe_mesh_plates";
    const std::string F = "wo_globe_mesh_plates: ";
    if (!check_planet(p, fn)) return 1;
    if (!globe_outputs_ok(fn, numSides, positionsOut, colorsOut, outFloats)) return 1;
    if (colorsOut) {
        if (!r_plate) { set_error(F + "the plate view reads r_plate, it is NULL"); return 1; }
        if (numPlates < 0) { set_error(F + "numPlates is " + std::to_string(numPlates)); return 1; }
        if (!plateSeeds || !plateColors) { set_error(F + "the plate view needs a colour table, " + (plateSeeds ? "plateColors" : "plateSeeds") + " is NULL"); return 1; }
        for (int32_t i = 0; i < numPlates; ++i)
            if ((uint32_t)plateSeeds[i] >= (uint32_t)p->N) { set_error(F + "plateSeeds[" + std::to_string(i) + "] = " + std::to_string(plateSeeds[i]) + " is no region of the planet, which has " + std::to_string(p->N)); return 1; }
    }
    if (!globe_sides_ok(fn, p, numSides, triangles, halfedges)) return 1;
    WO_TRY
        const int32_t N = p->N;
        hipStream_t s = p->ctx->stream;
        DeviceArena T;                                        // the temporaries of this call
        const float* e = stage_elevation(p, T, r_elevation);
        float* rgb = nullptr;
        if (colorsOut) {
            rgb = T.dev<float>(3 * (size_t)N);
            int32_t* slot = T.dev<int32_t>((size_t)N);
            WO_HIP(hipMemsetAsync(slot, 0xFF, (size_t)N * 4, s));
            const int32_t* d_plate = up(T, r_plate, (size_t)N, s);
            if (numPlates > 0) {
                const int32_t* d_seeds = up(T, plateSeeds, (size_t)numPlates, s);
                launch(p, FAM_GLOBE_REGION_COLORS, k_globe_plate_slots, blocks_for(numPlates), WO_BLOCK, d_seeds, numPlates, slot);
            }
            const float* d_colors = numPlates > 0 ? up(T, plateColors, 3 * (size_t)numPlates, s) : nullptr;
            launch(p, FAM_GLOBE_REGION_COLORS, k_globe_plate_colors, blocks_for(N), WO_BLOCK, d_plate, (const int32_t*)slot, d_colors, rgb, N);
        }
        globe_tint(p, rgb);
        globe_mesh_run(p, T, numSides, triangles, halfedges, e, rgb, positionsOut, colorsOut, bounds);
        return 0;
    WO_CATCH("wo_globe_mesh_plates")
}

int wo_highlight_set(wo_planet* p, const int32_t* r_plate, int32_t numPending, const int32_t* pendingPlates, const uint8_t* pendingIsOcean, int32_t hoveredPlate,
                     int32_t hoveredKoppen, int64_t counts[4]) {
    const char* fn = "wo_highlight_set";
    const std::string F = "wo_highlight_set: ";
    if (!check_planet(p, fn)) return 1;
    const int32_t N = p->N;
    if (!r_plate) { set_error(F + "r_plate is NULL"); return 1; }
    if (numPending < 0) { set_error(F + "numPending is " + std::to_string(numPending)); return 1; }
    if (numPending > 0 && (!pendingPlates || !pendingIsOcean)) { set_error(F + (pendingPlates ? "pendingIsOcean" : "pendingPlates") + " is NULL with " + std::to_string(numPending) + " pending plates"); return 1; }
    if (numPending > N) { set_error(F + "numPending is " + std::to_string(numPending) + ", the planet has " + std::to_string(N) + " regions and no plate is listed twice"); return 1; }
    if (hoveredPlate >= N) { set_error(F + "hoveredPlate = " + std::to_string(hoveredPlate) + " is no region of the planet, which has " + std::to_string(N)); return 1; }
    {
        std::vector<uint8_t> seen(numPending > 0 ? (size_t)N : 0, 0);
        for (int32_t i = 0; i < numPending; ++i) {
            const int32_t id = pendingPlates[i];
            if ((uint32_t)id >= (uint32_t)N) { set_error(F + "pendingPlates[" + std::to_string(i) + "] = " + std::to_string(id) + " is no region of the planet, which has " + std::to_string(N)); return 1; }
            if (seen[id]) { set_error(F + "pendingPlates[" + std::to_string(i) + "] = " + std::to_string(id) + " is listed twice"); return 1; }
            seen[id] = 1;
        }
    }
    const uint8_t* koppen = nullptr;
    if (hoveredKoppen >= 0 && !(koppen = koppen_classes(p))) { set_error(F + "hoveredKoppen = " + std::to_string(hoveredKoppen) + " but there is no Koppen result on this planet (call wo_classify_koppen first)"); return 1; }
    WO_TRY
        hipStream_t s = p->ctx->stream;
        auto* B = new wo_highlight_block();
        try {
            DeviceArena T;                                    // the temporaries of this call
            B->cls = B->mem.dev<uint8_t>((size_t)N);
            uint8_t* kind = T.dev<uint8_t>((size_t)N);
            unsigned long long* d_counts = T.dev<unsigned long long>(4);
            unsigned long long* h_counts = T.pinned<unsigned long long>(4);
            WO_HIP(hipMemsetAsync(kind, 0, (size_t)N, s));
            WO_HIP(hipMemsetAsync(d_counts, 0, 32, s));
            const int32_t* d_plate = up(T, r_plate, (size_t)N, s);
            if (numPending > 0) {
                const int32_t* d_pending = up(T, pendingPlates, (size_t)numPending, s);
                const uint8_t* d_isOcean = up(T, pendingIsOcean, (size_t)numPending, s);
                launch(p, FAM_HIGHLIGHT, k_highlight_kinds, blocks_for(numPending), WO_BLOCK, d_pending, d_isOcean, numPending, kind);
            }
            launch(p, FAM_HIGHLIGHT, k_highlight_classes, blocks_for(N), WO_BLOCK, d_plate, (const uint8_t*)kind, hoveredPlate, koppen, hoveredKoppen, B->cls, N, d_counts);
            WO_HIP(hipMemcpyAsync(h_counts, d_counts, 32, hipMemcpyDeviceToHost, s));
            WO_HIP(hipStreamSynchronize(s));                  // before T frees the temporaries
            if (counts) for (int b = 0; b < 4; ++b) counts[b] = (int64_t)h_counts[b];
        } catch (...) { delete B; throw; }
        highlight_free(p);                                    // a second set replaces the first
        p->highlight = B;
        return 0;
    WO_CATCH("wo_highlight_set")
}

int wo_highlight_clear(wo_planet* p) {
    if (!check_planet(p, "wo_highlight_clear")) return 1;
    WO_TRY
        WO_HIP(hipStreamSynchronize(p->ctx->stream));
        highlight_free(p);
        return 0;
    WO_CATCH("wo_highlight_clear")
}

int wo_globe_lines(wo_planet* p, int32_t numSides, const int32_t* triangles, const int32_t* halfedges, int32_t kind, const float* r_elevation, const float* superPlates,
                   float* segmentsOut, int64_t capacity, int64_t* count) {
    const char* fn = "wo_globe_lines";
    const std::string F = "wo_globe_lines: ";
    if (!check_planet(p, fn)) return 1;
    if (!segmentsOut || !count) { set_error(F + "null pointer"); return 1; }
    if (kind != G::LINES_WIREFRAME && kind != G::LINES_SUPER_PLATE_BORDERS) { set_error(F + "unknown line kind " + std::to_string(kind)); return 1; }
    if (kind == G::LINES_SUPER_PLATE_BORDERS && !superPlates) { set_error(F + "the super-plate borders read one value per region, superPlates is NULL"); return 1; }
    if (kind == G::LINES_WIREFRAME && superPlates) { set_error(F + "the wireframe reads no super-plate values, superPlates must be NULL"); return 1; }
    if (capacity < (int64_t)numSides / 2) { set_error(F + "a mesh of " + std::to_string(numSides) + " sides can give " + std::to_string(numSides / 2) + " segments, capacity is " + std::to_string(capacity)); return 1; }
    if (!globe_sides_ok(fn, p, numSides, triangles, halfedges)) return 1;
    WO_TRY
        const int32_t N = p->N, numTriangles = numSides / 3, groups = blocks_for(numSides, 1 << 23);
        const int64_t room = (int64_t)numSides / 2;
        hipStream_t s = p->ctx->stream;
        DeviceArena T;                                        // the temporaries of this call
        const float* e = stage_elevation(p, T, r_elevation);
        const int32_t* d_tri = up(T, triangles, (size_t)numSides, s);
        const int32_t* d_he = up(T, halfedges, (size_t)numSides, s);
        const float* d_sp = kind == G::LINES_SUPER_PLATE_BORDERS ? up(T, superPlates, (size_t)N, s) : nullptr;
        G::Center* centers = T.dev<G::Center>((size_t)numTriangles);
        int32_t* offsets = T.dev<int32_t>((size_t)groups);
        int32_t* d_total = T.dev<int32_t>(1);
        int32_t* h_total = T.pinned<int32_t>(1);
        float* out = T.dev<float>(6 * (size_t)room);
        launch(p, FAM_GLOBE_TABLES, k_globe_centers, blocks_for(numTriangles), WO_BLOCK, d_tri, (const float*)p->d_xyz, e, centers, numTriangles);
        launch(p, FAM_GLOBE_LINE_COUNT, k_globe_line_count, groups, WO_BLOCK, kind, d_tri, d_he, d_sp, numSides, offsets);
        launch(p, FAM_GLOBE_LINE_SCAN, k_globe_line_scan, 1, WO_BLOCK, offsets, groups, d_total);
        launch(p, FAM_GLOBE_LINE_WRITE, k_globe_line_write, groups, WO_BLOCK, kind, d_tri, d_he, d_sp, (const G::Center*)centers, numSides, (const int32_t*)offsets, out, room);
        WO_HIP(hipMemcpyAsync(h_total, d_total, 4, hipMemcpyDeviceToHost, s));
        WO_HIP(hipStreamSynchronize(s));
        const int64_t n = *h_total;
        if (n > room) { set_error(F + "the mesh gave " + std::to_string(n) + " segments, more than numSides / 2: two sides name each other's lower index"); return 1; }
        if (n > 0) {
            WO_HIP(hipMemcpyAsync(segmentsOut, out, (size_t)n * 24, hipMemcpyDeviceToHost, s));
            WO_HIP(hipStreamSynchronize(s));                  // before T frees the temporaries
        }
        *count = n;
        return 0;
    WO_CATCH("wo_globe_lines")
}

}  // extern "C"
