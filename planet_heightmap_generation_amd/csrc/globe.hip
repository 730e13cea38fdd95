// The globe mesh on the device (the reference's buildMesh, updateMeshColors and updateSuperPlateBorders, js/planet-mesh.js:620-836,
// :840-957, :533-576): the displaced Voronoi-fan triangles of every side with one colour per region, the Voronoi wireframe and the
// super-plate borders.  The bodies and the contract are in globe_ops.h; everything runs on the planet's resident positions,
// elevation, Koppen block and climate blocks, on its stream.
//
// Launches of wo_globe_mesh / wo_globe_mesh_plates (no host round trip between them; the stream is waited for once, at the end):
//   k_globe_centers [1]        t_xyz and t_elevation of every triangle as one 16-byte record: 2 N records instead of 18 N sums
//   region colours [1-3]       one f32 triple per region, tinted by the highlight state if one is set: view_colors.hip
//   k_globe_mesh [1]           one lane per side: two centre records, the region's position and elevation, the colour; nine floats
//                              of positions and nine of colours per side.  A workgroup's 256 sides are 9216 contiguous bytes of each
//                              output: the lanes put their nine floats into LDS (stride 9, no bank conflict) and the workgroup
//                              stores them 16 bytes per lane and instruction.  The bounds of the stored positions are reduced here
//                              (block_ops.h: block_max_to_global, six words).  Either output may be absent: without positions it is
//                              updateMeshColors.
// Launches of wo_globe_lines, an order-preserving compaction: k_globe_centers [1], k_globe_line_count [1] (per workgroup),
//   k_block_offsets<1> [1] (one workgroup scans the workgroup counts in place and leaves the total), k_globe_line_write [1] (every
//   lane's place is its workgroup's offset + block_ops.h's block_place).  The segment count is waited for before the segments are
//   copied, so that nothing is written behind them.
// The editor's highlight state (wo_highlight_set / wo_highlight_clear; the bodies in pick_ops.h): one class byte per region, kept in a
//   block of its own.  k_highlight_kinds [1] scatters the pending plates' kinds over a cleared table of one byte per region id,
//   k_highlight_classes [1] gives every region its byte and counts the regions per bit (block_ops.h: block_add_to_global, four
//   words).  While the state is set, the colour kernels of view_colors.hip tint the regions whose byte is not 0, on the map and on
//   the globe.
// Memory (device_mem.h): everything is a temporary of the call, in an arena on its stack, but the class bytes, which the highlight
// block owns.
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "../../include/worogen.h"
#include "block_ops.h"
#include "device.h"
#include "globe_ops.h"
#include "pick_ops.h"
#include "view_colors.h"

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
    const bool has[4] = {(c & 1) != 0, (c & 2) != 0, (c & 4) != 0, (c & 8) != 0};
    block_add_to_global<4>(has, blockCount, counts);
}

__global__ __launch_bounds__(WO_BLOCK) void k_globe_centers(const int32_t* __restrict__ triangles, const float* __restrict__ xyz, const float* __restrict__ e,
                                                            G::Center* __restrict__ out, int32_t numTriangles) {
    const int32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < numTriangles) out[t] = G::center_of(triangles, xyz, e, t);
}

// view.hip's way to the kernel above: the globe view reads the same records
void globe_centers(wo_planet* p, int fam, const int32_t* d_tri, const float* e, G::Center* out, int32_t numTriangles) {
    launch(p, fam, k_globe_centers, blocks_for(numTriangles), WO_BLOCK, d_tri, (const float*)p->d_xyz, e, out, numTriangles);
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
        __syncthreads();                                      // blockB is cleared, stage is written
        block_max_to_global<6>(b.w, blockB, bounds);
        if (STAGED) globe_flush(stage, pos + first * 9, mine);
    }
    if (col) {
        if (STAGED) __syncthreads();                          // stage is free again
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
    __shared__ int32_t waveCount[BLOCK_WAVES];
    const int64_t s = (int64_t)blockIdx.x * WO_BLOCK + threadIdx.x;
    const BlockPlace at = block_place(s < numSides && G::side_has_segment(kind, triangles, halfedges, sp, s), waveCount);
    if (threadIdx.x == 0) blockCount[blockIdx.x] = at.total;
}

// capacity segments fit into out; a segment whose place lies behind it is dropped (the entry point asks for numSides / 2, which holds them all)
__global__ __launch_bounds__(WO_BLOCK) void k_globe_line_write(int32_t kind, const int32_t* __restrict__ triangles, const int32_t* __restrict__ halfedges, const float* __restrict__ sp,
                                                               const G::Center* __restrict__ centers, int32_t numSides, const int32_t* __restrict__ blockOffset,
                                                               float* __restrict__ out, int64_t capacity) {
    __shared__ int32_t waveCount[BLOCK_WAVES];
    const int64_t s = (int64_t)blockIdx.x * WO_BLOCK + threadIdx.x;
    const bool take = s < numSides && G::side_has_segment(kind, triangles, halfedges, sp, s);
    const int64_t at = (int64_t)blockOffset[blockIdx.x] + block_place(take, waveCount).place;
    if (!take || at >= capacity) return;
    float seg[6];
    G::line_segment(centers[s / 3], centers[halfedges[s] / 3], G::line_base(kind), seg);
    float2* o = reinterpret_cast<float2*>(out + 6 * at);      // 24 bytes per segment: 8-byte aligned
    o[0] = make_float2(seg[0], seg[1]); o[1] = make_float2(seg[2], seg[3]); o[2] = make_float2(seg[4], seg[5]);
}

// what both mesh entry points check of their outputs
static bool globe_outputs_ok(const char* fn, int32_t numSides, const float* positionsOut, const float* colorsOut, int64_t outFloats) {
    const std::string F = std::string(fn) + ": ";
    if (!positionsOut && !colorsOut) { set_error(F + "positionsOut and colorsOut are both NULL, there is nothing to build"); return false; }
    if (outFloats != (int64_t)numSides * 9) { set_error(F + "a mesh of " + std::to_string(numSides) + " sides takes " + std::to_string((int64_t)numSides * 9) + " floats per array, outFloats is " + std::to_string(outFloats)); return false; }
    return true;
}

// what both mesh entry points do once their outputs are checked: the request's checks around those of the sides, the region
// colours (an f32 triple per region, with colorsOut only), the tables, the mesh kernel and the copies
static int globe_mesh(wo_planet* p, const char* fn, const ViewRequest& q, int32_t numSides, const int32_t* triangles, const int32_t* halfedges, float* positionsOut, float* colorsOut,
                      float bounds[6]) {
    ViewPlan plan;
    if (!view_resolve(fn, p, q, plan, [&] { return sides_ok(fn, p, numSides, triangles, halfedges); })) return 1;
    WO_TRY
        DeviceArena T;                                            // the temporaries of this call
        const float* e = stage_elevation(p, T, q.r_elevation);
        float* rgb = nullptr;
        if (colorsOut) {
            rgb = T.dev<float>(3 * (size_t)p->N);
            view_region_colors(p, T, plan, e, ViewSink{rgb, nullptr, nullptr}, {FAM_GLOBE_REGION_COLORS, FAM_GLOBE_RANGE});
        }
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
        launch(p, FAM_GLOBE_MESH, kernel, blocks_for(numSides, 1 << 23), WO_BLOCK, d_tri, d_he, (const G::Center*)centers, (const float*)p->d_xyz, e, (const float*)rgb, numSides, pos, col, d_bounds);
        if (positionsOut) {
            WO_HIP(hipMemcpyAsync(h_bounds, d_bounds, 24, hipMemcpyDeviceToHost, s));
            WO_HIP(hipMemcpyAsync(positionsOut, pos, floats * 4, hipMemcpyDeviceToHost, s));
        }
        if (colorsOut) WO_HIP(hipMemcpyAsync(colorsOut, col, floats * 4, hipMemcpyDeviceToHost, s));
        WO_HIP(hipStreamSynchronize(s));                          // before T frees the temporaries
        if (positionsOut && bounds) G::bounds_decode(h_bounds, bounds);
        return 0;
    WO_CATCH(fn)
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
    if (source == G::SOURCE_TYPE && id == M::TYPE_LANDMASK) { set_error(F + "map type " + std::to_string(id) + " (landmask) is no view of the globe: buildMesh has no such branch"); return 1; }
    ViewRequest q;
    q.source = source; q.id = id; q.colors = colorsOut != nullptr; q.values = values; q.r_elevation = r_elevation;
    return globe_mesh(p, fn, q, numSides, triangles, halfedges, positionsOut, colorsOut, bounds);
}

int wo_globe_mesh_plates(wo_planet* p, int32_t numSides, const int32_t* triangles, const int32_t* halfedges, const int32_t* r_plate, int32_t numPlates,
                         const int32_t* plateSeeds, const float* plateColors, const float* r_elevation, float* positionsOut, float* colorsOut, int64_t outFloats,
                         float bounds[6]) {
    const char* fn = "wo_globe_mesh_plates";
    if (!check_planet(p, fn)) return 1;
    if (!globe_outputs_ok(fn, numSides, positionsOut, colorsOut, outFloats)) return 1;
    ViewRequest q;
    q.source = VIEW_PLATES; q.colors = colorsOut != nullptr; q.r_elevation = r_elevation;
    q.r_plate = r_plate; q.numPlates = numPlates; q.plateSeeds = plateSeeds; q.plateColors = plateColors;
    return globe_mesh(p, fn, q, numSides, triangles, halfedges, positionsOut, colorsOut, bounds);
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
    if (!sides_ok(fn, p, numSides, triangles, halfedges)) return 1;
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
        launch(p, FAM_GLOBE_LINE_SCAN, k_block_offsets<1>, 1, BLOCK_SCAN_THREADS, offsets, groups, d_total);
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
