// Region outlines on the device: the line where one class of cells ends and another begins, traced into ordered closed rings
// (ours: the reference draws no outline but the loose super-plate border segments).  The bodies and the whole contract are in
// outline_ops.h; everything runs on the planet's stream, on its resident positions, elevation, Koppen block and rivers block.
//
// Launches of wo_outline_build (the host reads M once after the compaction and the ring count once at the end):
//   k_outline_classify [1]       one lane per cell: its int32 class from the source
//   flags [2 + 1]                k_outline_flag_count (boundary flags per workgroup), k_block_offsets<1>, then, with M known,
//                                k_outline_flag_write: slotOf[side] and sideOf[slot], the order-preserving compaction of globe.hip's
//                                and rivers.hip's lines
//   k_outline_succ [1]           succ as slots, the start state of the ranking, and the check that pred(succ(s)) == s lands on a
//                                boundary side (a mesh that is no closed triangulation sets the fault word; every later index stays
//                                inside its array whatever the mesh)
//   k_outline_rank [K]           one round of pointer doubling per launch, K = ceil(log2(max(M, 2))): a lane reads its own 16-byte
//                                record (coalesced) and that of its jump slot (a gather from a random address), and writes one
//                                record.  A round reads what the round before wrote for other slots: two buffers, swapped per round.
//   rings [4]                    k_outline_leader_count (leaders and the sum of their rings' lengths per workgroup),
//                                k_block_offsets<2>, k_outline_ring_number (a leader's ring number is its place among the leaders,
//                                its ring's offset the sum of the lengths before it: ring_start, ring_class, the longest ring),
//                                k_outline_ring_write (sides[ring_start[ring] + rank] = side, ring_of_side, the three corners of
//                                the entry's triangle)
// With M == 0 nothing follows the scan of the flags: three launches, and nothing is launched over zero elements.
// Launches of wo_outline_positions and wo_outline_lonlat: k_outline_positions / k_outline_lonlat [1], one lane per entry.
// Memory (device_mem.h): the results live in the outline block's arena; everything else is a temporary of the call.
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstring>
#include <memory>
#include <stdexcept>
#include <string>

#include "../../include/worogen.h"
#include "block_ops.h"
#include "device.h"
#include "outline_ops.h"
#include "rivers_block.h"
#include "view_colors.h"

namespace O = wo::outline;

static_assert(O::SOURCE_COAST == WO_OUTLINE_COAST && O::SOURCE_LAKES == WO_OUTLINE_LAKES && O::SOURCE_KOPPEN == WO_OUTLINE_KOPPEN && O::SOURCE_LEVELS == WO_OUTLINE_LEVELS &&
              O::SOURCE_VALUES == WO_OUTLINE_VALUES, "the sources of outline_ops.h are those of worogen.h");
static_assert(sizeof(O::Rank) == 16, "one 16-byte load per gather");

struct wo_outline_block {
    wo::DeviceArena mem;                 // owns every buffer below
    int32_t M = 0, R = 0;
    int32_t* sides = nullptr;            // [M]
    int32_t* ringStart = nullptr;        // [R + 1]
    int32_t* ringClass = nullptr;        // [R]
    int32_t* ringOfSide = nullptr;       // [M]
    int32_t* corners = nullptr;          // [3 M]: the corners of triangle it(sides[k]), what the vertices are made of
    wo_outline_info info{};
};

namespace wo {

void outline_free(wo_planet* p) { delete p->outline; p->outline = nullptr; }

enum { CTL_RINGS = 0, CTL_LENGTHS = 1, CTL_LONGEST = 2, CTL_FAULT = 3, CTL_COUNT = 4 };      // the call's words: k_block_offsets<2> writes the first two

struct ClassSource { int32_t source; const float* e; const float* lake; const uint8_t* koppen; const int32_t* values; O::Levels levels; };

__global__ __launch_bounds__(WO_BLOCK) void k_outline_classify(ClassSource S, int32_t N, int32_t* __restrict__ cls) {
    const int32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= N) return;
    int32_t c;
    switch (S.source) {
        case O::SOURCE_COAST: c = O::class_coast(S.e[r]); break;
        case O::SOURCE_LAKES: c = O::class_lake(S.lake[r]); break;
        case O::SOURCE_KOPPEN: c = (int32_t)S.koppen[r]; break;
        case O::SOURCE_LEVELS: c = O::class_levels(S.e[r], S.levels); break;
        default: c = S.values[r]; break;
    }
    cls[r] = c;
}

// The grid covers numSides exactly: one workgroup per 256 sides.
__global__ __launch_bounds__(WO_BLOCK) void k_outline_flag_count(const int32_t* __restrict__ triangles, const int32_t* __restrict__ halfedges, const int32_t* __restrict__ cls,
                                                                 int32_t onlyClass, int32_t numSides, int32_t* __restrict__ blockCount) {
    __shared__ int32_t waveCount[BLOCK_WAVES];
    const int64_t s = (int64_t)blockIdx.x * WO_BLOCK + threadIdx.x;
    const BlockPlace at = block_place(s < numSides && O::is_boundary(triangles, halfedges, cls, onlyClass, (int32_t)s), waveCount);
    if (threadIdx.x == 0) blockCount[blockIdx.x] = at.total;
}

// slotOf was filled with -1; a flagged side whose place lies behind M is dropped (there is none: M is the count of the same flags)
__global__ __launch_bounds__(WO_BLOCK) void k_outline_flag_write(const int32_t* __restrict__ triangles, const int32_t* __restrict__ halfedges, const int32_t* __restrict__ cls,
                                                                 int32_t onlyClass, int32_t numSides, const int32_t* __restrict__ blockOffset, int32_t M,
                                                                 int32_t* __restrict__ slotOf, int32_t* __restrict__ sideOf) {
    __shared__ int32_t waveCount[BLOCK_WAVES];
    const int64_t s = (int64_t)blockIdx.x * WO_BLOCK + threadIdx.x;
    const bool take = s < numSides && O::is_boundary(triangles, halfedges, cls, onlyClass, (int32_t)s);
    const int64_t at = (int64_t)blockOffset[blockIdx.x] + block_place(take, waveCount).place;
    if (!take || at >= M) return;
    slotOf[s] = (int32_t)at;
    sideOf[at] = (int32_t)s;
}

// A successor that is no boundary side, or whose predecessor is another side, sets the fault word and points at the slot itself:
// succ is then still a map into [0, M).
__global__ __launch_bounds__(WO_BLOCK) void k_outline_succ(const int32_t* __restrict__ triangles, const int32_t* __restrict__ halfedges, const int32_t* __restrict__ cls,
                                                           const int32_t* __restrict__ sideOf, const int32_t* __restrict__ slotOf, int32_t M,
                                                           int32_t* __restrict__ succSlot, O::Rank* __restrict__ state, int32_t* __restrict__ ctl) {
    const int64_t i = (int64_t)blockIdx.x * WO_BLOCK + threadIdx.x;
    if (i >= M) return;
    const int32_t s = sideOf[i];
    const int32_t t = O::succ_side(triangles, halfedges, cls, s);
    int32_t j = slotOf[t];
    if ((uint32_t)j >= (uint32_t)M || O::pred_side(triangles, halfedges, cls, t) != s) { ctl[CTL_FAULT] = 1; j = (int32_t)i; }
    succSlot[i] = j;
    state[i] = O::rank_start((int32_t)i, j);
}

// in: the states after the rounds so far, out: after one more; span = 2^(rounds so far).  in and out are different buffers.
__global__ __launch_bounds__(WO_BLOCK) void k_outline_rank(const O::Rank* __restrict__ in, O::Rank* __restrict__ out, int32_t span, int32_t M) {
    const int64_t i = (int64_t)blockIdx.x * WO_BLOCK + threadIdx.x;
    if (i >= M) return;
    const O::Rank mine = in[i];
    const O::Rank far = in[mine.jump];                        // jump is a slot: succ maps into [0, M) (k_outline_succ)
    out[i] = O::rank_round(mine, far, span);
}

// the length of the ring that slot i leads
__device__ inline int32_t ring_length(const O::Rank* __restrict__ state, const int32_t* __restrict__ succSlot, int64_t i) { return state[succSlot[i]].dist + 1; }

// The workgroup calls it.  The sum of v over the lanes before this one, in thread order.  waveSum: BLOCK_WAVES words.
__device__ inline int32_t block_sum_before(int32_t v, int32_t* waveSum) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int32_t inc = v;
    for (int d = 1; d < 64; d <<= 1) {
        const int32_t u = __shfl_up(inc, d, 64);
        if (lane >= d) inc += u;
    }
    if (lane == 63) waveSum[wave] = inc;
    __syncthreads();
    int32_t before = inc - v;
    for (int w = 0; w < wave; ++w) before += waveSum[w];
    return before;
}

// counts[b][0]: the leaders of workgroup b, counts[b][1]: the sum of their rings' lengths.  The grid covers M exactly.
__global__ __launch_bounds__(WO_BLOCK) void k_outline_leader_count(const O::Rank* __restrict__ state, const int32_t* __restrict__ succSlot, int32_t M, int32_t* __restrict__ counts) {
    __shared__ int32_t waveCount[BLOCK_WAVES];
    __shared__ int32_t waveSum[BLOCK_WAVES];
    const int64_t i = (int64_t)blockIdx.x * WO_BLOCK + threadIdx.x;
    const bool leader = i < M && state[i].least == (int32_t)i;
    const int32_t len = leader ? ring_length(state, succSlot, i) : 0;
    const BlockPlace at = block_place(leader, waveCount);
    const int32_t before = block_sum_before(len, waveSum);
    if (threadIdx.x == WO_BLOCK - 1) { counts[2 * (int64_t)blockIdx.x] = at.total; counts[2 * (int64_t)blockIdx.x + 1] = before + len; }
}

// offsets: counts after k_block_offsets<2>.  A ring whose number or offset leaves [0, M) (a faulted mesh) is dropped.
__global__ __launch_bounds__(WO_BLOCK) void k_outline_ring_number(const O::Rank* __restrict__ state, const int32_t* __restrict__ succSlot, const int32_t* __restrict__ sideOf,
                                                                  const int32_t* __restrict__ triangles, const int32_t* __restrict__ cls, const int32_t* __restrict__ offsets, int32_t M,
                                                                  int32_t* __restrict__ ringOfSlot, int32_t* __restrict__ ringStart, int32_t* __restrict__ ringLen,
                                                                  int32_t* __restrict__ ringClass, int32_t* __restrict__ ctl) {
    __shared__ int32_t waveCount[BLOCK_WAVES];
    __shared__ int32_t waveSum[BLOCK_WAVES];
    __shared__ uint32_t blockLongest[1];
    if (threadIdx.x == 0) blockLongest[0] = 0u;
    const int64_t i = (int64_t)blockIdx.x * WO_BLOCK + threadIdx.x;
    const bool leader = i < M && state[i].least == (int32_t)i;
    const int32_t len = leader ? ring_length(state, succSlot, i) : 0;
    const int64_t ring = (int64_t)offsets[2 * (int64_t)blockIdx.x] + block_place(leader, waveCount).place;
    const int64_t start = (int64_t)offsets[2 * (int64_t)blockIdx.x + 1] + block_sum_before(len, waveSum);      // (its barrier: blockLongest is cleared)
    if (leader && ring < M && start < M) {
        ringOfSlot[i] = (int32_t)ring;
        ringStart[ring] = (int32_t)start;
        ringLen[ring] = len;
        ringClass[ring] = cls[triangles[sideOf[i]]];
    }
    const uint32_t longest[1] = {(uint32_t)len};
    block_max_to_global<1>(longest, blockLongest, reinterpret_cast<uint32_t*>(ctl + CTL_LONGEST));
}

// ringOfSlot was filled with -1.  An entry whose place leaves [0, M) (a faulted mesh) sets the fault word and is dropped.
__global__ __launch_bounds__(WO_BLOCK) void k_outline_ring_write(const O::Rank* __restrict__ state, const int32_t* __restrict__ ringOfSlot, const int32_t* __restrict__ ringStart,
                                                                 const int32_t* __restrict__ ringLen, const int32_t* __restrict__ sideOf, const int32_t* __restrict__ triangles, int32_t M,
                                                                 int32_t* __restrict__ sides, int32_t* __restrict__ ringOfSide, int32_t* __restrict__ corners, int32_t* __restrict__ ctl) {
    const int64_t i = (int64_t)blockIdx.x * WO_BLOCK + threadIdx.x;
    if (i >= M) return;
    const O::Rank mine = state[i];
    const int32_t ring = (uint32_t)mine.least < (uint32_t)M ? ringOfSlot[mine.least] : -1;
    if (ring < 0) { ctl[CTL_FAULT] = 1; return; }
    const int32_t len = ringLen[ring];
    const int64_t at = len > 0 ? (int64_t)ringStart[ring] + O::rank_in_ring(len, mine.dist % len) : -1;
    if (at < 0 || at >= M) { ctl[CTL_FAULT] = 1; return; }
    const int32_t s = sideOf[i];
    sides[at] = s;
    ringOfSide[at] = ring;
    const int32_t t3 = s - s % 3;
    corners[3 * at] = triangles[t3]; corners[3 * at + 1] = triangles[t3 + 1]; corners[3 * at + 2] = triangles[t3 + 2];
}

__global__ __launch_bounds__(WO_BLOCK) void k_outline_positions(const int32_t* __restrict__ corners, const float* __restrict__ xyz, const float* __restrict__ e, double base, int32_t M,
                                                                float* __restrict__ out) {
    const int64_t k = (int64_t)blockIdx.x * WO_BLOCK + threadIdx.x;
    if (k >= M) return;
    float v[3];
    O::vertex_position(corners, xyz, e, k, base, v);
    out[3 * k] = v[0]; out[3 * k + 1] = v[1]; out[3 * k + 2] = v[2];
}

__global__ __launch_bounds__(WO_BLOCK) void k_outline_lonlat(const int32_t* __restrict__ corners, const float* __restrict__ xyz, int32_t M, double2* __restrict__ out) {
    const int64_t k = (int64_t)blockIdx.x * WO_BLOCK + threadIdx.x;
    if (k >= M) return;
    const map::LonLat v = O::vertex_lonlat(corners, xyz, k);
    out[k] = make_double2(v.lon, v.lat);
}

// the extra mesh check of the outlines: every half-edge names the side that names it
static bool halfedges_symmetric(const char* fn, int32_t numSides, const int32_t* halfedges) {
    std::atomic<int64_t> bad{-1};
    parallel_ranges(numSides, [&](int64_t b, int64_t e, int) {
        for (int64_t s = b; s < e; ++s) if (halfedges[halfedges[s]] != s) bad.store(s);
    });
    if (bad.load() < 0) return true;
    int64_t s = 0;
    while (halfedges[halfedges[s]] == s) ++s;                 // the first offender, whichever the threads found
    set_error(std::string(fn) + ": half-edge not symmetric: halfedges[" + std::to_string(s) + "] = " + std::to_string(halfedges[s]) + ", but halfedges[" + std::to_string(halfedges[s]) +
              "] = " + std::to_string(halfedges[halfedges[s]]));
    return false;
}

static const char* const kSourceNames[O::SOURCE_COUNT] = {"WO_OUTLINE_COAST", "WO_OUTLINE_LAKES", "WO_OUTLINE_KOPPEN", "WO_OUTLINE_LEVELS", "WO_OUTLINE_VALUES"};

// the block of one build; throws on a device error, returns nullptr with the error set on a mesh the kernels found at fault
static std::unique_ptr<wo_outline_block> outline_run(wo_planet* p, const char* fn, int32_t numSides, const int32_t* triangles, const int32_t* halfedges, int32_t source,
                                                     const float* r_elevation, const int32_t* values, const float* levels, int32_t numLevels, int32_t onlyClass) {
    const int32_t N = p->N, groups = blocks_for(numSides, 1 << 23);
    hipStream_t s = p->ctx->stream;
    int32_t launches = 0;
    const auto run = [&](int fam, auto kernel, int grid, int block, auto... args) { ++launches; launch(p, fam, kernel, grid, block, args...); };
    std::unique_ptr<wo_outline_block> block(new wo_outline_block());
    wo_outline_block* B = block.get();
    DeviceArena T;                                            // the temporaries of this call
    ClassSource S{source, nullptr, nullptr, nullptr, nullptr, {}};
    if (source == O::SOURCE_COAST || source == O::SOURCE_LEVELS) S.e = stage_elevation(p, T, r_elevation);
    if (source == O::SOURCE_LAKES) S.lake = p->rivers->lake;
    if (source == O::SOURCE_KOPPEN) S.koppen = koppen_classes(p);
    if (source == O::SOURCE_VALUES) S.values = up(T, values, (size_t)N, s);
    S.levels.n = source == O::SOURCE_LEVELS ? numLevels : 0;
    for (int32_t k = 0; k < O::MAX_LEVELS; ++k) S.levels.v[k] = k < S.levels.n ? levels[k] : 0.0f;
    const int32_t* d_tri = up(T, triangles, (size_t)numSides, s);
    const int32_t* d_he = up(T, halfedges, (size_t)numSides, s);
    int32_t* cls = T.dev<int32_t>((size_t)N);
    int32_t* offsets = T.dev<int32_t>((size_t)groups);
    int32_t* d_total = T.dev<int32_t>(1);
    int32_t* ctl = T.dev<int32_t>(CTL_COUNT);
    int32_t* h_words = T.pinned<int32_t>(1 + CTL_COUNT);      // M, then the call's words
    run(FAM_OUTLINE_CLASSIFY, k_outline_classify, blocks_for(N), WO_BLOCK, S, N, cls);
    run(FAM_OUTLINE_FLAGS, k_outline_flag_count, groups, WO_BLOCK, d_tri, d_he, (const int32_t*)cls, onlyClass, numSides, offsets);
    run(FAM_OUTLINE_FLAGS, k_block_offsets<1>, 1, BLOCK_SCAN_THREADS, offsets, groups, d_total);
    WO_HIP(hipMemcpyAsync(h_words, d_total, 4, hipMemcpyDeviceToHost, s));
    WO_HIP(hipStreamSynchronize(s));
    const int32_t M = h_words[0];
    if (M < 0 || M > numSides) throw std::runtime_error("the compaction counted " + std::to_string(M) + " boundary sides of " + std::to_string(numSides));
    wo_outline_info I{};
    I.boundarySides = M;
    if (M == 0) {                                             // a valid result: no ring, ring_start == {0}
        B->ringStart = B->mem.dev<int32_t>(1);
        WO_HIP(hipMemsetAsync(B->ringStart, 0, 4, s));
        WO_HIP(hipStreamSynchronize(s));                      // before T frees the temporaries
        I.launches = launches;
        B->info = I;
        return block;
    }
    const size_t m = (size_t)M;
    const int32_t groupsM = blocks_for(M, 1 << 23);
    B->sides = B->mem.dev<int32_t>(m);
    B->ringOfSide = B->mem.dev<int32_t>(m);
    B->corners = B->mem.dev<int32_t>(3 * m);
    int32_t* slotOf = T.dev<int32_t>((size_t)numSides);
    int32_t* sideOf = T.dev<int32_t>(m);
    int32_t* succSlot = T.dev<int32_t>(m);
    O::Rank* state[2] = {T.dev<O::Rank>(m), T.dev<O::Rank>(m)};
    int32_t* counts = T.dev<int32_t>(2 * (size_t)groupsM);
    int32_t* ringOfSlot = T.dev<int32_t>(m);
    int32_t* ringStart = T.dev<int32_t>(m + 1);
    int32_t* ringLen = T.dev<int32_t>(m);
    int32_t* ringClass = T.dev<int32_t>(m);
    WO_HIP(hipMemsetAsync(ctl, 0, CTL_COUNT * 4, s));
    WO_HIP(hipMemsetAsync(slotOf, 0xFF, (size_t)numSides * 4, s));
    WO_HIP(hipMemsetAsync(ringOfSlot, 0xFF, m * 4, s));
    // a faulted mesh leaves entries unwritten: they read 0, never what the memory held before
    WO_HIP(hipMemsetAsync(B->sides, 0, m * 4, s));
    WO_HIP(hipMemsetAsync(B->ringOfSide, 0, m * 4, s));
    WO_HIP(hipMemsetAsync(B->corners, 0, 3 * m * 4, s));
    WO_HIP(hipMemsetAsync(ringStart, 0, (m + 1) * 4, s));
    WO_HIP(hipMemsetAsync(ringLen, 0, m * 4, s));
    WO_HIP(hipMemsetAsync(ringClass, 0, m * 4, s));
    run(FAM_OUTLINE_FLAGS, k_outline_flag_write, groups, WO_BLOCK, d_tri, d_he, (const int32_t*)cls, onlyClass, numSides, (const int32_t*)offsets, M, slotOf, sideOf);
    run(FAM_OUTLINE_SUCC, k_outline_succ, groupsM, WO_BLOCK, d_tri, d_he, (const int32_t*)cls, (const int32_t*)sideOf, (const int32_t*)slotOf, M, succSlot, state[0], ctl);
    const int32_t K = O::rank_rounds(M);
    int cur = 0;
    for (int32_t k = 0; k < K; ++k, cur ^= 1) run(FAM_OUTLINE_RANK, k_outline_rank, groupsM, WO_BLOCK, (const O::Rank*)state[cur], state[cur ^ 1], (int32_t)1 << k, M);
    const O::Rank* ranked = state[cur];
    run(FAM_OUTLINE_RINGS, k_outline_leader_count, groupsM, WO_BLOCK, ranked, (const int32_t*)succSlot, M, counts);
    run(FAM_OUTLINE_RINGS, k_block_offsets<2>, 1, BLOCK_SCAN_THREADS, counts, groupsM, ctl + CTL_RINGS);
    run(FAM_OUTLINE_RINGS, k_outline_ring_number, groupsM, WO_BLOCK, ranked, (const int32_t*)succSlot, (const int32_t*)sideOf, d_tri, (const int32_t*)cls, (const int32_t*)counts, M,
        ringOfSlot, ringStart, ringLen, ringClass, ctl);
    run(FAM_OUTLINE_RINGS, k_outline_ring_write, groupsM, WO_BLOCK, ranked, (const int32_t*)ringOfSlot, (const int32_t*)ringStart, (const int32_t*)ringLen, (const int32_t*)sideOf, d_tri, M,
        B->sides, B->ringOfSide, B->corners, ctl);
    WO_HIP(hipMemcpyAsync(h_words + 1, ctl, CTL_COUNT * 4, hipMemcpyDeviceToHost, s));
    WO_HIP(hipStreamSynchronize(s));
    const int32_t* H = h_words + 1;
    const int32_t R = H[CTL_RINGS];
    if (H[CTL_FAULT] || R < 1 || R > M || H[CTL_LENGTHS] != M) {
        set_error(std::string(fn) + ": the boundary sides form no closed rings (" + std::to_string(M) + " boundary sides, " + std::to_string(R) + " leaders, lengths that sum to " +
                  std::to_string(H[CTL_LENGTHS]) + "): the mesh is no closed triangulation");
        return nullptr;
    }
    B->ringStart = B->mem.dev<int32_t>((size_t)R + 1);
    B->ringClass = B->mem.dev<int32_t>((size_t)R);
    WO_HIP(hipMemcpyAsync(B->ringStart, ringStart, (size_t)R * 4, hipMemcpyDeviceToDevice, s));
    WO_HIP(hipMemcpyAsync(B->ringStart + R, h_words, 4, hipMemcpyHostToDevice, s));      // the closing entry: M
    WO_HIP(hipMemcpyAsync(B->ringClass, ringClass, (size_t)R * 4, hipMemcpyDeviceToDevice, s));
    WO_HIP(hipStreamSynchronize(s));                          // before T frees the temporaries
    B->M = M; B->R = R;
    I.rings = R; I.longestRing = H[CTL_LONGEST]; I.rounds = K; I.launches = launches;
    B->info = I;
    return block;
}

static bool outline_require(const wo_planet* p, const char* fn) {
    if (p->outline) return true;
    set_error(std::string(fn) + ": no outline result on this planet (call wo_outline_build first)");
    return false;
}

}  // namespace wo

using namespace wo;

extern "C" {

int wo_outline_build(wo_planet* p, int32_t numSides, const int32_t* triangles, const int32_t* halfedges, int32_t source, const float* r_elevation, const int32_t* values,
                     const float* levels, int32_t numLevels, int32_t onlyClass, wo_outline_info* info) {
    const char* fn = "wo_outline_build";
    const std::string F = "wo_outline_build: ";
    if (!check_planet(p, fn)) return 1;
    if (source < 0 || source >= O::SOURCE_COUNT) { set_error(F + "unknown source " + std::to_string(source)); return 1; }
    const std::string name = kSourceNames[source];
    if (r_elevation && source != O::SOURCE_COAST && source != O::SOURCE_LEVELS) { set_error(F + name + " reads no elevation, r_elevation must be NULL"); return 1; }
    if (values && source != O::SOURCE_VALUES) { set_error(F + name + " reads no values, values must be NULL"); return 1; }
    if (!values && source == O::SOURCE_VALUES) { set_error(F + "WO_OUTLINE_VALUES takes one int32 per region from the caller, values is NULL"); return 1; }
    if (source != O::SOURCE_LEVELS && (levels || numLevels != 0)) { set_error(F + name + " reads no levels, levels must be NULL and numLevels 0 (it is " + std::to_string(numLevels) + ")"); return 1; }
    if (source == O::SOURCE_LEVELS) {
        if (!levels) { set_error(F + "WO_OUTLINE_LEVELS takes its levels from the caller, levels is NULL"); return 1; }
        if (numLevels < 1 || numLevels > O::MAX_LEVELS) { set_error(F + "numLevels is " + std::to_string(numLevels) + ", it must be from 1 to " + std::to_string(O::MAX_LEVELS)); return 1; }
        const int32_t k = O::levels_offender(levels, numLevels);
        if (k >= 0) { set_error(F + "levels[" + std::to_string(k) + "] = " + std::to_string(levels[k]) + ": the levels must be finite and strictly ascending"); return 1; }
    }
    if (onlyClass < -1) { set_error(F + "onlyClass is " + std::to_string(onlyClass) + ", it must be a class or -1 for every class"); return 1; }
    if (source == O::SOURCE_LAKES && !block_require(p, fn, rivers_desc(), rivers_desc().all(), nullptr)) return 1;
    if (source == O::SOURCE_KOPPEN && !koppen_classes(p)) { set_error(F + "no Koppen result on this planet (call wo_classify_koppen first)"); return 1; }
    if (!sides_ok(fn, p, numSides, triangles, halfedges)) return 1;
    if (!halfedges_symmetric(fn, numSides, halfedges)) return 1;
    WO_TRY
        std::unique_ptr<wo_outline_block> B = outline_run(p, fn, numSides, triangles, halfedges, source, r_elevation, values, levels, numLevels, onlyClass);
        if (!B) return 1;
        if (info) *info = B->info;
        outline_free(p);                                      // a second build replaces the first
        p->outline = B.release();
        return 0;
    WO_CATCH(fn)
}

int wo_outline_download(wo_planet* p, const char* field, void* out, int64_t outBytes) {
    const char* fn = "wo_outline_download";
    const std::string F = "wo_outline_download: ";
    if (!check_planet(p, fn)) return 1;
    if (!field) { set_error(F + "null pointer"); return 1; }
    if (!outline_require(p, fn)) return 1;
    const wo_outline_block* B = p->outline;
    const void* src = nullptr;
    int64_t bytes = 0;
    if (!std::strcmp(field, "sides")) { src = B->sides; bytes = 4 * (int64_t)B->M; }
    else if (!std::strcmp(field, "ring_start")) { src = B->ringStart; bytes = 4 * ((int64_t)B->R + 1); }
    else if (!std::strcmp(field, "ring_class")) { src = B->ringClass; bytes = 4 * (int64_t)B->R; }
    else if (!std::strcmp(field, "ring_of_side")) { src = B->ringOfSide; bytes = 4 * (int64_t)B->M; }
    else { set_error(F + "unknown field '" + field + "'"); return 1; }
    if (outBytes < bytes) { set_error(F + field + " needs " + std::to_string(bytes) + " bytes, out has " + std::to_string(outBytes)); return 1; }
    if (bytes == 0) return 0;
    if (!out) { set_error(F + "null pointer"); return 1; }
    WO_TRY
        WO_HIP(hipMemcpyAsync(out, src, (size_t)bytes, hipMemcpyDeviceToHost, p->ctx->stream));
        WO_HIP(hipStreamSynchronize(p->ctx->stream));
        return 0;
    WO_CATCH(fn)
}

int wo_outline_positions(wo_planet* p, double base, const float* r_elevation, float* xyzOut, int64_t outFloats) {
    const char* fn = "wo_outline_positions";
    const std::string F = "wo_outline_positions: ";
    if (!check_planet(p, fn)) return 1;
    if (!(base - base == 0.0)) { set_error(F + "base is " + std::to_string(base) + ", it must be finite"); return 1; }
    if (!outline_require(p, fn)) return 1;
    const wo_outline_block* B = p->outline;
    const int64_t floats = 3 * (int64_t)B->M;
    if (outFloats < floats) { set_error(F + "an outline of " + std::to_string(B->M) + " sides takes " + std::to_string(floats) + " floats, outFloats is " + std::to_string(outFloats)); return 1; }
    if (floats == 0) return 0;
    if (!xyzOut) { set_error(F + "null pointer"); return 1; }
    WO_TRY
        hipStream_t s = p->ctx->stream;
        DeviceArena T;                                        // the temporaries of this call
        const float* e = stage_elevation(p, T, r_elevation);
        float* out = T.dev<float>((size_t)floats);
        launch(p, FAM_OUTLINE_POSITIONS, k_outline_positions, blocks_for(B->M, 1 << 23), WO_BLOCK, (const int32_t*)B->corners, (const float*)p->d_xyz, e, base, B->M, out);
        WO_HIP(hipMemcpyAsync(xyzOut, out, (size_t)floats * 4, hipMemcpyDeviceToHost, s));
        WO_HIP(hipStreamSynchronize(s));                      // before T frees the temporaries
        return 0;
    WO_CATCH(fn)
}

int wo_outline_lonlat(wo_planet* p, double* lonLatOut, int64_t outDoubles) {
    const char* fn = "wo_outline_lonlat";
    const std::string F = "wo_outline_lonlat: ";
    if (!check_planet(p, fn)) return 1;
    if (!outline_require(p, fn)) return 1;
    const wo_outline_block* B = p->outline;
    const int64_t doubles = 2 * (int64_t)B->M;
    if (outDoubles < doubles) { set_error(F + "an outline of " + std::to_string(B->M) + " sides takes " + std::to_string(doubles) + " doubles, outDoubles is " + std::to_string(outDoubles)); return 1; }
    if (doubles == 0) return 0;
    if (!lonLatOut) { set_error(F + "null pointer"); return 1; }
    WO_TRY
        hipStream_t s = p->ctx->stream;
        DeviceArena T;                                        // the temporaries of this call
        double2* out = T.dev<double2>((size_t)B->M);
        launch(p, FAM_OUTLINE_POSITIONS, k_outline_lonlat, blocks_for(B->M, 1 << 23), WO_BLOCK, (const int32_t*)B->corners, (const float*)p->d_xyz, B->M, out);
        WO_HIP(hipMemcpyAsync(lonLatOut, out, (size_t)doubles * 8, hipMemcpyDeviceToHost, s));
        WO_HIP(hipStreamSynchronize(s));                      // before T frees the temporaries
        return 0;
    WO_CATCH(fn)
}

int wo_outline_free(wo_planet* p) {
    if (!check_planet(p, "wo_outline_free")) return 1;
    WO_TRY
        WO_HIP(hipStreamSynchronize(p->ctx->stream));
        outline_free(p);
        return 0;
    WO_CATCH("wo_outline_free")
}

}  // extern "C"
