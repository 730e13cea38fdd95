// Rivers and lakes on the device: the drainage of the final terrain, its depressions resolved, the discharge, the river lines and the
// map tint, on the planet's resident mesh and stream.  The per-cell bodies, the host tree walk and the whole contract are in
// rivers_ops.h; the results stay in the planet's rivers block (rivers_block.h).
//
// Launch sequence of wo_compute_rivers (launches at N cells, P pits and R contraction rounds in brackets):
//   receivers      k_rivers_receivers [1]: land test, receiver, q and the start of the basin search per cell; land cells and pits counted
//   basins         k_rivers_jump x (ceil(log2 N) + 1): pointer jumping in place on the basin field.  A cell points at a pit (itself for
//                  the pit), at -1 once its chain is known to reach the ocean, or at a cell further down; every launch at least doubles
//                  the distance, so the count needs no read-back
//   pits           k_rivers_pits [1] (the pit list, one atomic per wave), k_rivers_pit_index [1], k_rivers_cell_pit [1]
//                  -- the one wait for P --
//   contraction    per round k_rivers_offer [1]: every land cell of a component that has not merged with the drained class sends the
//                  lowest key of its cross-component passes by one 64-bit atomicMin into its component's slot; k_rivers_hook [1]: every
//                  root decodes its slot, records the pass and names the component it hooks to; k_rivers_relabel [1]: every pit
//                  follows the hooks from its old root to the new one.  Then the host reads ONE word, the number of hooks so far: the
//                  rounds end when it stops growing or reaches P.  R is about log2 of the longest chain of basins.
//   tree walk      the chosen passes (24 bytes per pit) come to the host, rivers::resolve_spills roots them at the drained class and
//                  gives spillTo and W per pit, which go back: O(P), nothing of the size of the cells or the edges crosses
//   apply          k_rivers_apply [1]: final receivers, lake levels, the donor count of every receiver
//   discharge      k_rivers_climb [1]: the last-arriver climb (below)
//   finish         k_rivers_finish [1]: r_river_flow, the lake cells counted
// wo_river_lines is the order-preserving compaction of globe.hip's lines over the cells: k_rivers_line_count [1], k_block_offsets<1>
// [1], k_rivers_line_write [1].  wo_map_color_rivers (map.hip) runs wo_map_color's launches with k_rivers_tint [1] between the region
// colours and the pixels.
// Memory (device_mem.h): the five fields and the counters live in the block; everything else is a temporary of the call's arena.
// All values are written with plain vector stores or atomics.
#include <hip/hip_runtime.h>

#include <cstring>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/worogen.h"
#include "block_ops.h"
#include "device.h"
#include "precip_block.h"
#include "rivers_block.h"
#include "rivers_ops.h"
#include "stage_block.h"

static_assert(wo::rivers::RUNOFF_PRECIP == WO_RIVERS_RUNOFF_PRECIP && wo::rivers::RUNOFF_UNIFORM == WO_RIVERS_RUNOFF_UNIFORM && wo::rivers::RUNOFF_VALUES == WO_RIVERS_RUNOFF_VALUES,
              "the runoff sources of rivers_ops.h are those of worogen.h");

namespace R = wo::rivers;

namespace wo {

// the block's counters
enum : int { CTL_LAND = 0, CTL_PITS, CTL_PIT_LIST, CTL_HOOKS, CTL_FAULT, CTL_LAKE, CTL_COUNT };

__global__ __launch_bounds__(WO_BLOCK) void k_rivers_receivers(const int32_t* __restrict__ off, const int32_t* __restrict__ adj, const float* __restrict__ e, int32_t source,
                                                               const float* __restrict__ a, const float* __restrict__ b, int32_t N, int32_t* __restrict__ receiver,
                                                               int32_t* __restrict__ jump, unsigned long long* __restrict__ D, unsigned long long* __restrict__ ctl) {
    __shared__ uint32_t blockSum[2];
    if (threadIdx.x < 2) blockSum[threadIdx.x] = 0u;
    __syncthreads();
    const int32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    bool land = false, pit = false;
    if (r < N) {
        land = R::is_land(e[r]);
        int32_t rc = -1, j = R::BASIN_NOT_LAND;
        unsigned long long q = 0;
        if (land) {
            rc = R::receiver_of(off, adj, e, r);
            pit = rc < 0;
            j = pit ? r : (R::is_land(e[rc]) ? rc : (int32_t)R::BASIN_DRAINED);
            const float runoff = source == R::RUNOFF_PRECIP ? R::precip_runoff(a[r], b[r]) : (source == R::RUNOFF_VALUES ? a[r] : 1.0f);
            q = R::runoff_q(runoff);
        }
        receiver[r] = rc; jump[r] = j; D[r] = q;
    }
    const bool flags[2] = {land, pit};
    block_add_to_global<2>(flags, blockSum, ctl + CTL_LAND);
}

// In place, and other threads write while this one reads: every value a cell can hold is a cell further down its own chain, its
// chain's pit or -1 for a drained chain, and a 4-byte load sees one of them whole.  (No __restrict__: jump is read and written.)
__global__ __launch_bounds__(WO_BLOCK) void k_rivers_jump(int32_t* jump, int32_t N) {
    const int32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= N) return;
    const int32_t j = jump[r];
    if (j < 0 || j == r) return;
    const int32_t jj = jump[j];
    if (jj != j) jump[r] = jj;
}

__global__ __launch_bounds__(WO_BLOCK) void k_rivers_pits(const int32_t* __restrict__ basin, int32_t N, int32_t* __restrict__ pits, unsigned long long* __restrict__ ctl) {
    const int32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    wave_append(r < N && basin[r] == r, r, pits, reinterpret_cast<int32_t*>(ctl + CTL_PIT_LIST));      // the low word of the counter: at most N
}
__global__ __launch_bounds__(WO_BLOCK) void k_rivers_pit_index(const int32_t* __restrict__ pits, int32_t numPits, int32_t* __restrict__ pitIndex) {
    const int32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < numPits) pitIndex[pits[i]] = i;
}
// cellPit: the index of the cell's basin in the pit list, numPits for a drained cell, -1 off land
__global__ __launch_bounds__(WO_BLOCK) void k_rivers_cell_pit(const int32_t* __restrict__ basin, const int32_t* __restrict__ pitIndex, int32_t numPits, int32_t N,
                                                              int32_t* __restrict__ cellPit) {
    const int32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= N) return;
    const int32_t b = basin[r];
    cellPit[r] = b >= 0 ? pitIndex[b] : (b == R::BASIN_DRAINED ? numPits : -1);
}
__global__ __launch_bounds__(WO_BLOCK) void k_rivers_identity(int32_t* __restrict__ comp, int32_t n) {
    const int32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) comp[i] = i;
}

// best[] was filled with NO_PASS
__global__ __launch_bounds__(WO_BLOCK) void k_rivers_offer(const int32_t* __restrict__ off, const int32_t* __restrict__ adj, const float* __restrict__ e, const int32_t* __restrict__ cellPit,
                                                           const int32_t* __restrict__ comp, int32_t numPits, int32_t N, unsigned long long* __restrict__ best) {
    const int32_t u = blockIdx.x * blockDim.x + threadIdx.x;
    if (u >= N) return;
    const int32_t pu = cellPit[u];
    if (pu < 0) return;
    const int32_t cu = comp[pu];
    if (cu == numPits) return;                                // merged with the drained class: resolved
    const uint64_t key = R::cell_offer(off, adj, e, cellPit, comp, u, cu);
    if (key != R::NO_PASS) atomicMin(best + cu, (unsigned long long)key);
}

// next[c]: the component root c hooks to, c itself when it stays; the hooks go to an array of their own because the roots read comp
__global__ __launch_bounds__(WO_BLOCK) void k_rivers_hook(const int32_t* __restrict__ off, const int32_t* __restrict__ adj, const float* __restrict__ e, const int32_t* __restrict__ cellPit,
                                                          const int32_t* __restrict__ comp, const unsigned long long* __restrict__ best, int32_t numPits, int32_t N,
                                                          int32_t* __restrict__ next, R::PassEdge* __restrict__ edges, unsigned long long* __restrict__ ctl) {
    const int32_t c = blockIdx.x * blockDim.x + threadIdx.x;
    bool hooked = false;
    if (c <= numPits) {
        int32_t to = c;
        if (c < numPits && comp[c] == c) {
            R::PassEdge g;
            to = R::hook_of(off, adj, e, cellPit, comp, reinterpret_cast<const uint64_t*>(best), N, c, &g);
            hooked = to != c;
            if (hooked) edges[c] = g;                         // a pit hooks once: it is no root afterwards
        }
        next[c] = to;
    }
    const uint32_t n = wave_sum(hooked);
    if ((threadIdx.x & 63) == 0 && n) atomicAdd(ctl + CTL_HOOKS, (unsigned long long)n);
}

// The hooks of a round form a forest on the old roots (every root chose its lowest pass and the keys are distinct, so the only cycles
// would be the pairs k_rivers_hook broke); the walk is bounded all the same, and a walk that runs out says so in ctl.
__global__ __launch_bounds__(WO_BLOCK) void k_rivers_relabel(const int32_t* __restrict__ comp, const int32_t* __restrict__ next, int32_t numPits, int32_t* __restrict__ compOut,
                                                             unsigned long long* __restrict__ ctl) {
    const int32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i > numPits) return;
    int32_t x = comp[i];
    for (int32_t step = 0;; ++step) {
        const int32_t n = next[x];
        if (n == x) break;
        if (step > numPits) { ctl[CTL_FAULT] = 1ull; break; }
        x = n;
    }
    compOut[i] = x;
}

// cnt was cleared
__global__ __launch_bounds__(WO_BLOCK) void k_rivers_apply(const float* __restrict__ e, const int32_t* __restrict__ basin, const int32_t* __restrict__ cellPit,
                                                           const int32_t* __restrict__ spillTo, const float* __restrict__ W, int32_t numPits, int32_t N, int32_t* __restrict__ receiver,
                                                           float* __restrict__ lake, int32_t* __restrict__ cnt) {
    const int32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= N) return;
    const R::Applied a = R::apply_cell(r, e[r], receiver[r], basin[r], cellPit[r], numPits, spillTo, W);
    receiver[r] = a.receiver;
    lake[r] = a.lake;
    if (a.receiver >= 0) atomicAdd(cnt + a.receiver, 1);
}

// The discharge in ONE launch.  D[r] holds q(r); cnt[r] is the number of cells whose final receiver is r; arrived[] is zero.  Every
// leaf (cnt == 0) hands its total to its receiver j: an atomic add into D[j], then an atomic increment of arrived[j].  The thread
// whose increment completes the count carries on: D[j] is then q(j) plus every donor's total, so it reads D[j] and hands it to j's
// receiver, and so on to a root.  The sums are uint64, so the order of the arrivals changes no bit.
// Why the last arriver reads a complete D[j].  erode's k_flow_climb packs total and count into one word and needs no ordering; two
// words do.  (1) Every donor's add to D[j] is performed before its own increment of arrived[j]: the add is the returning form and
// the increment's operand depends on the value it returned (old >> 63 is 0: totals stay below 2^46), so the increment cannot issue
// before the add came back from the memory side, and an agent-scope release fence stands between them as well.  (2) The increments
// of one word are a single modification order; the thread that reads count - 1 is behind every other donor's increment, hence
// behind every other donor's add.  (3) After it, an agent-scope acquire fence and an agent-scope atomic load of D[j], which does not
// come from this CU's L1, so no stale line can answer.  All accesses to D and arrived inside the launch are agent-scope atomics;
// cnt, receiver and a leaf's own D are fixed since the launches before and read plainly.
// Cost: two dependent device-scope round trips per hop and chain, one launch however long the rivers are; the walk is bounded by N.
__global__ __launch_bounds__(WO_BLOCK) void k_rivers_climb(const int32_t* __restrict__ receiver, const int32_t* __restrict__ cnt, unsigned long long* D, int32_t* arrived, int32_t N) {
    const int32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= N || cnt[r] != 0) return;
    int32_t j = receiver[r];
    if (j < 0) return;
    unsigned long long v = D[r];
    for (int32_t step = 0; step < N; ++step) {
        const int32_t need = cnt[j], jj = receiver[j];
        const unsigned long long old = __hip_atomic_fetch_add(D + j, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        const int32_t before = __hip_atomic_fetch_add(arrived + j, 1 + (int32_t)(old >> 63), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (before + 1 != need) break;                        // other donors of j are still out
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        if (jj < 0) break;                                    // a root keeps the sum
        v = __hip_atomic_load(D + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        j = jj;
    }
}

__global__ __launch_bounds__(WO_BLOCK) void k_rivers_finish(const unsigned long long* __restrict__ D, const float* __restrict__ lake, int32_t N, float* __restrict__ flow,
                                                            unsigned long long* __restrict__ ctl) {
    __shared__ uint32_t blockSum[1];
    if (threadIdx.x == 0) blockSum[0] = 0u;
    __syncthreads();
    const int32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    bool inLake = false;
    if (r < N) {
        flow[r] = R::flow_of(D[r]);
        const float l = lake[r];
        inLake = l == l;
    }
    const bool flags[1] = {inLake};
    block_add_to_global<1>(flags, blockSum, ctl + CTL_LAKE);
}

// ---- lines: an order-preserving compaction over the cells ---------------------------------------------------------------------
struct RiverView { const float* e; const unsigned long long* D; const int32_t *receiver, *basin; const float* lake; uint64_t minQ; int32_t N; };
__device__ inline bool river_at(const RiverView& V, int64_t r) {
    return r < V.N && R::river_cell(V.e[r], V.D[r], V.minQ, V.receiver[r], V.basin[r], (int32_t)r, V.lake[r]);
}
__global__ __launch_bounds__(WO_BLOCK) void k_rivers_line_count(RiverView V, int32_t* __restrict__ blockCount) {
    __shared__ int32_t waveCount[BLOCK_WAVES];
    const BlockPlace at = block_place(river_at(V, (int64_t)blockIdx.x * WO_BLOCK + threadIdx.x), waveCount);
    if (threadIdx.x == 0) blockCount[blockIdx.x] = at.total;
}
__global__ __launch_bounds__(WO_BLOCK) void k_rivers_line_write(RiverView V, const float* __restrict__ xyz, const float* __restrict__ flow, const int32_t* __restrict__ blockOffset,
                                                                float* __restrict__ out, float* __restrict__ flowsOut) {
    __shared__ int32_t waveCount[BLOCK_WAVES];
    const int64_t r = (int64_t)blockIdx.x * WO_BLOCK + threadIdx.x;
    const bool take = river_at(V, r);
    const int64_t at = (int64_t)blockOffset[blockIdx.x] + block_place(take, waveCount).place;
    if (!take || at >= V.N) return;                           // the outputs hold N segments, which is all there can be
    float seg[6];
    R::river_segment(xyz, V.e, (int32_t)r, V.receiver[r], seg);
    float2* o = reinterpret_cast<float2*>(out + 6 * at);      // 24 bytes per segment: 8-byte aligned
    o[0] = make_float2(seg[0], seg[1]); o[1] = make_float2(seg[2], seg[3]); o[2] = make_float2(seg[4], seg[5]);
    flowsOut[at] = flow[r];
}

__global__ __launch_bounds__(WO_BLOCK) void k_rivers_tint(RiverView V, uint32_t* __restrict__ regionRgba) {
    const int32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r < V.N && R::tinted_cell(V.e[r], V.D[r], V.minQ, V.receiver[r], V.basin[r], r, V.lake[r])) regionRgba[r] = R::TINT_RGBA;
}

void rivers_free(wo_planet* p) { delete p->rivers; p->rivers = nullptr; }

static void rivers_alloc(wo_planet* p) {
    if (p->rivers) return;
    std::unique_ptr<wo_rivers_block> block(new wo_rivers_block());      // the planet gets the block once it is complete
    wo_rivers_block* B = block.get(); DeviceArena& a = B->mem;
    const size_t n = (size_t)p->N;
    B->receiver = a.dev<int32_t>(n);
    B->basin = a.dev<int32_t>(n);
    B->lake = a.dev<float>(n);
    B->discharge = a.dev<unsigned long long>(n);
    B->flow = a.dev<float>(n);
    B->ctl = a.dev<unsigned long long>(CTL_COUNT);
    B->h_ctl = a.pinned<unsigned long long>(CTL_COUNT);
    p->rivers = block.release();
}

static Slot rivers_slot(StageBlock* b, int f, size_t N) {
    auto* B = static_cast<wo_rivers_block*>(b);
    switch (f) {
        case R::FIELD_RECEIVER: return Slot{B->receiver, N * 4, false};
        case R::FIELD_BASIN: return Slot{B->basin, N * 4, false};
        case R::FIELD_LAKE: return Slot{B->lake, N * 4, false};
        case R::FIELD_DISCHARGE: return Slot{B->discharge, N * 8, false};
        default: return Slot{B->flow, N * 4, false};
    }
}

static RiverView river_view(const wo_planet* p, const float* e, uint64_t minQ) {
    const auto* B = p->rivers;
    return RiverView{e, B->discharge, B->receiver, B->basin, B->lake, minQ, p->N};
}

void rivers_tint_regions(wo_planet* p, const float* e, uint64_t minQ, uint32_t* regionRgba) {
    launch(p, FAM_RIVERS_LINES, k_rivers_tint, blocks_for(p->N), WO_BLOCK, river_view(p, e, minQ), regionRgba);
}

// the counters on the host (waits for the stream)
static const unsigned long long* read_ctl(wo_planet* p, wo_rivers_block* B) {
    hipStream_t s = p->ctx->stream;
    WO_HIP(hipMemcpyAsync(B->h_ctl, B->ctl, CTL_COUNT * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    WO_HIP(hipStreamSynchronize(s));
    return B->h_ctl;
}

static void rivers_run(wo_planet* p, const float* r_elevation, int32_t source, const float* runoffValues) {
    auto* B = p->rivers;
    const int32_t N = p->N, g = blocks_for(N);
    const size_t n = (size_t)N;
    hipStream_t s = p->ctx->stream;
    B->have = 0;
    int32_t launches = 0;
    const auto run = [&](int fam, auto kernel, int grid, auto... args) { ++launches; launch(p, fam, kernel, grid, WO_BLOCK, args...); };
    const int32_t* off = p->d_off; const int32_t* adj = p->d_adj;
    DeviceArena T;                                            // the temporaries of this call
    WO_HIP(hipMemsetAsync(B->ctl, 0, CTL_COUNT * sizeof(unsigned long long), s));
    const float* e = stage_elevation(p, T, r_elevation);
    const float *ra = nullptr, *rb = nullptr;
    if (source == R::RUNOFF_PRECIP) { ra = p->precip->out[PF_PRECIP0]; rb = p->precip->out[PF_PRECIP0 + 1]; }
    if (source == R::RUNOFF_VALUES) ra = up(T, runoffValues, n, s);
    // receivers, basins, pits
    run(FAM_RIVERS, k_rivers_receivers, g, off, adj, e, source, ra, rb, N, B->receiver, B->basin, B->discharge, B->ctl);
    int32_t jumps = 1;
    while ((1ll << (jumps - 1)) < (long long)N) ++jumps;      // ceil(log2 N) + 1
    for (int32_t k = 0; k < jumps; ++k) run(FAM_RIVERS, k_rivers_jump, g, B->basin, N);
    int32_t* pits = T.dev<int32_t>(n);
    int32_t* pitIndex = T.dev<int32_t>(n);
    int32_t* cellPit = T.dev<int32_t>(n);
    run(FAM_RIVERS, k_rivers_pits, g, (const int32_t*)B->basin, N, pits, B->ctl);
    const unsigned long long* H = read_ctl(p, B);
    wo_rivers_info I{};
    I.landCells = (int32_t)H[CTL_LAND]; I.pits = (int32_t)H[CTL_PITS];
    const int32_t P = I.pits;
    if ((int32_t)H[CTL_PIT_LIST] != P) throw std::runtime_error("the pit list holds " + std::to_string(H[CTL_PIT_LIST]) + " cells, the receivers pass counted " + std::to_string(P));
    if (P > 0) run(FAM_RIVERS, k_rivers_pit_index, blocks_for(P), (const int32_t*)pits, P, pitIndex);
    run(FAM_RIVERS, k_rivers_cell_pit, g, (const int32_t*)B->basin, (const int32_t*)pitIndex, P, N, cellPit);
    // contraction
    int32_t* spillTo = T.dev<int32_t>((size_t)P);
    float* W = T.dev<float>((size_t)P);
    if (P > 0) {
        const int32_t gp = blocks_for((int64_t)P + 1);
        int32_t* comp[2] = {T.dev<int32_t>((size_t)P + 1), T.dev<int32_t>((size_t)P + 1)};
        int32_t* next = T.dev<int32_t>((size_t)P + 1);
        unsigned long long* best = T.dev<unsigned long long>((size_t)P + 1);
        R::PassEdge* edges = T.dev<R::PassEdge>((size_t)P);
        R::PassEdge* h_edges = T.pinned<R::PassEdge>((size_t)P);
        WO_HIP(hipMemsetAsync(edges, 0xFF, (size_t)P * sizeof(R::PassEdge), s));      // u == -1: the pit never hooked
        run(FAM_RIVERS, k_rivers_identity, gp, comp[0], P + 1);
        unsigned long long hooks = 0;
        for (int cur = 0;; cur ^= 1) {
            WO_HIP(hipMemsetAsync(best, 0xFF, ((size_t)P + 1) * 8, s));
            run(FAM_RIVERS, k_rivers_offer, g, off, adj, e, (const int32_t*)cellPit, (const int32_t*)comp[cur], P, N, best);
            run(FAM_RIVERS, k_rivers_hook, gp, off, adj, e, (const int32_t*)cellPit, (const int32_t*)comp[cur], (const unsigned long long*)best, P, N, next,
                               edges, B->ctl);
            run(FAM_RIVERS, k_rivers_relabel, gp, (const int32_t*)comp[cur], (const int32_t*)next, P, comp[cur ^ 1], B->ctl);
            H = read_ctl(p, B);
            if (H[CTL_FAULT]) throw std::runtime_error("the hooks of a contraction round form a cycle");
            if (H[CTL_HOOKS] == hooks) break;                 // no component found a pass: what is left is endorheic
            hooks = H[CTL_HOOKS];
            ++I.rounds;
            if (hooks >= (unsigned long long)P) break;        // every pit has hooked
        }
        // the tree walk on the host: O(P)
        WO_HIP(hipMemcpyAsync(h_edges, edges, (size_t)P * sizeof(R::PassEdge), hipMemcpyDeviceToHost, s));
        WO_HIP(hipStreamSynchronize(s));
        std::vector<R::PassEdge> chosen;
        chosen.reserve((size_t)hooks);
        for (int32_t i = 0; i < P; ++i)
            if (h_edges[i].u >= 0) chosen.push_back(h_edges[i]);
        std::vector<int32_t> hSpill;
        std::vector<float> hW;
        I.spilledBasins = R::resolve_spills(P, chosen, hSpill, hW);
        int32_t* pSpill = T.pinned<int32_t>((size_t)P);
        float* pW = T.pinned<float>((size_t)P);
        std::memcpy(pSpill, hSpill.data(), (size_t)P * 4);
        std::memcpy(pW, hW.data(), (size_t)P * 4);
        WO_HIP(hipMemcpyAsync(spillTo, pSpill, (size_t)P * 4, hipMemcpyHostToDevice, s));
        WO_HIP(hipMemcpyAsync(W, pW, (size_t)P * 4, hipMemcpyHostToDevice, s));
    }
    I.endorheicBasins = P - I.spilledBasins;
    // apply, discharge, flow
    int32_t* cnt = T.dev<int32_t>(n);
    int32_t* arrived = T.dev<int32_t>(n);
    WO_HIP(hipMemsetAsync(cnt, 0, n * 4, s));
    WO_HIP(hipMemsetAsync(arrived, 0, n * 4, s));
    run(FAM_RIVERS, k_rivers_apply, g, e, (const int32_t*)B->basin, (const int32_t*)cellPit, (const int32_t*)spillTo, (const float*)W, P, N, B->receiver, B->lake,
                       cnt);
    run(FAM_RIVERS_CLIMB, k_rivers_climb, g, (const int32_t*)B->receiver, (const int32_t*)cnt, B->discharge, arrived, N);
    run(FAM_RIVERS, k_rivers_finish, g, (const unsigned long long*)B->discharge, (const float*)B->lake, N, B->flow, B->ctl);
    H = read_ctl(p, B);                                       // also before T frees the temporaries
    I.lakeCells = (int32_t)H[CTL_LAKE];
    I.launches = launches;
    B->info = I;
    B->have = rivers_desc().all();
}

}  // namespace wo

using namespace wo;

static const char* const kRiversFields[R::FIELD_COUNT] = {"r_river_receiver", "r_river_basin", "r_lake_level", "r_river_discharge", "r_river_flow"};
static StageBlock* rivers_of(const wo_planet* p) { return p->rivers; }
const BlockDesc& wo::rivers_desc() {
    static const BlockDesc D{"rivers", "wo_compute_rivers", kRiversFields, R::FIELD_COUNT, rivers_of, rivers_alloc, rivers_slot};
    return D;
}

extern "C" {

int wo_compute_rivers(wo_planet* p, int32_t numRegions, const float* r_elevation, int32_t runoffSource, const float* runoffValues, wo_rivers_info* info) {
    const char* fn = "wo_compute_rivers";
    const std::string F = "wo_compute_rivers: ";
    if (!check_planet(p, fn)) return 1;
    if (numRegions != p->N) { set_error(F + "numRegions is " + std::to_string(numRegions) + ", the planet has " + std::to_string(p->N)); return 1; }
    if (!R::runoff_source_ok(runoffSource)) { set_error(F + "unknown runoff source " + std::to_string(runoffSource)); return 1; }
    if (runoffSource == R::RUNOFF_VALUES && !runoffValues) { set_error(F + "WO_RIVERS_RUNOFF_VALUES takes its runoff from the caller, runoffValues is NULL"); return 1; }
    if (runoffSource != R::RUNOFF_VALUES && runoffValues) { set_error(F + "runoffValues must be NULL unless the source is WO_RIVERS_RUNOFF_VALUES"); return 1; }
    if (runoffSource == R::RUNOFF_PRECIP && !block_require(p, fn, precip_desc(), PF_PRECIP_BOTH, "wo_precip_upload r_precip_summer r_precip_winter")) return 1;
    WO_TRY
        rivers_alloc(p);
        rivers_run(p, r_elevation, runoffSource, runoffValues);
        if (info) *info = p->rivers->info;
        return 0;
    WO_CATCH(fn)
}

int wo_rivers_download(wo_planet* p, const char* field, void* out, int64_t outBytes) { return block_download(p, "wo_rivers_download", rivers_desc(), field, out, outBytes); }

int wo_river_lines(wo_planet* p, double minFlow, const float* r_elevation, float* segmentsOut, float* flowsOut, int64_t capacity, int64_t* count) {
    const char* fn = "wo_river_lines";
    const std::string F = "wo_river_lines: ";
    if (!check_planet(p, fn)) return 1;
    if (!segmentsOut || !count) { set_error(F + "null pointer"); return 1; }
    if (!(minFlow - minFlow == 0.0)) { set_error(F + "minFlow is " + std::to_string(minFlow) + ", it must be finite"); return 1; }
    if (capacity < (int64_t)p->N) { set_error(F + "a planet of " + std::to_string(p->N) + " regions can give as many segments, capacity is " + std::to_string(capacity)); return 1; }
    if (!block_require(p, fn, rivers_desc(), rivers_desc().all(), nullptr)) return 1;
    WO_TRY
        const int32_t N = p->N, groups = blocks_for(N);
        hipStream_t s = p->ctx->stream;
        DeviceArena T;                                        // the temporaries of this call
        const float* e = stage_elevation(p, T, r_elevation);
        int32_t* offsets = T.dev<int32_t>((size_t)groups);
        int32_t* d_total = T.dev<int32_t>(1);
        int32_t* h_total = T.pinned<int32_t>(1);
        float* out = T.dev<float>(6 * (size_t)N);
        float* flows = T.dev<float>((size_t)N);
        const RiverView V = river_view(p, e, R::min_q(minFlow));
        launch(p, FAM_RIVERS_LINES, k_rivers_line_count, groups, WO_BLOCK, V, offsets);
        launch(p, FAM_RIVERS_LINES, k_block_offsets<1>, 1, BLOCK_SCAN_THREADS, offsets, groups, d_total);
        launch(p, FAM_RIVERS_LINES, k_rivers_line_write, groups, WO_BLOCK, V, (const float*)p->d_xyz, (const float*)p->rivers->flow, (const int32_t*)offsets, out, flows);
        WO_HIP(hipMemcpyAsync(h_total, d_total, 4, hipMemcpyDeviceToHost, s));
        WO_HIP(hipStreamSynchronize(s));
        const int64_t m = *h_total;
        if (m > 0) {
            WO_HIP(hipMemcpyAsync(segmentsOut, out, (size_t)m * 24, hipMemcpyDeviceToHost, s));
            if (flowsOut) WO_HIP(hipMemcpyAsync(flowsOut, flows, (size_t)m * 4, hipMemcpyDeviceToHost, s));
            WO_HIP(hipStreamSynchronize(s));                  // before T frees the temporaries
        }
        *count = m;
        return 0;
    WO_CATCH(fn)
}

}  // extern "C"
