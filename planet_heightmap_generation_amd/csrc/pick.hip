// The editor's hit test on the device (the reference's findNearestRegion, js/edit-mode.js:18-28): for every query direction the
// region of the planet's resident positions with the greatest dot product, the lowest index among equals.  The bodies and the
// contract are in pick_ops.h.
//
// Launches of wo_pick_regions, per batch of tiles (a tile is pick::TILE queries):
//   k_pick [1]          a group of workgroups per tile.  One pass over the positions serves a whole tile: a lane loads a region's position
//                       once, converts it to double and updates the tile's running (dot, index) pairs, which live in registers.  The
//                       queries are uniform across the wave, so they come through scalar loads.  The workgroups are capped
//                       (PICK_BLOCKS, test hook pick_blocks) and walk the regions in a grid-stride loop in ascending index order, so
//                       that within a lane the loop's strict `>` keeps the lowest index.  Then a wave64 shuffle reduction and a
//                       4-wave LDS step under pick::beats, and one partial per query and workgroup.
//   k_pick_reduce [1]   one workgroup per query reduces its partials the same way and writes the region and the dot.
// No float atomics and no order dependence: `beats` is a total order, so two calls give identical words.
// Bounds: lanes past N never load (r < N guards the loop) and keep the invalid entry; the device copy of the queries is padded to
// whole tiles with NaN, whose dots never win, so the queries past Q carry the invalid entry too and k_pick_reduce does not write
// them (query < Q).  A partial lies at (tile in batch * TILE + k) * workgroups + workgroup, inside the batch's allocation of
// batch * TILE * workgroups entries.
// Memory (device_mem.h): everything is a temporary of the call, in an arena on its stack.
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/worogen.h"
#include "block_ops.h"
#include "device.h"
#include "pick_ops.h"

namespace P = wo::pick;

static_assert(P::MAX_QUERIES == WO_PICK_MAX_QUERIES, "the query limit of pick_ops.h is that of worogen.h");

// block_ops.h's wave_reduce finds it in Best's namespace: the pair goes field by field
namespace wo { namespace pick {
__device__ inline Best lane_down(Best b, int d) { return Best{__shfl_down(b.dot, d, 64), __shfl_down(b.idx, d, 64)}; }
} }

namespace wo {

constexpr int PICK_BLOCKS = 1024;                     // workgroups per tile at most: four per compute unit
constexpr int64_t PICK_PARTIALS = 1 << 20;            // partials per batch at most (12 MB)

// the workgroup's best entry under P::beats; the result is valid in thread 0.  sDot / sIdx: BLOCK_WAVES entries, free to be overwritten.
__device__ inline P::Best pick_block_best(P::Best b, double* sDot, int32_t* sIdx) {
    b = wave_reduce(b, [](P::Best x, P::Best y) { return P::better_of(x, y); });
    __syncthreads();                                          // the previous use of sDot / sIdx is over
    if ((threadIdx.x & 63) == 0) { sDot[threadIdx.x >> 6] = b.dot; sIdx[threadIdx.x >> 6] = b.idx; }
    __syncthreads();
    if (threadIdx.x == 0)
        for (int w = 1; w < BLOCK_WAVES; ++w) b = P::better_of(b, P::Best{sDot[w], sIdx[w]});
    return b;
}

// queries: 3 doubles per query, padded to whole tiles with NaN.  The grid is `blocks` workgroups per tile of the batch, tile by tile.
__global__ __launch_bounds__(WO_BLOCK) void k_pick(const float* __restrict__ xyz, int32_t N, const double* __restrict__ queries, int32_t tile0, int32_t blocks,
                                                   double* __restrict__ partDot, int32_t* __restrict__ partIdx) {
    __shared__ double sDot[BLOCK_WAVES];
    __shared__ int32_t sIdx[BLOCK_WAVES];
    const int32_t tile = (int32_t)blockIdx.x / blocks, block = (int32_t)blockIdx.x % blocks;      // the tile within the batch
    const double* __restrict__ q = queries + (int64_t)(tile0 + tile) * (P::TILE * 3);
    P::Best best[P::TILE];
#pragma unroll
    for (int k = 0; k < P::TILE; ++k) best[k] = P::best_none();
    const int64_t stride = (int64_t)blocks * WO_BLOCK;
    for (int64_t r = (int64_t)block * WO_BLOCK + threadIdx.x; r < N; r += stride) {
        const float x = xyz[3 * r], y = xyz[3 * r + 1], z = xyz[3 * r + 2];
#pragma unroll
        for (int k = 0; k < P::TILE; ++k) P::take_in_order(best[k], P::dot_of(q[3 * k], q[3 * k + 1], q[3 * k + 2], x, y, z), (int32_t)r);
    }
#pragma unroll
    for (int k = 0; k < P::TILE; ++k) {
        const P::Best b = pick_block_best(best[k], sDot, sIdx);
        if (threadIdx.x == 0) {
            const int64_t at = ((int64_t)tile * P::TILE + k) * blocks + block;
            partDot[at] = b.dot; partIdx[at] = b.idx;
        }
    }
}

// workgroup i reduces the `parts` partials of query tile0 * TILE + i
__global__ __launch_bounds__(WO_BLOCK) void k_pick_reduce(const double* __restrict__ partDot, const int32_t* __restrict__ partIdx, int32_t parts, int32_t tile0, int32_t numQueries,
                                                          int32_t* __restrict__ regions, double* __restrict__ dots) {
    __shared__ double sDot[BLOCK_WAVES];
    __shared__ int32_t sIdx[BLOCK_WAVES];
    const int64_t query = (int64_t)tile0 * P::TILE + blockIdx.x;
    if (query >= numQueries) return;                          // the whole workgroup: a query of the last tile's padding
    const int64_t base = (int64_t)blockIdx.x * parts;
    P::Best b = P::best_none();
    for (int32_t i = threadIdx.x; i < parts; i += WO_BLOCK) b = P::better_of(b, P::Best{partDot[base + i], partIdx[base + i]});
    b = pick_block_best(b, sDot, sIdx);
    if (threadIdx.x == 0) { regions[query] = b.idx; dots[query] = b.idx < 0 ? P::NO_DOT : b.dot; }
}

}  // namespace wo

using namespace wo;

extern "C" {

int wo_pick_regions(wo_planet* p, int32_t numQueries, const double* directions, int32_t* regionsOut, double* dotsOut) {
    const std::string F = "wo_pick_regions: ";
    if (!check_planet(p, "wo_pick_regions")) return 1;
    if (numQueries < 0 || numQueries > P::MAX_QUERIES) { set_error(F + "numQueries is " + std::to_string(numQueries) + ", it must lie in [0, " + std::to_string(P::MAX_QUERIES) + "]"); return 1; }
    if (!directions || !regionsOut) { set_error(F + (directions ? "regionsOut" : "directions") + " is NULL"); return 1; }
    if (numQueries == 0) return 0;
    WO_TRY
        const int32_t N = p->N, Q = numQueries;
        hipStream_t s = p->ctx->stream;
        const int32_t tiles = (Q + P::TILE - 1) / P::TILE;
        const int32_t blocks = blocks_for(N, p->opt.pickBlocks > 0 ? p->opt.pickBlocks : PICK_BLOCKS);
        const int32_t batch = (int32_t)std::max<int64_t>(1, std::min<int64_t>(tiles, PICK_PARTIALS / ((int64_t)blocks * P::TILE)));
        DeviceArena T;                                        // the temporaries of this call
        double* d_q = T.dev<double>((size_t)tiles * P::TILE * 3);
        WO_HIP(hipMemsetAsync(d_q, 0xFF, (size_t)tiles * P::TILE * 3 * sizeof(double), s));       // all ones: a NaN
        WO_HIP(hipMemcpyAsync(d_q, directions, (size_t)Q * 3 * sizeof(double), hipMemcpyHostToDevice, s));
        double* partDot = T.dev<double>((size_t)batch * P::TILE * blocks);
        int32_t* partIdx = T.dev<int32_t>((size_t)batch * P::TILE * blocks);
        int32_t* d_regions = T.dev<int32_t>((size_t)Q);
        double* d_dots = T.dev<double>((size_t)Q);
        for (int32_t tile0 = 0; tile0 < tiles; tile0 += batch) {
            const int32_t n = std::min(batch, tiles - tile0);
            launch(p, FAM_PICK, k_pick, blocks * n, WO_BLOCK, (const float*)p->d_xyz, N, (const double*)d_q, tile0, blocks, partDot, partIdx);
            launch(p, FAM_PICK_REDUCE, k_pick_reduce, n * P::TILE, WO_BLOCK, (const double*)partDot, (const int32_t*)partIdx, blocks, tile0, Q, d_regions, d_dots);
        }
        WO_HIP(hipMemcpyAsync(regionsOut, d_regions, (size_t)Q * sizeof(int32_t), hipMemcpyDeviceToHost, s));
        if (dotsOut) WO_HIP(hipMemcpyAsync(dotsOut, d_dots, (size_t)Q * sizeof(double), hipMemcpyDeviceToHost, s));
        WO_HIP(hipStreamSynchronize(s));                      // before T frees the temporaries
        return 0;
    WO_CATCH("wo_pick_regions")
}

}  // extern "C"
