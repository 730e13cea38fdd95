// What the kernels of more than one translation unit share: the loop shapes of a per-cell pass and the noise tables' way into LDS;
// the wave and workgroup primitives (wave_append among them) are in block_ops.h.
// (Each kernel is defined in the .hip that launches it, or in that file's *_kernels.h.)
#pragma once
#include <hip/hip_runtime.h>

#include "block_ops.h"
#include "device.h"

namespace wo {

#define WO_GRID_STRIDE(i, n) for (int32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < (n); i += gridDim.x * blockDim.x)

// XCD-aware cell loop for index-order passes.  Workgroup b is observed to run on XCD b % 8 (MI355X_MICROARCH.md);
// with the natural mapping the eight L2s each fetch the same +-4.9*sqrt(N) neighbour windows (measured: ~8x the
// algorithmic bytes in FETCH_SIZE).  Here the blocks are cut into tiles of F.xcdTile consecutive blocks and whole
// tiles are dealt round-robin to the XCDs: an L2 then sees contiguous index ranges (tile + halo), while land and
// ocean bands still spread evenly over the eight dies (one contiguous eighth per XCD was measured slower: the land
// fraction varies with latitude).  Launch with xcd_grid(N, tile) blocks; placement only affects speed, never results.
#define WO_XCD_CELLS(r, n)                                                                                           \
    for (int32_t xi_ = (int32_t)(blockIdx.x >> 3), xt_ = F.xcdTile,                                                  \
                 r = (int32_t)((((xi_ / xt_) * 8 + (int32_t)(blockIdx.x & 7u)) * xt_ + (xi_ % xt_)) * (int32_t)blockDim.x + (int32_t)threadIdx.x), \
                 once_ = 1;                                                                                          \
         once_ && r < (n); once_ = 0)

// Block-uniform strided loop: every thread of the workgroup runs the same number of trips (needed around
// block_append's barriers); `valid` tells whether index i is in range.
#define WO_BLOCK_STRIDE(i, valid, n)                                                              \
    for (int32_t base_ = blockIdx.x * blockDim.x, i = base_ + threadIdx.x, valid = (i < (n));   \
         base_ < (n); base_ += gridDim.x * blockDim.x, i = base_ + threadIdx.x, valid = (i < (n)))

// the permutation tables of a noise instance (perm[512] + pm12[512]) into the workgroup's LDS
__device__ inline void load_tables(const uint8_t* tables, uint8_t* sP, uint8_t* sM) {
    for (int i = threadIdx.x; i < 512; i += blockDim.x) { sP[i] = tables[i]; sM[i] = tables[512 + i]; }
    __syncthreads();
}

}  // namespace wo
