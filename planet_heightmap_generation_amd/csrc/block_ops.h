// The wave and workgroup primitives of the kernels, once: the one-atomic-per-wave append, the wave64 shuffle reduction, the
// reduction of a workgroup into words of global memory, the place of a flagged lane in its workgroup (the order-preserving
// compaction) and the scan of the workgroup counts that goes with it.  Wave64, workgroups of WO_BLOCK threads; none of them keeps
// state beyond the LDS the caller hands in.  A function that says "the workgroup calls it" has a barrier inside: every thread of the
// workgroup must reach it, the same number of times.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "device.h"

namespace wo {

constexpr int BLOCK_WAVES = WO_BLOCK / 64;
constexpr int BLOCK_SCAN_THREADS = 1024;                      // the workgroup of k_block_offsets

// Append `value` of every thread with `flag` to list[] with one atomic per wavefront (ballot + popcount); every lane of the wave
// calls it together
__device__ inline void wave_append(bool flag, int32_t value, int32_t* list, int32_t* counter) {
    const unsigned long long mask = __ballot(flag);
    if (mask == 0) return;
    const int lane = threadIdx.x & 63;
    const int leader = __ffsll((long long)mask) - 1;
    int32_t base = 0;
    if (lane == leader) base = atomicAdd(counter, (int32_t)__popcll(mask));
    base = __shfl(base, leader);
    if (flag) list[base + __popcll(mask & ((1ull << lane) - 1ull))] = value;
}

struct OpMax { template <class T> __device__ T operator()(T a, T b) const { return a > b ? a : b; } };
struct OpAdd { template <class T> __device__ T operator()(T a, T b) const { return a + b; } };

// the value of the lane d places up; a type that is no scalar brings an overload of its own, in its namespace (pick.hip)
template <class T> __device__ inline T lane_down(T v, int d) { return __shfl_down(v, d, 64); }

// op over the wave's 64 values, left to right in pairs; the result is valid in lane 0
template <class T, class Op> __device__ inline T wave_reduce(T v, Op op) {
    for (int d = 32; d > 0; d >>= 1) v = op(v, lane_down(v, d));
    return v;
}

// The workgroup calls it.  out[k] = max(out[k], the workgroup's maximum of v[k]) for K words that only grow from 0: a shuffle
// reduction, one LDS atomic per wave and word, then at most one global atomic per workgroup and word, which a workgroup whose
// maximum does not exceed what the word already holds (a relaxed read) leaves out, so that the atomics on a word do not queue behind
// one another.  lds: K words that the caller cleared before a barrier.
template <int K> __device__ inline void block_max_to_global(const uint32_t (&v)[K], uint32_t* lds, uint32_t* __restrict__ out) {
    for (int k = 0; k < K; ++k) {
        const uint32_t m = wave_reduce(v[k], OpMax{});
        if ((threadIdx.x & 63) == 0 && m) atomicMax(&lds[k], m);
    }
    __syncthreads();
    if (threadIdx.x < K && lds[threadIdx.x] > __hip_atomic_load(out + threadIdx.x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(out + threadIdx.x, lds[threadIdx.x]);
}

// the wave's sum, valid in lane 0; of flags it is the popcount of their ballot
template <class T> __device__ inline T wave_sum(T v) { return wave_reduce(v, OpAdd{}); }
__device__ inline uint32_t wave_sum(bool flag) { return (uint32_t)__popcll(__ballot(flag)); }

// The workgroup calls it.  out[k] += the workgroup's sum of v[k] (numbers, or flags that count 1): the same steps; a sum of 0 sends
// no atomic.  lds: K words that the caller cleared before a barrier.
template <int K, class V, class T> __device__ inline void block_add_to_global(const V (&v)[K], T* lds, unsigned long long* __restrict__ out) {
    for (int k = 0; k < K; ++k) {
        const T sum = wave_sum(v[k]);
        if ((threadIdx.x & 63) == 0 && sum) atomicAdd(&lds[k], sum);
    }
    __syncthreads();
    if (threadIdx.x < K && lds[threadIdx.x]) atomicAdd(out + threadIdx.x, (unsigned long long)lds[threadIdx.x]);
}

// The workgroup calls it.  The place of a flagged lane among the workgroup's flagged lanes in thread order (ballot and popcount,
// the waves' counts through LDS), and how many there are.  waveCount: BLOCK_WAVES words; a barrier stands between two calls on the
// same words.
struct BlockPlace { int32_t place, total; };
__device__ inline BlockPlace block_place(bool flag, int32_t* waveCount) {
    const unsigned long long mask = __ballot(flag);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) waveCount[wave] = (int32_t)__popcll(mask);
    __syncthreads();
    BlockPlace p{(int32_t)__popcll(mask & ((1ull << lane) - 1ull)), 0};
    for (int w = 0; w < BLOCK_WAVES; ++w) {
        if (w < wave) p.place += waveCount[w];
        p.total += waveCount[w];
    }
    return p;
}

// One workgroup of BLOCK_SCAN_THREADS: counts[b][j], the LISTS counts of workgroup b, become the exclusive offsets of workgroup b
// in list j, in place; totals[j] is the length of list j.  Every thread owns a run of consecutive workgroups.
template <int LISTS>
__global__ __launch_bounds__(BLOCK_SCAN_THREADS) void k_block_offsets(int32_t* __restrict__ counts, int32_t nBlocks, int32_t* __restrict__ totals) {
    __shared__ int32_t part[2][LISTS][BLOCK_SCAN_THREADS];
    const int t = threadIdx.x;
    const int64_t chunk = ((int64_t)nBlocks + BLOCK_SCAN_THREADS - 1) / BLOCK_SCAN_THREADS;
    const int64_t b0 = t * chunk < nBlocks ? t * chunk : nBlocks, b1 = b0 + chunk < nBlocks ? b0 + chunk : nBlocks;
    int32_t s[LISTS];
    for (int j = 0; j < LISTS; ++j) s[j] = 0;
    for (int64_t b = b0; b < b1; ++b)
        for (int j = 0; j < LISTS; ++j) s[j] += counts[b * LISTS + j];
    for (int j = 0; j < LISTS; ++j) part[0][j][t] = s[j];
    __syncthreads();
    int cur = 0;
    for (int d = 1; d < BLOCK_SCAN_THREADS; d <<= 1) {        // inclusive Hillis-Steele scan of the runs' sums
        for (int j = 0; j < LISTS; ++j) part[cur ^ 1][j][t] = part[cur][j][t] + (t >= d ? part[cur][j][t - d] : 0);
        cur ^= 1;
        __syncthreads();
    }
    int32_t run[LISTS];
    for (int j = 0; j < LISTS; ++j) run[j] = part[cur][j][t] - s[j];
    for (int64_t b = b0; b < b1; ++b)
        for (int j = 0; j < LISTS; ++j) {
            const int32_t c = counts[b * LISTS + j];
            counts[b * LISTS + j] = run[j];
            run[j] += c;
        }
    if (t == BLOCK_SCAN_THREADS - 1)
        for (int j = 0; j < LISTS; ++j) totals[j] = part[cur][j][t];
}

}  // namespace wo
