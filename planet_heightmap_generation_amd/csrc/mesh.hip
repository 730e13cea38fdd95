// The sphere-mesh producer on the device: spherical Delaunay (every point gift-wraps its own star from the candidates of a hashed
// 3-D grid), triangles and half-edges, the CSR neighbour graph and the neighbour distances.  The arithmetic is mesh_ops.h's, the
// same bodies the host builder (mesh_builder.cc) compiles, and the result is defined as the host's: every array equals the host
// route's on the same points.
//
// Launches of wo_sphere_mesh_device, in order (V points, WO_BLOCK threads where nothing else is said):
//   (wo_sphere_mesh_seed_device: k_fib_points of points.hip writes the points where the other two entries upload them)
//   k_mesh_points [1]        normalised f64 points (x / l, the host's bits) and the grid key of every point
//   k_mesh_cell_insert [1]   the occupied cells into an open-addressing table (64-bit atomicCAS of key + 1) and their point counts.
//                            No dense G^3 table: the table has 2 min(V, G^3) + 8 slots rounded up to a power of two, so it is never
//                            full.  A cell is named by its slot; which slot a cell gets does not reach the result.
//   scan                     cellStart = exclusive scan of the counts over the slots (k_scan_sums, k_block_offsets, k_scan_apply)
//   k_mesh_cell_scatter [1]  the points into their cell's range, in arrival order
//   k_mesh_cell_rank [1]     every point counts the lower ids of its cell: its place.  Ids ascend inside a cell, as after the host's
//                            stable sort, and that defines the candidate order.
//   k_mesh_stars_l1 [1]      level 1 for all points, one thread per point, 64 threads per workgroup.  The candidates of the 3x3x3
//                            block are staged in LDS, L1_CAP per point (41 on average, up to 141 on jittered spheres); the Jarvis
//                            scan is per thread and sequential in candidate order, the host's by construction.  A point whose
//                            candidates overflow the buffer or whose star is not certified goes to the retry list (wave_append).
//   k_mesh_stars_retry [b]   the retry list in batches of RETRY_BATCH: levels 1..5 and brute per thread, candidates in global scratch,
//                            RETRY_CAP per point.  THE HAND-OVER: a level whose candidates do not fit RETRY_CAP (brute on more than
//                            RETRY_CAP + 1 points included), a level above the hook mesh_device_levels, or a star of more than
//                            STAR_INLINE neighbours that finds the pool of big stars full sends the point to the host list; the host's
//                            star_of finishes those on the same normalised points (stars_on_host) and k_mesh_place_stars stores them.
//                            The predicates' bits are the same on both sides, so the stars are mutually consistent.
//   scan, k_mesh_own_count, scan      star offsets; triangles per owner (the lowest vertex); T is checked against 2V - 4
//   k_mesh_triangles [1], k_mesh_halfedges [1]     the host's passes 2 and 3; unmatched half-edges are counted on the device
//   (reference closure: on the host, between the download of the triangles and the CSR stage, by wo_sphere_reference_closure)
//   k_mesh_first_side [1], k_mesh_csr_count [1], scan, k_mesh_csr_fill [1]     mesh_csr's circulation rule: the lowest side leaving r
//                            (atomicMin), then s <- next(halfedges[s]), at most 4096 steps; adjTriList and neighborDist in the fill
// Bounds: every kernel guards its index against its count.  Candidates are point ids below V by construction, so are the stars'
// entries; a push past a buffer's capacity only counts.  Loops: 6 levels, MAX_STAR wrap steps, a probe of at most the table's
// size, the 4096-step guard of the CSR walk; the fill walks exactly the counted steps.  The CSR stage runs on triangles that either
// this file built or wo_sphere_reference_closure checked.
// Memory (device_mem.h): everything is a temporary of the call, in an arena on its stack.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <string>
#include <vector>

#include "../../include/worogen.h"
#include "block_ops.h"
#include "device.h"
#include "mesh_ops.h"
#include "points_ops.h"

namespace M = wo::mesh;

namespace wo {

// points.hip
WO_LOCAL bool fib_points_to_device(hipStream_t s, DeviceArena& A, int32_t N, double jitter, double seed, float* d_xyz);

constexpr int L1_THREADS = 64;                    // workgroup of k_mesh_stars_l1: one wave, 32 KB of LDS
constexpr int L1_CAP = 128;                       // candidates per point at level 1 (test hook mesh_cand_cap lowers it)
constexpr int RETRY_CAP = 4096;                   // candidates per point in the retry kernel's global scratch
constexpr int RETRY_BATCH = 16384;                // points per retry launch: 256 MB of scratch
constexpr int SCAN_ITEMS = 8;                     // consecutive elements per thread of the scan kernels
constexpr int SCAN_TILE = WO_BLOCK * SCAN_ITEMS;

// the call's words on the device
enum Ctrl : int { C_ZERO_LEN = 0, C_RETRY, C_HOST, C_FAILED, C_BIG, C_BAD_HE, C_TOTAL_DEG, C_TOTAL_T, C_CSR_BAD, C_TOTAL_ADJ, C_TOTAL_CELLS, C_OUTSIDE, C_COUNT = 16 };

// where the stars live: STAR_INLINE entries per point, and a pool of MAX_STAR entries per big star
struct StarStore {
    int32_t* deg; int32_t* starBuf; int32_t* bigIndex; int32_t* bigPool; int32_t bigCap; int32_t* ctrl;
};
__device__ inline const int32_t* star_of(const StarStore& S, int32_t p) {
    const int32_t b = S.bigIndex[p];
    return b >= 0 ? S.bigPool + (int64_t)b * M::MAX_STAR : S.starBuf + (int64_t)p * M::STAR_INLINE;
}
// stores the star rotated to its lowest neighbour; false: it is a big star and the pool is full
__device__ inline bool store_rotated(const StarStore& S, int32_t p, const int32_t* st, int32_t d, int32_t m) {
    int32_t* dst;
    if (d <= M::STAR_INLINE) dst = S.starBuf + (int64_t)p * M::STAR_INLINE;
    else {
        const int32_t slot = atomicAdd(&S.ctrl[C_BIG], 1);            // may run past bigCap: the host clamps it
        if (slot >= S.bigCap) return false;
        S.bigIndex[p] = slot;
        dst = S.bigPool + (int64_t)slot * M::MAX_STAR;
    }
    for (int32_t i = 0; i < d; ++i) { int32_t k = m + i; if (k >= d) k -= d; dst[i] = st[k]; }
    S.deg[p] = d;
    return true;
}

// a candidate list on every stride-th word of a buffer; a push past the capacity only counts
struct StridedCand {
    int32_t* base; int32_t stride, cap, n;
    __device__ inline int32_t size() const { return n; }
    __device__ inline int32_t operator[](int32_t i) const { return base[(int64_t)i * stride]; }
    __device__ inline void push(int32_t q) { if (n < cap) base[(int64_t)n * stride] = q; ++n; }
};

// ---------------------------------------------------------------------------------------------------------------------------
// exclusive scan of n int32 into out[0..n] (out[n] and *total: the sum)
// ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(WO_BLOCK) void k_scan_sums(const int32_t* __restrict__ in, int64_t n, int32_t* __restrict__ tileSums) {
    __shared__ int32_t sWave[BLOCK_WAVES];
    const int64_t i0 = (int64_t)blockIdx.x * SCAN_TILE + (int64_t)threadIdx.x * SCAN_ITEMS;
    int32_t s = 0;
    for (int j = 0; j < SCAN_ITEMS; ++j) if (i0 + j < n) s += in[i0 + j];
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) sWave[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) { int32_t t = 0; for (int w = 0; w < BLOCK_WAVES; ++w) t += sWave[w]; tileSums[blockIdx.x] = t; }
}
__global__ __launch_bounds__(WO_BLOCK) void k_scan_apply(const int32_t* __restrict__ in, int64_t n, const int32_t* __restrict__ tileOffsets,
                                                         const int32_t* __restrict__ total, int32_t* __restrict__ out) {
    __shared__ int32_t part[2][WO_BLOCK];
    const int t = threadIdx.x;
    const int64_t i0 = (int64_t)blockIdx.x * SCAN_TILE + (int64_t)t * SCAN_ITEMS;
    int32_t v[SCAN_ITEMS], s = 0;
    for (int j = 0; j < SCAN_ITEMS; ++j) { v[j] = i0 + j < n ? in[i0 + j] : 0; s += v[j]; }
    part[0][t] = s;
    __syncthreads();
    int cur = 0;
    for (int d = 1; d < WO_BLOCK; d <<= 1) {                  // inclusive Hillis-Steele scan of the threads' sums
        part[cur ^ 1][t] = part[cur][t] + (t >= d ? part[cur][t - d] : 0);
        cur ^= 1;
        __syncthreads();
    }
    int32_t run = tileOffsets[blockIdx.x] + part[cur][t] - s;
    for (int j = 0; j < SCAN_ITEMS; ++j) if (i0 + j < n) { out[i0 + j] = run; run += v[j]; }
    if (blockIdx.x == 0 && t == 0) out[n] = *total;
}

// ---------------------------------------------------------------------------------------------------------------------------
// points and grid
// ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(WO_BLOCK) void k_mesh_points(const float* __restrict__ xyz, int32_t V, M::GridView g, M::P3* __restrict__ pts,
                                                          unsigned long long* __restrict__ keys, int32_t* __restrict__ ctrl) {
    const int32_t i = blockIdx.x * WO_BLOCK + threadIdx.x;
    if (i >= V) return;
    M::P3 P{0.0, 0.0, 0.0};
    if (!M::normalise(xyz[3 * (int64_t)i], xyz[3 * (int64_t)i + 1], xyz[3 * (int64_t)i + 2], P)) atomicOr(&ctrl[C_ZERO_LEN], 1);
    pts[i] = P;
    keys[i] = g.key(g.coord(P.x), g.coord(P.y), g.coord(P.z));
}

__global__ __launch_bounds__(WO_BLOCK) void k_mesh_cell_insert(const unsigned long long* __restrict__ keys, int32_t V, unsigned long long* __restrict__ hkey,
                                                               unsigned long long hmask, int32_t* __restrict__ cnt, int32_t* __restrict__ slotOf) {
    const int32_t i = blockIdx.x * WO_BLOCK + threadIdx.x;
    if (i >= V) return;
    const unsigned long long k = keys[i];
    unsigned long long slot = M::GridView::mix(k) & hmask;
    int32_t found = -1;
    for (unsigned long long n = 0; n <= hmask; ++n) {         // the table has more slots than there are cells: a free one turns up
        const unsigned long long prev = atomicCAS(&hkey[slot], 0ull, k + 1);
        if (prev == 0ull || prev == k + 1) { found = (int32_t)slot; break; }
        slot = (slot + 1) & hmask;
    }
    slotOf[i] = found;
    if (found >= 0) atomicAdd(&cnt[found], 1);
}

__global__ __launch_bounds__(WO_BLOCK) void k_mesh_cell_scatter(int32_t V, const int32_t* __restrict__ slotOf, const int32_t* __restrict__ cellStart,
                                                                int32_t* __restrict__ fill, int32_t* __restrict__ unsorted) {
    const int32_t i = blockIdx.x * WO_BLOCK + threadIdx.x;
    if (i >= V) return;
    const int32_t c = slotOf[i];
    if (c < 0) return;
    const int32_t at = cellStart[c] + atomicAdd(&fill[c], 1);
    if (at < cellStart[c + 1]) unsorted[at] = i;
}

__global__ __launch_bounds__(WO_BLOCK) void k_mesh_cell_rank(int32_t V, const int32_t* __restrict__ slotOf, const int32_t* __restrict__ cellStart,
                                                             const int32_t* __restrict__ unsorted, int32_t* __restrict__ sortedIdx) {
    const int32_t i = blockIdx.x * WO_BLOCK + threadIdx.x;
    if (i >= V) return;
    const int32_t c = slotOf[i];
    if (c < 0) return;
    const int32_t b = cellStart[c], e = cellStart[c + 1];
    int32_t lower = 0;
    for (int32_t k = b; k < e; ++k) lower += unsorted[k] < i ? 1 : 0;
    sortedIdx[b + lower] = i;                                  // ids are distinct: lower < e - b
}

// ---------------------------------------------------------------------------------------------------------------------------
// stars
// ---------------------------------------------------------------------------------------------------------------------------
// an accepted star of degree d: stored, or counted as failed (the host's d < 3).  false: the pool of big stars is full
__device__ inline bool take_star(const StarStore& S, int32_t p, const int32_t* st, int32_t d) {
    if (d < 3) { atomicAdd(&S.ctrl[C_FAILED], 1); return true; }
    return store_rotated(S, p, st, d, M::lowest_position(st, d));
}

__global__ __launch_bounds__(L1_THREADS) void k_mesh_stars_l1(int32_t V, const M::P3* __restrict__ pts, M::GridView g, int32_t cap, StarStore S,
                                                              int32_t* __restrict__ retryList) {
    __shared__ int32_t sCand[L1_CAP * L1_THREADS];
    const int32_t p = blockIdx.x * L1_THREADS + threadIdx.x;
    bool retry = false;
    if (p < V) {
        retry = true;
        StridedCand cand{sCand + threadIdx.x, L1_THREADS, cap, 0};
        const M::P3 P = pts[p];
        const int cx = g.coord(P.x), cy = g.coord(P.y), cz = g.coord(P.z);
        M::gather_candidates(p, V, g, cx, cy, cz, 1, false, cand);
        if (cand.n <= cap) {
            int32_t st[M::MAX_STAR];
            int failcode = -1;
            const int d = M::star_at_level(p, pts, g, cx, cy, cz, 1, false, cand, st, failcode);
            if (d >= 0) retry = !take_star(S, p, st, d);
        }
    }
    wave_append(retry, p, retryList, S.ctrl + C_RETRY);
}

// entries first .. first + n of the list; scratch: cap words per entry, entry e on the words e + i * stride
__global__ __launch_bounds__(WO_BLOCK) void k_mesh_stars_retry(const int32_t* __restrict__ list, int32_t first, int32_t n, int32_t V, const M::P3* __restrict__ pts,
                                                               M::GridView g, int32_t* __restrict__ scratch, int32_t stride, int32_t cap, int32_t deviceLevels,
                                                               StarStore S, int32_t* __restrict__ hostList) {
    const int32_t e = blockIdx.x * WO_BLOCK + threadIdx.x;
    bool toHost = false;
    int32_t p = -1;
    if (e < n) {
        p = list[first + e];
        StridedCand cand{scratch + e, stride, cap, 0};
        const M::P3 P = pts[p];
        const int cx = g.coord(P.x), cy = g.coord(P.y), cz = g.coord(P.z);
        int32_t st[M::MAX_STAR];
        int failcode = -1;
        bool settled = false;
        for (int level = 1; level <= M::MAX_LEVEL; ++level) {
            const bool brute = M::level_is_brute(level, g.G);
            if (level > deviceLevels || (brute && V - 1 > cap)) { toHost = true; break; }
            cand.n = 0;
            M::gather_candidates(p, V, g, cx, cy, cz, level, brute, cand);
            if (cand.n > cap) { toHost = true; break; }           // wider levels hold no fewer
            const int d = M::star_at_level(p, pts, g, cx, cy, cz, level, brute, cand, st, failcode);
            if (d >= 0) { toHost = !take_star(S, p, st, d); settled = true; break; }
        }
        if (!settled && !toHost) {
            atomicAdd(&S.ctrl[C_FAILED], 1);
            if (failcode == M::FAIL_CENTRE_OUTSIDE) atomicAdd(&S.ctrl[C_OUTSIDE], 1);       // only the brute level sets it, and it is the last
        }
    }
    wave_append(toHost, p, hostList, S.ctrl + C_HOST);
}

// the stars the host finished: star i of point ids[i] lies at stars[off[i] .. off[i] + deg[i]), already rotated; the pool has room
__global__ __launch_bounds__(WO_BLOCK) void k_mesh_place_stars(int32_t n, const int32_t* __restrict__ ids, const int32_t* __restrict__ hdeg,
                                                               const int32_t* __restrict__ off, const int32_t* __restrict__ stars, StarStore S) {
    const int32_t i = blockIdx.x * WO_BLOCK + threadIdx.x;
    if (i >= n) return;
    const int32_t d = hdeg[i];
    if (d < 3 || d > M::MAX_STAR) return;
    store_rotated(S, ids[i], stars + off[i], d, 0);
}

// ---------------------------------------------------------------------------------------------------------------------------
// triangles, half-edges (the host's passes 2 and 3)
// ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(WO_BLOCK) void k_mesh_own_count(int32_t V, StarStore S, int32_t* __restrict__ ownCount) {
    const int32_t p = blockIdx.x * WO_BLOCK + threadIdx.x;
    if (p >= V) return;
    const int32_t* s = star_of(S, p);
    const int32_t d = S.deg[p];
    int32_t c = 0;
    for (int32_t i = 0; i < d; ++i) { const int32_t q = s[i], r = s[i + 1 < d ? i + 1 : 0]; if (M::owns(p, q, r)) ++c; }
    ownCount[p] = c;
}

__global__ __launch_bounds__(WO_BLOCK) void k_mesh_triangles(int32_t V, StarStore S, const int32_t* __restrict__ starOff, const int32_t* __restrict__ ownOff,
                                                             int32_t* __restrict__ triangles, int32_t* __restrict__ triOfStar) {
    const int32_t p = blockIdx.x * WO_BLOCK + threadIdx.x;
    if (p >= V) return;
    const int32_t* s = star_of(S, p);
    const int32_t d = S.deg[p];
    int32_t t = ownOff[p];
    for (int32_t i = 0; i < d; ++i) {
        const int32_t q = s[i], r = s[i + 1 < d ? i + 1 : 0];
        if (M::owns(p, q, r)) {
            triangles[3 * (int64_t)t] = p; triangles[3 * (int64_t)t + 1] = q; triangles[3 * (int64_t)t + 2] = r;
            triOfStar[starOff[p] + i] = t; ++t;
        }
    }
}

// one thread per side; triOfStar is -1 where a star position owns no triangle
__global__ __launch_bounds__(WO_BLOCK) void k_mesh_halfedges(int32_t numSides, StarStore S, const int32_t* __restrict__ starOff, const int32_t* __restrict__ triangles,
                                                             const int32_t* __restrict__ triOfStar, int32_t* __restrict__ halfedges) {
    const int32_t side = blockIdx.x * WO_BLOCK + threadIdx.x;
    if (side >= numSides) return;
    const int32_t t = side / 3, k = side - 3 * t;
    const int32_t u = triangles[side], v = triangles[3 * t + (k + 1) % 3];
    int32_t result = -1;
    const int32_t* sv = star_of(S, v); const int32_t dv = S.deg[v];
    int32_t i = -1;
    for (int32_t j = 0; j < dv; ++j) if (sv[j] == u) { i = j; break; }
    if (i >= 0) {
        const int32_t w = sv[i + 1 < dv ? i + 1 : 0];
        int m, a;                                         // triangle as (m, a, .) counter-clockwise
        M::owner_of(v, u, w, m, a);
        const int32_t* sm = star_of(S, m); const int32_t dm = S.deg[m];
        int32_t j2 = -1;
        for (int32_t j = 0; j < dm; ++j) if (sm[j] == a) { j2 = j; break; }
        const int32_t t2 = (j2 >= 0) ? triOfStar[starOff[m] + j2] : -1;
        if (t2 >= 0) {
            int32_t s2 = -1;
            for (int32_t c = 0; c < 3; ++c) if (triangles[3 * t2 + c] == v && triangles[3 * t2 + (c + 1) % 3] == u) s2 = c;
            if (s2 >= 0) result = 3 * t2 + s2;
        }
    }
    if (result < 0) atomicAdd(&S.ctrl[C_BAD_HE], 1);
    halfedges[side] = result;
}

// ---------------------------------------------------------------------------------------------------------------------------
// CSR and neighbour distances (mesh_csr, neighbor_dist)
// ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(WO_BLOCK) void k_mesh_first_side(int32_t numSides, const int32_t* __restrict__ triangles, int32_t* __restrict__ firstSide) {
    const int32_t s = blockIdx.x * WO_BLOCK + threadIdx.x;
    if (s < numSides) atomicMin(&firstSide[triangles[s]], s);        // lowest side wins
}

__global__ __launch_bounds__(WO_BLOCK) void k_mesh_csr_count(int32_t V, int32_t numSides, const int32_t* __restrict__ firstSide, const int32_t* __restrict__ halfedges,
                                                             int32_t* __restrict__ cnt, int32_t* __restrict__ ctrl) {
    const int32_t r = blockIdx.x * WO_BLOCK + threadIdx.x;
    if (r >= V) return;
    const int32_t s0 = firstSide[r];
    int32_t c = 0;
    if (s0 < numSides) {
        int32_t s = s0;
        do {
            ++c;
            const int32_t h = halfedges[s];
            if (h < 0 || h >= numSides || c > 4096) { atomicAdd(&ctrl[C_CSR_BAD], 1); c = 0; break; }
            s = M::next_side(h);
        } while (s != s0);
    }
    cnt[r] = c;
}

__global__ __launch_bounds__(WO_BLOCK) void k_mesh_csr_fill(int32_t V, const int32_t* __restrict__ firstSide, const int32_t* __restrict__ adjOffset,
                                                            const int32_t* __restrict__ triangles, const int32_t* __restrict__ halfedges, const float* __restrict__ xyz,
                                                            int32_t* __restrict__ adjList, int32_t* __restrict__ adjTri, float* __restrict__ dist) {
    const int32_t r = blockIdx.x * WO_BLOCK + threadIdx.x;
    if (r >= V) return;
    const int32_t b = adjOffset[r], e = adjOffset[r + 1];
    if (e <= b) return;
    const double x = xyz[3 * (int64_t)r], y = xyz[3 * (int64_t)r + 1], z = xyz[3 * (int64_t)r + 2];
    int32_t s = firstSide[r];
    for (int32_t idx = b; idx < e; ++idx) {                   // exactly the steps k_mesh_csr_count walked
        const int32_t nb = triangles[M::next_side(s)];
        adjList[idx] = nb;
        adjTri[idx] = s / 3;
        dist[idx] = M::chord(x, y, z, xyz[3 * (int64_t)nb], xyz[3 * (int64_t)nb + 1], xyz[3 * (int64_t)nb + 2]);
        s = M::next_side(halfedges[s]);
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------------------
namespace {

struct StatusError { int code; std::string msg; };

template <class... KArgs, class... Args>
inline void mlaunch(hipStream_t s, void (*kernel)(KArgs...), int64_t n, int block, Args... args) {
    const int64_t grid = std::max<int64_t>(1, (n + block - 1) / block);
    hipLaunchKernelGGL(kernel, dim3((unsigned)grid), dim3(block), 0, s, args...);
    WO_HIP(hipGetLastError());
}

// out[0..n]: exclusive scan of in[0..n), out[n] = *total = the sum
void exclusive_scan(hipStream_t s, DeviceArena& A, const int32_t* in, int64_t n, int32_t* out, int32_t* total) {
    const int64_t tiles = std::max<int64_t>(1, (n + SCAN_TILE - 1) / SCAN_TILE);
    int32_t* tileSums = A.dev<int32_t>((size_t)tiles);
    hipLaunchKernelGGL(k_scan_sums, dim3((unsigned)tiles), dim3(WO_BLOCK), 0, s, in, n, tileSums);
    WO_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_block_offsets<1>, dim3(1), dim3(BLOCK_SCAN_THREADS), 0, s, tileSums, (int32_t)tiles, total);
    WO_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_scan_apply, dim3((unsigned)tiles), dim3(WO_BLOCK), 0, s, in, n, (const int32_t*)tileSums, (const int32_t*)total, out);
    WO_HIP(hipGetLastError());
}

struct MeshOut {
    int32_t *triangles, *halfedges, *adjOffset, *adjList, *adjTriList; float* neighborDist;
    bool csr, closure;
};
// where the points come from: the caller's array (xyz, uploaded), or the seed (gen: V - 1 Fibonacci points and the pole are generated
// into the buffer the stages read and downloaded into outXyz, which is complete before the host reads it: stars_on_host)
struct MeshIn { const float* xyz; bool gen; double jitter, seed; float* outXyz; };

void mesh_device(wo_ctx* ctx, int32_t V, const MeshIn& in, const MeshOut& out) {
    WO_HIP(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const int32_t candCap = (int32_t)std::max<long long>(0, std::min<long long>(test_hook_int("mesh_cand_cap", L1_CAP), L1_CAP));
    const int32_t deviceLevels = (int32_t)std::max<long long>(0, std::min<long long>(test_hook_int("mesh_device_levels", M::MAX_LEVEL), M::MAX_LEVEL));
    const int32_t T = 2 * V - 4, numSides = 3 * T;

    DeviceArena A;                                            // the temporaries of this call
    int32_t* ctrl = A.dev<int32_t>(C_COUNT);
    int32_t* h_ctrl = A.pinned<int32_t>(C_COUNT);
    WO_HIP(hipMemsetAsync(ctrl, 0, C_COUNT * sizeof(int32_t), s));
    auto read_ctrl = [&]() {
        WO_HIP(hipMemcpyAsync(h_ctrl, ctrl, C_COUNT * sizeof(int32_t), hipMemcpyDeviceToHost, s));
        WO_HIP(hipStreamSynchronize(s));
    };

    // ---- points and grid
    const float* xyz = in.gen ? in.outXyz : in.xyz;           // the host's copy
    float* d_xyz;
    if (in.gen) {
        d_xyz = A.dev<float>((size_t)3 * V);
        if (!fib_points_to_device(s, A, V - 1, in.jitter, in.seed, d_xyz)) throw StatusError{1, "fib_sphere_points: chain table overflow"};
        WO_HIP(hipMemcpyAsync(in.outXyz, d_xyz, (size_t)3 * V * sizeof(float), hipMemcpyDeviceToHost, s));     // every later read_ctrl waits for it
    } else d_xyz = up(A, in.xyz, (size_t)3 * V, s);
    M::P3* pts = A.dev<M::P3>((size_t)V);
    M::GridView g{};
    M::grid_dims(V, g.h, g.G);
    const double cells = std::min((double)V, (double)g.G * g.G * g.G);
    uint64_t cap = 16;
    while ((double)cap < cells * 2 + 8) cap <<= 1;
    g.hmask = cap - 1;
    DeviceArena gridTmp;                                      // what only the grid's construction needs
    unsigned long long* keys = gridTmp.dev<unsigned long long>((size_t)V);
    unsigned long long* hkey = A.dev<unsigned long long>((size_t)cap);
    int32_t* cnt = gridTmp.dev<int32_t>((size_t)cap);
    int32_t* slotOf = gridTmp.dev<int32_t>((size_t)V);
    int32_t* unsorted = gridTmp.dev<int32_t>((size_t)V);
    int32_t* cellStart = A.dev<int32_t>((size_t)cap + 1);
    int32_t* sortedIdx = A.dev<int32_t>((size_t)V);
    WO_HIP(hipMemsetAsync(hkey, 0, (size_t)cap * sizeof(unsigned long long), s));
    WO_HIP(hipMemsetAsync(cnt, 0, (size_t)cap * sizeof(int32_t), s));
    mlaunch(s, k_mesh_points, V, WO_BLOCK, (const float*)d_xyz, V, g, pts, keys, ctrl);
    mlaunch(s, k_mesh_cell_insert, V, WO_BLOCK, (const unsigned long long*)keys, V, hkey, (unsigned long long)g.hmask, cnt, slotOf);
    exclusive_scan(s, gridTmp, cnt, (int64_t)cap, cellStart, ctrl + C_TOTAL_CELLS);
    WO_HIP(hipMemsetAsync(cnt, 0, (size_t)cap * sizeof(int32_t), s));         // now the cells' fill counters
    mlaunch(s, k_mesh_cell_scatter, V, WO_BLOCK, V, (const int32_t*)slotOf, (const int32_t*)cellStart, cnt, unsorted);
    mlaunch(s, k_mesh_cell_rank, V, WO_BLOCK, V, (const int32_t*)slotOf, (const int32_t*)cellStart, (const int32_t*)unsorted, sortedIdx);
    g.hkey = (const uint64_t*)hkey; g.hval = nullptr; g.cellStart = cellStart; g.sortedIdx = sortedIdx;

    // ---- stars
    StarStore S{};
    S.ctrl = ctrl;
    S.deg = A.dev<int32_t>((size_t)V + 1);
    S.starBuf = A.dev<int32_t>((size_t)V * M::STAR_INLINE);
    S.bigIndex = A.dev<int32_t>((size_t)V);
    S.bigCap = V / 16 + 64;
    S.bigPool = A.dev<int32_t>((size_t)S.bigCap * M::MAX_STAR);
    int32_t* retryList = A.dev<int32_t>((size_t)V);
    WO_HIP(hipMemsetAsync(S.deg, 0, ((size_t)V + 1) * sizeof(int32_t), s));
    WO_HIP(hipMemsetAsync(S.bigIndex, 0xFF, (size_t)V * sizeof(int32_t), s));
    mlaunch(s, k_mesh_stars_l1, V, L1_THREADS, V, (const M::P3*)pts, g, M::level_is_brute(1, g.G) ? 0 : candCap, S, retryList);
    read_ctrl();
    gridTmp.clear();
    if (h_ctrl[C_ZERO_LEN]) throw StatusError{1, "sphere_delaunay: zero-length point"};
    const int32_t nRetry = h_ctrl[C_RETRY];
    int64_t failed = 0, outside = 0;
    if (nRetry > 0) {
        DeviceArena R;
        const int32_t batch = std::min(nRetry, RETRY_BATCH);
        int32_t* scratch = R.dev<int32_t>((size_t)batch * RETRY_CAP);
        int32_t* hostList = R.dev<int32_t>((size_t)nRetry);
        for (int32_t first = 0; first < nRetry; first += batch) {
            const int32_t n = std::min(batch, nRetry - first);
            mlaunch(s, k_mesh_stars_retry, n, WO_BLOCK, (const int32_t*)retryList, first, n, V, (const M::P3*)pts, g, scratch, batch, (int32_t)RETRY_CAP,
                    deviceLevels, S, hostList);
        }
        read_ctrl();
        const int32_t nHost = h_ctrl[C_HOST];
        if (nHost > 0) {                                      // the hand-over: the host's star_of finishes these
            std::vector<int32_t> ids((size_t)nHost), hdeg, hstars;
            WO_HIP(hipMemcpyAsync(ids.data(), hostList, (size_t)nHost * sizeof(int32_t), hipMemcpyDeviceToHost, s));
            WO_HIP(hipStreamSynchronize(s));
            std::sort(ids.begin(), ids.end());
            int hostOutside = 0;
            const int hostFailed = stars_on_host(V, xyz, nHost, ids.data(), hdeg, hstars, &hostOutside);
            if (hostFailed < 0) throw StatusError{1, "sphere_delaunay: zero-length point"};
            failed += hostFailed; outside += hostOutside;
            std::vector<int32_t> hoff((size_t)nHost + 1, 0);
            int32_t nBig = 0;
            for (int32_t i = 0; i < nHost; ++i) { hoff[i + 1] = hoff[i] + hdeg[i]; if (hdeg[i] > M::STAR_INLINE) ++nBig; }
            const int32_t bigUsed = std::min(h_ctrl[C_BIG], S.bigCap);
            if (bigUsed + nBig > S.bigCap) {                  // a larger pool, the stars it holds carried over
                const int32_t newCap = bigUsed + nBig;
                int32_t* pool = A.dev<int32_t>((size_t)newCap * M::MAX_STAR);
                WO_HIP(hipMemcpyAsync(pool, S.bigPool, (size_t)bigUsed * M::MAX_STAR * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
                WO_HIP(hipStreamSynchronize(s));
                A.release(S.bigPool);
                S.bigPool = pool; S.bigCap = newCap;
            }
            WO_HIP(hipMemcpyAsync(ctrl + C_BIG, &bigUsed, sizeof(int32_t), hipMemcpyHostToDevice, s));
            const int32_t* d_ids = up(R, (const int32_t*)ids.data(), (size_t)nHost, s);
            const int32_t* d_hdeg = up(R, (const int32_t*)hdeg.data(), (size_t)nHost, s);
            const int32_t* d_hoff = up(R, (const int32_t*)hoff.data(), (size_t)nHost + 1, s);
            const int32_t* d_hstars = up(R, (const int32_t*)hstars.data(), std::max<size_t>(1, hstars.size()), s);
            mlaunch(s, k_mesh_place_stars, nHost, WO_BLOCK, nHost, d_ids, d_hdeg, d_hoff, d_hstars, S);
            WO_HIP(hipStreamSynchronize(s));                  // before the host vectors and R go
        }
    }
    failed += h_ctrl[C_FAILED]; outside += h_ctrl[C_OUTSIDE];
    if (failed != 0) throw StatusError{2, star_failure_message(failed, outside)};

    // ---- triangles and half-edges
    int32_t* starOff = A.dev<int32_t>((size_t)V + 1);
    int32_t* ownCount = A.dev<int32_t>((size_t)V);
    int32_t* ownOff = A.dev<int32_t>((size_t)V + 1);
    exclusive_scan(s, A, S.deg, V, starOff, ctrl + C_TOTAL_DEG);
    mlaunch(s, k_mesh_own_count, V, WO_BLOCK, V, S, ownCount);
    exclusive_scan(s, A, ownCount, V, ownOff, ctrl + C_TOTAL_T);
    read_ctrl();
    if (h_ctrl[C_TOTAL_T] != T) throw StatusError{3, "sphere_delaunay: triangle count " + std::to_string(h_ctrl[C_TOTAL_T]) + " != 2V-4 (inconsistent stars)"};
    const int32_t totalDeg = h_ctrl[C_TOTAL_DEG];
    int32_t* triOfStar = A.dev<int32_t>((size_t)std::max(totalDeg, 1));
    int32_t* d_tri = A.dev<int32_t>((size_t)numSides);
    int32_t* d_he = A.dev<int32_t>((size_t)numSides);
    WO_HIP(hipMemsetAsync(triOfStar, 0xFF, (size_t)std::max(totalDeg, 1) * sizeof(int32_t), s));
    mlaunch(s, k_mesh_triangles, V, WO_BLOCK, V, S, (const int32_t*)starOff, (const int32_t*)ownOff, d_tri, triOfStar);
    mlaunch(s, k_mesh_halfedges, numSides, WO_BLOCK, numSides, S, (const int32_t*)starOff, (const int32_t*)d_tri, (const int32_t*)triOfStar, d_he);
    read_ctrl();
    if (h_ctrl[C_BAD_HE] != 0) throw StatusError{4, "sphere_delaunay: " + std::to_string(h_ctrl[C_BAD_HE]) + " unmatched half-edges (inconsistent stars)"};
    WO_HIP(hipMemcpyAsync(out.triangles, d_tri, (size_t)numSides * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    WO_HIP(hipMemcpyAsync(out.halfedges, d_he, (size_t)numSides * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    WO_HIP(hipStreamSynchronize(s));
    if (!out.csr) return;

    // ---- the reference's pole-fan numbering: the host function on the downloaded arrays, then back
    if (out.closure) {
        const int rc = wo_sphere_reference_closure(V, out.triangles, out.halfedges);
        if (rc) throw StatusError{rc, wo_last_error()};
        WO_HIP(hipMemcpyAsync(d_tri, out.triangles, (size_t)numSides * sizeof(int32_t), hipMemcpyHostToDevice, s));
        WO_HIP(hipMemcpyAsync(d_he, out.halfedges, (size_t)numSides * sizeof(int32_t), hipMemcpyHostToDevice, s));
    }

    // ---- CSR and neighbour distances
    int32_t* firstSide = A.dev<int32_t>((size_t)V);
    int32_t* rowCount = ownCount;                             // free again
    int32_t* d_off = ownOff;
    int32_t* d_adj = A.dev<int32_t>((size_t)numSides);
    int32_t* d_adjTri = A.dev<int32_t>((size_t)numSides);
    float* d_dist = A.dev<float>((size_t)numSides);
    WO_HIP(hipMemsetAsync(firstSide, 0x7F, (size_t)V * sizeof(int32_t), s));          // 0x7f7f7f7f: above every side
    mlaunch(s, k_mesh_first_side, numSides, WO_BLOCK, numSides, (const int32_t*)d_tri, firstSide);
    mlaunch(s, k_mesh_csr_count, V, WO_BLOCK, V, numSides, (const int32_t*)firstSide, (const int32_t*)d_he, rowCount, ctrl);
    exclusive_scan(s, A, rowCount, V, d_off, ctrl + C_TOTAL_ADJ);
    read_ctrl();
    if (h_ctrl[C_CSR_BAD] != 0) throw StatusError{5, "mesh_csr: open or malformed half-edge structure"};
    const int32_t E = h_ctrl[C_TOTAL_ADJ];
    if (E > numSides) throw StatusError{5, "mesh_csr: adjacency larger than side count"};
    mlaunch(s, k_mesh_csr_fill, V, WO_BLOCK, V, (const int32_t*)firstSide, (const int32_t*)d_off, (const int32_t*)d_tri, (const int32_t*)d_he, (const float*)d_xyz,
            d_adj, d_adjTri, d_dist);
    WO_HIP(hipMemcpyAsync(out.adjOffset, d_off, ((size_t)V + 1) * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    WO_HIP(hipMemcpyAsync(out.adjList, d_adj, (size_t)E * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    if (out.adjTriList) WO_HIP(hipMemcpyAsync(out.adjTriList, d_adjTri, (size_t)E * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    if (out.neighborDist) WO_HIP(hipMemcpyAsync(out.neighborDist, d_dist, (size_t)E * sizeof(float), hipMemcpyDeviceToHost, s));
    WO_HIP(hipStreamSynchronize(s));                          // before A frees the temporaries
}

int run_mesh_device(const char* fn, wo_ctx* ctx, int32_t V, const MeshIn& in, const MeshOut& out) {
    WO_TRY
        try { mesh_device(ctx, V, in, out); }
        catch (const StatusError& e) {
            (void)hipStreamSynchronize(ctx->stream);          // nothing of this call is in flight when its arenas go
            set_error(e.msg); return e.code;
        }
        return 0;
    WO_CATCH(fn)
}

}  // namespace
}  // namespace wo

using namespace wo;

extern "C" {

int wo_sphere_delaunay_device(wo_ctx* ctx, int32_t numRegions, const float* r_xyz, int32_t* triangles, int32_t* halfedges) {
    if (!ctx) { set_error("wo_sphere_delaunay_device: null context"); return 1; }
    if (!r_xyz || !triangles || !halfedges) { set_error("wo_sphere_delaunay_device: null pointer"); return 1; }
    if (numRegions < 4) { set_error("sphere_delaunay: need at least 4 points"); return 1; }
    return run_mesh_device("wo_sphere_delaunay_device", ctx, numRegions, MeshIn{r_xyz, false, 0.0, 0.0, nullptr}, MeshOut{triangles, halfedges, nullptr, nullptr, nullptr, nullptr, false, false});
}

int wo_sphere_mesh_device(wo_ctx* ctx, int32_t numRegions, const float* r_xyz, int32_t referenceClosure, int32_t* triangles, int32_t* halfedges,
                          int32_t* adjOffset, int32_t* adjList, int32_t* adjTriList, float* neighborDist) {
    if (!ctx) { set_error("wo_sphere_mesh_device: null context"); return 1; }
    if (!r_xyz || !triangles || !halfedges || !adjOffset || !adjList) { set_error("wo_sphere_mesh_device: null pointer"); return 1; }
    if (numRegions < 4) { set_error("sphere_delaunay: need at least 4 points"); return 1; }
    return run_mesh_device("wo_sphere_mesh_device", ctx, numRegions, MeshIn{r_xyz, false, 0.0, 0.0, nullptr},
                           MeshOut{triangles, halfedges, adjOffset, adjList, adjTriList, neighborDist, true, referenceClosure != 0});
}

int wo_sphere_mesh_seed_device(wo_ctx* ctx, int32_t N, double jitter, double seed, int32_t referenceClosure, float* r_xyz, int32_t* triangles,
                               int32_t* halfedges, int32_t* adjOffset, int32_t* adjList, int32_t* adjTriList, float* neighborDist) {
    if (!ctx) { set_error("wo_sphere_mesh_seed_device: null context"); return 1; }
    if (!r_xyz || !triangles || !halfedges || !adjOffset || !adjList) { set_error("wo_sphere_mesh_seed_device: null pointer"); return 1; }
    if (N < 3 || N > points::FIB_MAX_N) { set_error("wo_sphere_mesh_seed_device: need at least 4 points (N + 1), N in range"); return 1; }
    return run_mesh_device("wo_sphere_mesh_seed_device", ctx, N + 1, MeshIn{nullptr, true, jitter, seed, r_xyz},
                           MeshOut{triangles, halfedges, adjOffset, adjList, adjTriList, neighborDist, true, referenceClosure != 0});
}

}  // extern "C"
