// ---------------------------------------------------------------------------------------------------
// Patch-major mirror of the mesh for erodeComposite.  The reference numbers the cells along the Fibonacci spiral, where the
// neighbours of consecutive cells lie in ~8 separate clusters 5*sqrt(N) ids apart and a 128-byte line of per-cell state
// holds 32 cells of which 9 are land: the neighbour gathers of every erosion pass cost an L2 transaction each.
// Inside erodeComposite nothing depends on the NAME of a cell except (i) the initial order of landCells (ascending id,
// js/terrain-post.js:384-390; later orders are stable sorts of it) and (ii) the flood's cellNoise(r) — rows keep the
// reference's adjacency order, ranks are positions in landCells.  So the whole call runs on a renamed copy of the graph
// (cells in Morton order of their positions: a wave's 64 cells and their neighbours share a few lines), with the initial
// land order mapped through the renaming and the field moved back to the planet's own order around each flood and at the end.
// Results are bit-identical (same operations on the same values in the same order); measured at 10 M cells the step went
// 1.10 -> 0.85 s.  WO_LAYOUT=index switches the mirror off.
// ---------------------------------------------------------------------------------------------------
#include <hip/hip_runtime.h>

#include <cstring>

#include "common_kernels.h"
#include "device.h"
#include "erode_ops.h"
#include "mirror.h"
#include "stage_clock.h"

namespace wo {

// perm: mirror id -> cell id, inv: the inverse
__global__ __launch_bounds__(WO_BLOCK) void k_mirror_gather_f32(const float* src, const int32_t* perm, float* dst, int32_t n) { WO_GRID_STRIDE(i, n) dst[i] = src[perm[i]]; }
__global__ __launch_bounds__(WO_BLOCK) void k_mirror_scatter_f32(const float* src, const int32_t* perm, float* dst, int32_t n) { WO_GRID_STRIDE(i, n) dst[perm[i]] = src[i]; }
__global__ __launch_bounds__(WO_BLOCK) void k_mirror_gather_u8(const uint8_t* src, const int32_t* perm, uint8_t* dst, int32_t n) { WO_GRID_STRIDE(i, n) dst[i] = src[perm[i]]; }
__global__ __launch_bounds__(WO_BLOCK) void k_mirror_map_i32(const int32_t* in, const int32_t* map, int32_t* out, int32_t n) { WO_GRID_STRIDE(i, n) out[i] = map[in[i]]; }
__global__ __launch_bounds__(WO_BLOCK) void k_mirror_invert(const int32_t* perm, int32_t* inv, int32_t n) { WO_GRID_STRIDE(i, n) inv[perm[i]] = i; }
// rows keep their order (the reference's adjacency order is part of its semantics); only the ids are renamed
__global__ __launch_bounds__(WO_BLOCK) void k_mirror_rows(const int32_t* off, const int32_t* adj, const float* dist, const float* xyz, const int32_t* perm,
                                                           const int32_t* inv, const int32_t* moff, int32_t* madj, float* mdist, float* mxyz, int32_t n) {
    WO_GRID_STRIDE(i, n) {
        const int32_t r = perm[i];
        const int32_t b = off[r], deg = off[r + 1] - b, mb = moff[i];
        for (int32_t k = 0; k < deg; ++k) { madj[mb + k] = inv[adj[b + k]]; mdist[mb + k] = dist[b + k]; }
        mxyz[3 * i] = xyz[3 * r]; mxyz[3 * i + 1] = xyz[3 * r + 1]; mxyz[3 * i + 2] = xyz[3 * r + 2];
    }
}

static bool mirror_wanted(const wo_planet* p) {
    return !p->opt.layoutIndex && !p->h_xyz.empty() && p->N > 1;
}
// mask (may be null): the ocean mask of the call the mirror is entered for.  With a mask the renaming is LAND FIRST: the land
// cells in Morton order take the ids 0 .. L-1, the ocean cells follow in Morton order.  Every per-cell array of the erosion
// passes is then dense over the land (the passes touch land cells only: 28 % of a synthetic planet, so in plain Morton order a
// 64-byte line of per-cell state held ~4.5 useful entries of 16 and every 4-8-byte store of a pass was a partial line), the land
// list of the index-order passes is the identity, and a land cell's land neighbours sit 3.6x closer in memory.  The renaming is
// still only a renaming (rows keep their order, the initial land order is mapped through it): bit-identical results.  The mirror
// is rebuilt when a call arrives with a different mask (~50 ms at 10 M cells; the bench's steps all have the same one).
static void mirror_build(wo_planet* p, const uint8_t* mask = nullptr) {
    auto& M = p->mirror;
    const int32_t N = p->N; const size_t E = (size_t)p->E;
    // (the planet's own host mask carries a version: the 10 MB comparison — 0.4 ms of host time with the device idle, at the top of every call — is only made for other masks)
    const bool ownMask = mask && mask == p->h_ocean.data();
    if (M.built && ownMask && M.h_mask.size() == (size_t)N && p->mirrorMaskVersion == p->oceanVersion) return;
    if (M.built && (!mask || (M.h_mask.size() == (size_t)N && std::memcmp(M.h_mask.data(), mask, (size_t)N) == 0))) { if (ownMask) p->mirrorMaskVersion = p->oceanVersion; return; }
    hipStream_t s = p->ctx->stream;
    HostLap lap{"mirror", 18, p->opt.floodTiming};          // WO_FLOOD_TIMING: what a new terrain's tables cost (bench.py: new_terrain_step_ms)
    if (M.h_morton.empty()) { morton_order_cells(N, p->h_xyz.data(), M.h_morton); lap("morton order"); }
    M.h_perm.resize(N);
    if (mask) {
        // land cells first, each class in Morton order: per range of the Morton list the land count, then both classes written behind the ranges before
        std::vector<int64_t> cnt(host_threads() + 2, 0);
        const int32_t* mo = M.h_morton.data();
        parallel_ranges(N, [&](int64_t b, int64_t e, int t) { int64_t c = 0; for (int64_t i = b; i < e; ++i) c += mask[mo[i]] ? 0 : 1; cnt[t + 1] = c; });
        for (size_t t = 1; t < cnt.size(); ++t) cnt[t] += cnt[t - 1];
        const int64_t nl = cnt.back();
        int32_t* perm = M.h_perm.data();
        parallel_ranges(N, [&](int64_t b, int64_t e, int t) {
            int64_t a = cnt[t], o = nl + (b - cnt[t]);          // land before this range: cnt[t]; ocean before it: b - cnt[t]
            for (int64_t i = b; i < e; ++i) { const int32_t r = mo[i]; if (mask[r]) perm[o++] = r; else perm[a++] = r; }
        });
        M.h_mask.assign(mask, mask + N);
        p->mirrorMaskVersion = ownMask ? p->oceanVersion : -1;
    } else {
        std::memcpy(M.h_perm.data(), M.h_morton.data(), (size_t)N * 4);
        M.h_mask.clear();
    }
    lap("land-first perm");
    hvec<int32_t> moff((size_t)N + 1);
    moff[0] = 0;
    {
        const int32_t* perm = M.h_perm.data(); const int32_t* ho = p->h_off.data(); int32_t* mo = moff.data();
        parallel_ranges(N, [&](int64_t b, int64_t e, int) { for (int64_t i = b; i < e; ++i) { const int32_t r = perm[i]; mo[i + 1] = ho[r + 1] - ho[r]; } });
        inclusive_scan_parallel(mo + 1, (int64_t)N);
    }
    lap("row offsets");
    if (!M.coast) {
        // built in an arena of its own and handed over whole; coast, assigned last, says that the buffers are there
        DeviceArena a;
        M.perm = a.dev<int32_t>(N); M.inv = a.dev<int32_t>(N); M.off = a.dev<int32_t>((size_t)N + 1); M.adj = a.dev<int32_t>(E + WO_ROW);
        M.dist = a.dev<float>(E + WO_ROW);
        WO_HIP(hipMemsetAsync(M.adj + E, 0, WO_ROW * sizeof(int32_t), s)); WO_HIP(hipMemsetAsync(M.dist + E, 0, WO_ROW * sizeof(float), s));
        M.xyz = a.dev<float>(3 * (size_t)N); M.e = a.dev<float>(N); M.e2 = a.dev<float>(N);
        M.ocean = a.dev<uint8_t>(N); uint8_t* coast = a.dev<uint8_t>(N);
        M.mem.adopt(a); M.coast = coast;
    }
    // the mirror's rows are rebuilt from the planet's own arrays: a scope must not be active (its pointers would be the mirror's)
    const int32_t* o_off = M.active ? M.o_off : p->d_off; const int32_t* o_adj = M.active ? M.o_adj : p->d_adj;
    const float* o_dist = M.active ? M.o_dist : p->d_dist; const float* o_xyz = M.active ? M.o_xyz : p->d_xyz;
    WO_HIP(hipMemcpyAsync(M.perm, M.h_perm.data(), (size_t)N * 4, hipMemcpyHostToDevice, s));
    WO_HIP(hipMemcpyAsync(M.off, moff.data(), ((size_t)N + 1) * 4, hipMemcpyHostToDevice, s));
    launch(p, FAM_MISC, k_mirror_invert, blocks_for(N, 4096), WO_BLOCK, (const int32_t*)M.perm, M.inv, N);
    launch(p, FAM_MISC, k_mirror_rows, blocks_for(N, 4096), WO_BLOCK, o_off, o_adj, o_dist, o_xyz, (const int32_t*)M.perm, (const int32_t*)M.inv, (const int32_t*)M.off, M.adj, M.dist, M.xyz, N);
    WO_HIP(hipStreamSynchronize(s));                    // moff / h_perm uploads done
    lap("upload + rows");
    M.built = true;
    ++M.version;
}

void MirrorScope::enter(const uint8_t* mask) {
    if (!mirror_wanted(p) || p->mirror.active) return;
    mirror_build(p, mask);
    auto& M = p->mirror;
    const int32_t N = p->N;
    launch(p, FAM_MISC, k_mirror_gather_f32, blocks_for(N, 4096), WO_BLOCK, (const float*)p->d_e, (const int32_t*)M.perm, M.e, N);
    launch(p, FAM_MISC, k_mirror_gather_u8, blocks_for(N, 4096), WO_BLOCK, (const uint8_t*)p->d_ocean, (const int32_t*)M.perm, M.ocean, N);
    M.o_off = p->d_off; M.o_adj = p->d_adj; M.o_dist = p->d_dist; M.o_xyz = p->d_xyz; M.o_e = p->d_e; M.o_e2 = p->d_e2; M.o_ocean = p->d_ocean; M.o_coast = p->d_coast;
    point_at_mirror(M.e, M.e2);
    M.active = on = true;
}
void MirrorScope::suspend() {
    if (!on) return;
    auto& M = p->mirror;
    launch(p, FAM_MISC, k_mirror_scatter_f32, blocks_for(p->N, 4096), WO_BLOCK, (const float*)p->d_e, (const int32_t*)M.perm, M.o_e, p->N);
    cur = p->d_e; cur2 = p->d_e2;
    point_at_planet();
}
void MirrorScope::resume() {
    if (!on) return;
    auto& M = p->mirror;
    launch(p, FAM_MISC, k_mirror_gather_f32, blocks_for(p->N, 4096), WO_BLOCK, (const float*)M.o_e, (const int32_t*)M.perm, cur, p->N);
    point_at_mirror(cur, cur2);
}

void mirror_gather_f32(wo_planet* p, const float* src, float* dst) {
    launch(p, FAM_MISC, k_mirror_gather_f32, blocks_for(p->N, 4096), WO_BLOCK, src, (const int32_t*)p->mirror.perm, dst, p->N);
}
void mirror_map_i32(wo_planet* p, const int32_t* in, int32_t* out, int32_t n) {
    launch(p, FAM_MISC, k_mirror_map_i32, blocks_for(n, 4096), WO_BLOCK, in, (const int32_t*)p->mirror.inv, out, n);
}

}  // namespace wo
