// ---------------------------------------------------------------------------------------------------
// priorityFloodCarve (js/terrain-post.js:59-215).  Pass 1 (the noise-keyed best-first flood) runs on the device as a
// label-correcting fixed point (flood_ops.h / flood_kernels.h); passes 2 and 3 (sequential carve along the drain
// paths, ordered fix-up) run per drainage tree on host threads (flood_host.cc) from the downloaded drainTo / surface.
// Which pass 1 runs is read from the environment at every call: WO_FLOOD=device selects the device formulation; the
// default is the host heap walk (the reference's own order, and at 10^7 cells still the faster of the two: see
// DESIGN.md).  The device result is the reference's whenever no decision hinged on two EQUAL keys (the heap orders
// those by its array mechanics); the decisions that did are counted and, if there are any, pass 1 is redone on the host.
// ---------------------------------------------------------------------------------------------------
#include <hip/hip_runtime.h>

#include <chrono>
#include <cstring>

#include "device.h"
#include "erode_block.h"
#include "flood.h"
#include "flood_kernels.h"
#include "stage_clock.h"

namespace wo {

static void flood_gpu_upload_static(wo_planet* p) {
    wo_flood_gpu& G = p->fgpu;
    const FloodScratch& S = p->flood;
    hipStream_t s = p->ctx->stream;
    const int32_t L = S.L;
    if (L > G.cap) {
        // the old state goes first; the capacity is set once every buffer is there, so a failure on the way leaves a state that the next call drops again
        G = wo_flood_gpu{};
        const size_t C = (size_t)L + L / 16 + 1024;
        DeviceArena& a = G.mem;
        G.off = a.dev<int32_t>(C + 1); G.cell = a.dev<int32_t>(C); G.seedIdx = a.dev<int32_t>(C); G.seeds = a.dev<int32_t>(C); G.nz = a.dev<double>(C);
        G.e = a.dev<float>(C);
        G.A = a.dev<FlHead>(C); G.P = a.dev<FlHead>(C); G.F = a.dev<FlHead>(C);
        G.Astk = a.dev<unsigned long long>(C * FL_LD); G.Pstk = a.dev<unsigned long long>(C * FL_LD); G.Fstk = a.dev<unsigned long long>(C * FL_LD);
        G.fdEpoch = a.dev<int32_t>(C); G.inDirty = a.dev<int32_t>(C); G.isPending = a.dev<uint8_t>(C);
        for (auto& l : G.lists) l = a.dev<int32_t>(C);
        G.ctrl = a.dev<FlCtrl>(1);
        G.h_ctrl = a.pinned<FlCtrl>(1);
        G.jump = a.dev<int32_t>(C); G.outPar = a.dev<int32_t>(C); G.outRoot = a.dev<int32_t>(C); G.outSurf = a.dev<float>(C);
        G.h_par = a.pinned<int32_t>(C); G.h_root = a.pinned<int32_t>(C); G.h_surf = a.pinned<float>(C);
        G.cap = (int32_t)C;
    }
    G.mem.release(G.adj);
    G.adj = G.mem.dev<int32_t>(S.adjL.size());
    std::vector<double> nz((size_t)L);
    flood_cell_noise(S, nz.data());
    std::vector<int32_t> seedIdx((size_t)L, -1);
    for (size_t k = 0; k < S.seedCell.size(); ++k) seedIdx[S.seedCell[k]] = (int32_t)k;
    WO_HIP(hipMemcpyAsync(G.off, S.offL.data(), (size_t)(L + 1) * 4, hipMemcpyHostToDevice, s));
    WO_HIP(hipMemcpyAsync(G.adj, S.adjL.data(), S.adjL.size() * 4, hipMemcpyHostToDevice, s));
    WO_HIP(hipMemcpyAsync(G.cell, S.landCell.data(), (size_t)L * 4, hipMemcpyHostToDevice, s));
    WO_HIP(hipMemcpyAsync(G.seedIdx, seedIdx.data(), (size_t)L * 4, hipMemcpyHostToDevice, s));
    WO_HIP(hipMemcpyAsync(G.seeds, S.seedCell.data(), S.seedCell.size() * 4, hipMemcpyHostToDevice, s));
    WO_HIP(hipMemcpyAsync(G.nz, nz.data(), (size_t)L * 8, hipMemcpyHostToDevice, s));
    WO_HIP(hipStreamSynchronize(s));          // the staging vectors go out of scope
    G.L = L; G.nSeeds = (int32_t)S.seedCell.size(); G.version = S.staticVersion;
}

// Returns true when the device result (h_par / h_surf / h_root, land-index space) is valid and may be imported.
static bool flood_device_pass1(wo_planet* p, FloodRun& R) {
    wo_flood_gpu& G = p->fgpu;
    hipStream_t s = p->ctx->stream;
    if (G.version != p->flood.staticVersion) flood_gpu_upload_static(p);
    const int32_t L = G.L;
    if (L == 0) return false;
    FloodDev D{};
    D.L = L; D.off = G.off; D.adj = G.adj; D.cell = G.cell; D.nz = G.nz; D.seedIdx = G.seedIdx; D.e = G.e;
    D.A = G.A; D.Astk = G.Astk; D.P = G.P; D.Pstk = G.Pstk; D.F = G.F; D.Fstk = G.Fstk; D.fdEpoch = G.fdEpoch; D.inDirty = G.inDirty; D.isPending = G.isPending;
    FlLists Ls{{G.lists[0], G.lists[1]}, {G.lists[2], G.lists[3]}, G.lists[4]};
    FlCtrl* C = (FlCtrl*)G.ctrl; FlCtrl* hC = (FlCtrl*)G.h_ctrl;
    hipEvent_t e0 = profile_event(p), e1 = profile_event(p);
    WO_HIP(hipEventRecord(e0, s));
    launch(p, FAM_FLOOD_MISC, k_fl_init, blocks_for(L, 4096), WO_BLOCK, D, G.e, (const float*)p->d_e, C);
    launch(p, FAM_FLOOD_MISC, k_fl_seed_dirty, blocks_for(G.nSeeds, 1024), WO_BLOCK, D, (const int32_t*)G.seeds, G.nSeeds, Ls, C);
    const int grid = blocks_for(L / 4 + 1, 1024);
    constexpr int64_t maxRounds = 200000;
    bool done = false, over = false;
    int batch = 32;
    for (int64_t launched = 0; launched < maxRounds && !done;) {
        for (int b = 0; b < batch; ++b) {
            launch(p, FAM_FLOOD_EVAL, k_fl_eval, grid, WO_BLOCK, D, Ls, C);
            launch(p, FAM_FLOOD_APPLY, k_fl_apply, grid, WO_BLOCK, D, Ls, C);
        }
        launched += batch;
        WO_HIP(hipMemcpyAsync(hC, C, sizeof(FlCtrl), hipMemcpyDeviceToHost, s));
        WO_HIP(hipStreamSynchronize(s));
        done = hC->done != 0; over = hC->overflow != 0;
        if (over) break;
        if (batch < 256) batch *= 2;
    }
    bool ok = done && !over;
    if (ok) {
        launch(p, FAM_FLOOD_MISC, k_fl_verify, blocks_for(L, 4096), WO_BLOCK, D, C);
        launch(p, FAM_FLOOD_MISC, k_fl_jump_init, blocks_for(L, 4096), WO_BLOCK, D, G.jump);
        for (int k = 0; k < 16; ++k) launch(p, FAM_FLOOD_MISC, k_fl_jump, blocks_for(L, 4096), WO_BLOCK, G.jump, L);    // 2^16 hops
        launch(p, FAM_FLOOD_MISC, k_fl_export, blocks_for(L, 4096), WO_BLOCK, D, (const int32_t*)G.jump, G.outPar, G.outSurf, G.outRoot);
        WO_HIP(hipMemcpyAsync(G.h_par, G.outPar, (size_t)L * 4, hipMemcpyDeviceToHost, s));
        WO_HIP(hipMemcpyAsync(G.h_surf, G.outSurf, (size_t)L * 4, hipMemcpyDeviceToHost, s));
        WO_HIP(hipMemcpyAsync(G.h_root, G.outRoot, (size_t)L * 4, hipMemcpyDeviceToHost, s));
        WO_HIP(hipMemcpyAsync(hC, C, sizeof(FlCtrl), hipMemcpyDeviceToHost, s));
    }
    WO_HIP(hipEventRecord(e1, s));
    WO_HIP(hipStreamSynchronize(s));
    float ms = 0; WO_HIP(hipEventElapsedTime(&ms, e0, e1));
    p->eventPool.push_back(e0); p->eventPool.push_back(e1);
    R.deviceMs += ms; R.rounds += hC->rounds; R.epochs += hC->epochs; R.evals += hC->evals; R.usedDevice = true;
    if (ok && hC->notFixed != 0) ok = false;                // cannot happen at termination; refuse the result if it does
    if (ok) {
        R.ties += hC->ties;
        if (hC->ties > 0) ok = false;
    }
    if (!ok) R.fellBack = true;
    return ok;
}

// every cell of the planet in Morton order, if the mirror has worked it out (mask-independent, once per planet): the flood's tables filter it
static const int32_t* morton_if_known(const wo_planet* p) {
    return (!p->h_xyz.empty() && p->mirror.h_morton.size() == (size_t)p->N) ? p->mirror.h_morton.data() : nullptr;
}
static const float* host_xyz(const wo_planet* p) { return p->h_xyz.empty() ? nullptr : p->h_xyz.data(); }
// the flood's tables for the planet's current mask
void ensure_flood_static(wo_planet* p) {
    FloodScratch& S = p->flood;
    if (!S.staticValid || S.staticN != p->N)
        flood_build_static(p->N, p->h_off.data(), p->h_adj.data(), host_xyz(p), p->h_ocean.data(), S, morton_if_known(p));
}
void flood_exchange(wo_planet* p, double carveStrength, FloodHostStats* stats) {
    const int rc = flood_host_passes_exchange(p->N, p->h_off.data(), p->h_adj.data(), host_xyz(p), p->h_pinned, carveStrength, p->flood, stats, p->floodX);
    if (rc) throw HipError{"flood exchange: the host's exchange function failed (status " + std::to_string(rc) + ")"};
}
void flood_stage(wo_planet* p, double carveStrength, FloodRun& R) {
    hipStream_t s = p->ctx->stream;
    const size_t bytes = (size_t)p->N * sizeof(float);
    const bool timing = p->opt.floodTiming;
    HostLap lap{"flood stage", 12, timing};
    if (timing) { WO_HIP(hipStreamSynchronize(s)); lap("drain gpu"); }
    refresh_host_ocean(p);
    lap("ocean mask");
    ensure_flood_static(p);
    lap("static");
    FloodScratch& S = p->flood;
    if (S.L == 0 && !p->floodX.on) return;       // (a share without land still takes part in the exchange)
    const bool hostOnly = p->floodX.on || !p->opt.floodDevice;
    WO_HIP(hipMemcpyAsync(p->h_pinned, p->d_e, bytes, hipMemcpyDeviceToHost, s));
    const bool useDevice = !hostOnly && flood_device_pass1(p, R);       // synchronises the stream
    if (hostOnly) WO_HIP(hipStreamSynchronize(s));
    lap(hostOnly ? "D2H" : "device pass1");
    if (useDevice) {
        flood_gather(p->h_pinned, S);
        flood_import_pass1(p->fgpu.h_par, p->fgpu.h_surf, p->fgpu.h_root, S);
        flood_pass23_host(p->h_pinned, carveStrength, S);
    } else if (p->floodX.on) {
        if (p->floodX.trueOcean.size() != (size_t)p->N) throw HipError{"flood exchange: the true ocean mask does not fit the planet"};
        flood_exchange(p, carveStrength, &R.host);
    } else {
        flood_host_passes(p->h_pinned, carveStrength, S, &R.host);
    }
    lap(useDevice ? "import + host pass2+3" : "host passes");
    WO_HIP(hipMemcpyAsync(p->d_e, p->h_pinned, bytes, hipMemcpyHostToDevice, s));
    if (timing) { WO_HIP(hipStreamSynchronize(s)); lap("H2D"); }
}

// The flood stage of a planet inside its land-first mirror.  The mirror numbers the land cells 0 .. L-1 in Morton order of their positions,
// which is the order of the host flood's own land list (both come from morton_order_cells on the same mask; checked once per (mirror,
// flood tables) pair by comparing the two lists): the first L floats of the mirrored field ARE the flood's land heights.  So the stage
// copies 4 L bytes each way instead of 4 N (11 instead of 40 MB at the benched size), the host passes index them directly
// (FloodScratch::landOrder) and the field never leaves the mirror (no scatter into the planet's order before, no gather after).
bool flood_land_is_mirror_prefix(wo_planet* p) {
    auto& M = p->mirror;
    const FloodScratch& S = p->flood;
    if (p->floodPrefixMirror != M.version || p->floodPrefixStatic != S.staticVersion) {
        p->floodPrefixMirror = M.version; p->floodPrefixStatic = S.staticVersion;
        p->floodPrefixOk = p->erode && S.L == p->erode->L && M.h_perm.size() == (size_t)p->N && (size_t)S.L <= M.h_perm.size() &&
                           std::memcmp(M.h_perm.data(), S.landCell.data(), sizeof(int32_t) * (size_t)S.L) == 0;
    }
    return p->floodPrefixOk;
}
void flood_stage_land(wo_planet* p, double carveStrength, FloodRun& R) {
    hipStream_t s = p->ctx->stream;
    FloodScratch& S = p->flood;
    const size_t bytes = (size_t)S.L * sizeof(float);
    const bool timing = p->opt.floodTiming;
    HostLap lap{"flood stage", 12, timing};
    if (timing) { WO_HIP(hipStreamSynchronize(s)); lap("drain gpu"); }
    // The land heights travel through the planet's own hipHostMalloc'ed buffer (allocated once per planet, N floats).  Round 5 page-locked the flood's
    // own array instead (hipHostRegister of a THP-advised heap block, 0.5 ms of a 312 ms step): user-pointer registrations of transparent-huge-page memory
    // are invalidated whenever the kernel collapses or splits those pages, and a copy in flight at that moment faults — the SIGABRT under
    // hipStreamSynchronize of the round-5 GPU suite.  Nothing in this library registers memory it did not get from hipHostMalloc.
    float* host = p->h_pinned;
    WO_HIP(hipMemcpyAsync(host, p->d_e, bytes, hipMemcpyDeviceToHost, s));
    WO_HIP(hipStreamSynchronize(s));
    lap("D2H (land)");
    S.landOrder = true;
    try { flood_host_passes(host, carveStrength, S, &R.host); } catch (...) { S.landOrder = false; throw; }
    S.landOrder = false;
    lap("host passes");
    WO_HIP(hipMemcpyAsync(p->d_e, host, bytes, hipMemcpyHostToDevice, s));
    if (timing) { WO_HIP(hipStreamSynchronize(s)); lap("H2D (land)"); }
}

}  // namespace wo
