// erodeComposite on the planet's resident field (js/terrain-post.js:369-707; its caller: js/planet-worker.js:40-102).
//
// Orchestration follows the reference's call structure, but every per-cell loop is a kernel launch on the planet's
// stream and every order-defined loop is executed as synchronous dependency rounds (erode_ops.h).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>

#include "../../include/worogen.h"
#include "erode_block.h"
#include "flood.h"
#include "kernels_impl.h"
#include "mirror.h"
#include "stage_clock.h"

namespace wo {

__global__ __launch_bounds__(WO_BLOCK) void k_fill_i32(int32_t* a, int32_t v, int32_t n) { WO_GRID_STRIDE(i, n) a[i] = v; }

constexpr int WO_PATCH_TOTAL_SLOTS = 4096;         // pending-total slots of the patch solve (one per launch, reused modulo)

// What every call needs of the erosion block
static void ensure_scratch(wo_planet* p) {
    wo_erode_block& B = *p->erode; auto& S = B.scratch; const size_t N = (size_t)p->N;
    build_group(B, S, [&](DeviceArena& a) {
        S.landIdx = a.dev<int32_t>(N); S.land[0] = a.dev<int32_t>(N); S.land[1] = a.dev<int32_t>(N);
        S.keys[0] = a.dev<uint32_t>(N); S.keys[1] = a.dev<uint32_t>(N);
        S.rank = a.dev<int32_t>(N);
        S.cellDist = a.dev<float>(N); S.flow = a.dev<float>(N); S.task = a.dev<SolveTask>(N);
        // tags of the unchecked basin passes count up from here: no stale tag may look like a coming one
        S.out = a.dev<SolveOut>(N); WO_HIP(hipMemset(S.out, 0, N * sizeof(SolveOut)));
        S.flowCnt = a.dev<int32_t>(N); WO_HIP(hipMemset(S.flowCnt, 0, (size_t)N * 4));
        S.tr = a.dev<TargetRank>(N); S.ev = a.dev<EventList>(N); S.me = a.dev<float>(N); S.carveSlot = a.dev<int32_t>(N);
        S.accCnt = a.dev<unsigned long long>(N); S.jump = a.dev<int32_t>(N); S.nj = a.dev<int32_t>(N);
        S.doneAt = a.dev<int32_t>(N);
        S.totalExcess = a.dev<double>(N);
        S.glac = a.dev<float>(N); S.iceFlow = a.dev<float>(N); S.iceTarget = a.dev<int32_t>(N); S.arank = a.dev<int32_t>(N);
        S.iceUp = a.dev<uint8_t>(N);
        S.listA = a.dev<int32_t>(N); S.listB = a.dev<int32_t>(N); S.counters = a.dev<int32_t>(8);
        S.patchOrder = a.dev<int32_t>(N); S.slotOf = a.dev<int32_t>(N); S.patchPending = a.dev<int32_t>(N / WO_PATCH + 2);
        S.patchTotals = a.dev<int32_t>(WO_PATCH_TOTAL_SLOTS); S.patchBlk = a.dev<int32_t>(N);
        S.h_patchTotals = a.pinned<int32_t>(WO_PATCH_TOTAL_SLOTS);          // read-back buffer of run_solve_patches
        S.sortTemp = a.dev<uint8_t>(std::max<size_t>(sort_temp_bytes(p->N), 16));
        WO_HIP(hipMemsetAsync(S.glac, 0, N * sizeof(float), p->ctx->stream));
    });
}

// Basin solve driver (basin.hip): the first launch of the pass is k_solve_basin on the group-major store order of basin_layout(), which
// normally leaves nothing pending; whatever it does leave (layout off: see basin.hip) is finished by k_solve_patch launches until no task
// is pending.  Returns the number of launches.  The pass's setup launch (k_solve_setup_batched) has cleared the patch counters and the
// pending totals: one slot per launch, cleared once per pass (a memset per launch was 13.6 k fill kernels per step).
static int64_t run_solve_patches(wo_planet* p, const Fields& F, double K, double m, double dt, bool deferCheck, int32_t passTag) {
    wo_erode_block& B = *p->erode; auto& S = B.scratch;
    hipStream_t s = p->ctx->stream;
    const int np = S.numPatches;
    if (deferCheck) {
        // the one launch of the basin solve, and no look at what it left: tasks left pending are counted into a word that is not
        // cleared during the call and looked at where the host synchronises anyway (erode_composite: RedoWithChecks)
        basin_solve_launch(p, F, passTag, B.redo.pendingEver);
        S.lastPatchLaunches = 1;
        return 1;
    }
    int32_t* tot = S.patchTotals;
    int64_t launches = 0;
    // polling passes per visit (kernels_impl.h); launches from lateFrom on (few patches still open: no queue of visits behind a
    // long one) may poll longer
    constexpr int spinCap = WO_PATCH_SPIN_CAP, lateFrom = WO_PATCH_LATE_FROM, lateCap = WO_PATCH_LATE_SPIN_CAP;
    int64_t need = 0;
    for (int32_t tag = 1;; ) {
        // The pending totals are read back (one stream sync) after every burst.  The number of launches a pass needs barely
        // changes from one erosion iteration to the next, so the first burst is the previous need plus one; then small bursts.
        // Launches after the one that emptied the list find nothing pending and return at once.
        const int32_t first = tag;
        const int burst = (tag == 1) ? std::max<int>(1, (int)std::min<int64_t>(S.lastPatchLaunches, WO_PATCH_TOTAL_SLOTS / 2)) : 3;
        for (int b = 0; b < burst; ++b, ++tag) {
            // A burst never spans a wrap of the slot ring: the wrap's memset would clear the slots of the burst's earlier
            // tags before they are read back (they would read as 0 = "nothing pending").  The wrap starts the next burst.
            if (tag % WO_PATCH_TOTAL_SLOTS == 0) {
                if (b > 0) break;
                WO_HIP(hipMemsetAsync(tot, 0, (size_t)WO_PATCH_TOTAL_SLOTS * sizeof(int32_t), s));   // wrapped: every earlier slot has been read back
            }
            if (tag == 1) basin_solve_launch(p, F, tag, tot + 1);
            else {
                // the first k_solve_patch launch after a lean setup: its blocker hints are made from the records now (only tasks the basin
                // launch left pending get one; normally there is no such launch at all)
                if (tag == 2 && F.solveLean) launch(p, FAM_MISC, k_solve_blk_init, blocks_for(B.L, 4096), WO_BLOCK, F, B.L);
                launch(p, FAM_SOLVE_PATCH, k_solve_patch, np, WO_PATCH_THREADS, F, B.L, tag, S.patchPending, tot + (tag % WO_PATCH_TOTAL_SLOTS), K, m, dt,
                       (int32_t*)nullptr, (int32_t)(tag >= lateFrom ? lateCap : spinCap));
            }
            ++launches;
        }
        if (first == 1 && tag == 2) {                     // the usual case: the one launch of the basin solve, one total to look at
            if (read_count(p, tot + 1) == 0) need = 1;
        } else {
            WO_HIP(hipMemcpyAsync(S.h_patchTotals, tot, (size_t)WO_PATCH_TOTAL_SLOTS * sizeof(int32_t), hipMemcpyDeviceToHost, s));
            WO_HIP(hipStreamSynchronize(s));
            for (int32_t t = first; t < tag && !need; ++t) if (S.h_patchTotals[t % WO_PATCH_TOTAL_SLOTS] == 0) need = t;
        }
        if (need) break;
        if (launches > 4 * (int64_t)p->N + 1024) throw HipError{"patch solve does not converge"};
    }
    S.lastPatchLaunches = need;      // the first burst is exactly what the last pass needed (its first launch is the basin one)
    return need;
}

// The planet's side stream (the basin layout beside the flow accumulation).  No arena owns a stream or an event: side_destroy drops them
static void side_destroy(wo_erode_block::Side& S) {
    if (S.stream) { (void)hipStreamSynchronize(S.stream); (void)hipStreamDestroy(S.stream); }
    if (S.fork) (void)hipEventDestroy(S.fork);
    if (S.join) (void)hipEventDestroy(S.join);
    S = wo_erode_block::Side{};
}
static void ensure_side_stream(wo_planet* p) {
    auto& S = p->erode->side;
    if (S.built) return;
    side_destroy(S);                       // (what an attempt that failed half-way left)
    // the layout's chain of short launches is the longer of the two: at equal priority its workgroups queue behind the thousands of
    // the flow kernels' (a 22 us scatter pass took 108 us beside k_flow_final), so the side stream gets the highest priority
    int prLeast = 0, prGreatest = 0;
    WO_HIP(hipDeviceGetStreamPriorityRange(&prLeast, &prGreatest));
    WO_HIP(hipStreamCreateWithPriority(&S.stream, hipStreamNonBlocking, prGreatest));
    WO_HIP(hipEventCreateWithFlags(&S.fork, hipEventDisableTiming)); WO_HIP(hipEventCreateWithFlags(&S.join, hipEventDisableTiming));
    S.built = true;
}

// erodeComposite on the resident field (js/terrain-post.js:369-707)
// Thrown by erode_composite when a basin-solve launch whose result was not checked on the spot turns out to have left tasks pending:
// the caller restores the field and runs the call again with the check after every pass (erode_composite_checked).
struct RedoWithChecks {};

// One erodeComposite call: its parameters, the constants that follow from them, and what its stages count (wo_last_erode_stats)
struct ErodeCall {
    wo_planet* p;
    int32_t hIters; double K, m, dt; int32_t tIters; double talus, kThermal; int32_t gIters; double gStrength; bool checkEveryPass;
    int32_t total, midIter; double gCarve, gConv, gDep, gFjord;
    int gridN, gridL = 0;                   // gridL: index-order passes over the ascending land list (set by erode_setup)
    StageClock clk; MirrorScope mir; FloodRun floodRun;
    int64_t sorts = 0, maxSolve = 0, patchLaunches = 0, basinPasses = 0, basinLeftoverPasses = 0, iceRounds = 0, carveRounds = 0, carveActive = 0, carveFlowLeft = 0;
    double floodHostMs = 0;
    ErodeCall(wo_planet* pl, int32_t h, double K_, double m_, double dt_, int32_t t, double talus_, double kT, int32_t g, double gs, bool check)
        : p(pl), hIters(h), K(K_), m(m_), dt(dt_), tIters(t), talus(talus_), kThermal(kT), gIters(std::max(g, 0)), gStrength(gs != gs ? 0 : gs),
          checkEveryPass(check), total(std::max(hIters, std::max(tIters, gIters))), midIter((int32_t)std::floor(total * 0.75 + 0.5)),
          gridN(xcd_grid(pl->N)), clk(pl), mir(pl) {
        const double gScale = gIters > 0 ? 1.0 / gIters : 0;
        gCarve = 0.02 * gScale; gConv = 0.01 * gScale; gDep = 0.005 * gScale; gFjord = 0.015 * gScale;
    }
    void stats(bool mirrored) const {
        const wo_erode_block& B = *p->erode; const auto& S = B.scratch;
        p->erodeStats = {{"land_cells", (double)B.L}, {"mirror_layout", mirrored ? 1.0 : 0.0}, {"iterations", (double)total}, {"sorts", (double)sorts},
                         {"solve_launches_max_per_pass", (double)maxSolve}, {"solve_patch_launches_total", (double)patchLaunches},
                         {"solve_basin_passes", (double)basinPasses}, {"solve_basin_passes_with_leftovers", (double)basinLeftoverPasses},
                         {"flow_two_level", (B.tiles.built && S.identity && hIters > 0) ? 1.0 : 0.0}, {"ice_rounds_total", (double)iceRounds},
                         {"carve_rounds_total", (double)carveRounds}, {"carve_active_total", (double)carveActive}, {"carve_flow_launches_with_leftovers", (double)carveFlowLeft}, {"solve_check_every_pass", checkEveryPass ? 1.0 : 0.0}, {"calls_run_again_with_checks", (double)B.redo.calls}, {"flood_stage_ms", floodHostMs},
                         {"flood_device_pass1_ms", floodRun.deviceMs}, {"flood_device_rounds", (double)floodRun.rounds}, {"flood_device_epochs", (double)floodRun.epochs},
                         {"flood_device_evaluations", (double)floodRun.evals}, {"flood_equal_key_decisions", (double)floodRun.ties}, {"flood_pass1_on_host", (floodRun.usedDevice && !floodRun.fellBack) ? 0.0 : 1.0},
                         {"flood_host_calls", (double)floodRun.host.calls}, {"flood_host_serial_pass1", (double)floodRun.host.serialPass1}, {"flood_host_tie_groups", (double)floodRun.host.tieGroups}, {"flood_host_contested", (double)floodRun.host.contested},
                         {"flood_host_open_parents", (double)floodRun.host.openParents}, {"flood_host_unresolved", (double)floodRun.host.unresolved},
                         {"flood_host_path_redo", (double)floodRun.host.pathRedo}, {"flood_host_replays", (double)floodRun.host.replays}, {"flood_host_replayed_landmasses", (double)floodRun.host.replayedLandmasses}, {"flood_host_pass1_ms", floodRun.host.pass1Ms},
                         {"flood_host_pass23_ms", floodRun.host.pass23Ms},
                         {"relaxed_sort_every", (double)p->opt.relaxedSortEvery}, {"relaxed_full", p->opt.relaxedFull ? 1.0 : 0.0}, {"flood_exchange_calls", (double)p->floodX.calls}, {"flood_exchange_gathers", (double)p->floodX.gathers}, {"flood_exchange_whole_planet_floods", (double)p->floodX.globalFloods}, {"flood_exchange_received", (double)p->floodX.received}};
    }
};
// The indices i in [0, n) whose cell cell(i) is land, ascending, into out (on the host's workers); returns their number
template <class Cell>
static int32_t compact_land(int64_t n, const uint8_t* ocean, Cell cell, int32_t* out) {
    std::vector<int64_t> cnt(host_threads() + 2, 0);
    parallel_ranges(n, [&](int64_t b, int64_t e, int t) { int64_t c = 0; for (int64_t i = b; i < e; ++i) c += ocean[cell(i)] ? 0 : 1; cnt[t + 1] = c; });
    for (size_t t = 1; t < cnt.size(); ++t) cnt[t] += cnt[t - 1];
    parallel_ranges(n, [&](int64_t b, int64_t e, int t) { int64_t o = cnt[t]; for (int64_t i = b; i < e; ++i) if (!ocean[cell(i)]) out[o++] = (int32_t)i; });
    return (int32_t)cnt.back();
}
// A share without land (landmass decomposition of a small planet) still answers the other shares' flood exchanges; then the call is over
static void erode_without_land(ErodeCall& c) {
    wo_planet* p = c.p;
    if (p->floodX.on) {
        hipStream_t s = p->ctx->stream;
        const int calls = (c.hIters > 0 ? 1 : 0) + (c.midIter < c.total ? 1 : 0);
        WO_HIP(hipMemcpyAsync(p->h_pinned, c.mir.on ? p->mirror.o_e : p->d_e, (size_t)p->N * sizeof(float), hipMemcpyDeviceToHost, s));
        WO_HIP(hipStreamSynchronize(s));
        ensure_flood_static(p);
        for (int k = 0; k < calls; ++k) flood_exchange(p, 0.5, nullptr);
    }
    c.mir.finish();
    c.clk.end(); c.clk.finish();
}
// The "setup" stage: the field into the land-first mirror, the land lists, the ranks, the solve's patch order and the ocean cells'
// constants.  Returns false for a share without land (the call is over then).
static bool erode_setup(ErodeCall& c) {
    wo_planet* p = c.p; hipStream_t s = p->ctx->stream; wo_erode_block& B = *p->erode; auto& S = B.scratch;
    const int32_t N = p->N;
    c.clk.begin("setup");
    refresh_host_ocean(p);          // the planet's own mask, before the pointers move
    c.mir.enter(p->h_ocean.data());          // land first (mirror_build)
    S.identity = c.mir.on && p->mirror.h_mask.size() == (size_t)N;      // land cells are the ids 0 .. L-1: the index-order passes skip the land list
    coast_flags(p);
    // landCells in ascending r (js/terrain-post.js:384-390): host-side compaction of the ocean mask
    int32_t* hl = reinterpret_cast<int32_t*>(p->h_pinned);
    const uint8_t* oc = p->h_ocean.data();
    // both lists only depend on the mask (and on whether the call runs on the mirror): a call with the mask of the previous one takes them as they are
    const bool listsKept = B.lists.built && B.lists.ocean == p->oceanVersion && B.lists.mirror == c.mir.on && B.lists.L >= 0;
    const int32_t L = listsKept ? B.lists.L : compact_land(N, oc, [](int64_t r) { return r; }, hl);
    B.L = L;
    if (L == 0) { erode_without_land(c); return false; }
    if (listsKept) {
        WO_HIP(hipMemcpyAsync(S.land[0], B.lists.init, (size_t)L * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
    } else if (c.mir.on) {
        // initial landCells: the same cells in the same (ascending-r) order, under their mirror names
        WO_HIP(hipMemcpyAsync(S.listA, hl, (size_t)L * sizeof(int32_t), hipMemcpyHostToDevice, s));
        mirror_map_i32(p, S.listA, S.land[0], L);
        WO_HIP(hipStreamSynchronize(s));
        // the list the index-order passes iterate: land cells in ascending mirror id
        const int32_t* perm = p->mirror.h_perm.data();
        compact_land(N, oc, [perm](int64_t i) { return perm[i]; }, hl);
        WO_HIP(hipMemcpyAsync(S.landIdx, hl, (size_t)L * sizeof(int32_t), hipMemcpyHostToDevice, s));
    } else {
        WO_HIP(hipMemcpyAsync(S.landIdx, hl, (size_t)L * sizeof(int32_t), hipMemcpyHostToDevice, s));
        WO_HIP(hipMemcpyAsync(S.land[0], S.landIdx, (size_t)L * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
    }
    if (!listsKept) {
        build_group(B, B.lists, [&](DeviceArena& a) { B.lists.init = a.dev<int32_t>((size_t)N); });
        WO_HIP(hipMemcpyAsync(B.lists.init, S.land[0], (size_t)L * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
        B.lists.ocean = p->oceanVersion; B.lists.mirror = c.mir.on; B.lists.L = L;
    }
    WO_HIP(hipStreamSynchronize(s));       // h_pinned is reused by the flood stage
    S.cur = 0;
    launch(p, FAM_MISC, k_init_rank, c.gridN, WO_BLOCK, S.rank, N);
    rank_from_land(p);      // thermal-only runs never sort: landCells stays in ascending-r order
    // spatial patches for the patch-local solve: land cells in Morton order (shared with the host flood's layout)
    if (c.hIters > 0) {
        ensure_flood_static(p);
        if (S.patchVersion != p->flood.staticVersion || S.patchMirror != c.mir.on) {
            S.patchMirror = c.mir.on;
            if (c.mir.on) WO_HIP(hipMemcpyAsync(S.patchOrder, S.landIdx, (size_t)L * sizeof(int32_t), hipMemcpyDeviceToDevice, s));   // ascending mirror id IS Morton order
            else WO_HIP(hipMemcpyAsync(S.patchOrder, p->flood.landCell.data(), (size_t)L * sizeof(int32_t), hipMemcpyHostToDevice, s));
            launch(p, FAM_MISC, k_fill_i32, c.gridN, WO_BLOCK, S.slotOf, -1, N);
            launch(p, FAM_MISC, k_slot_scatter, blocks_for(L, 4096), WO_BLOCK, (const int32_t*)S.patchOrder, S.slotOf, L);
            WO_HIP(hipStreamSynchronize(s));
            S.patchVersion = p->flood.staticVersion;
            S.lastPatchLaunches = 1;
            S.numPatches = (L + WO_PATCH - 1) / WO_PATCH;
        }
    } else S.patchVersion = -1;
    c.gridL = xcd_grid(L);
    if (c.hIters > 0 || c.tIters > 0) {
        // ocean cells keep these values through the whole call: both elevation buffers hold them, and the per-ocean-cell
        // constants of the land passes are written once
        WO_HIP(hipMemcpyAsync(p->d_e2, p->d_e, (size_t)N * sizeof(float), hipMemcpyDeviceToDevice, s));
        launch(p, FAM_MISC, k_erode_ocean_init, blocks_for(N, 4096), WO_BLOCK, fields(p));
    }
    c.clk.end();
    return true;
}
// The host is about to read the field: an unchecked basin launch of this call that left tasks pending sends the call back to run again with checks
static void leftovers_so_far(ErodeCall& c) {
    wo_planet* p = c.p; wo_erode_block& B = *p->erode;
    if (c.checkEveryPass || !B.redo.built || read_count(p, B.redo.pendingEver) == 0) return;
    if (p->opt.floodTiming) {          // (diagnostic runs only) which of the two reasons: a splitter-sort bucket that did not fit, or a basin launch with leftovers
        int32_t h[8] = {0};
        WO_HIP(hipMemcpy(h, B.redo.pendingEver, sizeof(h), hipMemcpyDeviceToHost));
        std::fprintf(stderr, "[erode] call runs again with checks: %d basin-solve tasks were left pending\n", h[0]);
    }
    throw RedoWithChecks{};
}
static void erode_flood(ErodeCall& c, double carveStrength) {
    wo_planet* p = c.p; auto& S = p->erode->scratch;
    leftovers_so_far(c);
    c.clk.begin("priority_flood");
    const auto t0 = std::chrono::steady_clock::now();
    // inside the land-first mirror, with the mask and the flood's tables in place: the land heights straight from the mirrored field
    const bool landOnly = c.mir.on && S.identity && !p->floodX.on && !p->opt.floodDevice && p->h_ocean_valid && p->flood.staticValid &&
                          p->flood.staticN == p->N && p->flood.L > 0 && flood_land_is_mirror_prefix(p);
    if (landOnly) flood_stage_land(p, carveStrength, c.floodRun);
    else { c.mir.suspend(); flood_stage(p, carveStrength, c.floodRun); c.mir.resume(); }
    c.floodHostMs += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    c.clk.end();
}
static void erode_sort(ErodeCall& c) { c.clk.begin("sort"); sort_land_by_elevation(c.p); ++c.sorts; c.clk.end(); }
// ice accumulation: the receivers, then one launch in which the last donor to arrive runs its receiver's task (k_ice_climb)
static void ice_flow(ErodeCall& c, const Fields& F) {
    launch(c.p, FAM_ICE_RECV, k_ice_receivers, c.gridN, WO_BLOCK, F);
    launch(c.p, FAM_ICE_ROUND, k_ice_climb, c.gridL, WO_BLOCK, F, F.blocker); ++c.iceRounds;
}
// RELAXED glacial step: the carve from a snapshot of the heights, one sweep
static void glacial_step_relaxed(ErodeCall& c) {
    wo_planet* p = c.p;
    c.clk.begin("glacial");
    const Fields F = fields(p);
    ice_flow(c, F);
    launch(p, FAM_CARVE_ROUND, k_carve_jacobi, c.gridL, WO_BLOCK, F, (const float*)p->d_e, p->d_e2, c.gCarve, c.gConv, c.gStrength);
    swap_elev(p);
    launch(p, FAM_MORAINE, k_moraine_fjord, c.gridN, WO_BLOCK, fields(p), c.gDep, c.gFjord);
    c.clk.end();
}
// the carve's per-task buffers, for at least `active` tasks
static void ensure_carve_capacity(wo_planet* p, int32_t active) {
    wo_erode_block& B = *p->erode; auto& C = B.carve;
    if ((int64_t)active <= C.cap) return;
    const size_t cap = (size_t)active + active / 4 + 1024;
    regrow_group(B, C, (int64_t)cap, [&](DeviceArena& a) {
        C.deps = a.dev<int32_t>(cap * WO_CARVE_DEPS);
        C.depCnt = a.dev<int32_t>(cap); C.depPos = a.dev<int32_t>(cap);
        C.recs = a.dev<CarveRec>(cap); C.slotDone = a.dev<int32_t>(cap); C.expect = a.dev<CarveExpect>(cap);
    });
}
// k_carve_granules' grid, every task in one launch: what is certainly resident at once, the occupancy query's blocks per CU less one
// (the query is known to answer one too many near register-file edges).  Asked once per process.
static int carve_granule_blocks() {
    static int blocks = 0;
    if (!blocks) {
        int perCu = 0, dev = 0; hipDeviceProp_t prop;
        WO_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&perCu, k_carve_granules, WO_BLOCK, 0));
        WO_HIP(hipGetDevice(&dev)); WO_HIP(hipGetDeviceProperties(&prop, dev));
        blocks = std::max(1, std::min(perCu, 8) - 1) * prop.multiProcessorCount;
    }
    return blocks;
}
// The carve of the active tasks (> 0): the one launch (k_carve_granules), then — for whatever it leaves — rounds over the static activation list
// (k_carve_round_static): every launch covers all active tasks, a finished one leaves after one load, an open one issues its loads at once; the
// number of finished tasks is read back after a burst.  Returns the number of carve launches.  (Round 2 also tried all rounds in ONE cooperative
// launch with a grid barrier: slower, profiles/r02f_*; the done-word form of the one launch, k_carve_flow, and the rounds-only route were removed in round 6.)
static int64_t carve_launches(ErodeCall& c, const Fields& F, int32_t active) {
    wo_planet* p = c.p; wo_erode_block& B = *p->erode; auto& S = B.scratch;
    const int32_t* const count = S.counters + 3; int32_t* const done = S.counters + 4;
    // (the dependency lists — a two-hop walk per task — are for the rounds: the granule launch waits on the heights themselves and the lists are only
    // made if it leaves tasks to the rounds)
    launch(p, FAM_CARVE_SETUP, k_carve_records, blocks_for(active), WO_BLOCK, F, (const int32_t*)S.listB, count, B.carve.recs, B.carve.slotDone, c.gCarve, c.gConv, c.gStrength,
           (int32_t)0, (int32_t)1);
    WO_HIP(hipMemsetAsync(done, 0, sizeof(int32_t), p->ctx->stream));
    const int grid = blocks_for(active);
    // hook carve_blocks=<n>: at most n workgroups, so that every thread takes many tasks in turn
    const int blocksNow = p->opt.carveBlocks > 0 ? std::max(1, std::min(carve_granule_blocks(), p->opt.carveBlocks)) : carve_granule_blocks();
    const long long flowBudget = p->opt.carveBudgetMs * 100000ll;   // 100 MHz ticks
    build_group(B, B.granules, [&](DeviceArena& a) { B.granules.g = a.dev<unsigned long long>((size_t)p->N); });
    launch(p, FAM_CARVE_SETUP, k_carve_expect, grid, WO_BLOCK, F, (const CarveRec*)B.carve.recs, count, B.carve.expect);
    launch(p, FAM_CARVE_SETUP, k_carve_pack, blocks_for(p->N, 4096), WO_BLOCK, (const float*)F.e, B.granules.g, p->N);
    launch(p, FAM_CARVE_ROUND, k_carve_granules, std::min(grid, blocksNow), WO_BLOCK, F, (const CarveRec*)B.carve.recs, (const CarveExpect*)B.carve.expect, B.granules.g,
           B.carve.slotDone, count, done, flowBudget);
    launch(p, FAM_CARVE_SETUP, k_carve_unpack, blocks_for(p->N, 4096), WO_BLOCK, (const unsigned long long*)B.granules.g, F.e, p->N);
    int64_t k = 2;          // the number of the next launch
    if (read_count(p, done) >= active) return k - 1;
    // the rounds want the dependency lists after all
    ++c.carveFlowLeft;
    launch(p, FAM_CARVE_SETUP, k_carve_deps, grid, WO_BLOCK, F, (const int32_t*)S.listB, count, S.carveSlot);
    launch(p, FAM_CARVE_SETUP, k_carve_records, grid, WO_BLOCK, F, (const int32_t*)S.listB, count, B.carve.recs, B.carve.slotDone, c.gCarve, c.gConv, c.gStrength, (int32_t)1, (int32_t)0);
    // the depth of the carve DAG falls from one glacial iteration to the next (the ice smooths its bed), so the count of
    // finished tasks is read back every 32 rounds (a read-back costs about as much as three empty rounds)
    constexpr int burst = 32;
    for (;;) {
        for (int b = 0; b < burst; ++b, ++k)
            launch(p, FAM_CARVE_ROUND, k_carve_round_static, grid, WO_BLOCK, F, (const CarveRec*)B.carve.recs, B.carve.slotDone, count, (int32_t)k, c.gCarve, c.gConv, c.gStrength, done);
        if (read_count(p, done) >= active) return k - 1;
        if (k > 4 * (int64_t)p->N + 1024) throw HipError{"carve rounds do not converge"};
    }
}
// Exact glacial step: ice accumulation, the active carve tasks in landCells order, their carve, moraines and fjords
static void glacial_step_exact(ErodeCall& c) {
    wo_planet* p = c.p; wo_erode_block& B = *p->erode; auto& S = B.scratch;
    c.clk.begin("glacial");
    Fields F = fields(p);
    ice_flow(c, F);
    launch(p, FAM_CARVE_SETUP, k_carve_setup_cells, c.gridN, WO_BLOCK, F);
    select_active_by_rank(p, F.arank, S.listB, S.counters + 3);     // the active tasks in landCells order
    const int32_t active = read_count(p, S.counters + 3);
    c.carveActive += active; ensure_carve_capacity(p, active);
    F.carveDeps = B.carve.deps; F.carveDepCnt = B.carve.depCnt; F.carveDepPos = B.carve.depPos;
    if (active > 0) c.carveRounds += carve_launches(c, F, active);
    launch(p, FAM_MORAINE, k_moraine_fjord, c.gridN, WO_BLOCK, F, c.gDep, c.gFjord);
    c.clk.end();
}
// The two-level flow accumulation's buffers (k_flow_tiles)
static FlowTiles flow_tiles_buffers(wo_planet* p) {
    const size_t N = (size_t)p->N;
    wo_erode_block& B = *p->erode; auto& T = B.tiles;
    build_group(B, T, [&](DeviceArena& a) {
        T.parent = a.dev<int32_t>(N); T.extCnt = a.dev<int32_t>(N); T.inflow = a.dev<uint32_t>(N); T.rootAcc = a.dev<unsigned long long>(N); T.lr = a.dev<int32_t>(N);
        WO_HIP(hipMemsetAsync(T.inflow, 0, N * 4, p->ctx->stream)); WO_HIP(hipMemsetAsync(T.extCnt, 0, N * 4, p->ctx->stream));
    });
    FlowTiles FT{};
    FT.lr = T.lr; FT.parent = T.parent; FT.rootAcc = T.rootAcc; FT.inflow = T.inflow; FT.extCnt = T.extCnt;
    return FT;
}
static int flow_tile_count(int32_t L) { return (int)(((int64_t)L + FT_CELLS - 1) / FT_CELLS); }
// The receivers pass (+ the flow's start state and donor counts, + the start state of the basin layout's search), then the layout's fork
static void erode_receivers(ErodeCall& c, const Fields& F, const FlowTiles& FT, int32_t* donorCnt, bool basin, bool slotIdentity, bool tilesBeforeFork) {
    wo_planet* p = c.p; hipStream_t s = p->ctx->stream; wo_erode_block& B = *p->erode;
    Fields Fr = F; if (basin) Fr.basinJ = B.basin.J;          // (the layout's start state)
    c.clk.begin("receivers");
    launch(p, FAM_RECEIVERS, k_receivers_flow_init, c.gridL, WO_BLOCK, Fr, donorCnt);
    c.clk.end();
    if (!basin) return;
    // basin-local solve (basin.hip): this pass's store order groups every drainage component with everything it depends on.
    // The layout needs the receivers only and touches none of the flow accumulation's arrays: it runs on the planet's side stream
    // beside the flow accumulation and the solve's setup waits for both.  (A third stream for the solve's event lists was measured in
    // round 3 and a side stream for the elevation sort in round 6 — profiles/r03bc_*, r06d_*: no faster, a launch of these sizes already
    // occupies the chip's workgroup slots and two side by side take turns; both removed.)
    ensure_side_stream(p);
    if (tilesBeforeFork) {
        // (the root links too before the fork: beside the layout's first kernel — high-priority stream — they took 33 us instead of 15; flow stage 45.9 -> 43.8 ms per step, profiles/r05h_*)
        launch(p, FAM_FLOW_TILES, k_flow_tiles<false>, flow_tile_count(B.L), FT_THREADS, F, FT);
        launch(p, FAM_FLOW_TILES, k_flow_root_links, blocks_for(B.L, 4096), WO_BLOCK, F, FT);
    }
    WO_HIP(hipEventRecord(B.side.fork, s));
    WO_HIP(hipStreamWaitEvent(B.side.stream, B.side.fork, 0));
    B.side.on = true;
    try { basin_layout(p, slotIdentity); } catch (...) { B.side.on = false; throw; }
    B.side.on = false;
    WO_HIP(hipEventRecord(B.side.join, B.side.stream));
}
// Flow accumulation = subtree sizes of the forward forest (integers: any order of the additions is exact): in two levels under the mirror
// (kernels_impl.h: k_flow_tiles), else one launch in which every leaf hands its total to its receiver and the thread that completes a
// receiver carries on with it (k_flow_climb).  Every cell with a forward receiver is retired either way; k_flow_final reads the packed totals.
// (10 M cells, flow stage per step: round 2's rake rounds + pointer doubling 108 ms, the climb 45, two levels 29: profiles/r02r_*, r05g_*.)
static void erode_flow(ErodeCall& c, const Fields& F, const FlowTiles& FT, int32_t* donorCnt, bool flowTiles, bool tilesBeforeFork, bool clearOut) {
    wo_planet* p = c.p; wo_erode_block& B = *p->erode; auto& S = B.scratch;
    c.clk.begin("flow");
    if (flowTiles) {
        const int tiles = flow_tile_count(B.L);
        if (!tilesBeforeFork) {
            launch(p, FAM_FLOW_TILES, k_flow_tiles<false>, tiles, FT_THREADS, F, FT);
            launch(p, FAM_FLOW_TILES, k_flow_root_links, blocks_for(B.L, 4096), WO_BLOCK, F, FT);
        }
        launch(p, FAM_FLOW_TILES, k_flow_root_climb, blocks_for(B.L, 4096), WO_BLOCK, F, FT);
        launch(p, FAM_FLOW_TILES, k_flow_tiles<true>, tiles, FT_THREADS, F, FT);
    } else
        launch(p, FAM_FLOW_SNAP, k_flow_climb, c.gridL, WO_BLOCK, F, (const int32_t*)S.flowCnt, (int32_t)0x7fffffff);
    Fields Ff = F;
    if (p->opt.relaxedFull) Ff.ev = nullptr;                // (no event lists: the relaxed solve has no order)
    // the solve's outputs are cleared (tags 0) only for a pass whose result is checked on the spot (k_solve_patch / k_solve_final read
    // the tags as launch numbers); the unchecked pass stamps them with a tag of its own instead (erode_solve_basin): 16 B per land cell less to write
    launch(p, FAM_FLOW_FINAL, k_flow_final, c.gridL, WO_BLOCK, Ff, donorCnt, clearOut ? S.out : (SolveOut*)nullptr);
    c.clk.end();
}
// Exact mode: the basin-local solve, once the layout on the side stream has joined
static void erode_solve_basin(ErodeCall& c, Fields F, int32_t iter) {
    wo_planet* p = c.p; hipStream_t s = p->ctx->stream; wo_erode_block& B = *p->erode; auto& S = B.scratch;
    WO_HIP(hipStreamWaitEvent(s, B.side.join, 0));
    F.slotOf = B.basin.slot; F.solveLean = 1;
    // (the outputs' tags were cleared by k_flow_final: one coalesced sweep instead of one scattered 16-byte write per task)
    // an unchecked pass: the solve launch writes the final heights itself (SolveTask finality flags) and no k_solve_final then
    const bool unchecked = !c.checkEveryPass; F.solveFinals = unchecked ? 1 : 0;
    // (the setup launch also clears the counters and pending totals of the solve launches: run_solve_patches)
    launch(p, FAM_SOLVE_SETUP, k_solve_setup_batched<true>, c.gridL, WO_BLOCK, F, S.patchPending, (int32_t)S.numPatches, S.patchTotals, (int32_t)WO_PATCH_TOTAL_SLOTS);
    // the unchecked pass's one launch tags what it produces with a number no earlier pass of this planet used
    int32_t passTag = 1;
    if (unchecked) {
        if (S.solvePassSerial >= 0x3ff00000) { WO_HIP(hipMemsetAsync(S.out, 0, (size_t)p->N * sizeof(SolveOut), s)); S.solvePassSerial = 0; }
        passTag = (1 << 20) + (int32_t)(++S.solvePassSerial);
    }
    const int64_t r = run_solve_patches(p, F, c.K, c.m, c.dt, unchecked, passTag);
    ++c.basinPasses; if (r > 1) ++c.basinLeftoverPasses;
    c.patchLaunches += r; c.maxSolve = std::max(c.maxSolve, r);
    if (!unchecked) launch(p, FAM_SOLVE_FINAL, k_solve_final, c.gridL, WO_BLOCK, F, p->d_e2, (iter < c.tIters) ? S.me : (float*)nullptr);
}
// RELAXED: h' = a + b h'(receiver) composed by pointer jumping (12 doublings cover chains of 4 096 cells), then heights + deposits in one sweep
static void erode_solve_affine(ErodeCall& c, const Fields& F) {
    wo_planet* p = c.p; wo_erode_block& B = *p->erode;
    build_group(B, B.affine, [&](DeviceArena& a) { B.affine.buf[1] = a.dev<Affine>((size_t)p->N); B.affine.buf[0] = a.dev<Affine>((size_t)p->N); });
    launch(p, FAM_SOLVE_SETUP, k_affine_init, c.gridL, WO_BLOCK, F, B.affine.buf[0]);
    int cur = 0;
    for (int q = 0; q < 12; ++q, cur ^= 1) launch(p, FAM_SOLVE_ROUND, k_affine_jump, c.gridL, WO_BLOCK, F, (const Affine*)B.affine.buf[cur], B.affine.buf[cur ^ 1]);
    launch(p, FAM_SOLVE_FINAL, k_affine_apply, c.gridL, WO_BLOCK, F, (const Affine*)B.affine.buf[cur], p->d_e2);
}
// The hydraulic step: receivers, flow accumulation, the implicit solve (exact: basin-local, basin.hip; relaxed: the affine recurrence)
static void hydraulic_step(ErodeCall& c, int32_t iter) {
    wo_planet* p = c.p; wo_erode_block& B = *p->erode; auto& S = B.scratch;
    Fields F = fields(p);
    F.solveK = c.K; F.solveM = c.m; F.solveDt = c.dt;
    const bool basin = !p->opt.relaxedFull;
    const bool slotIdentity = c.mir.on && p->mirror.h_mask.size() == (size_t)p->N;          // land-first mirror: a land cell's Morton slot is its id
    if (basin) { basin_alloc(p); F.basinMslot = slotIdentity ? nullptr : S.slotOf; }
    // two-level accumulation (k_flow_tiles): needs the land cells to be the ids 0 .. L-1 in Morton order (land-first mirror); on the planet's
    // own cell order (WO_LAYOUT=index) the one-launch climb over all cells (k_flow_climb)
    const bool flowTiles = S.identity;
    FlowTiles FT = flowTiles ? flow_tiles_buffers(p) : FlowTiles{};
    // the two-level accumulation's first kernel also shortens the layout's start state inside every tile (k_flow_tiles<false>: J[c] <- an
    // ancestor at most a tile away), so it runs before the fork and the layout's component search starts from chains of tiles instead of cells
    const bool tilesBeforeFork = basin && flowTiles && slotIdentity;
    if (tilesBeforeFork) FT.basinJ = B.basin.J;
    int32_t* const donorCnt = flowTiles ? (int32_t*)nullptr : S.flowCnt;
    erode_receivers(c, F, FT, donorCnt, basin, slotIdentity, tilesBeforeFork);
    erode_flow(c, F, FT, donorCnt, flowTiles, tilesBeforeFork, basin && c.checkEveryPass);
    c.clk.begin("solve");
    if (basin) erode_solve_basin(c, F, iter); else erode_solve_affine(c, F);
    swap_elev(p);
    c.clk.end();
}
static void thermal_step(ErodeCall& c, bool afterSolve) {
    wo_planet* p = c.p;
    c.clk.begin("thermal");
    const Fields F = fields(p);
    if (!afterSolve) launch(p, FAM_THERMAL_EXCESS, k_masked_elev, c.gridL, WO_BLOCK, F);      // else written by the solve
    launch(p, FAM_THERMAL_EXCESS, k_thermal_excess, c.gridL, WO_BLOCK, F, c.talus);
    if (p->maxDeg <= 12) launch(p, FAM_THERMAL_APPLY, k_thermal_apply_reg<12>, c.gridL, WO_BLOCK, F, p->d_e2, c.talus, c.kThermal);
    else if (p->maxDeg <= 16) launch(p, FAM_THERMAL_APPLY, k_thermal_apply_reg<16>, c.gridL, WO_BLOCK, F, p->d_e2, c.talus, c.kThermal);
    else launch_shmem(p, FAM_THERMAL_APPLY, k_thermal_apply, c.gridL, WO_BLOCK, (size_t)p->maxDeg * WO_BLOCK * 12, F, p->d_e2, c.talus, c.kThermal, (int32_t)p->maxDeg);
    swap_elev(p);
    c.clk.end();
}

static void erode_composite(wo_planet* p, int32_t hIters, double K, double m, double dt, int32_t tIters, double talus,
                            double kThermal, int32_t gIters, double gStrength, bool checkEveryPass = true) {
    ErodeCall c(p, hIters, K, m, dt, tIters, talus, kThermal, gIters, gStrength, checkEveryPass);
    release_stage_brackets(p);
    p->stageTiming.clear(); p->erodeStats.clear();
    p->floodX.calls = 0; p->floodX.gathers = 0; p->floodX.globalFloods = 0; p->floodX.received = 0;       // per call (the stats of a step, not of the planet's life)
    if (c.total <= 0) return;
    ensure_scratch(p);
    wo_erode_block& B = *p->erode; auto& S = B.scratch;
    hipStream_t s = p->ctx->stream;
    if (hIters > 0) WO_HIP(hipMemsetAsync(S.flowCnt, 0, (size_t)p->N * sizeof(int32_t), s));   // k_flow_final keeps it zero between iterations; a call that was cut short may not have
    if (hIters > 0 && B.tiles.built) { WO_HIP(hipMemsetAsync(B.tiles.inflow, 0, (size_t)p->N * 4, s)); WO_HIP(hipMemsetAsync(B.tiles.extCnt, 0, (size_t)p->N * 4, s)); }   // (k_flow_tiles<true> keeps them zero)
    if (!erode_setup(c)) return;
    if (hIters > 0) erode_flood(c, 0.5);

    const bool glacial = c.gIters > 0 && c.gStrength > 0;
    if (glacial) launch(p, FAM_GLAC_INDEX, k_glac_index, c.gridN, WO_BLOCK, fields(p), c.gStrength);
    // (round 2's river-aligned patch lists, WO_RIVER_PATCHES, were measured and dropped: profiles/r02c_river_patch_experiment.txt)
    // (one composite iteration as a hipGraph — captured once per call, replayed 167 times — was built and measured in round 4: 499.5 ms per step against 384.1 with
    // plain launches, profiles/r04j_*: a graph launch costs more than the ~25 stream launches it replaces; removed in round 6)
    const bool relaxedFull = p->opt.relaxedFull;           // RELAXED MODE, not parity (kernels_impl.h): one sort per flood, affine solve, Jacobi carve
    bool midDone = false, sortAfterFlood = false;
    for (int32_t iter = 0; iter < c.total; ++iter) {
        c.clk.on = true;
        if (!midDone && iter >= c.midIter) { midDone = true; erode_flood(c, 0.85); sortAfterFlood = true; }
        c.clk.on = p->opt.stageTimingAll || p->profiling || c.total <= 16 || iter % 8 == 0;
        const bool gNow = iter < c.gIters && glacial, hNow = iter < hIters;
        // WO_RELAXED_SORT_EVERY=K (relaxed mode, NOT the reference's semantics: SURVEY 7.3): landCells is re-sorted only every K-th
        // iteration; in between the passes run with a stale visiting order (still a consistent order: every pass compares ranks
        // pairwise, so the dataflow is well defined, it is just not the reference's).  Measured, never reported as parity.
        const bool sortNow = relaxedFull ? (iter == 0 || sortAfterFlood) : (p->opt.relaxedSortEvery <= 1 || iter % p->opt.relaxedSortEvery == 0);
        if ((gNow || hNow) && sortNow) { sortAfterFlood = false; erode_sort(c); }
        if (gNow) { if (relaxedFull) glacial_step_relaxed(c); else glacial_step_exact(c); }
        if (hNow) {
            if (gNow && sortNow) erode_sort(c);
            hydraulic_step(c, iter);
        }
        if (iter < tIters) thermal_step(c, hNow);
    }
    c.clk.on = true;
    leftovers_so_far(c);
    if (glacial) {
        c.clk.begin("glacial_blend");
        launch(p, FAM_GLAC_BLEND, k_glacial_blend, c.gridN, WO_BLOCK, fields(p), (const float*)p->d_e, p->d_e2);
        swap_elev(p);
        c.clk.end();
    }
    const bool mirrored = c.mir.on;
    if (mirrored) { c.clk.begin("setup"); c.mir.finish(); c.clk.end(); }
    c.clk.finish();
    c.stats(mirrored);
}

// The host used to look at the basin solve's pending count after every pass (a read-back and ~30 us of idle GPU per iteration, and
// the host never got ahead of the device).  No real layout has ever left a task pending, so the look is deferred: the launches add
// into one word per call, the word is read where the host synchronises anyway (before the second flood, at the end), and if it is
// not zero the field is restored from a copy taken at entry and the call runs again with the check after every pass — the form
// that finishes pending tasks with k_solve_patch launches.
static void erode_composite_checked(wo_planet* p, int32_t hIters, double K, double m, double dt, int32_t tIters, double talus,
                                    double kThermal, int32_t gIters, double gStrength) {
    // (no hydraulic passes: nothing to check.)  With a flood exchange set (shares of one planet) every flood call of this rank is a pair of
    // collectives with its peers: a rank that ran the call a second time would repeat them alone (its peers are past them and no longer hold
    // that call's heights).  Such a call is therefore checked pass by pass from the start — pending tasks are finished where they arise and
    // nothing is ever run again.
    if (!p->erode) p->erode = new wo_erode_block();          // made by the planet's first call
    if (hIters <= 0 || p->floodX.on) { erode_composite(p, hIters, K, m, dt, tIters, talus, kThermal, gIters, gStrength, true); return; }
    hipStream_t s = p->ctx->stream;
    wo_erode_block& B = *p->erode;
    build_group(B, B.redo, [&](DeviceArena& a) { B.redo.e = a.dev<float>((size_t)p->N); B.redo.pendingEver = a.dev<int32_t>(16); });
    WO_HIP(hipMemcpyAsync(B.redo.e, p->d_e, (size_t)p->N * sizeof(float), hipMemcpyDeviceToDevice, s));
    WO_HIP(hipMemsetAsync(B.redo.pendingEver, 0, 16 * sizeof(int32_t), s));
    try {
        erode_composite(p, hIters, K, m, dt, tIters, talus, kThermal, gIters, gStrength, false);
    } catch (const RedoWithChecks&) {
        WO_HIP(hipStreamSynchronize(s));
        if (B.side.built) WO_HIP(hipStreamSynchronize(B.side.stream));
        WO_HIP(hipMemcpyAsync(p->d_e, B.redo.e, (size_t)p->N * sizeof(float), hipMemcpyDeviceToDevice, s));
        ++B.redo.calls;
        erode_composite(p, hIters, K, m, dt, tIters, talus, kThermal, gIters, gStrength, true);
    }
}

void erode_free(wo_planet* p) {
    if (p->erode) side_destroy(p->erode->side);
    delete p->erode; p->erode = nullptr;
}

}  // namespace wo

using namespace wo;

extern "C" {

int wo_erode_composite_resident(wo_planet* p, int32_t hIters, double K, double m, double dt, int32_t tIters, double talusSlope,
                                double kThermal, int32_t gIters, double glacialStrength) {
    if (!check_planet(p, "wo_erode_composite_resident")) return 1;
    WO_TRY
    erode_composite_checked(p, hIters, K, m, dt, tIters, talusSlope, kThermal, gIters, glacialStrength);
    return 0;
    WO_CATCH("wo_erode_composite_resident")
}

struct ErodeArgs { int32_t h; double K, m, dt; int32_t t; double talus, kT; int32_t g; double gs; };
int wo_erode_composite(wo_planet* p, float* e, const uint8_t* oc, int32_t hIters, double K, double m, double dt, int32_t tIters,
                       double talusSlope, double kThermal, int32_t gIters, double glacialStrength) {
    ErodeArgs a{hIters, K, m, dt, tIters, talusSlope, kThermal, gIters, glacialStrength};
    return with_host_field(p, "wo_erode_composite", e, oc, true,
                           [](wo_planet* q, void* v) { auto* x = (ErodeArgs*)v; erode_composite_checked(q, x->h, x->K, x->m, x->dt, x->t, x->talus, x->kT, x->g, x->gs); }, &a);
}

}  // extern "C"
