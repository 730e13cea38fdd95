// ---------------------------------------------------------------------------------------------------
// assignElevation (js/elevation.js:216-1391): collisions on the device, order-defined graph work on the
// host (elevation_host.cc), the fused per-cell uplift pass on the device.
// ---------------------------------------------------------------------------------------------------
#include <hip/hip_runtime.h>

#include <chrono>
#include <cmath>
#include <cstring>

#include "../../include/worogen.h"
#include "common_kernels.h"
#include "device.h"
#include "elevation_bfs.h"
#include "elevation_host.h"
#include "elevation_kernels.h"
#include "noise.h"
#include "plates_ops.h"

namespace wo {

__global__ void k_set_counters(int32_t* c, int32_t v0, int32_t v1, int32_t v2, int32_t v3) {
    if (threadIdx.x == 0 && blockIdx.x == 0) { c[0] = v0; c[1] = v1; c[2] = v2; c[3] = v3; }
}

// ---------------------------------------------------------------- plate projection --------------
// js/coarse-plates.js:51-117: one thread per hi-res cell (12 noise3D from LDS tables, then a greedy ascent over the
// 20 k-cell coarse mesh, which stays in L2); the start cells come from a small (z, longitude) bucket grid.
__global__ __launch_bounds__(WO_BLOCK) void k_plate_grid(CoarsePlates C, int32_t* grid) {
    WO_GRID_STRIDE(b, C.gridZ * C.gridLon) grid[b] = plate_grid_cell(C, b);
}
__global__ __launch_bounds__(WO_BLOCK) void k_plate_project(CoarsePlates C, const uint8_t* tables, const float* r_xyz, int32_t N, double perturbAmp,
                                                             int32_t* r_plate) {
    __shared__ uint8_t sP[512], sM[512];
    load_tables(tables, sP, sM);
    WO_GRID_STRIDE(r, N) r_plate[r] = plate_project_cell(C, sP, sM, r_xyz, r, perturbAmp);
}

}  // namespace wo

using namespace wo;

namespace wo {

// a plate table on the device, its arrays in `a`
static PlateTable upload_table(DeviceArena& a, const wo_plate_table& h, hipStream_t s) {
    const size_t n = (size_t)h.numIds;
    PlateTable t{};
    t.numIds = h.numIds; t.hasVec = up(a, h.hasVec, n, s); t.pole = up(a, h.pole, 3 * n, s); t.omega = up(a, h.omega, n, s);
    t.isOcean = up(a, h.isOcean, n, s); t.density = up(a, h.density, n, s);
    return t;
}

struct DevCollision {
    CollisionOut o{};
    void alloc(DeviceArena& a, size_t N) {
        o.stress = a.dev<float>(N); o.subduct = a.dev<float>(N); o.btype = a.dev<int8_t>(N);
        o.bothOcean = a.dev<uint8_t>(N); o.hasOcean = a.dev<uint8_t>(N); o.setCode = a.dev<uint8_t>(N);
    }
    void download(CollisionHost& h, size_t N, hipStream_t s) {
        h.resize((int32_t)N);
        WO_HIP(hipMemcpyAsync(h.stress.data(), o.stress, N * 4, hipMemcpyDeviceToHost, s)); WO_HIP(hipMemcpyAsync(h.subduct.data(), o.subduct, N * 4, hipMemcpyDeviceToHost, s));
        WO_HIP(hipMemcpyAsync(h.btype.data(), o.btype, N, hipMemcpyDeviceToHost, s)); WO_HIP(hipMemcpyAsync(h.bothOcean.data(), o.bothOcean, N, hipMemcpyDeviceToHost, s));
        WO_HIP(hipMemcpyAsync(h.hasOcean.data(), o.hasOcean, N, hipMemcpyDeviceToHost, s)); WO_HIP(hipMemcpyAsync(h.setCode.data(), o.setCode, N, hipMemcpyDeviceToHost, s));
    }
};

static PlateTable host_table(const wo_plate_table& h) { PlateTable t; t.numIds = h.numIds; t.hasVec = h.hasVec; t.pole = h.pole; t.omega = h.omega; t.isOcean = h.isOcean; t.density = h.density; return t; }

template <class T, class A> static T* upload_vec(DeviceArena& a, const std::vector<T, A>& v, hipStream_t s) {
    T* d = a.dev<T>(v.size());
    WO_HIP(hipMemcpyAsync(d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, s));
    return d;
}

static void assign_elevation(wo_planet* p, const int32_t* r_plate, const wo_plate_table* plates, const int32_t* plateSeeds, int32_t numPlateSeeds,
                             const int32_t* r_superPlate, const wo_plate_table* superPlates, const uint8_t* perm, const uint8_t* pm12,
                             double noiseMag, double seed, double spread, float* r_elevation, float* r_stress, float* debugLayers,
                             int32_t* mountain_r, int32_t* coastline_r, int32_t* ocean_r, int32_t* setCounts) {
    hipStream_t s = p->ctx->stream;
    const int32_t N = p->N;
    const int gridN = blocks_for(N);
    const bool hasSuper = r_superPlate != nullptr && superPlates != nullptr;
    for (int32_t r = 0; r < N; ++r) if (r_plate[r] < 0 || r_plate[r] >= plates->numIds) throw HipError{"r_plate entry outside the plate table"};
    if (hasSuper) for (int32_t r = 0; r < N; ++r) if (r_superPlate[r] < 0 || r_superPlate[r] >= superPlates->numIds) throw HipError{"r_superPlate entry outside the super-plate table"};
    std::vector<std::pair<std::string, double>> timing;
    auto t0 = std::chrono::steady_clock::now();
    auto lap = [&](const char* stage) { WO_HIP(hipStreamSynchronize(s)); auto now = std::chrono::steady_clock::now(); timing.push_back({stage, std::chrono::duration<double, std::milli>(now - t0).count()}); t0 = now; };

    // noise instances: the caller's `noise` plus the nine the reference seeds itself (js/elevation.js:539,636,980-982,1056,1127-1129)
    std::vector<uint8_t> tabs(EL_TAB_COUNT * 1024), hs3(1024);
    std::memcpy(tabs.data(), perm, 512); std::memcpy(tabs.data() + 512, pm12, 512);
    const double offs[EL_TAB_COUNT] = {0, 419, 557, 77, 133, 211, 307, 501, 502};
    for (int k = 1; k < EL_TAB_COUNT; ++k) noise_tables(seed + offs[k], tabs.data() + k * 1024, tabs.data() + k * 1024 + 512);
    noise_tables(seed + 503, hs3.data(), hs3.data() + 512);
    DeviceArena mem;                        // every device buffer of the call: freed when the call ends, however it ends
    uint8_t* d_tabs = upload_vec(mem, tabs, s);
    int32_t* d_plate = up(mem, r_plate, (size_t)N, s);
    const PlateTable dT = upload_table(mem, *plates, s);
    DevCollision cS, cP; cS.alloc(mem, N);
    CollisionHost hS, hP;
    launch(p, FAM_ELEV_COLLISION, k_collision, gridN, WO_BLOCK, N, (const int32_t*)p->d_off, (const int32_t*)p->d_adj, (const float*)p->d_xyz,
           (const int32_t*)d_plate, dT, (const uint8_t*)d_tabs, cS.o);
    cS.download(hS, N, s);
    if (hasSuper) {
        int32_t* d_super = up(mem, r_superPlate, (size_t)N, s);
        const PlateTable dTS = upload_table(mem, *superPlates, s); cP.alloc(mem, N);
        launch(p, FAM_ELEV_COLLISION, k_collision, gridN, WO_BLOCK, N, (const int32_t*)p->d_off, (const int32_t*)p->d_adj, (const float*)p->d_xyz,
               (const int32_t*)d_super, dTS, (const uint8_t*)d_tabs, cP.o);
        cP.download(hP, N, s);
    }
    lap(hasSuper ? "Collisions (dual)" : "Collisions");

    // host stage
    if (p->h_xyz.empty()) throw HipError{"planet has no host copy of r_xyz"};
    ElevMesh M{N, p->h_off.data(), p->h_adj.data(), p->h_xyz.data()};
    ElevInputs I{};
    I.plate = r_plate; I.plates = host_table(*plates); I.plateSeeds = plateSeeds; I.numPlateSeeds = numPlateSeeds;
    I.superPlate = hasSuper ? r_superPlate : nullptr; if (hasSuper) I.superPlates = host_table(*superPlates);
    I.seed = seed; I.spread = spread; I.noiseMag = noiseMag; I.hsNoise3 = NoiseTab{hs3.data(), hs3.data() + 512};
    ElevHostState H; ElevParams Q{}; std::vector<Dome> domes;
    // The FIFO BFS fields (js/elevation.js:464-631, 1059-1086) run on the device (elevation_bfs.h), started from inside the
    // host stage as soon as their inputs exist and overlapped with the serial RNG-ordered distance fields on the host.
    ElevFields F{};
    F.xyz = p->d_xyz; F.plate = d_plate;
    auto up = [&](auto& v) { return upload_vec(mem, v, s); };
    auto dev = [&](auto* proto, size_t n) { return mem.dev<std::remove_pointer_t<decltype(proto)>>(n); };
    float *b_dBdry = nullptr, *b_csm = nullptr, *b_cssm = nullptr, *b_rift = nullptr, *b_ridge = nullptr, *b_frac = nullptr, *b_ba = nullptr, *b_bas = nullptr, *b_arc = nullptr, *b_arcs = nullptr;
    uint8_t* b_conv = nullptr;
    std::vector<std::vector<int32_t>> bfsSeeds;             // host seed lists stay alive until the stream has consumed them
    bfsSeeds.reserve(8);
    auto bfs_on_device = [&](const ElevParams& Qs, int32_t maxCD, double maxStress) {
        const size_t n = (size_t)N;
        F.isOcean = up(H.isOcean); F.stress = up(H.stress); F.subduct = up(H.subduct); F.btype = up(H.btype);
        const uint8_t* d_both = up(H.bothOcean); const uint8_t* d_has = up(H.hasOcean); (void)d_both; (void)d_has;
        b_dBdry = dev((float*)nullptr, n); b_csm = dev((float*)nullptr, n); b_cssm = dev((float*)nullptr, n); b_conv = dev((uint8_t*)nullptr, n);
        b_rift = dev((float*)nullptr, n); b_ridge = dev((float*)nullptr, n); b_frac = dev((float*)nullptr, n);
        b_ba = dev((float*)nullptr, n); b_bas = dev((float*)nullptr, n); b_arc = dev((float*)nullptr, n); b_arcs = dev((float*)nullptr, n);
        int32_t* listA = dev((int32_t*)nullptr, n); int32_t* listB = dev((int32_t*)nullptr, n);
        int32_t* cnt = dev((int32_t*)nullptr, n); int32_t* base = dev((int32_t*)nullptr, n); int32_t* pushPos = dev((int32_t*)nullptr, n);
        unsigned long long* attrKey = dev((unsigned long long*)nullptr, n);
        int32_t* counters = dev((int32_t*)nullptr, 4);
        BfsCtx B{N, p->d_off, p->d_adj, F.isOcean, d_plate};
        // seed lists in ascending id (the reference's scan order), built on the host from the arrays the host stage holds
        auto seeds_of = [&](auto pred) {
            std::vector<std::vector<int32_t>> part(host_threads() + 1);
            parallel_ranges(N, [&](int64_t b, int64_t e, int t) { for (int64_t r = b; r < e; ++r) if (pred((int32_t)r)) part[t].push_back((int32_t)r); });
            std::vector<int32_t> q; for (auto& v : part) q.insert(q.end(), v.begin(), v.end());
            return q;
        };
        const int grid = 512;
        auto run_field = [&](int32_t mode, std::vector<int32_t>&& seedList, float* dist, float init, float* a0, float* a1, uint8_t* a2, int32_t maxDist) {
            bfsSeeds.push_back(std::move(seedList));
            const std::vector<int32_t>& seeds = bfsSeeds.back();
            const bool carry = a0 != nullptr;
            launch(p, FAM_ELEV_COLLISION, k_bfs_init, blocks_for(N, 4096), WO_BLOCK, dist, init, a0, a1, a2, carry ? pushPos : (int32_t*)nullptr,
                   mode == BFS_COAST ? attrKey : (unsigned long long*)nullptr, N);
            const int32_t ns = (int32_t)seeds.size();
            if (ns == 0) return;
            WO_HIP(hipMemcpyAsync(listA, seeds.data(), (size_t)ns * 4, hipMemcpyHostToDevice, s));       // no host wait: the device keeps running the previous field
            hipLaunchKernelGGL(k_set_counters, dim3(1), dim3(1), 0, s, counters, ns, 0, 0, 0);
            launch(p, FAM_ELEV_COLLISION, k_bfs_seed, blocks_for(ns, 1024), WO_BLOCK, mode, (const int32_t*)listA, ns, dist, a0, a1, a2,
                   (const float*)F.stress, (const float*)F.subduct, (const int8_t*)F.btype, maxStress);
            int32_t* cur = listA; int32_t* nxt = listB;
            for (int32_t level = 1; level <= maxDist; ++level) {
                int32_t* cc = counters + ((level - 1) % 3); int32_t* nc = counters + (level % 3); int32_t* zc = counters + ((level + 1) % 3);
                if (!carry) {
                    launch(p, FAM_ELEV_COLLISION, k_bfs_plain, grid, WO_BLOCK, B, mode, dist, (const int32_t*)cur, (const int32_t*)cc, nxt, nc, zc, level);
                } else {
                    launch(p, FAM_ELEV_COLLISION, k_bfs_push, grid, WO_BLOCK, B, mode, (const float*)dist, (const int32_t*)cur, (const int32_t*)cc, pushPos,
                           mode == BFS_COAST ? attrKey : (unsigned long long*)nullptr, (const float*)a0, level);
                    launch(p, FAM_ELEV_COLLISION, k_bfs_count, grid, WO_BLOCK, B, (const float*)dist, (const int32_t*)cur, (const int32_t*)cc, (const int32_t*)pushPos, cnt, level);
                    launch(p, FAM_ELEV_COLLISION, k_bfs_scan, 1, 1024, (const int32_t*)cnt, (const int32_t*)cc, base, nc);
                    launch(p, FAM_ELEV_COLLISION, k_bfs_assign, grid, WO_BLOCK, B, mode, dist, (const int32_t*)cur, (const int32_t*)cc, (const int32_t*)pushPos,
                           (const unsigned long long*)(mode == BFS_COAST ? attrKey : nullptr), (const int32_t*)base, nxt, a0, a1, a2, level);
                }
                std::swap(cur, nxt);
            }
        };
        const uint8_t* oc = H.isOcean.data(); const int8_t* bt = H.btype.data(); const uint8_t* both = H.bothOcean.data(); const uint8_t* has = H.hasOcean.data();
        const float* sub = H.subduct.data();
        run_field(BFS_COAST, seeds_of([&](int32_t r) { const uint8_t o = oc[r]; for (int32_t ni = M.off[r]; ni < M.off[r + 1]; ++ni) if (oc[M.adj[ni]] != o) return true; return false; }),
                  b_dBdry, (float)(maxCD + 1), b_csm, b_cssm, b_conv, maxCD);
        run_field(BFS_RIFT, seeds_of([&](int32_t r) { return bt[r] == 2 && !has[r]; }), b_rift, INFINITY, nullptr, nullptr, nullptr, Qs.riftHalfWidth);
        run_field(BFS_RIDGE, seeds_of([&](int32_t r) { return bt[r] == 2 && both[r]; }), b_ridge, INFINITY, nullptr, nullptr, nullptr, Qs.ridgeHalfWidth);
        run_field(BFS_FRACTURE, seeds_of([&](int32_t r) { return bt[r] == 3 && both[r]; }), b_frac, INFINITY, nullptr, nullptr, nullptr, Qs.fractureHalfWidth);
        run_field(BFS_BACKARC, seeds_of([&](int32_t r) { return bt[r] == 1 && has[r] && (double)sub[r] < 0.50; }), b_ba, INFINITY, b_bas, nullptr, nullptr, Qs.baEnd);
        run_field(BFS_ARC, seeds_of([&](int32_t r) { return bt[r] == 1 && both[r] && (double)sub[r] < 0.45; }), b_arc, (float)(Qs.maxArcDist + 1), b_arcs, nullptr, nullptr, Qs.maxArcDist);
    };
    elevation_host_stage(M, I, hS, hasSuper ? &hP : nullptr, H, Q, domes, bfs_on_device);
    lap("Stress, sets, distance fields (host) || BFS fields (device)");

    // per-cell pass
    F.dBdry = b_dBdry; F.coastStressMax = b_csm; F.coastSubductMax = b_cssm; F.coastConvergent = b_conv; F.riftDist = b_rift; F.ridgeDist = b_ridge;
    F.fractureDist = b_frac; F.backArcDist = b_ba; F.backArcStress = b_bas; F.arcDist = b_arc; F.arcStress = b_arcs;
    F.distMountain = up(H.distMountain); F.distOcean = up(H.distOcean); F.distCoastline = up(H.distCoastline); F.distCoast = up(H.distCoast);
    F.distCoastLand = up(H.distCoastLand);
    F.elev = p->d_e;
    float* d_dl = nullptr;
    if (debugLayers) { d_dl = mem.dev<float>((size_t)DL_COUNT * N); WO_HIP(hipMemsetAsync(d_dl, 0, (size_t)DL_COUNT * N * 4, s)); }
    F.dl = d_dl;
    if (domes.empty()) domes.push_back(Dome{});
    Dome* d_domes = upload_vec(mem, domes, s);
    launch(p, FAM_ELEV_MAIN, k_elevation, gridN, WO_BLOCK, F, Q, dT, (const uint8_t*)d_tabs, (const Dome*)d_domes);
    if (r_elevation) WO_HIP(hipMemcpyAsync(r_elevation, p->d_e, (size_t)N * 4, hipMemcpyDeviceToHost, s));
    if (debugLayers) WO_HIP(hipMemcpyAsync(debugLayers, d_dl, (size_t)DL_COUNT * N * 4, hipMemcpyDeviceToHost, s));
    lap("Elevation loop + coastal + arcs + hotspots + compression (device)");
    if (r_stress) std::memcpy(r_stress, H.stress.data(), (size_t)N * 4);
    if (mountain_r) std::memcpy(mountain_r, H.mountain.data(), H.mountain.size() * 4);
    if (coastline_r) std::memcpy(coastline_r, H.coastline.data(), H.coastline.size() * 4);
    if (ocean_r) std::memcpy(ocean_r, H.ocean.data(), H.ocean.size() * 4);
    if (setCounts) { setCounts[0] = (int32_t)H.mountain.size(); setCounts[1] = (int32_t)H.coastline.size(); setCounts[2] = (int32_t)H.ocean.size(); }
    release_stage_brackets(p);
    p->stageTiming = timing;
}

}  // namespace wo

extern "C" int wo_assign_elevation(wo_planet* p, const int32_t* r_plate, const wo_plate_table* plates, const int32_t* plateSeeds,
                                   int32_t numPlateSeeds, const int32_t* r_superPlate, const wo_plate_table* superPlates,
                                   const uint8_t* noisePerm512, const uint8_t* noisePm12_512, double noiseMag, double seed, double spread,
                                   float* r_elevation, float* r_stress, float* debugLayers, int32_t* mountain_r, int32_t* coastline_r,
                                   int32_t* ocean_r, int32_t* setCounts) {
    if (!check_planet(p, "wo_assign_elevation")) return 1;
    if (!r_plate || !plates || !plateSeeds || !noisePerm512 || !noisePm12_512) { set_error("wo_assign_elevation: null pointer"); return 1; }
    WO_TRY
    assign_elevation(p, r_plate, plates, plateSeeds, numPlateSeeds, r_superPlate, superPlates, noisePerm512, noisePm12_512, noiseMag, seed, spread,
                     r_elevation, r_stress, debugLayers, mountain_r, coastline_r, ocean_r, setCounts);
    return 0;
    WO_CATCH("wo_assign_elevation")
}

// projectCoarsePlates (js/coarse-plates.js:51-117) on the planet's resident r_xyz
extern "C" int wo_project_coarse_plates(wo_planet* p, int32_t coarseRegions, const int32_t* coarseAdjOffset, const int32_t* coarseAdjList,
                             const float* coarse_xyz, const int32_t* coarse_r_plate, double seed, int32_t numPlates, int32_t* r_plate) {
    if (!check_planet(p, "wo_project_coarse_plates")) return 1;
    if (coarseRegions < 1 || !coarseAdjOffset || !coarseAdjList || !coarse_xyz || !coarse_r_plate || !r_plate) {
        set_error("wo_project_coarse_plates: bad arguments"); return 1;
    }
    {   // the kernel walks this CSR on the device: validate it the way wo_planet_create validates the planet's
        if (coarseAdjOffset[0] != 0) { set_error("wo_project_coarse_plates: coarseAdjOffset[0] != 0"); return 1; }
        for (int32_t r = 0; r < coarseRegions; ++r)
            if (coarseAdjOffset[r + 1] < coarseAdjOffset[r]) { set_error("wo_project_coarse_plates: coarseAdjOffset is not monotone"); return 1; }
        const int32_t Ec = coarseAdjOffset[coarseRegions];
        for (int32_t i = 0; i < Ec; ++i)
            if (coarseAdjList[i] < 0 || coarseAdjList[i] >= coarseRegions) { set_error("wo_project_coarse_plates: coarseAdjList entry out of range"); return 1; }
    }
    WO_TRY
    hipStream_t s = p->ctx->stream;
    const int32_t NC = coarseRegions, E = coarseAdjOffset[NC];
    CoarsePlates C;
    C.NC = NC; C.gridZ = 64; C.gridLon = 128;
    DeviceArena B;
    C.off = up(B, coarseAdjOffset, (size_t)NC + 1, s); C.adj = up(B, coarseAdjList, (size_t)E, s); C.plate = up(B, coarse_r_plate, (size_t)NC, s);
    C.xyz = up(B, coarse_xyz, 3 * (size_t)NC, s); C.grid = nullptr;
    int32_t* d_grid = B.dev<int32_t>((size_t)C.gridZ * C.gridLon); int32_t* d_out = B.dev<int32_t>(p->N);
    launch(p, FAM_PLATE_GRID, k_plate_grid, blocks_for((int64_t)C.gridZ * C.gridLon), WO_BLOCK, C, d_grid);
    C.grid = d_grid;
    upload_tables(p, seed + 999);                                                       // :57
    const double coarseEdgeRad = 3.141592653589793 / std::sqrt((double)NC);              // :58
    double lowPlateT = 0;                                                                // :59 (numPlates < 0: null)
    if (numPlates >= 0) lowPlateT = std::max(0.0, std::min(1.0, (80 - numPlates) / 60.0));
    const double perturbAmp = coarseEdgeRad * (1.5 + 1.0 * lowPlateT);                   // :60
    launch(p, FAM_PLATE_PROJECT, k_plate_project, blocks_for(p->N), WO_BLOCK, C, (const uint8_t*)p->d_tables, (const float*)p->d_xyz, p->N, perturbAmp, d_out);
    WO_HIP(hipMemcpyAsync(r_plate, d_out, (size_t)p->N * 4, hipMemcpyDeviceToHost, s));
    WO_HIP(hipStreamSynchronize(s));
    return 0;
    WO_CATCH("wo_project_coarse_plates")
}
