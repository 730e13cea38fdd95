// Device context and planet handle: their life cycle and the transfer half of the C ABI (include/worogen.h) — upload, download,
// saved state, halo exchange of the banded passes, the flood exchange's set-up, timers — and what every stage leans on: the
// environment switches, the handle check, the Fields view of a planet and the host's look at a device counter.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstring>

#include "../../include/worogen.h"
#include "common_kernels.h"
#include "device.h"
#include "erode_block.h"

namespace wo {

hipStream_t cur_stream(const wo_planet* p) { return (p->erode && p->erode->side.on && p->erode->side.stream) ? p->erode->side.stream : p->ctx->stream; }

Fields fields(const wo_planet* p) {
    Fields F{};
    F.N = p->N; F.xcdTile = xcd_tile(p->N); F.tileLds = p->opt.tileLds ? 1 : 0; F.off = p->d_off; F.adj = p->d_adj; F.dist = p->d_dist; F.xyz = p->d_xyz; F.ocean = p->d_ocean; F.coast = p->d_coast;
    F.e = p->d_e; F.e2 = p->d_e2; F.xcdTileL = xcd_tile(1);
    if (!p->erode) return F;                 // (a planet that never eroded: the Jacobi and warp kernels read the mesh and the field only)
    const wo_erode_block& B = *p->erode; const auto& S = B.scratch;
    F.L = B.L; F.land = S.land[S.cur]; F.landIdx = S.identity ? nullptr : S.landIdx; F.xcdTileL = xcd_tile(B.L > 0 ? B.L : 1); F.rank = S.rank; F.tr = S.tr; F.ev = S.ev; F.me = S.me; F.carveSlot = S.carveSlot; F.carveDepCnt = B.carve.depCnt; F.carveDepPos = B.carve.depPos; F.cellDist = S.cellDist;
    F.flow = S.flow; F.accCnt = S.accCnt; F.jumpA = S.jump;
    F.task = S.task; F.out = S.out; F.slotOf = (S.patchVersion >= 0) ? S.slotOf : nullptr; F.blk = S.patchBlk; F.doneAt = S.doneAt;
    F.totalExcess = S.totalExcess; F.glac = S.glac; F.iceTarget = S.iceTarget; F.iceFlow = S.iceFlow; F.iceUp = S.iceUp; F.arank = S.arank; F.blocker = S.nj;
    return F;
}

__global__ __launch_bounds__(WO_BLOCK) void k_ocean_from_elev(const float* e, uint8_t* ocean, int32_t N) {
    WO_GRID_STRIDE(r, N) ocean[r] = (e[r] <= 0.0f) ? 1 : 0;
}

// ---------------------------------------------------------------- halo pack / unpack (banded Jacobi) ----
__global__ __launch_bounds__(WO_BLOCK) void k_halo_pack(const float* e, const int32_t* idx, int32_t n, float* out) { WO_GRID_STRIDE(i, n) out[i] = e[idx[i]]; }
__global__ __launch_bounds__(WO_BLOCK) void k_halo_unpack(float* e, const int32_t* idx, int32_t n, const float* in) { WO_GRID_STRIDE(i, n) e[idx[i]] = in[i]; }

// {serial, value} of a device counter into a host-mapped word: the host polls the word instead of paying a copy, a stream
// synchronisation and its wake-up for one integer (read_count)
__global__ void k_publish_count(const int32_t* __restrict__ src, unsigned long long* hostWord, uint32_t serial) {
    if (threadIdx.x == 0 && blockIdx.x == 0)
        __hip_atomic_store(hostWord, ((unsigned long long)serial << 32) | (unsigned long long)(uint32_t)*src, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

__global__ __launch_bounds__(wo::WO_BLOCK) void k_mask_differs(const uint8_t* __restrict__ a, const uint8_t* __restrict__ b, int32_t N, int32_t* flag) {
    bool diff = false;
    for (int32_t r = blockIdx.x * blockDim.x + threadIdx.x; r < N; r += gridDim.x * blockDim.x) diff |= a[r] != b[r];
    if (diff) atomicOr(flag, 1);
}
// The host's copy of the ocean mask, brought up to date.  A mask written on the device (ocean_from_elevation, restore_state, synthetic_terrain) is
// first compared ON the device with the mask the host copy describes (a copy of it kept there): a step that re-derives the same mask — every step of
// the bench — then costs one 10 us kernel and one word instead of a 10 MB download and a 10 MB memcmp.
void refresh_host_ocean(wo_planet* p) {
    if (p->h_ocean_valid) return;
    hipStream_t s = p->ctx->stream;
    if (p->d_oceanKnown && p->oceanKnownValid && p->h_ocean.size() == (size_t)p->N) {
        WO_HIP(hipMemsetAsync(p->d_maskDiff, 0, sizeof(int32_t), s));
        hipLaunchKernelGGL(k_mask_differs, dim3(wo::blocks_for(p->N, 1 << 15)), dim3(wo::WO_BLOCK), 0, s, (const uint8_t*)p->d_ocean, (const uint8_t*)p->d_oceanKnown, p->N, p->d_maskDiff);
        if (read_count(p, p->d_maskDiff) == 0) { p->h_ocean_valid = true; return; }
    }
    hvec<uint8_t> tmp(p->N);
    WO_HIP(hipMemcpyAsync(tmp.data(), p->d_ocean, p->N, hipMemcpyDeviceToHost, s));
    WO_HIP(hipStreamSynchronize(s));
    if (tmp.size() != p->h_ocean.size() || std::memcmp(tmp.data(), p->h_ocean.data(), tmp.size()) != 0) {
        p->h_ocean.swap(tmp);
        p->flood.staticValid = false; ++p->oceanVersion;
    }
    p->h_ocean_valid = true;
    if (!p->d_maskDiff) p->d_maskDiff = p->mem.dev<int32_t>(1);
    if (!p->d_oceanKnown) p->d_oceanKnown = p->mem.dev<uint8_t>(p->N);          // (the last of the two: the comparison above looks at this one)
    WO_HIP(hipMemcpyAsync(p->d_oceanKnown, p->d_ocean, (size_t)p->N, hipMemcpyDeviceToDevice, s));
    p->oceanKnownValid = true;
}

// One device integer for the host, through a host-mapped word the host polls: ~10 us from the producing kernel's end to the next
// launch instead of ~30 (copy kernel, stream synchronisation, wake-up).  Falls back to the copy when the word is not there or the
// poll outlasts 2 s (a faulted stream must surface as an error, not as a hang).
int32_t read_count(wo_planet* p, const int32_t* d_ptr) {
    hipStream_t s = p->ctx->stream;
    if (!p->h_word) {
        p->h_word = p->mem.try_pinned<unsigned long long>(8, hipHostMallocMapped);
        if (!p->h_word || hipHostGetDevicePointer((void**)&p->d_word, p->h_word, 0) != hipSuccess) { p->mem.release(p->h_word); p->d_word = nullptr; (void)hipGetLastError(); }
        else *p->h_word = 0;
    }
    if (p->h_word) {
        const uint32_t serial = ++p->wordSerial;
        hipLaunchKernelGGL(k_publish_count, dim3(1), dim3(1), 0, s, d_ptr, p->d_word, serial);
        const auto t0 = std::chrono::steady_clock::now();
        for (uint64_t spins = 0;; ++spins) {
            const unsigned long long w = __atomic_load_n(p->h_word, __ATOMIC_ACQUIRE);
            if ((uint32_t)(w >> 32) == serial) return (int32_t)(uint32_t)w;
            if ((spins & 0xfff) == 0xfff && std::chrono::steady_clock::now() - t0 > std::chrono::seconds(2)) break;
            __builtin_ia32_pause();
        }
        WO_HIP(hipStreamSynchronize(s));                           // surfaces a device fault; a merely slow kernel ends up here too
        const unsigned long long w = __atomic_load_n(p->h_word, __ATOMIC_ACQUIRE);
        if ((uint32_t)(w >> 32) == serial) return (int32_t)(uint32_t)w;
    }
    WO_HIP(hipMemcpyAsync(p->h_count, d_ptr, sizeof(int32_t), hipMemcpyDeviceToHost, s));
    WO_HIP(hipStreamSynchronize(s));
    return p->h_count[0];
}

}  // namespace wo

// =====================================================================================================
// C ABI
// =====================================================================================================
using namespace wo;

Options Options::from_env() {
    auto str = [](const char* n) { const char* v = std::getenv(n); return std::string(v ? v : ""); };
    auto on = [](const char* n) { const char* v = std::getenv(n); return v && std::atoi(v) != 0; };
    auto set = [](const char* n) { return std::getenv(n) != nullptr; };
    Options o;
    o.layoutIndex = str("WO_LAYOUT") == "index";
    o.tileLds = on("WO_TILE_LDS");
    o.floodDevice = str("WO_FLOOD") == "device";
    o.floodTiming = set("WO_FLOOD_TIMING");
    o.stageTimingAll = str("WO_STAGE_TIMING") == "all";
    if (set("WO_RELAXED_SORT_EVERY")) o.relaxedSortEvery = std::max(1, std::atoi(std::getenv("WO_RELAXED_SORT_EVERY")));
    o.relaxedFull = str("WO_RELAXED") == "full";
    o.basinScramble = test_hook_int("basin_scramble", 0) != 0;
    o.carveBudgetMs = test_hook_int("carve_budget_ms", 200);
    o.carveBlocks = (int)std::max<long long>(0, test_hook_int("carve_blocks", 0));
    o.oceanSplitSmooth = test_hook_int("ocean_split_smooth", 0) != 0;
    o.tempSplitDiffuse = test_hook_int("temp_split_diffuse", 0) != 0;
    o.globeDirectStores = test_hook_int("globe_direct_stores", 0) != 0;
    o.overlayPrecheck = test_hook_int("overlay_precheck", 0) != 0;
    o.pickBlocks = (int)std::max<long long>(0, std::min<long long>(test_hook_int("pick_blocks", 0), 1 << 16));
    return o;
}

bool wo::check_planet(wo_planet* p, const char* fn) {
    if (!p) { set_error(std::string(fn) + ": null planet handle"); return false; }
    p->opt = Options::from_env();
    hipError_t e = hipSetDevice(p->ctx->device);
    if (e != hipSuccess) { set_error(std::string(fn) + ": hipSetDevice failed: " + hipGetErrorString(e)); return false; }
    return true;
}

extern "C" {

int wo_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

wo_ctx* wo_ctx_create(int32_t device) {
    try {
        int n = 0;
        if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) {
            set_error("wo_ctx_create: no usable HIP device (libworogen has no CPU fallback)");
            return nullptr;
        }
        if (device < 0 || device >= n) { set_error("wo_ctx_create: device index out of range"); return nullptr; }
        auto* c = new wo_ctx();
        c->device = device;
        WO_HIP(hipSetDevice(device));
        WO_HIP(hipGetDeviceProperties(&c->prop, device));
        WO_HIP(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
        return c;
    } catch (const HipError& e) { set_error(std::string("wo_ctx_create: ") + e.msg); return nullptr; }
}

void wo_ctx_destroy(wo_ctx* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

wo_planet* wo_planet_create(wo_ctx* ctx, int32_t numRegions, const int32_t* adjOffset, const int32_t* adjList,
                            const float* r_xyz, const float* neighborDist) {
    if (!ctx || numRegions < 1 || !adjOffset || !adjList || !r_xyz) { set_error("wo_planet_create: bad arguments"); return nullptr; }
    wo_planet* p = nullptr;
    try {
        WO_HIP(hipSetDevice(ctx->device));
        const int32_t N = numRegions, E = adjOffset[N];
        int32_t maxDeg = 0;
        if (adjOffset[0] != 0) { set_error("wo_planet_create: adjOffset[0] != 0"); return nullptr; }
        for (int32_t r = 0; r < N; ++r) {
            const int32_t d = adjOffset[r + 1] - adjOffset[r];
            if (d < 0) { set_error("wo_planet_create: adjOffset is not monotone"); return nullptr; }
            maxDeg = std::max(maxDeg, d);
        }
        if (maxDeg > WO_MAX_DEG) { set_error("wo_planet_create: vertex degree " + std::to_string(maxDeg) + " exceeds the supported maximum " + std::to_string(WO_MAX_DEG)); return nullptr; }
        for (int32_t i = 0; i < E; ++i) if (adjList[i] < 0 || adjList[i] >= N) { set_error("wo_planet_create: adjList entry out of range"); return nullptr; }
        {   // simple graph: the order-exact parallel passes rely on a cell's neighbours being distinct cells other than itself
            std::atomic<int> bad{0};
            parallel_ranges(N, [&](int64_t b, int64_t e, int) {
                for (int64_t r = b; r < e && !bad.load(std::memory_order_relaxed); ++r)
                    for (int32_t i = adjOffset[r]; i < adjOffset[r + 1]; ++i) {
                        if (adjList[i] == r) { bad = 1; break; }
                        for (int32_t j = adjOffset[r]; j < i; ++j) if (adjList[j] == adjList[i]) { bad = 2; break; }
                    }
            });
            if (bad) { set_error(bad == 1 ? "wo_planet_create: a cell lists itself as a neighbour" : "wo_planet_create: a cell lists the same neighbour twice"); return nullptr; }
        }
        p = new wo_planet();
        p->ctx = ctx; p->N = N; p->E = E; p->maxDeg = maxDeg;
        p->h_off.assign(adjOffset, adjOffset + N + 1);
        p->h_adj.assign(adjList, adjList + E);
        p->h_xyz.assign(r_xyz, r_xyz + 3 * (size_t)N);
        hipStream_t s = ctx->stream;
        DeviceArena& a = p->mem;
        // + WO_ROW: load_row reads whole 16-byte pieces
        p->d_off = a.dev<int32_t>(N + 1); p->d_adj = a.dev<int32_t>((size_t)E + WO_ROW); p->d_dist = a.dev<float>((size_t)E + WO_ROW); p->d_xyz = a.dev<float>(3 * (size_t)N);
        WO_HIP(hipMemsetAsync(p->d_adj + E, 0, WO_ROW * sizeof(int32_t), s)); WO_HIP(hipMemsetAsync(p->d_dist + E, 0, WO_ROW * sizeof(float), s));
        p->d_e = a.dev<float>(N); p->d_e2 = a.dev<float>(N); p->d_hot = a.dev<float>(N); p->d_orig = a.dev<float>(N);
        p->d_ocean = a.dev<uint8_t>(N); p->d_coast = a.dev<uint8_t>(N); p->d_tables = a.dev<uint8_t>(1024);
        p->h_pinned = a.pinned<float>(std::max<size_t>(N, 16));
        p->h_count = a.pinned<int32_t>(16);
        WO_HIP(hipMemcpyAsync(p->d_off, adjOffset, (size_t)(N + 1) * 4, hipMemcpyHostToDevice, s));
        WO_HIP(hipMemcpyAsync(p->d_adj, adjList, (size_t)E * 4, hipMemcpyHostToDevice, s));
        WO_HIP(hipMemcpyAsync(p->d_xyz, r_xyz, (size_t)N * 12, hipMemcpyHostToDevice, s));
        if (neighborDist) {
            WO_HIP(hipMemcpyAsync(p->d_dist, neighborDist, (size_t)E * 4, hipMemcpyHostToDevice, s));
        } else {
            std::vector<float> nd(E);
            neighbor_dist(N, adjOffset, adjList, r_xyz, nd.data());
            WO_HIP(hipMemcpyAsync(p->d_dist, nd.data(), (size_t)E * 4, hipMemcpyHostToDevice, s));
            WO_HIP(hipStreamSynchronize(s));
        }
        WO_HIP(hipMemsetAsync(p->d_e, 0, (size_t)N * 4, s));
        WO_HIP(hipMemsetAsync(p->d_ocean, 0, (size_t)N, s));
        WO_HIP(hipEventCreate(&p->evStart)); WO_HIP(hipEventCreate(&p->evStop));
        WO_HIP(hipStreamSynchronize(s));
        return p;
    } catch (const HipError& e) {
        set_error(std::string("wo_planet_create: ") + e.msg);
        if (p) wo_planet_destroy(p);
        return nullptr;
    }
}

void wo_planet_destroy(wo_planet* p) {
    if (!p) return;
    (void)hipSetDevice(p->ctx->device);
    (void)hipStreamSynchronize(p->ctx->stream);
    if (p->floodLink && p->floodLinkFree) p->floodLinkFree(p->floodLink);
    p->floodLink = nullptr;
    highlight_free(p);
    outline_free(p);
    map_free(p);
    temp_free(p);
    rivers_free(p);
    erode_free(p);
    precip_free(p);
    ocean_free(p);
    wind_free(p);
    for (auto& pe : p->pending) { (void)hipEventDestroy(pe.a); (void)hipEventDestroy(pe.b); }
    for (auto& b : p->stageBrackets) { (void)hipEventDestroy(b.a); (void)hipEventDestroy(b.b); }
    for (auto e : p->eventPool) (void)hipEventDestroy(e);
    if (p->evStart) (void)hipEventDestroy(p->evStart);
    if (p->evStop) (void)hipEventDestroy(p->evStop);
    delete p;                           // its arenas (the planet's own, flood state, import scratch, mirror) free the memory
}

int wo_planet_upload(wo_planet* p, const float* r_elevation, const uint8_t* r_isOcean) {
    if (!check_planet(p, "wo_planet_upload")) return 1;
    WO_TRY
    hipStream_t s = p->ctx->stream;
    if (r_elevation) WO_HIP(hipMemcpyAsync(p->d_e, r_elevation, (size_t)p->N * 4, hipMemcpyHostToDevice, s));
    if (r_isOcean) {
        WO_HIP(hipMemcpyAsync(p->d_ocean, r_isOcean, (size_t)p->N, hipMemcpyHostToDevice, s));
        if (p->h_ocean.size() != (size_t)p->N || std::memcmp(p->h_ocean.data(), r_isOcean, (size_t)p->N) != 0) {
            p->h_ocean.assign(r_isOcean, r_isOcean + p->N);
            p->flood.staticValid = false; ++p->oceanVersion;
            p->oceanKnownValid = false;                    // (the device-side copy of the known mask is brought up to date by the next download)
        }
        p->h_ocean_valid = true;
    }
    WO_HIP(hipStreamSynchronize(s));
    return 0;
    WO_CATCH("wo_planet_upload")
}

// ---- halo lists of a band-decomposed Jacobi pass (planet = one band + its one-ring halo, see banded.py) ----
int wo_planet_set_halo(wo_planet* p, const int32_t* sendIdx, int32_t nSend, const int32_t* recvIdx, int32_t nRecv) {
    if (!check_planet(p, "wo_planet_set_halo")) return 1;
    if (nSend < 0 || nRecv < 0 || (nSend && !sendIdx) || (nRecv && !recvIdx)) { set_error("wo_planet_set_halo: bad arguments"); return 1; }
    for (int32_t i = 0; i < nSend; ++i) if (sendIdx[i] < 0 || sendIdx[i] >= p->N) { set_error("wo_planet_set_halo: send index out of range"); return 1; }
    for (int32_t i = 0; i < nRecv; ++i) if (recvIdx[i] < 0 || recvIdx[i] >= p->N) { set_error("wo_planet_set_halo: receive index out of range"); return 1; }
    WO_TRY
    hipStream_t s = p->ctx->stream;
    // the old lists go first; the counts are set once the new buffers are there
    DeviceArena& a = p->mem;
    a.release(p->d_haloSend); a.release(p->d_haloRecv); a.release(p->d_haloBuf); a.release(p->h_haloBuf);
    p->nHaloSend = 0; p->nHaloRecv = 0;
    const size_t m = (size_t)std::max(nSend, nRecv);
    p->d_haloSend = a.dev<int32_t>(nSend); p->d_haloRecv = a.dev<int32_t>(nRecv); p->d_haloBuf = a.dev<float>(m);
    p->h_haloBuf = a.pinned<float>(std::max<size_t>(m, 16));
    p->nHaloSend = nSend; p->nHaloRecv = nRecv;
    if (nSend) WO_HIP(hipMemcpyAsync(p->d_haloSend, sendIdx, (size_t)nSend * 4, hipMemcpyHostToDevice, s));
    if (nRecv) WO_HIP(hipMemcpyAsync(p->d_haloRecv, recvIdx, (size_t)nRecv * 4, hipMemcpyHostToDevice, s));
    WO_HIP(hipStreamSynchronize(s));
    return 0;
    WO_CATCH("wo_planet_set_halo")
}
// ---- landmass decomposition: the shares' flood exchange (flood_host.cc: flood_host_passes_exchange) ----
int wo_planet_set_flood_exchange(wo_planet* p, const uint8_t* trueOcean, wo_flood_exchange_fn fn, void* user) {
    if (!check_planet(p, "wo_planet_set_flood_exchange")) return 1;
    try {
        if (p->floodLink && p->floodLinkFree) { p->floodLinkFree(p->floodLink); }
        p->floodLink = nullptr; p->floodLinkFree = nullptr;
        FloodExchange& X = p->floodX;
        if (!fn) { X.on = false; X.fn = nullptr; X.user = nullptr; X.trueOcean.clear(); X.global = FloodScratch{}; return 0; }
        if (!trueOcean) { set_error("wo_planet_set_flood_exchange: the planet's true ocean mask is required"); return 1; }
        const bool same = X.trueOcean.size() == (size_t)p->N && std::memcmp(X.trueOcean.data(), trueOcean, (size_t)p->N) == 0;
        if (!same) { X.trueOcean.assign(trueOcean, trueOcean + p->N); X.global.staticValid = false; }
        // protocol handshake (phase -1): the callback must know THIS protocol (phases 0-3; round 4's had 0-1 only, and a callback written for it that
        // treats every phase != 0 as the all-gather would gather over the wrong buffer on phases 2 / 3 and report success)
        int32_t hello = WO_FLOOD_EXCHANGE_PROTOCOL;
        const int hrc = fn(user, -1, &hello, 1);
        if (hrc != 0 || hello != -WO_FLOOD_EXCHANGE_PROTOCOL) {
            X.on = false; X.fn = nullptr; X.user = nullptr;
            set_error("wo_planet_set_flood_exchange: the callback did not acknowledge exchange protocol " + std::to_string(WO_FLOOD_EXCHANGE_PROTOCOL) +
                      " (phase -1: negate buf[0] and return 0; return non-zero for any phase it does not implement)");
            return 1;
        }
        X.fn = fn; X.user = user; X.on = true;
        X.calls = X.gathers = X.globalFloods = X.received = 0; X.posVersion = -1; X.landTotal = -1;
        return 0;
    WO_CATCH("wo_planet_set_flood_exchange")
}

int wo_planet_pack_halo(wo_planet* p, float* hostOut, void* deviceOut) {
    if (!check_planet(p, "wo_planet_pack_halo")) return 1;
    if ((hostOut == nullptr) == (deviceOut == nullptr)) { set_error("wo_planet_pack_halo: pass exactly one of hostOut / deviceOut"); return 1; }
    WO_TRY
    hipStream_t s = p->ctx->stream;
    const int32_t n = p->nHaloSend;
    if (n > 0) {
        float* dst = deviceOut ? (float*)deviceOut : p->d_haloBuf;
        launch(p, FAM_MISC, k_halo_pack, blocks_for(n), WO_BLOCK, (const float*)p->d_e, (const int32_t*)p->d_haloSend, n, dst);
        if (hostOut) {
            WO_HIP(hipMemcpyAsync(p->h_haloBuf, p->d_haloBuf, (size_t)n * 4, hipMemcpyDeviceToHost, s));
            WO_HIP(hipStreamSynchronize(s));
            std::memcpy(hostOut, p->h_haloBuf, (size_t)n * 4);
            return 0;
        }
    }
    WO_HIP(hipStreamSynchronize(s));           // deviceOut is handed to another stream (RCCL) next
    return 0;
    WO_CATCH("wo_planet_pack_halo")
}
int wo_planet_unpack_halo(wo_planet* p, const float* hostIn, const void* deviceIn) {
    if (!check_planet(p, "wo_planet_unpack_halo")) return 1;
    if ((hostIn == nullptr) == (deviceIn == nullptr)) { set_error("wo_planet_unpack_halo: pass exactly one of hostIn / deviceIn"); return 1; }
    WO_TRY
    hipStream_t s = p->ctx->stream;
    const int32_t n = p->nHaloRecv;
    if (n > 0) {
        const float* src = (const float*)deviceIn;
        if (hostIn) {
            std::memcpy(p->h_haloBuf, hostIn, (size_t)n * 4);
            WO_HIP(hipMemcpyAsync(p->d_haloBuf, p->h_haloBuf, (size_t)n * 4, hipMemcpyHostToDevice, s));
            src = p->d_haloBuf;
        }
        launch(p, FAM_MISC, k_halo_unpack, blocks_for(n), WO_BLOCK, p->d_e, (const int32_t*)p->d_haloRecv, n, src);
        WO_HIP(hipStreamSynchronize(s));       // the caller may reuse its buffer; the next pass reads d_e on this stream anyway
    }
    return 0;
    WO_CATCH("wo_planet_unpack_halo")
}

int wo_planet_download(wo_planet* p, float* r_elevation) {
    if (!check_planet(p, "wo_planet_download") || !r_elevation) { if (p) set_error("wo_planet_download: null pointer"); return 1; }
    WO_TRY
    WO_HIP(hipMemcpyAsync(r_elevation, p->d_e, (size_t)p->N * 4, hipMemcpyDeviceToHost, p->ctx->stream));
    WO_HIP(hipStreamSynchronize(p->ctx->stream));
    return 0;
    WO_CATCH("wo_planet_download")
}

int wo_planet_ocean_from_elevation(wo_planet* p) {
    if (!check_planet(p, "wo_planet_ocean_from_elevation")) return 1;
    WO_TRY
    launch(p, FAM_OCEAN, k_ocean_from_elev, blocks_for(p->N), WO_BLOCK, (const float*)p->d_e, p->d_ocean, p->N);
    ocean_changed(p);
    return 0;
    WO_CATCH("wo_planet_ocean_from_elevation")
}

int wo_planet_download_ocean(wo_planet* p, uint8_t* r_isOcean) {
    if (!check_planet(p, "wo_planet_download_ocean") || !r_isOcean) { if (p) set_error("wo_planet_download_ocean: null pointer"); return 1; }
    WO_TRY
    WO_HIP(hipMemcpyAsync(r_isOcean, p->d_ocean, (size_t)p->N, hipMemcpyDeviceToHost, p->ctx->stream));
    WO_HIP(hipStreamSynchronize(p->ctx->stream));
    return 0;
    WO_CATCH("wo_planet_download_ocean")
}

int wo_planet_sync(wo_planet* p) {
    if (!check_planet(p, "wo_planet_sync")) return 1;
    WO_TRY
    WO_HIP(hipStreamSynchronize(p->ctx->stream));
    return 0;
    WO_CATCH("wo_planet_sync")
}

int wo_planet_save_state(wo_planet* p) {
    if (!check_planet(p, "wo_planet_save_state")) return 1;
    WO_TRY
    if (!p->d_savedOcean) p->d_savedOcean = p->mem.dev<uint8_t>(p->N);
    if (!p->d_savedE) p->d_savedE = p->mem.dev<float>(p->N);
    WO_HIP(hipMemcpyAsync(p->d_savedE, p->d_e, (size_t)p->N * 4, hipMemcpyDeviceToDevice, p->ctx->stream));
    WO_HIP(hipMemcpyAsync(p->d_savedOcean, p->d_ocean, (size_t)p->N, hipMemcpyDeviceToDevice, p->ctx->stream));
    p->saved = true;
    return 0;
    WO_CATCH("wo_planet_save_state")
}

int wo_planet_restore_state(wo_planet* p) {
    if (!check_planet(p, "wo_planet_restore_state")) return 1;
    if (!p->saved) { set_error("wo_planet_restore_state: nothing saved"); return 1; }
    WO_TRY
    WO_HIP(hipMemcpyAsync(p->d_e, p->d_savedE, (size_t)p->N * 4, hipMemcpyDeviceToDevice, p->ctx->stream));
    WO_HIP(hipMemcpyAsync(p->d_ocean, p->d_savedOcean, (size_t)p->N, hipMemcpyDeviceToDevice, p->ctx->stream));
    ocean_changed(p);
    return 0;
    WO_CATCH("wo_planet_restore_state")
}

int wo_planet_upload_hotspot(wo_planet* p, const float* r_hotspot) {
    if (!check_planet(p, "wo_planet_upload_hotspot") || !r_hotspot) { if (p) set_error("wo_planet_upload_hotspot: null pointer"); return 1; }
    WO_TRY
    WO_HIP(hipMemcpyAsync(p->d_hot, r_hotspot, (size_t)p->N * 4, hipMemcpyHostToDevice, p->ctx->stream));
    WO_HIP(hipStreamSynchronize(p->ctx->stream));
    p->hot_valid = true;
    return 0;
    WO_CATCH("wo_planet_upload_hotspot")
}

int32_t wo_planet_num_regions(const wo_planet* p) { return p ? p->N : 0; }

int wo_memory_in_use(int64_t* deviceBytes, int64_t* pinnedBytes, int64_t* allocCalls) {
    const MemoryInUse& m = memory_in_use();
    if (deviceBytes) *deviceBytes = m.deviceBytes.load();
    if (pinnedBytes) *pinnedBytes = m.pinnedBytes.load();
    if (allocCalls) *allocCalls = m.allocCalls.load();
    return 0;
}

// ---- measurement ----
int wo_timer_start(wo_planet* p) {
    if (!check_planet(p, "wo_timer_start")) return 1;
    WO_TRY WO_HIP(hipEventRecord(p->evStart, p->ctx->stream)); return 0; WO_CATCH("wo_timer_start")
}
int wo_timer_stop_ms(wo_planet* p, double* ms) {
    if (!check_planet(p, "wo_timer_stop_ms") || !ms) return 1;
    WO_TRY
    WO_HIP(hipEventRecord(p->evStop, p->ctx->stream));
    WO_HIP(hipEventSynchronize(p->evStop));
    float f = 0; WO_HIP(hipEventElapsedTime(&f, p->evStart, p->evStop));
    *ms = f;
    return 0;
    WO_CATCH("wo_timer_stop_ms")
}

}  // extern "C"
