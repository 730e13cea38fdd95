// Device-side state of libworogen: context (device + stream), planet (resident mesh + fields + scratch),
// launch / profiling helpers.  gfx950 only.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <map>
#include <string>
#include <utility>
#include <vector>

#include "device_mem.h"
#include "host_util.h"

#include "flood_ops.h"
#include "wo_internal.h"

namespace wo {

// The entry points' try / catch pair: WO_TRY body WO_CATCH("wo_name") turns a HipError into status 2 and any other exception into 3
#define WO_TRY try {
#define WO_CATCH(fn)                                                                                   \
    } catch (const ::wo::HipError& e) { ::wo::set_error(std::string(fn) + ": " + e.msg); return 2; }   \
      catch (const std::exception& e) { ::wo::set_error(std::string(fn) + ": " + e.what()); return 3; }

// A helper that several translation units of the library share but that is no part of its surface: kept out of the dynamic symbol table
#define WO_LOCAL __attribute__((visibility("hidden")))

constexpr int WO_BLOCK = 256;
inline int blocks_for(int64_t n, int maxBlocks = 1 << 20) {
    int64_t b = (n + WO_BLOCK - 1) / WO_BLOCK;
    if (b < 1) b = 1;
    if (b > maxBlocks) b = maxBlocks;
    return (int)b;
}

// grid for WO_XCD_CELLS kernels: one cell per thread, block count rounded up to a multiple of 8
inline int xcd_tile(int64_t n) {          // blocks per tile: a power of two, ~1/64 of the grid, at most 256 (65 k cells)
    const int64_t b = (n + WO_BLOCK - 1) / WO_BLOCK;
    int t = 1;
    while (t < 256 && (int64_t)t * 128 <= b) t <<= 1;
    return t;
}
inline int xcd_grid(int64_t n) {          // block count padded to whole rounds of 8 tiles
    const int64_t b = (n + WO_BLOCK - 1) / WO_BLOCK, per = 8 * (int64_t)xcd_tile(n);
    return (int)(((b + per - 1) / per) * per);
}

// Kernel families for HIP-event profiling (wo_profile_*) — one entry per distinct kernel of the path.
enum Family : int {
    FAM_COAST = 0, FAM_SMOOTH, FAM_SHARPEN, FAM_CREEP, FAM_WARP, FAM_NOISE, FAM_SYNTH, FAM_OCEAN,
    FAM_SORT_KEYS, FAM_SORT_RADIX, FAM_RANK, FAM_RECEIVERS, FAM_FLOW_SNAP, FAM_FLOW_FINAL,
    FAM_SOLVE_SETUP, FAM_SOLVE_ROUND, FAM_SOLVE_FINAL, FAM_THERMAL_EXCESS, FAM_THERMAL_APPLY,
    FAM_GLAC_INDEX, FAM_ICE_RECV, FAM_ICE_ROUND, FAM_CARVE_SETUP, FAM_CARVE_ROUND, FAM_MORAINE, FAM_GLAC_BLEND,
    FAM_SOLVE_PATCH, FAM_ELEV_COLLISION, FAM_ELEV_MAIN, FAM_PLATE_GRID, FAM_PLATE_PROJECT, FAM_SMOOTH_FIELD,
    FAM_FLOOD_EVAL, FAM_FLOOD_APPLY, FAM_FLOOD_MISC, FAM_CLIMATE, FAM_BASIN, FAM_BASIN_SORT, FAM_SOLVE_BASIN, FAM_FLOW_TILES, FAM_MISC, FAM_EVENT_PAIR, FAM_EVENT_PAIR_NOOP, FAM_EVENT_PAIR_NOOP2,
    FAM_MAP_LONLAT, FAM_MAP_FILL, FAM_MAP_SIDES, FAM_MAP_BIG_BOXES, FAM_MAP_RESOLVE, FAM_MAP_REGION_COLORS, FAM_MAP_PIXELS,
    FAM_MAP_RANGE, FAM_MAP_LAYER_COLORS,
    FAM_GLOBE_TABLES, FAM_GLOBE_REGION_COLORS, FAM_GLOBE_RANGE, FAM_GLOBE_MESH, FAM_GLOBE_LINE_COUNT, FAM_GLOBE_LINE_SCAN, FAM_GLOBE_LINE_WRITE,
    FAM_OVERLAY_BINS, FAM_OVERLAY_ARROWS,
    FAM_PICK, FAM_PICK_REDUCE, FAM_HIGHLIGHT,
    FAM_CUBE_CENTERS, FAM_CUBE_FILL, FAM_CUBE_SIDES, FAM_CUBE_BIG_BOXES, FAM_CUBE_RESOLVE,
    FAM_RELIEF_TRI_ELEVATION, FAM_RELIEF_HEIGHTS, FAM_RELIEF_HEIGHT16, FAM_RELIEF_TABLES, FAM_RELIEF_NORMALS,
    FAM_RIVERS, FAM_RIVERS_CLIMB, FAM_RIVERS_LINES,
    FAM_VIEW_TABLES, FAM_VIEW_FILL, FAM_VIEW_SIDES, FAM_VIEW_BIG_BOXES, FAM_VIEW_RESOLVE, FAM_VIEW_SHADE,
    FAM_OUTLINE_CLASSIFY, FAM_OUTLINE_FLAGS, FAM_OUTLINE_SUCC, FAM_OUTLINE_RANK, FAM_OUTLINE_RINGS, FAM_OUTLINE_POSITIONS, FAM_COUNT
};
extern const char* const kFamilyNames[FAM_COUNT];

}  // namespace wo

struct wo_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    hipDeviceProp_t prop{};
};

// device state of the flood's pass 1 (flood_kernels.h); static part per land mask, the rest per call
struct wo_flood_gpu {
    wo::DeviceArena mem;                 // owns every buffer below
    int64_t version = -1; int32_t L = 0, cap = 0, nSeeds = 0;
    int32_t *off = nullptr, *adj = nullptr, *cell = nullptr, *seedIdx = nullptr, *seeds = nullptr; double* nz = nullptr;
    float* e = nullptr;
    wo::FlHead *A = nullptr, *P = nullptr, *F = nullptr;
    unsigned long long *Astk = nullptr, *Pstk = nullptr, *Fstk = nullptr;
    int32_t *fdEpoch = nullptr, *inDirty = nullptr; uint8_t* isPending = nullptr;
    int32_t* lists[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};      // dirty x2, pending x2, changed
    void* ctrl = nullptr; void* h_ctrl = nullptr;
    int32_t *jump = nullptr, *outPar = nullptr, *outRoot = nullptr; float* outSurf = nullptr;
    int32_t *h_par = nullptr, *h_root = nullptr; float* h_surf = nullptr;   // pinned
};

namespace wo {
// Environment switches, read once per API call (check_planet -> Options::from_env), never inside an iteration: cross-check routes the tests drive
// (every one must give the default route's bits), the labelled relaxed mode, diagnostics.  The full list with the host-side ones (WO_HOST_THREADS,
// WO_FLOOD_THREADS, WO_FLOOD_HOST, WO_FLOOD_PIN, WO_ELEV_TIMING) is in include/worogen.h; the test suite's hooks come in ONE variable (host_util.h: WO_TEST_HOOKS).
struct Options {
    bool layoutIndex = false;          // WO_LAYOUT=index          no patch-major mirror: the call runs on the planet's own cell order (flow accumulation by k_flow_climb)
    bool tileLds = false;              // WO_TILE_LDS=1            neighbour window of a workgroup's tile staged in LDS (receivers, thermal)
    bool floodDevice = false;          // WO_FLOOD=device          pass 1 of the flood as the device label-correcting fixed point
    bool floodTiming = false;          // WO_FLOOD_TIMING          stage laps -> stderr
    bool stageTimingAll = false;       // WO_STAGE_TIMING=all      bracket every iteration
    int  relaxedSortEvery = 1;         // WO_RELAXED_SORT_EVERY=K  RELAXED MODE (not parity): re-sort landCells every K-th iteration only
    bool relaxedFull = false;          // WO_RELAXED=full          RELAXED MODE (not parity): one sort per flood, affine pointer-jumping solve with deferred deposition, Jacobi carve (kernels_impl.h)
    // test hooks (WO_TEST_HOOKS)
    bool basinScramble = false;        // basin_scramble=1         a deliberately wrong basin layout (leftovers for the patch finisher)
    long long carveBudgetMs = 200;     // carve_budget_ms=<n>      spin budget of the one-launch carve (0: it gives up at once and the rounds finish)
    int  carveBlocks = 0;              // carve_blocks=<n>         at most this many workgroups for the one-launch carve
    bool oceanSplitSmooth = false;     // ocean_split_smooth=1     ocean currents: the masked smoothing field by field instead of one interleaved gather (the A/B of DESIGN section 8.3)
    bool tempSplitDiffuse = false;     // temp_split_diffuse=1     temperature: diffuseOceanWarmth season by season with the single-field kernels instead of one float2 gather
    bool globeDirectStores = false;    // globe_direct_stores=1    globe mesh: every lane stores its own nine floats instead of staging the workgroup's in LDS (the A/B of DESIGN section 8.11)
    bool overlayPrecheck = false;      // overlay_precheck=1       arrow overlays: a candidate reads the bin's key first and sends its atomicMin only when its own is smaller (the A/B of DESIGN section 8.12)
    int  pickBlocks = 0;               // pick_blocks=<n>          the hit test: at most this many workgroups per tile of queries (0: the default cap), so that the stride loop and the partial reduction run on a small planet
    static Options from_env();
};
}  // namespace wo

struct wo_planet {
    wo_ctx* ctx = nullptr;
    wo::Options opt;
    int32_t N = 0, E = 0, maxDeg = 0;
    wo::DeviceArena mem;                 // owns the planet's own device and pinned buffers (device_mem.h); the members below are views
    // host copies kept for the host-resident flood stage
    wo::hvec<int32_t> h_off, h_adj;          // host mirrors walked in data-dependent order: huge-page advised (host_util.h)
    wo::hvec<float> h_xyz;
    wo::hvec<uint8_t> h_ocean;
    bool h_ocean_valid = false;
    float* h_pinned = nullptr;          // N floats, pinned
    int32_t* h_count = nullptr;         // pinned scalar(s) for round-count read-back
    // host-mapped {serial, value} word the host polls (read_count)
    unsigned long long *h_word = nullptr, *d_word = nullptr; uint32_t wordSerial = 0;
    wo::FloodScratch flood;
    wo::FloodExchange floodX;           // landmass decomposition: the shares pool their heights when a flood call needs the whole planet's heap (wo_planet_set_flood_exchange)
    void* floodLink = nullptr; void (*floodLinkFree)(void*) = nullptr;   // comm.hip: state of the RCCL form of that exchange
    wo_flood_gpu fgpu;

    // resident mesh
    int32_t *d_off = nullptr, *d_adj = nullptr;
    float *d_dist = nullptr, *d_xyz = nullptr;
    // resident fields
    float *d_e = nullptr, *d_e2 = nullptr, *d_hot = nullptr, *d_orig = nullptr;
    uint8_t *d_ocean = nullptr, *d_coast = nullptr;
    int64_t mirrorMaskVersion = -1;      // oceanVersion of the mask the mirror was built for (mirror_build), -1: another mask
    uint8_t* d_oceanKnown = nullptr; int32_t* d_maskDiff = nullptr; bool oceanKnownValid = false;   // the mask h_ocean describes, on the device (refresh_host_ocean)
    bool hot_valid = false;
    float* d_savedE = nullptr; uint8_t* d_savedOcean = nullptr; bool saved = false;
    uint8_t* d_tables = nullptr;        // perm[512] + pm12[512]
    int64_t oceanVersion = 0;            // counts the changes of the mask h_ocean describes (the flood tables' and the land lists' cache key)
    int64_t floodPrefixMirror = -1, floodPrefixStatic = -1;      // (mirror version, flood static version) for which the mirror's first L ids were checked to be the flood's land order
    bool floodPrefixOk = false;
    // banded Jacobi passes
    int32_t *d_haloSend = nullptr, *d_haloRecv = nullptr; float *d_haloBuf = nullptr, *h_haloBuf = nullptr; int32_t nHaloSend = 0, nHaloRecv = 0;

    // heightmap import scratch (heightmap.hip), allocated on first use and grown when needed
    struct Import {
        wo::DeviceArena mem;
        uint8_t* img = nullptr; int64_t imgCap = 0;          // the uploaded grayscale image
        int32_t* label = nullptr;                           // union-find parents, then the component labels
        uint8_t* flags = nullptr;                           // classification + seed bits per cell (import_ops.h: CLS_*)
        int32_t* lists = nullptr;                           // 4 x N: plateSeeds, mountain_r, coastline_r, ocean_r
        uint8_t* seedOcean = nullptr;                       // plateIsOcean.has(seed), parallel to the seed list
        int32_t* blockCounts = nullptr;                     // [blocks][4] counts, scanned in place into offsets
        int32_t* totals = nullptr; int32_t* h_totals = nullptr;   // the four list lengths (device, pinned host)
    } imp;

    // seasonal pressure and wind (wind.hip): the wind block — results and scratch of wo_compute_wind, allocated on its first
    // call; deleted by wo_planet_destroy (wind_free)
    struct wo_wind_block* wind = nullptr;
    // ocean surface currents (ocean.hip): the ocean block — results and scratch of wo_compute_ocean_currents, allocated on its
    // first call; deleted by wo_planet_destroy (ocean_free)
    struct wo_ocean_block* ocean = nullptr;
    // precipitation (precip.hip): the precipitation block — the four results of wo_compute_precipitation, allocated on its first
    // call; deleted by wo_planet_destroy (precip_free)
    struct wo_precip_block* precip = nullptr;
    // temperature and Koppen classes (temp.hip): the temperature block (8 bytes per cell) and the Koppen block (1 byte per cell),
    // allocated on the first call of their stage or upload; deleted by wo_planet_destroy (temp_free)
    struct wo_temp_block* temp = nullptr;
    struct wo_koppen_block* koppen = nullptr;
    // map export (map.hip, cube.hip; map_block.h): the map block — the region map of the last wo_map_raster or wo_map_raster_cube
    // (4 bytes per pixel) and, after wo_relief_raster or wo_relief_raster_cube, the height map of the same shape (4 bytes per
    // pixel), allocated by that call; deleted by wo_map_free and wo_planet_destroy (map_free)
    struct wo_map_block* map = nullptr;
    // the editor's highlight state (globe.hip): one class byte per region (pick_ops.h: CLS_*), set by wo_highlight_set; deleted by
    // wo_highlight_clear and wo_planet_destroy (highlight_free)
    struct wo_highlight_block* highlight = nullptr;
    // rivers and lakes (rivers.hip; rivers_block.h): the rivers block — the five results of wo_compute_rivers (24 bytes per cell),
    // allocated on its first call; deleted by wo_planet_destroy (rivers_free)
    struct wo_rivers_block* rivers = nullptr;
    // erodeComposite (erode.hip, basin.hip, sort.hip, radix.hip; erode_block.h): the erosion block — land lists, sort, flow, solve,
    // ice and carve state, built group by group from the planet's first erodeComposite call on; deleted by wo_planet_destroy (erode_free)
    struct wo_erode_block* erode = nullptr;
    // region outlines (outline.hip): the outline block — the rings of the last wo_outline_build (8 bytes per boundary side and per
    // ring, and 12 per side for the corners its vertices are made of); deleted by wo_outline_free and wo_planet_destroy (outline_free)
    struct wo_outline_block* outline = nullptr;

    // Patch-major mirror of the mesh for erodeComposite (mirror.hip, MirrorScope): the same graph with the cells renamed in
    // Morton order of their positions, rows in the reference's order.  While a scope is active the pointers above (mesh, d_e,
    // d_e2, d_ocean, d_coast) point at the mirror and the o_* members hold the planet's own buffers.
    struct Mirror {
        wo::DeviceArena mem;
        bool built = false, active = false;
        int32_t *perm = nullptr, *inv = nullptr, *off = nullptr, *adj = nullptr;       // perm: mirror id -> cell id
        float *dist = nullptr, *xyz = nullptr, *e = nullptr, *e2 = nullptr, *hot = nullptr;
        uint8_t *ocean = nullptr, *coast = nullptr;
        wo::hvec<int32_t> h_perm, h_morton;           // h_morton: all cells in Morton order (mask-independent)
        wo::hvec<uint8_t> h_mask;                     // the ocean mask the renaming was built for (land first), empty: plain Morton order
        int64_t version = 0;
        int32_t *o_off = nullptr, *o_adj = nullptr; float *o_dist = nullptr, *o_xyz = nullptr, *o_e = nullptr, *o_e2 = nullptr;
        uint8_t *o_ocean = nullptr, *o_coast = nullptr;
    } mirror;

    // measurement
    hipEvent_t evStart = nullptr, evStop = nullptr;
    bool profiling = false;
    struct Pending { int fam; hipEvent_t a, b; };
    std::vector<Pending> pending;
    std::vector<hipEvent_t> eventPool;
    double famMs[wo::FAM_COUNT] = {0};
    int64_t famLaunches[wo::FAM_COUNT] = {0};
    std::vector<std::pair<std::string, double>> stageTiming;
    // the stage brackets of the last erodeComposite call, not yet turned into milliseconds (wo_last_stage_timing does that: the queries are a
    // millisecond of host work that the call itself no longer waits for)
    struct StageBracket { std::string name; hipEvent_t a, b; };
    std::vector<StageBracket> stageBrackets; std::vector<std::pair<std::string, std::pair<int64_t, int64_t>>> stageSeen; bool stagePending = false;
    std::vector<std::pair<std::string, double>> erodeStats;
};

namespace wo {

// profile.hip: profiling-aware launch: when p->profiling every launch is bracketed by events on the planet's stream
hipEvent_t profile_event(wo_planet* p);
void profile_resolve(wo_planet* p);

// planet.hip: the stream launches of this planet currently go to (its context's stream, or the erosion block's side stream while that is on)
hipStream_t cur_stream(const wo_planet* p);

// shmem: bytes of dynamic LDS
template <class... KArgs, class... Args>
inline void launch_shmem(wo_planet* p, int fam, void (*kernel)(KArgs...), int grid, int block, size_t shmem, Args... args) {
    hipStream_t s = cur_stream(p);
    hipEvent_t a = nullptr, b = nullptr;
    if (p->profiling) { a = profile_event(p); b = profile_event(p); WO_HIP(hipEventRecord(a, s)); }
    if (shmem > (size_t)(64 << 10)) WO_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem));
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(block), shmem, s, args...);
    WO_HIP(hipGetLastError());                     // a launch that cannot be configured would otherwise be a silent no-op
    if (p->profiling) { WO_HIP(hipEventRecord(b, s)); p->pending.push_back({fam, a, b}); if (p->pending.size() >= 4096) profile_resolve(p); }
}
template <class... KArgs, class... Args>
inline void launch(wo_planet* p, int fam, void (*kernel)(KArgs...), int grid, int block, Args... args) { launch_shmem(p, fam, kernel, grid, block, (size_t)0, args...); }

// radix.hip: the in-tree stable radix sort, shared by the erosion's sorts and the wind stage (scratch: radix_scratch_words(nMax) u32, zero
// before the first use; flip: call parity kept by the caller)
size_t radix_scratch_words(int32_t nMax);
int radix_sort_pairs(wo_planet* p, int family, uint32_t* const keys[2], int32_t* const vals[2], int32_t n, int beginBit, int endBit, int32_t* posOut,
                     uint32_t* scratch, int32_t nMax, int& flip);
// wind.hip, ocean.hip: drop the wind block / the ocean block (and with it its memory)
void wind_free(wo_planet* p);
void ocean_free(wo_planet* p);
void precip_free(wo_planet* p);
void temp_free(wo_planet* p);
void rivers_free(wo_planet* p);
// outline.hip: drops the outline block
void outline_free(wo_planet* p);
// map.hip: drops the map block
void map_free(wo_planet* p);
// globe.hip: drops the highlight state; its class bytes (on the device), nullptr when no state is set
void highlight_free(wo_planet* p);
const uint8_t* highlight_classes(const wo_planet* p);
// globe.hip: one launch of its k_globe_centers in family fam: the centre records (globe_ops.h) of every triangle from the elevation e
namespace globe { struct Center; }
WO_LOCAL void globe_centers(wo_planet* p, int fam, const int32_t* d_tri, const float* e, globe::Center* out, int32_t numTriangles);
// temp.hip: the class ids of the planet's Koppen block (one byte per cell, on the device), nullptr when it has no Koppen result
const uint8_t* koppen_classes(const wo_planet* p);
// planet.hip: the entry points' handle check (refreshes p->opt from the environment, selects the device)
bool check_planet(wo_planet* p, const char* fn);
// planet.hip: one device integer for the host (through a host-mapped word the host polls); the host's copy of the ocean mask, brought up to date
WO_LOCAL int32_t read_count(wo_planet* p, const int32_t* d_ptr);
WO_LOCAL void refresh_host_ocean(wo_planet* p);
static inline void swap_elev(wo_planet* p) { std::swap(p->d_e, p->d_e2); }
// The device ocean mask changed (or may have): the host copy is refreshed lazily.  The flood's cached
// open-ocean / seed data is only rebuilt when the mask really differs (a "reapply" with the same mask keeps it).
static inline void ocean_changed(wo_planet* p) { p->h_ocean_valid = false; }
// profile.hip: drops the stage brackets an earlier erodeComposite left pending (a call that sets p->stageTiming itself calls it first)
void release_stage_brackets(wo_planet* p);
// terrain.hip: the coast flags of the current field and mask; a noise instance's tables into p->d_tables; a pass on host arrays
// (upload, body, download: the JS call surface, host arrays mutated in place)
WO_LOCAL void coast_flags(wo_planet* p);
WO_LOCAL void upload_tables(wo_planet* p, double seed);
WO_LOCAL int with_host_field(wo_planet* p, const char* fn, float* e, const uint8_t* oc, bool needOcean, void (*body)(wo_planet*, void*), void* arg);
// climate_sweeps.hip: smoothField on a resident field (returns the buffer that holds the result)
float* smooth_field_resident(wo_planet* p, float* a, float* b, int32_t passes);
// climate_sweeps.hip: diffuseOceanWarmth of one season on resident fields with the single-field kernels (seeds a, ping-pongs a and b and
// returns the buffer that holds the result)
float* diffuse_warmth_resident(wo_planet* p, const float* warmth, const uint8_t* isLand, const float* plateCont, int32_t passes, float* a, float* b);
// climate_sweeps.hip: computeWindConvergence and advectMoisture on resident fields (the advection seeds a, ping-pongs a and b and returns
// the buffer that holds the result)
void wind_convergence_resident(wo_planet* p, const float* wx, const float* wy, const float* wz, float* out);
float* advect_moisture_resident(wo_planet* p, const float* heightKm, const uint8_t* isLand, const float* windE, const float* windN, const float* wx, const float* wy,
                                const float* wz, const float* warmth, const int32_t* coastDist, int32_t maxHops, double depletionBase, float* a, float* b);

}  // namespace wo
