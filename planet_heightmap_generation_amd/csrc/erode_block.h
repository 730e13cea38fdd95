// The erosion block of a planet: everything erodeComposite (erode.hip, basin.hip, sort.hip, radix.hip) keeps on the device between its calls.  Made by the
// planet's first erodeComposite call, dropped by wo_planet_destroy (erode_free).  Its buffers come in GROUPS, one nested struct each, every group built whole
// at its first use by build_group(): a planet that only runs thermal passes pays for no carve, basin, flow-tile or affine buffers.  The members are views.
#pragma once
#include "device.h"
#include "erode_ops.h"

struct wo_erode_block {
    wo::DeviceArena mem;                 // owns every buffer below
    int32_t L = 0;                       // land cells of the current call
    // the initial land list (ascending r, js/terrain-post.js:384-390; like the index-order list a function of the ocean mask alone: kept while the mask
    // stays) and what it was made for: the planet's oceanVersion, mirror or not, the number of land cells
    struct Lists { bool built = false; int32_t* init = nullptr; int64_t ocean = -1; bool mirror = false; int32_t L = -1; } lists;
    // what every call needs (erode.hip: ensure_scratch)
    struct Scratch {
        bool built = false;
        // land lists: index order, the sort's ping-pong (cur: which of land[] holds the current order), rank = position in it; the sort's keys
        int32_t *landIdx = nullptr, *land[2] = {nullptr, nullptr}, *rank = nullptr; int cur = 0; uint32_t* keys[2] = {nullptr, nullptr};
        bool identity = false;           // under the land-first mirror: landIdx[i] == i
        void* sortTemp = nullptr;        // tile counts of select_active_by_rank
        // receivers and flow accumulation
        wo::TargetRank* tr = nullptr; float *cellDist = nullptr, *flow = nullptr, *me = nullptr; int32_t* flowCnt = nullptr;
        unsigned long long* accCnt = nullptr; int32_t *jump = nullptr, *nj = nullptr, *doneAt = nullptr;
        // solve: tasks, outputs, event lists; the patch finisher's order, slots, counters (h_patchTotals: pinned, the pending totals of a burst of
        // k_solve_patch launches) and version keys; solvePassSerial: unchecked basin passes so far (their output tag: erode.hip, passTag)
        wo::SolveTask* task = nullptr; wo::SolveOut* out = nullptr; wo::EventList* ev = nullptr;
        int32_t *patchOrder = nullptr, *slotOf = nullptr, *patchPending = nullptr, *patchTotals = nullptr, *patchBlk = nullptr, *h_patchTotals = nullptr;
        int64_t patchVersion = -1; bool patchMirror = false; int32_t numPatches = 0; int64_t lastPatchLaunches = 1, solvePassSerial = 0;
        // thermal, ice, carve (round lists + 8 counters)
        double* totalExcess = nullptr; float *glac = nullptr, *iceFlow = nullptr; int32_t *iceTarget = nullptr, *arank = nullptr; uint8_t* iceUp = nullptr;
        int32_t *carveSlot = nullptr, *listA = nullptr, *listB = nullptr, *counters = nullptr;
    } scratch;
    // radix.hip scratch: [0] elevation sort, [1] basin sort; flip: parity of the passes run so far on it
    struct Radix { bool built = false; uint32_t* words = nullptr; int flip = 0; } radix[2];
    // two-level flow accumulation (kernels_impl.h: FlowTiles)
    struct Tiles { bool built = false; int32_t *lr = nullptr, *parent = nullptr, *extCnt = nullptr; uint32_t* inflow = nullptr; unsigned long long* rootAcc = nullptr; } tiles;
    // basin.hip: component roots (Morton slot space), group-major store order of the pass, range starts and the long ranges' flags
    struct Basin {
        bool built = false; int64_t launches = 0;
        int32_t *J = nullptr, *slot = nullptr, *vals[2] = {nullptr, nullptr}, *range = nullptr; uint32_t* key = nullptr; uint8_t* isLong = nullptr;
    } basin;
    // the carve's per-task buffers (dependency lists, records, expected tags), for cap tasks: the regrown group
    struct Carve {
        bool built = false; int64_t cap = 0;
        int32_t *deps = nullptr, *depCnt = nullptr, *depPos = nullptr, *slotDone = nullptr; wo::CarveRec* recs = nullptr; wo::CarveExpect* expect = nullptr;
        void drop(wo::DeviceArena& m) { m.release(deps); m.release(depCnt); m.release(depPos); m.release(recs); m.release(slotDone); m.release(expect); }
    } carve;
    struct Granules { bool built = false; unsigned long long* g = nullptr; } granules;      // k_carve_granules: height granules per cell
    struct Affine { bool built = false; wo::Affine* buf[2] = {nullptr, nullptr}; } affine;   // relaxed mode: the affine recurrence, ping-pong
    // erode_composite_checked: the field at entry, tasks any basin launch of the call left pending, calls that had to run again
    struct Redo { bool built = false; float* e = nullptr; int32_t* pendingEver = nullptr; int64_t calls = 0; } redo;
    // the side stream (the basin layout beside the flow accumulation), its fork and join events (erode.hip: ensure_side_stream; no arena owns
    // these: erode_free destroys them); on: launches go to it (cur_stream)
    struct Side { bool built = false, on = false; hipStream_t stream = nullptr; hipEvent_t fork = nullptr, join = nullptr; } side;
};

namespace wo {

// The one way a group is built: the builder fills the group's views from a fresh arena, the block's arena takes that over whole, and only then the group
// counts as built.  A builder that throws leaves nothing behind: the fresh arena frees what was made and the group goes back to its initial state, so no
// view is left pointing at freed memory and the next call starts again.
template <class Group, class Build>
inline void build_group(wo_erode_block& b, Group& g, Build&& build) {
    if (g.built) return;
    DeviceArena fresh;
    try { build(fresh); } catch (...) { g = Group{}; throw; }
    b.mem.adopt(fresh);
    g.built = true;
}
// The regrown group: the old buffers go first, the capacity is set once every new one is there
template <class Group, class Build>
inline void regrow_group(wo_erode_block& b, Group& g, int64_t cap, Build&& build) {
    g.drop(b.mem); g.built = false; g.cap = 0;
    build_group(b, g, build);
    g.cap = cap;
}

// planet.hip: the Fields view of a planet: mesh and field pointers from the planet, the rest from its erosion block (null without one)
Fields fields(const wo_planet* p);
// erode.hip: synchronises and destroys the side stream and its events, then drops the block (and with its arena its memory)
void erode_free(wo_planet* p);
// sort.hip: stable descending sort of the land list by current elevation + rank scatter; the carve tasks in landCells order
void sort_land_by_elevation(wo_planet* p);
size_t sort_temp_bytes(int32_t n);
void rank_from_land(wo_planet* p);
void select_active_by_rank(wo_planet* p, const int32_t* arank, int32_t* out, int32_t* outCount);
// radix.hip: the block's scratch of the radix sort, 0: elevation sort, 1: basin sort (built and cleared on first use)
wo_erode_block::Radix& radix_scratch(wo_planet* p, int which);
// basin.hip: group-major store order of the solve (basin.slot, sorted group keys in scratch.keys[1]) and the one-launch solve over it
void basin_alloc(wo_planet* p);
void basin_layout(wo_planet* p, bool slotIdentity);
void basin_solve_launch(wo_planet* p, const Fields& F, int32_t launchTag, int32_t* totalPending);

}  // namespace wo
