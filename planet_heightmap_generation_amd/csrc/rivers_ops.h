// Rivers and lakes of the final terrain (ours: the reference has no hydrology beyond the scratch of erodeComposite): the per-cell
// bodies and the host tree walk shared by the device stage (rivers.hip) and the test-only CPU emulator (tests/emu_rivers), so that
// both compile the very same rules.  Nothing here is floating-point arithmetic beyond comparisons, one f32 mean and two exact
// conversions, so the contract is bit equality of all five fields with any other statement of it (tests/rivers_common.py holds a
// serial one that shares no code with this file).
//
// Inputs.  The planet's CSR neighbour graph (off, adj; symmetric, no row names a cell twice), e, the f32 elevation, and one runoff
//   value per cell from one of three sources: RUNOFF_PRECIP (r_precip_summer + r_precip_winter) * 0.5f evaluated in f32,
//   RUNOFF_UNIFORM 1 per cell, RUNOFF_VALUES the caller's floats.
// 1. Land.  A cell is land iff e > 0; NaN is not land.  key(r) = (e[r], r), compared lexicographically, e by value: a total order
//   on the cells that are not NaN, so flats need no special case.
// 2. Receivers.  The receiver of a land cell is its neighbour with the lowest key, if that key is below its own; otherwise the cell
//   is a pit.  Ocean neighbours take part with their own e, so a coast cell drains to an ocean cell; a NaN neighbour never wins.
//   A cell whose chain of receivers ends in an ocean cell is drained; the cells whose chain ends in pit b are basin b.
// 3. Passes.  A pass is an adjacent pair (u, v) of land cells in different classes, the classes being the basins and the single
//   class "drained".  level = max(e[u], e[v]).  Its key is (order_key(level) << 32) | slot, where order_key is the order of floats
//   as an order of uint32 words (globe_ops.h) and slot is the index into adj at which max(u, v) stands in the row of min(u, v):
//   an index into the whole list, not into the row, so that all pass keys are distinct (on a plateau every level is the same).
// 4. Spills.  The resolved set starts as the drained class.  Repeatedly the lowest-key pass with u in an unresolved basin B and v
//   resolved is taken: spillTo(B) = v, outlet(B) = u, passLevel(B) = level, B becomes resolved, and its water level is W(B) = W(P)
//   if v lies in a basin P and e[v] < W(P) (B is drowned in P's lake), else passLevel(B).  This is Prim's algorithm from the
//   drained class; with distinct keys its tree is THE minimum spanning tree of the basin graph (of the part connected to the drained
//   class), so any construction of that tree rooted at the drained class gives the same spills.  Here: Boruvka rounds.  Every
//   unresolved component takes its lowest cross-component pass (cell_offer, atomicMin on the device); those are tree edges by the cut
//   property; the components hook along them (two components that chose the same pass: the lower id stays a root) and are
//   relabelled.  A component that merged with the drained class stops offering.  The chosen edges, at most one per pit, go to
//   resolve_spills below, which roots the tree at the drained class and walks it: W(B) needs W of B's parent only, so the walk's
//   order is free.  Basins the walk does not reach (a landmass that touches no drained cell) stay endorheic.
// 5. Final receiver.  That of step 2, except that a spilled basin's pit receives spillTo(B).  A forest rooted at ocean cells and
//   endorheic pits.  -1 at roots and off land.
// 6. Lake level.  W(B) where the cell lies in a spilled basin and e < W(B); otherwise the quiet NaN 0x7FC00000.
// 7. Discharge.  q(r) = floor(min(max(runoff, 0), 16) * 65536 + 0.5) as uint64 on land, 0 for a NaN runoff and off land.
//   D(r) = q(r) + the sum of D over the cells whose final receiver is r: uint64 sums, exact in any order (16 * 2^16 * 40 M < 2^46).
//   Ocean cells hold the discharge that reaches them.  r_river_flow = (float)((double)D * 2^-16).
// Lines and tint.  A cell is a river cell under minFlow iff it is land, D >= ceil(minFlow * 65536), it has a receiver of step 2
//   (the jump from a spilled pit to spillTo is never drawn: its ends need not be neighbours) and no lake level of its own.  Its
//   segment runs from the cell to its receiver, each end r_xyz * (1.003 + (e > 0 ? e * 0.04 : e * 0.04 * 0.3)) in double, stored
//   f32 (globe_ops.h: disp).  The map tint paints the regions that are river cells or have a lake level.
#pragma once
#include <cstdint>
#include <vector>

#include "globe_ops.h"

namespace wo {
namespace rivers {

namespace M = wo::map;
namespace G = wo::globe;

enum : int32_t { RUNOFF_PRECIP = 0, RUNOFF_UNIFORM = 1, RUNOFF_VALUES = 2 };      // WO_RIVERS_RUNOFF_* of worogen.h
enum : int32_t { BASIN_DRAINED = -1, BASIN_NOT_LAND = -2 };
enum : int32_t { FIELD_RECEIVER = 0, FIELD_BASIN, FIELD_LAKE, FIELD_DISCHARGE, FIELD_FLOW, FIELD_COUNT };
constexpr uint64_t NO_PASS = ~0ull;
constexpr uint32_t QUIET_NAN_BITS = 0x7FC00000u;
constexpr double LINE_BASE = 1.003;
constexpr uint32_t TINT_RGBA = 41u | (98u << 8) | (168u << 16) | (255u << 24);      // bytes R, G, B, A

WO_IMP_HD inline bool runoff_source_ok(int32_t s) { return s == RUNOFF_PRECIP || s == RUNOFF_UNIFORM || s == RUNOFF_VALUES; }
WO_IMP_HD inline float quiet_nan() { return M::f32_of_bits(QUIET_NAN_BITS); }
WO_IMP_HD inline bool is_land(float e) { return e > 0.0f; }
// key(a) < key(b); false when either elevation is a NaN
WO_IMP_HD inline bool key_less(float ea, int32_t a, float eb, int32_t b) { return ea < eb || (ea == eb && a < b); }

// step 2: the receiver of land cell r, -1 for a pit
WO_IMP_HD inline int32_t receiver_of(const int32_t* off, const int32_t* adj, const float* e, int32_t r) {
    float be = e[r];
    int32_t best = r;
    for (int32_t k = off[r]; k < off[r + 1]; ++k) {
        const int32_t n = adj[k];
        const float en = e[n];
        if (key_less(en, n, be, best)) { be = en; best = n; }
    }
    return best == r ? -1 : best;
}

// step 7
WO_IMP_HD inline float precip_runoff(float summer, float winter) { return (summer + winter) * 0.5f; }
WO_IMP_HD inline uint64_t runoff_q(float runoff) {
    if (runoff != runoff) return 0;
    const float c = runoff < 0.0f ? 0.0f : (runoff > 16.0f ? 16.0f : runoff);
    return (uint64_t)((double)c * 65536.0 + 0.5);            // the value is not negative: the conversion is the floor
}
WO_IMP_HD inline float flow_of(uint64_t D) { return (float)((double)D * (1.0 / 65536.0)); }
// ceil(minFlow * 65536) as a threshold on D; minFlow is finite (the entry points check it)
inline uint64_t min_q(double minFlow) {
    const double m = minFlow * 65536.0;
    if (!(m > 0.0)) return 0;
    if (m >= 18446744073709549568.0) return ~0ull;
    const uint64_t f = (uint64_t)m;
    return (double)f < m ? f + 1 : f;
}

// step 3
WO_IMP_HD inline uint64_t pass_key(float level, uint32_t slot) { return ((uint64_t)G::order_key(level) << 32) | slot; }
// the index into adj at which hi stands in the row of lo, -1 when the row does not name it
WO_IMP_HD inline int64_t slot_of(const int32_t* off, const int32_t* adj, int32_t lo, int32_t hi) {
    for (int32_t k = off[lo]; k < off[lo + 1]; ++k)
        if (adj[k] == hi) return k;
    return -1;
}
// the row that holds index `slot` of adj: the largest r with off[r] <= slot
WO_IMP_HD inline int32_t row_of(const int32_t* off, int32_t N, uint32_t slot) {
    int32_t lo = 0, hi = N - 1;
    while (lo < hi) {
        const int32_t mid = lo + (hi - lo + 1) / 2;
        if ((uint32_t)off[mid] <= slot) lo = mid; else hi = mid - 1;
    }
    return lo;
}
// The lowest key among the passes of land cell u whose other end lies in another component, NO_PASS when it has none.
// cellPit[r]: the index of r's basin in the pit list, numPits for a drained cell, -1 off land; comp[i]: the component of pit i
// (comp[numPits] == numPits, the drained class).
WO_IMP_HD inline uint64_t cell_offer(const int32_t* off, const int32_t* adj, const float* e, const int32_t* cellPit, const int32_t* comp, int32_t u, int32_t cu) {
    uint64_t best = NO_PASS;
    const float eu = e[u];
    for (int32_t k = off[u]; k < off[u + 1]; ++k) {
        const int32_t v = adj[k];
        const int32_t pv = cellPit[v];
        if (pv < 0 || comp[pv] == cu) continue;
        const int64_t slot = u < v ? (int64_t)k : slot_of(off, adj, v, u);
        if (slot < 0) continue;
        const float ev = e[v];
        const uint64_t key = pass_key(eu > ev ? eu : ev, (uint32_t)slot);
        if (key < best) best = key;
    }
    return best;
}

// A chosen pass, as the device hands it to the host: its cells, u in the component that chose it, the pit-list indices of their
// basins (numPits: drained) and their elevations
struct PassEdge { int32_t u, v, pu, pv; float eu, ev; };

// What a root component c does with its lowest pass best[c], whose cells are decoded here: -> the component it hooks to, or c when
// it stays a root (no pass, or the other component chose the same pass and has the higher id).  edge: the pass, written when c hooks.
WO_IMP_HD inline int32_t hook_of(const int32_t* off, const int32_t* adj, const float* e, const int32_t* cellPit, const int32_t* comp, const uint64_t* best, int32_t N, int32_t c,
                                 PassEdge* edge) {
    const uint64_t key = best[c];
    if (key == NO_PASS) return c;
    const uint32_t slot = (uint32_t)(key & 0xFFFFFFFFull);
    const int32_t lo = row_of(off, N, slot), hi = adj[slot];
    const bool loMine = comp[cellPit[lo]] == c;
    const int32_t u = loMine ? lo : hi, v = loMine ? hi : lo;
    const int32_t co = comp[cellPit[v]];
    if (best[co] == key && c < co) return c;
    *edge = PassEdge{u, v, cellPit[u], cellPit[v], e[u], e[v]};
    return co;
}

// steps 5 and 6 for one cell; spillTo[i], W[i]: of pit i (-1 and a NaN for an endorheic basin)
struct Applied { int32_t receiver; float lake; };
WO_IMP_HD inline Applied apply_cell(int32_t r, float er, int32_t receiver, int32_t basin, int32_t pit, int32_t numPits, const int32_t* spillTo, const float* W) {
    Applied a{receiver, quiet_nan()};
    if (pit < 0 || pit >= numPits || spillTo[pit] < 0) return a;
    if (basin == r) a.receiver = spillTo[pit];
    if (er < W[pit]) a.lake = W[pit];
    return a;
}

// the river cells (see "Lines and tint")
WO_IMP_HD inline bool river_cell(float er, uint64_t D, uint64_t minQ, int32_t receiver, int32_t basin, int32_t r, float lake) {
    return is_land(er) && D >= minQ && receiver >= 0 && basin != r && lake != lake;
}
WO_IMP_HD inline bool tinted_cell(float er, uint64_t D, uint64_t minQ, int32_t receiver, int32_t basin, int32_t r, float lake) {
    return lake == lake || river_cell(er, D, minQ, receiver, basin, r, lake);
}
WO_IMP_HD inline void river_segment(const float* xyz, const float* e, int32_t r, int32_t to, float out[6]) {
    const double d1 = G::disp(e[r], LINE_BASE), d2 = G::disp(e[to], LINE_BASE);
    for (int a = 0; a < 3; ++a) {
        out[a] = (float)((double)xyz[3 * (int64_t)r + a] * d1);
        out[3 + a] = (float)((double)xyz[3 * (int64_t)to + a] * d2);
    }
}

// Step 4's rooting: the chosen passes (a forest on the pits and the drained class, node numPits) walked from the drained class.
// -> spillTo[i], W[i] per pit (-1, NaN where the walk does not come), and the number of basins it reached.  Host code.
inline int32_t resolve_spills(int32_t numPits, const std::vector<PassEdge>& edges, std::vector<int32_t>& spillTo, std::vector<float>& W) {
    const int32_t nodes = numPits + 1;
    std::vector<int32_t> head((size_t)nodes + 1, 0), list(2 * edges.size()), queue;
    for (const PassEdge& g : edges) { ++head[(size_t)g.pu + 1]; ++head[(size_t)g.pv + 1]; }
    for (int32_t i = 0; i < nodes; ++i) head[(size_t)i + 1] += head[i];
    std::vector<int32_t> fill(head.begin(), head.end() - 1);
    for (size_t k = 0; k < edges.size(); ++k) { list[fill[edges[k].pu]++] = (int32_t)k; list[fill[edges[k].pv]++] = (int32_t)k; }
    spillTo.assign((size_t)numPits, -1);
    W.assign((size_t)numPits, quiet_nan());
    std::vector<uint8_t> seen((size_t)nodes, 0);
    seen[numPits] = 1;
    queue.push_back(numPits);
    int32_t spilled = 0;
    for (size_t at = 0; at < queue.size(); ++at) {
        const int32_t a = queue[at];
        for (int32_t k = head[a]; k < head[(size_t)a + 1]; ++k) {
            const PassEdge& g = edges[list[k]];
            const bool uInA = g.pu == a;
            const int32_t b = uInA ? g.pv : g.pu;
            if (seen[b]) continue;
            seen[b] = 1;
            const int32_t v = uInA ? g.u : g.v;              // the resolved end
            const float ev = uInA ? g.eu : g.ev;
            const float level = g.eu > g.ev ? g.eu : g.ev;
            spillTo[b] = v;
            W[b] = (a != numPits && ev < W[a]) ? W[a] : level;
            ++spilled;
            queue.push_back(b);
        }
    }
    return spilled;
}

}  // namespace rivers
}  // namespace wo
