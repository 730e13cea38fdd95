// Region outlines as ordered closed rings (ours: the reference draws no outline but the loose super-plate border segments): the
// per-cell, per-side and per-slot bodies shared by the device kernels (outline.hip) and the test-only CPU emulator
// (tests/emu_outline), so that both compile the very same arithmetic.  Everything but the positions is integer arithmetic: every
// output is defined bit for bit.
//
// The mesh is a closed triangulation: halfedges has no -1, halfedges[halfedges[s]] == s, and every Voronoi vertex (triangle centre)
//   has exactly three cells around it, so two cells never touch in a point only.
// Notation.  For side s: t = s / 3, next(s) = 3 t + (s + 1) % 3, prev(s) = 3 t + (s + 2) % 3, h = halfedges[s], a = triangles[s]
//   (the side's own cell, whose fan globe_ops.h builds from s), b = triangles[h], it(s) = s / 3, ot(s) = h / 3.  The Voronoi edge of
//   s runs from the centre of it to the centre of ot: the order in which next(halfedges[.]) circulates around a.
// Classes.  One int32 per cell, from a source: COAST e > 0 ? 1 : 0 (a NaN is ocean, as disp treats it); LAKES 1 where the lake
//   level is no NaN; KOPPEN the class byte; LEVELS the number of levels[k] <= e for at most 32 finite, strictly ascending levels (a
//   NaN is class 0); VALUES the caller's own.
// Boundary sides.  s is one iff class[a] != class[b], and with onlyClass >= 0 also class[a] == onlyClass.  With onlyClass == -1
//   every undirected boundary edge appears twice, once per class, in opposite directions.  A ring keeps its class on the side of a.
// Successor, with c = class[a]: d = triangles[prev(h)]; succ(s) = class[d] != c ? next(h) : prev(h).
// Predecessor: e = triangles[prev(s)]; pred(s) = class[e] != c ? halfedges[prev(s)] : halfedges[next(s)].
//   Both are boundary sides of class c, ot(s) == it(succ(s)), and pred(succ(s)) == s: the boundary sides form a permutation whose
//   cycles are the rings.
// Rings.  The boundary sides in ascending order take the slots 0 .. M - 1.  A ring is a cycle of succ; its leader is its lowest
//   slot; rings are numbered by ascending leader; inside a ring the order is succ from the leader on.
// Ranking: pointer doubling over the slots.  After k rounds slot i knows jump = succ^(2^k)(i), the least slot of the window
//   i, succ(i), .., succ^(2^k - 1)(i), and the forward distance to its first occurrence there.  A round joins the window of i with
//   that of jump; on a tie the first half is kept: an equal minimum is the same slot met again after the window wrapped.  After
//   K = ceil(log2(max(M, 2))) rounds the window holds the whole ring: least is the leader, dist the distance `off` to it.
//   len = off[succ[leader]] + 1 and rank = (len - off) % len.  A round reads what the round before wrote for other slots: the
//   caller ping-pongs two buffers.
// Vertices.  The vertex of entry k is the centre of triangle it(sides[k]): t_xyz[it] * disp(t_e[it], base) with globe_ops.h's
//   center_of and disp (base 0: t_xyz itself), or map_ops.h's lonlat_of_center.  A ring is closed implicitly.
#pragma once
#include <cstdint>

#include "globe_ops.h"
#include "map_ops.h"

namespace wo {
namespace outline {

enum : int32_t { SOURCE_COAST = 0, SOURCE_LAKES = 1, SOURCE_KOPPEN = 2, SOURCE_LEVELS = 3, SOURCE_VALUES = 4, SOURCE_COUNT = 5 };   // WO_OUTLINE_* of worogen.h
constexpr int32_t MAX_LEVELS = 32;

struct Levels { float v[MAX_LEVELS]; int32_t n; };                       // a kernel argument: 132 bytes

// ---- classes ------------------------------------------------------------------------------------------------------------------
WO_IMP_HD inline int32_t class_coast(float e) { return e > 0.0f ? 1 : 0; }
WO_IMP_HD inline int32_t class_lake(float lakeLevel) { return lakeLevel == lakeLevel ? 1 : 0; }
WO_IMP_HD inline int32_t class_levels(float e, const Levels& L) {
    int32_t c = 0;
    for (int32_t k = 0; k < L.n; ++k) c += L.v[k] <= e ? 1 : 0;
    return c;
}
// at most MAX_LEVELS, finite, strictly ascending; -> the index of the first offender, -1 when all is well
inline int32_t levels_offender(const float* levels, int32_t n) {
    for (int32_t k = 0; k < n; ++k) {
        if (!(levels[k] - levels[k] == 0.0f)) return k;
        if (k > 0 && !(levels[k - 1] < levels[k])) return k;
    }
    return -1;
}

// ---- sides --------------------------------------------------------------------------------------------------------------------
WO_IMP_HD inline int32_t next_side(int32_t s) { return s - s % 3 + (s + 1) % 3; }
WO_IMP_HD inline int32_t prev_side(int32_t s) { return s - s % 3 + (s + 2) % 3; }

WO_IMP_HD inline bool is_boundary(const int32_t* triangles, const int32_t* halfedges, const int32_t* cls, int32_t onlyClass, int32_t s) {
    const int32_t c = cls[triangles[s]];
    return c != cls[triangles[halfedges[s]]] && (onlyClass < 0 || c == onlyClass);
}
WO_IMP_HD inline int32_t succ_side(const int32_t* triangles, const int32_t* halfedges, const int32_t* cls, int32_t s) {
    const int32_t h = halfedges[s], c = cls[triangles[s]];
    return cls[triangles[prev_side(h)]] != c ? next_side(h) : prev_side(h);
}
WO_IMP_HD inline int32_t pred_side(const int32_t* triangles, const int32_t* halfedges, const int32_t* cls, int32_t s) {
    const int32_t c = cls[triangles[s]];
    return cls[triangles[prev_side(s)]] != c ? halfedges[prev_side(s)] : halfedges[next_side(s)];
}

// ---- ranking ------------------------------------------------------------------------------------------------------------------
struct alignas(16) Rank { int32_t jump, least, dist, pad; };             // one 16-byte load per gather

WO_IMP_HD inline Rank rank_start(int32_t slot, int32_t succSlot) { return Rank{succSlot, slot, 0, 0}; }
// mine: the state of a slot after k rounds, far: the state of mine.jump after k rounds, span = 2^k
WO_IMP_HD inline Rank rank_round(const Rank& mine, const Rank& far, int32_t span) {
    Rank r{far.jump, mine.least, mine.dist, 0};
    if (far.least < mine.least) { r.least = far.least; r.dist = span + far.dist; }
    return r;
}
WO_IMP_HD inline int32_t rank_rounds(int32_t M) {
    int32_t k = 1;
    while ((int64_t)1 << k < (int64_t)M) ++k;                            // ceil(log2(max(M, 2)))
    return k;
}
WO_IMP_HD inline int32_t rank_in_ring(int32_t len, int32_t off) { return (len - off) % len; }

// ---- vertices -----------------------------------------------------------------------------------------------------------------
// corners: three cells per entry, the corners of triangle it(sides[k])
WO_IMP_HD inline void vertex_position(const int32_t* corners, const float* r_xyz, const float* r_elevation, int64_t k, double base, float out[3]) {
    const globe::Center c = globe::center_of(corners, r_xyz, r_elevation, k);
    if (base == 0.0) { out[0] = c.x; out[1] = c.y; out[2] = c.z; return; }
    const double d = globe::disp(c.e, base);
    out[0] = (float)((double)c.x * d); out[1] = (float)((double)c.y * d); out[2] = (float)((double)c.z * d);
}
WO_IMP_HD inline map::LonLat vertex_lonlat(const int32_t* corners, const float* r_xyz, int64_t k) { return map::lonlat_of_center(corners, r_xyz, k); }

}  // namespace outline
}  // namespace wo
