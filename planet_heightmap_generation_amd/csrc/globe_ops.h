// The globe mesh (the reference's buildMesh, updateMeshColors and updateSuperPlateBorders, js/planet-mesh.js:620-836, :840-957,
// :533-576): the per-triangle, per-side and per-word bodies shared by the device kernels (globe.hip) and the test-only CPU emulator
// (tests/emu_globe), so that both compile the very same arithmetic.  The library compiles with -ffp-contract=off: no FMA changes a
// result.  The reference defines these buffers, plain arithmetic in double on f32 inputs stored into Float32Arrays, so the
// contract is bit equality with its arrays.
//
// Tables.  t_xyz is generateTriangleCenters' (map_ops.h: triangle_center), t_elevation is (e[a] + e[b] + e[c]) / 3 summed left to
//   right in double and stored as f32 (js/planet-worker.js:33-35).  One 16-byte record per triangle holds both.
// Positions (:661-708).  For every side s (the closing pole fan included): it = s / 3, ot = halfedges[s] / 3, br = triangles[s].
//   disp(e) = 1.0 + (e > 0 ? e * V : (e * V) * 0.3), V = 0.04, in double on the f32 elevation (waterLevel is 0; a NaN takes the
//   second branch and stays a NaN).  v0 = t_xyz[it] * disp(t_e[it]), v1 = t_xyz[ot] * disp(t_e[ot]), v2 = r_xyz[br] * disp(r_e[br]).
//   Winding (:693-704): e1 = v1 - v0, e2 = v2 - v0, n = e1 x e2, c = (v0 + v1 + v2) / 3, all in double on the double vertices, the
//   sums left to right; if n.x * c.x + n.y * c.y + n.z * c.z < 0 then v1 and v2 change places (a NaN never swaps).  Nine f32 stores
//   at 9 * s.
// Colours (:710-752, :912-921).  The colour of region br three times, nine f32 at 9 * s: the f32 values the reference hands to
//   three.js, no quantiser and no gamma table.  The colour functions are map_ops.h's and map_layer_ops.h's; for the plate view
//   (:734-736) plateColors[r_plate[br]], or (0.3, 0.3, 0.3) for a plate the table does not hold.
// Lines.  Wireframe (:775-788): every side with s < halfedges[s] in ascending s gives one segment, the two centres t_xyz[it] and
//   t_xyz[ot] scaled by base + (t_e > 0 ? t_e * V : (t_e * V) * 0.3) with base 1.001, six f32.  Super-plate borders, globe form
//   (:551-567): the same with base 1.002 for the sides that also have sp[triangles[s]] !== sp[triangles[halfedges[s]]]; sp is a
//   Float32Array, so the test is the float one: NaN differs from everything, -0 equals +0.
// Bounds.  Per axis the minimum and the maximum of the stored f32 positions, NaN skipped, ordered by the sign-magnitude key
//   (-0 < +0).  A bound is a maximum over uint32 words that start at 0, the maximum's over the keys, the minimum's over their
//   complements: exact, so any reduction tree gives the same bits.  Both bounds of an axis with nothing but NaN are 0.
#pragma once
#include <cstdint>

#include "map_layer_ops.h"
#include "map_ops.h"

namespace wo {
namespace globe {

namespace M = wo::map;

enum : int32_t { SOURCE_TYPE = 0, SOURCE_LAYER = 1 };                    // WO_GLOBE_SOURCE_* of worogen.h
enum : int32_t { LINES_WIREFRAME = 0, LINES_SUPER_PLATE_BORDERS = 1 };   // WO_GLOBE_LINES_*

constexpr double V = 0.04, BASE_MESH = 1.0, BASE_WIREFRAME = 1.001, BASE_BORDERS = 1.002;

// ---- tables -------------------------------------------------------------------------------------------------------------------
struct Center { float x, y, z, e; };                                     // t_xyz and t_elevation of one triangle

WO_IMP_HD inline float triangle_elevation(const int32_t* triangles, const float* r_elevation, int64_t t) {
    double s = (double)r_elevation[triangles[3 * t]] + (double)r_elevation[triangles[3 * t + 1]];
    s = s + (double)r_elevation[triangles[3 * t + 2]];
    return (float)(s / 3.0);
}
WO_IMP_HD inline Center center_of(const int32_t* triangles, const float* r_xyz, const float* r_elevation, int64_t t) {
    float c[3];
    M::triangle_center(triangles, r_xyz, t, c);
    return Center{c[0], c[1], c[2], triangle_elevation(triangles, r_elevation, t)};
}

// ---- positions ----------------------------------------------------------------------------------------------------------------
WO_IMP_HD inline double disp(float elevation, double base) {
    const double e = (double)elevation;
    return base + (e > 0.0 ? e * V : e * V * 0.3);
}
// the same with v in the place of V: the globe view's exaggeration (view_ops.h: v = V * exaggeration; v == V gives disp's bits)
WO_IMP_HD inline double disp(float elevation, double base, double v) {
    const double e = (double)elevation;
    return base + (e > 0.0 ? e * v : e * v * 0.3);
}

// the nine floats of a side from its two centre records and its region, displaced with v in the place of V; returns whether the
// winding was swapped
WO_IMP_HD inline bool side_positions(const Center& a, const Center& b, const float r[3], float re, double v, float out[9]) {
    const double d0 = disp(a.e, BASE_MESH, v), d1 = disp(b.e, BASE_MESH, v), d2 = disp(re, BASE_MESH, v);
    const double v0x = (double)a.x * d0, v0y = (double)a.y * d0, v0z = (double)a.z * d0;
    double v1x = (double)b.x * d1, v1y = (double)b.y * d1, v1z = (double)b.z * d1;
    double v2x = (double)r[0] * d2, v2y = (double)r[1] * d2, v2z = (double)r[2] * d2;
    const double e1x = v1x - v0x, e1y = v1y - v0y, e1z = v1z - v0z;
    const double e2x = v2x - v0x, e2y = v2y - v0y, e2z = v2z - v0z;
    const double nx = e1y * e2z - e1z * e2y;
    const double ny = e1z * e2x - e1x * e2z;
    const double nz = e1x * e2y - e1y * e2x;
    const double cx = (v0x + v1x + v2x) / 3.0, cy = (v0y + v1y + v2y) / 3.0, cz = (v0z + v1z + v2z) / 3.0;
    const bool swap = nx * cx + ny * cy + nz * cz < 0.0;
    if (swap) {
        double t;
        t = v1x; v1x = v2x; v2x = t;
        t = v1y; v1y = v2y; v2y = t;
        t = v1z; v1z = v2z; v2z = t;
    }
    out[0] = (float)v0x; out[1] = (float)v0y; out[2] = (float)v0z;
    out[3] = (float)v1x; out[4] = (float)v1y; out[5] = (float)v1z;
    out[6] = (float)v2x; out[7] = (float)v2y; out[8] = (float)v2z;
    return swap;
}
// the globe mesh's own
WO_IMP_HD inline bool side_positions(const Center& a, const Center& b, const float r[3], float re, float out[9]) { return side_positions(a, b, r, re, V, out); }

// ---- lines --------------------------------------------------------------------------------------------------------------------
WO_IMP_HD inline double line_base(int32_t kind) { return kind == LINES_SUPER_PLATE_BORDERS ? BASE_BORDERS : BASE_WIREFRAME; }

// whether side s gives a segment; sp is read by the borders only
WO_IMP_HD inline bool side_has_segment(int32_t kind, const int32_t* triangles, const int32_t* halfedges, const float* sp, int64_t s) {
    const int64_t opp = halfedges[s];
    if (!(s < opp)) return false;
    return kind == LINES_SUPER_PLATE_BORDERS ? sp[triangles[s]] != sp[triangles[opp]] : true;
}
WO_IMP_HD inline void line_segment(const Center& a, const Center& b, double base, float out[6]) {
    const double d1 = disp(a.e, base), d2 = disp(b.e, base);
    out[0] = (float)((double)a.x * d1); out[1] = (float)((double)a.y * d1); out[2] = (float)((double)a.z * d1);
    out[3] = (float)((double)b.x * d2); out[4] = (float)((double)b.y * d2); out[5] = (float)((double)b.z * d2);
}

// ---- plate colours ------------------------------------------------------------------------------------------------------------
// slot: the row of plateColors that holds a region's plate, -1 where the table has none (slots are built per region id of the seeds)
WO_IMP_HD inline M::Rgb plate_color(int32_t plate, int32_t N, const int32_t* slotOfRegion, const float* plateColors) {
    const int32_t k = ((uint32_t)plate < (uint32_t)N) ? slotOfRegion[plate] : -1;
    if (k < 0) return M::Rgb{(float)0.3, (float)0.3, (float)0.3};
    return M::Rgb{plateColors[3 * (int64_t)k], plateColors[3 * (int64_t)k + 1], plateColors[3 * (int64_t)k + 2]};
}

// ---- bounds -------------------------------------------------------------------------------------------------------------------
// the order of floats as an order of uint32 keys: -inf < ... < -0 < +0 < ... < +inf; no key of a number is 0 or 0xFFFFFFFF
WO_IMP_HD inline uint32_t order_key(float v) {
    const uint32_t u = M::f32_bits(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
WO_IMP_HD inline float of_order_key(uint32_t k) { return M::f32_of_bits((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k); }

// w[axis]: the maximum of ~key (the minimum), w[3 + axis]: the maximum of key; 0: no number was taken
struct BoundsBits { uint32_t w[6]; };
WO_IMP_HD inline void bounds_take(BoundsBits& b, int axis, float v) {
    if (v != v) return;
    const uint32_t k = order_key(v);
    if (~k > b.w[axis]) b.w[axis] = ~k;
    if (k > b.w[3 + axis]) b.w[3 + axis] = k;
}
// -> min x, y, z, max x, y, z
WO_IMP_HD inline void bounds_decode(const uint32_t w[6], float out[6]) {
    for (int a = 0; a < 3; ++a) {
        out[a] = w[a] ? of_order_key(~w[a]) : 0.0f;
        out[3 + a] = w[3 + a] ? of_order_key(w[3 + a]) : 0.0f;
    }
}

}  // namespace globe
}  // namespace wo
