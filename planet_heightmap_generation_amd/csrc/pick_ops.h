// The editor's hit test and highlights (js/edit-mode.js:18-93, js/planet-mesh.js:953-1244): bodies shared by the device kernels
// (pick.hip, globe.hip, map.hip), the host front ends (api_host.cc) and the test-only CPU emulator (tests/emu_editor), so that all
// of them compile the very same arithmetic.
//
// Contract (bit-identical to the reference):
//   * findNearestRegion (:18-28): dot = nx * x + ny * y + nz * z in double on the f32 position, left to right, no contraction.  The
//     loop starts at bestDot = -2 and takes a region when dot > bestDot: what it leaves is the LOWEST index among the regions whose
//     dot equals the maximum of the dots above -2.  The comparison is by value: -0 equals +0, a NaN dot never wins.  No dot above -2:
//     region -1, dot -2.
//   * The reduction form keeps the pair (dot, index).  `beats` is its comparator: greater dot, or equal dot and lower index; an entry
//     with index -1 loses to anything.  It is a total order on the valid entries (their dots are above -2 and never NaN) with the
//     invalid entry at the bottom, so any reduction tree gives the loop's answer.  A 64-bit key on the bits of the dot would not do:
//     the key needs 96 bits, and bit order disagrees with value order at +-0.
//   * direction_globe (getHitInfoGlobe, :43-59) and direction_map (getHitInfoMap, :77-92) give the direction that reaches
//     findNearestRegion, or nothing (the reference's `return null`).  As in the reference a NaN passes both validity tests and reaches
//     the loop, which answers it with no region.  Math.sin / Math.cos are the fdlibm ports of import_ops.h (their domain: |x| below
//     about 1.6e6, NaN beyond it).
//   * The class byte of a region (class_of) and the three tints (tint): pending, then plate hover, then Koppen hover, every step
//     stored as f32 as the reference's Float32Array does between updatePendingHighlight, updateHoverHighlight and
//     updateKoppenHoverHighlight.  Double arithmetic on the f32 value; Math.min is map_ops.h's js_min, so NaN propagates.
#pragma once
#include <cmath>
#include <cstdint>

#include "import_ops.h"
#include "map_ops.h"

namespace wo {
namespace pick {

constexpr int TILE = 16;                    // queries one pass over the positions serves
constexpr int32_t MAX_QUERIES = 65536;
constexpr double NO_DOT = -2.0;             // the loop's start value, and the dot of "no region"
constexpr double GLOBE_RADIUS = 1.08;       // js/edit-mode.js:47
constexpr double PI = 3.141592653589793;

enum : uint8_t { CLS_PENDING_OCEAN = 1, CLS_PENDING_LAND = 2, CLS_HOVER_PLATE = 4, CLS_HOVER_KOPPEN = 8 };

struct Best { double dot; int32_t idx; };
WO_IMP_HD inline Best best_none() { return Best{NO_DOT, -1}; }

WO_IMP_HD inline double dot_of(double nx, double ny, double nz, float x, float y, float z) { return nx * (double)x + ny * (double)y + nz * (double)z; }
// the loop's step: regions must come in ascending order
WO_IMP_HD inline void take_in_order(Best& b, double dot, int32_t r) {
    if (dot > b.dot) { b.dot = dot; b.idx = r; }
}
// the reduction's comparator: does a beat b?
WO_IMP_HD inline bool beats(Best a, Best b) {
    if (a.idx < 0) return false;
    if (b.idx < 0) return true;
    return a.dot > b.dot || (a.dot == b.dot && a.idx < b.idx);
}
WO_IMP_HD inline Best better_of(Best a, Best b) {
    const bool take = beats(b, a);
    return Best{take ? b.dot : a.dot, take ? b.idx : a.idx};  // by value and field by field: the pair stays in registers
}

WO_IMP_HD inline void direction_nan(double out[3]) {
    const double n = __builtin_nan("");
    out[0] = n; out[1] = n; out[2] = n;
}
// ray: origin xyz, direction xyz (normalised by the caller, as three's Ray is); false: no hit, out is NaN
WO_IMP_HD inline bool direction_globe(const double ray[6], double out[3]) {
    const double ox = ray[0], oy = ray[1], oz = ray[2], dx = ray[3], dy = ray[4], dz = ray[5];
    const double R = GLOBE_RADIUS;
    const double b = 2.0 * (ox * dx + oy * dy + oz * dz);
    const double c = ox * ox + oy * oy + oz * oz - R * R;
    const double disc = b * b - 4.0 * c;
    if (disc < 0.0) { direction_nan(out); return false; }
    const double t = (-b - std::sqrt(disc)) * 0.5;
    if (t < 0.0) { direction_nan(out); return false; }
    const double hx = ox + t * dx, hy = oy + t * dy, hz = oz + t * dz;
    double len = std::sqrt(hx * hx + hy * hy + hz * hz);
    if (len == 0.0 || len != len) len = 1.0;                  // `|| 1`
    out[0] = hx / len; out[1] = hy / len; out[2] = hz / len;
    return true;
}
// point: wx, wy on the map plane (the map is 4 x 2 units, sx = 2 / PI); false: outside the map, out is NaN
WO_IMP_HD inline bool direction_map(double wx, double wy, double centerLon, double out[3]) {
    const double sx = 2.0 / PI;
    const double center = (centerLon == 0.0 || centerLon != centerLon) ? 0.0 : centerLon;     // `|| 0`
    double lon = wx / sx + center;
    const double lat = wy / sx;
    if (lat < -PI / 2.0 || lat > PI / 2.0) { direction_nan(out); return false; }
    if (lon > PI) lon -= 2.0 * PI;
    else if (lon < -PI) lon += 2.0 * PI;
    const double cosLat = imp::fd_cos(lat);
    out[0] = cosLat * imp::fd_sin(lon);
    out[1] = imp::fd_sin(lat);
    out[2] = cosLat * imp::fd_cos(lon);
    return true;
}

// kind: one byte per region id, 0 not pending, CLS_PENDING_OCEAN or CLS_PENDING_LAND for a pending plate of that id; koppen may be
// nullptr with hoveredKoppen < 0.  A pid outside [0, N) matches nothing.
WO_IMP_HD inline uint8_t class_of(int32_t pid, int32_t N, const uint8_t* kind, int32_t hoveredPlate, const uint8_t* koppen, int32_t r, int32_t hoveredKoppen) {
    uint8_t c = 0;
    if (pid >= 0 && pid < N) {
        c |= kind[pid];
        if (hoveredPlate >= 0 && pid == hoveredPlate) c |= CLS_HOVER_PLATE;
    }
    if (hoveredKoppen >= 0 && (int32_t)koppen[r] == hoveredKoppen) c |= CLS_HOVER_KOPPEN;
    return c;
}

WO_IMP_HD inline float tint_scale(float v) { return (float)((double)v * 0.7); }
WO_IMP_HD inline float tint_lift(float v, double by) { return (float)map::js_min(1.0, (double)v + by); }
WO_IMP_HD inline map::Rgb tint(map::Rgb c, uint8_t cls) {
    if (cls & CLS_PENDING_OCEAN) { c.r = tint_scale(c.r); c.g = tint_lift(c.g, 0.25); c.b = tint_scale(c.b); }
    else if (cls & CLS_PENDING_LAND) { c.r = tint_scale(c.r); c.g = tint_scale(c.g); c.b = tint_lift(c.b, 0.25); }
    if (cls & CLS_HOVER_PLATE) { c.r = tint_lift(c.r, 0.22); c.g = tint_lift(c.g, 0.22); c.b = tint_lift(c.b, 0.22); }
    if (cls & CLS_HOVER_KOPPEN) { c.r = tint_lift(c.r, 0.22); c.g = tint_lift(c.g, 0.22); c.b = tint_lift(c.b, 0.22); }
    return c;
}

}  // namespace pick
}  // namespace wo
