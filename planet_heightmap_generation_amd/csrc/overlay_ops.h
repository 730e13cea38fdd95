// The arrow overlays of the wind and ocean-current views (the reference's buildWindArrows and buildOceanCurrentArrows,
// js/planet-mesh.js:1289-1465, :1545-1720): the per-region and per-bin bodies shared by the device kernels (overlay.hip) and the
// test-only CPU emulator (tests/emu_overlay), so that both compile the very same arithmetic.  The library compiles with
// -ffp-contract=off: no FMA changes a result.  The reference defines these buffers by plain double arithmetic on f32 inputs, stored
// into Float32Arrays, so the contract is bit equality with its arrays.
//
// Bins (:1325-1345, :1584-1607).  Every region r in index order: lat = asin(max(-1, min(1, y))), lon = atan2(x, z) (V8's fdlibm,
//   import_ops.h), li = max(0, min(59, floor((lat + PI / 2) / (3 * DEG)))), lo = max(0, min(119, floor((lon + PI) / (3 * DEG)))),
//   the centre of the 3 x 3 degree cell, d2 = dlat * dlat + dlon * dlon, all in double.  A NaN lat or lon gives a NaN index: the
//   region takes part in no bin.  With skipLand (the ocean form) a region with r_elevation > 0 takes part in none; a NaN does.
//   The reference keeps per bin `gridDist2`, a Float32Array that starts at 1e9, and `gridRegions`: a region wins when its double d2
//   is below the stored f32, which then becomes fround(d2).  What its loop leaves is: with m the minimum of fround(d2) over the bin's
//   members, the HIGHEST index among the members with fround(d2) == m and d2 < m (their d2 rounded up, so each of them beats the
//   value the one before it stored) if there is one, otherwise the LOWEST index with fround(d2) == m.  (Stored values never rise;
//   the first member with fround(d2) == m brings the stored value to m, since every f32 above m is above its d2; after that only a
//   d2 < m wins, and such a d2 rounds to m.)  That is the minimum of one 64-bit key per region: the bits of fround(d2) in the high
//   word (d2 >= +0, so the bits order as the values), and below them class 0 with the complemented index for a d2 that rounded up,
//   class 1 with the index otherwise.  A minimum is exact whatever the order, so one atomicMin per candidate gives the loop's
//   winner.  tests/test_overlays.py holds the key form against the loop.
// Arrows (:1356-1465, :1618-1720).  Every bin in ascending index with a winner r >= 0 whose speed is not below the threshold
//   (wind: sqrt(we * we + wn * wn) < 0.001; ocean: r_ocean_speed[r] < 0.01; a NaN speed is kept) gives four runs of 18 floats: the
//   shaft and the two wings of the arrowhead on the globe, their colours, the same on the map, their colours.  `x || 1` is 1 for
//   +0, -0 and NaN.  cosA and sinA are fdlibm's of 25 * DEG.  The map form subtracts centerLon || 0 and wraps once (:1434-1435).
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>

#include "map_ops.h"

namespace wo {
namespace overlay {

namespace M = wo::map;

enum : int32_t { KIND_WIND = 0, KIND_OCEAN = 1 };                        // WO_OVERLAY_WIND, WO_OVERLAY_OCEAN of worogen.h
constexpr int32_t LAT_BANDS = 60, LON_BANDS = 120, BINS = LAT_BANDS * LON_BANDS;
constexpr int32_t ARROW_FLOATS = 18;                                     // three segments of two vertices
constexpr double PI = 3.141592653589793, DEG = PI / 180;
constexpr unsigned long long EMPTY_KEY = ~0ull;

// ---- bins ---------------------------------------------------------------------------------------------------------------------
struct Bin { int32_t idx; double d2; };                                  // idx < 0: the region takes part in no bin

WO_IMP_HD inline Bin bin_of(float x, float y, float z) {
    const double lat = imp::fd_asin(M::js_max(-1.0, M::js_min(1.0, (double)y)));
    const double lon = imp::fd_atan2((double)x, (double)z);
    if (lat != lat || lon != lon) return Bin{-1, 0.0};
    const double li = M::js_max(0.0, M::js_min((double)(LAT_BANDS - 1), floor((lat + PI / 2) / (3 * DEG))));
    const double lo = M::js_max(0.0, M::js_min((double)(LON_BANDS - 1), floor((lon + PI) / (3 * DEG))));
    const double cellLat = (-90 + li * 3 + 3 * 0.5) * DEG;
    const double cellLon = (-180 + lo * 3 + 3 * 0.5) * DEG;
    const double dlat = lat - cellLat, dlon = lon - cellLon;
    return Bin{(int32_t)li * LON_BANDS + (int32_t)lo, dlat * dlat + dlon * dlon};
}
// whether the region is a candidate at all: the ocean form's `if (r_elevation[r] > 0) continue`
WO_IMP_HD inline bool takes_part(bool skipLand, float elevation) { return !(skipLand && elevation > 0.0f); }

// the key of a candidate; EMPTY_KEY for a d2 that could not win against the initial 1e9
WO_IMP_HD inline unsigned long long key_of(double d2, int32_t r) {
    if (!(d2 < (double)1e9f)) return EMPTY_KEY;
    const float f = (float)d2;
    const uint32_t low = d2 < (double)f ? (0x7FFFFFFFu - (uint32_t)r) : (0x80000000u | (uint32_t)r);
    uint32_t bits;
    memcpy(&bits, &f, 4);
    return ((unsigned long long)bits << 32) | low;
}
WO_IMP_HD inline int32_t winner_of_key(unsigned long long key) {
    if (key == EMPTY_KEY) return -1;
    const uint32_t low = (uint32_t)key;
    return (low & 0x80000000u) ? (int32_t)(low & 0x7FFFFFFFu) : (int32_t)(0x7FFFFFFFu - low);
}

// ---- arrows -------------------------------------------------------------------------------------------------------------------
WO_IMP_HD inline double or_one(double v) { return (v != v || v == 0.0) ? 1.0 : v; }      // v || 1

// what an arrow reads of its region: the vector (wind east / north, current east / north), the ocean form's stored speed and warmth
struct Source { float a, b, speed, warmth; };

WO_IMP_HD inline double speed_of(int32_t kind, const Source& s) {
    if (kind == KIND_OCEAN) return (double)s.speed;
    const double we = (double)s.a, wn = (double)s.b;
    return sqrt(we * we + wn * wn);
}
WO_IMP_HD inline bool is_slow(int32_t kind, double speed) { return kind == KIND_OCEAN ? speed < 0.01 : speed < 0.001; }

WO_IMP_HD inline void arrow_color(int32_t kind, double speed, float warmth, double c[3]) {
    if (kind == KIND_OCEAN) {
        const double w = (double)warmth;
        if (w > 0.1) { c[0] = 0.9; c[1] = 0.15; c[2] = 0.15; }
        else if (w < -0.1) { c[0] = 0.15; c[1] = 0.3; c[2] = 0.9; }
        else { c[0] = 0.5; c[1] = 0.5; c[2] = 0.5; }
        return;
    }
    const double t = M::js_min(1.0, speed * 3);
    if (t < 0.5) {
        const double s = t * 2;
        c[0] = s; c[1] = s; c[2] = 1 - s * 0.5;
    } else {
        const double s = (t - 0.5) * 2;
        c[0] = 1; c[1] = 1 - s; c[2] = 0.5 - s * 0.5;
    }
}

// the four runs of one arrow; any of them may be nullptr.  centerLon is the caller's state.mapCenterLon.
WO_IMP_HD inline void arrow(int32_t kind, const float p[3], const Source& src, double centerLon, float* globePos, float* globeCol, float* mapPos, float* mapCol) {
    const bool ocean = kind == KIND_OCEAN;
    const double we = (double)src.a, wn = (double)src.b, speed = speed_of(kind, src);
    const double x = (double)p[0], y = (double)p[1], z = (double)p[2];
    const double HEAD_FRAC = 0.35, cosA = imp::fd_cos(25 * DEG), sinA = imp::fd_sin(25 * DEG);
    const double cap = ocean ? 0.014 : 0.012;
    double c[3];
    arrow_color(kind, speed, src.warmth, c);
    if (globeCol) for (int k = 0; k < ARROW_FLOATS; ++k) globeCol[k] = (float)c[k % 3];
    if (mapCol) for (int k = 0; k < ARROW_FLOATS; ++k) mapCol[k] = (float)c[k % 3];
    if (globePos) {
        double ex = z, ey = 0, ez = -x;
        const double elen = sqrt(ex * ex + ez * ez);
        if (elen > 1e-10) { ex /= elen; ez /= elen; }
        else { ex = 1; ez = 0; }
        double nx = y * ez - z * ey;
        double ny = z * ex - x * ez;
        double nz = x * ey - y * ex;
        const double nlen = or_one(sqrt(nx * nx + ny * ny + nz * nz));
        nx /= nlen; ny /= nlen; nz /= nlen;
        const double dirX = we * ex + wn * nx;
        const double dirY = we * ey + wn * ny;
        const double dirZ = we * ez + wn * nz;
        const double dirLen = or_one(sqrt(dirX * dirX + dirY * dirY + dirZ * dirZ));
        const double dxn = dirX / dirLen, dyn = dirY / dirLen, dzn = dirZ / dirLen;
        double px = y * dzn - z * dyn;
        double py = z * dxn - x * dzn;
        double pz = x * dyn - y * dxn;
        const double plen = or_one(sqrt(px * px + py * py + pz * pz));
        px /= plen; py /= plen; pz /= plen;
        const double arrowLen = (ocean ? 0.006 : 0.008) + M::js_min(cap, speed * 0.025);
        const double R = 1.007;
        const double ox = x * R, oy = y * R, oz = z * R;
        const double tx = ox + dxn * arrowLen;
        const double ty = oy + dyn * arrowLen;
        const double tz = oz + dzn * arrowLen;
        const double hLen = arrowLen * HEAD_FRAC;
        const double lwx = tx + (-dxn * cosA + px * sinA) * hLen;
        const double lwy = ty + (-dyn * cosA + py * sinA) * hLen;
        const double lwz = tz + (-dzn * cosA + pz * sinA) * hLen;
        const double rwx = tx + (-dxn * cosA - px * sinA) * hLen;
        const double rwy = ty + (-dyn * cosA - py * sinA) * hLen;
        const double rwz = tz + (-dzn * cosA - pz * sinA) * hLen;
        const double v[ARROW_FLOATS] = {ox, oy, oz, tx, ty, tz, tx, ty, tz, lwx, lwy, lwz, tx, ty, tz, rwx, rwy, rwz};
        for (int k = 0; k < ARROW_FLOATS; ++k) globePos[k] = (float)v[k];
    }
    if (mapPos) {
        const double sx = 2 / PI;
        double lon = imp::fd_atan2(x, z) - ((centerLon != centerLon || centerLon == 0.0) ? 0.0 : centerLon);
        if (lon > PI) lon -= 2 * PI; else if (lon < -PI) lon += 2 * PI;
        const double lat = imp::fd_asin(M::js_max(-1.0, M::js_min(1.0, y)));
        const double mx = lon * sx;
        const double my = lat * sx;
        const double norm = ocean ? or_one(sqrt(we * we + wn * wn)) : or_one(speed);
        const double arrowLen = 0.006 + M::js_min(cap, speed * 0.025);
        const double dx = (we / norm) * arrowLen;
        const double dy = (wn / norm) * arrowLen;
        const double tipX = mx + dx, tipY = my + dy;
        const double hLen = arrowLen * HEAD_FRAC;
        const double dLen = or_one(sqrt(dx * dx + dy * dy));
        const double ndx = -dx / dLen, ndy = -dy / dLen;
        const double lx = tipX + (ndx * cosA - ndy * sinA) * hLen;
        const double ly = tipY + (ndx * sinA + ndy * cosA) * hLen;
        const double rx = tipX + (ndx * cosA + ndy * sinA) * hLen;
        const double ry = tipY + (-ndx * sinA + ndy * cosA) * hLen;
        const double Z = 0.002;
        const double v[ARROW_FLOATS] = {mx, my, Z, tipX, tipY, Z, tipX, tipY, Z, lx, ly, Z, tipX, tipY, Z, rx, ry, Z};
        for (int k = 0; k < ARROW_FLOATS; ++k) mapPos[k] = (float)v[k];
    }
}

}  // namespace overlay
}  // namespace wo
