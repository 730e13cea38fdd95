// Equirectangular map export (the reference's exportMap / exportMapBatch, js/planet-mesh.js:1752-2180): the per-vertex, per-side,
// per-pixel and per-region bodies shared by the device kernels (map.hip, raster.hip) and the test-only CPU emulator (tests/emu_map), so that
// both compile the very same arithmetic.  The library compiles with -ffp-contract=off: no FMA changes a result.
//
// The reference draws its map triangles with WebGL, whose rasteriser (sub-pixel snapping, fill rule, float-to-UNORM rounding)
// differs between GPUs: there are no canonical reference pixels.  What the reference does define is reproduced bit for bit, the
// triangle list and the per-region colours; the remaining rules are fixed here.
//
// Geometry (:1776-1843, :1985-2031).  For every side s of the mesh (the closing pole fan included): it = s / 3, ot = halfedges[s] / 3,
//   br = triangles[s]; the vertices are t_xyz[it], t_xyz[ot], r_xyz[br], where t_xyz is generateTriangleCenters' (the sum left to
//   right in double, / 3, stored as f32).  lon = atan2(x, z), lat = asin(max(-1, min(1, y))) by the fdlibm ports of import_ops.h, in
//   double on the f32 inputs, once per region and once per triangle centre.  wraps = (maxLon - minLon) > pi: a wrapping side emits
//   two triangles, the first with every negative longitude raised by 2 pi, the second that triangle shifted by -2 pi; every other
//   side emits one.  Stored position: x = f32(clamp(lon * sx, -2, 2)), y = f32(clamp(lat * sx, -1, 1)), sx = 2 / pi in double.  The
//   clamp moves vertices and does not clip, as in the reference.
// Coverage.  The image is W x H, H = W / 2, row 0 north.  Centre of pixel (i, j): xc = -2 + 4 (i + 0.5) / W, yc = 1 - 2 (j + 0.5) / H
//   in double, in this order of operations.  For a triangle a, b, c (the f32 positions as doubles): area2 = (bx - ax)(cy - ay) -
//   (by - ay)(cx - ax), and the three edge functions have the same form against (xc, yc) in cyclic order.  area2 == 0 (or NaN) covers
//   nothing; otherwise the pixel is covered if all three edge functions are >= 0 (area2 > 0) or all <= 0 (area2 < 0): the
//   reference's material is double-sided.  The pixel belongs to the LOWEST side index that has a covering triangle; its region is
//   triangles[s], or -1 when nothing covers it.  The rule does not depend on thread order.
// Colour.  Per region the reference's colour function in double, stored as f32 as its Float32Array does: elevationToColor,
//   heightmapColor, landHeightmapColor, landMaskColor, koppenColor (an id outside the table takes class 0) and, for `biome`,
//   smoothBiomeColors (:30-59): biomeColor per region stored as f32, then raw * 0.65 + avg * 0.35 with the neighbour average summed
//   in CSR order in double; a region without neighbours keeps its raw colour.  Quantise: q = floor(c * 255 + 0.5) on the f32 value
//   (as a double) clamped to [0, 1], NaN gives 0.  Gamma: byte = LUT[q], LUT[k] the reference's own expression (:1908-1910) at
//   v = k / 255.  Alpha is 255 everywhere.
// Uncovered pixels: the three grey types get (0, 0, 0); the other three get LUT[q(SRGBToLinear(h / 255))] per channel h of 0x1a1a2e,
//   SRGBToLinear being three r160's.  This is OUR READING of what three r160 does with a hex background under colour management;
//   nobody has run it through WebGL.
// `biome` and `koppen` need Koppen ids.  The reference falls back silently to the colour map without them; that fallback is not
//   offered here: the entry point fails with "no Koppen result".
#pragma once
#include <cmath>
#include <cstdint>

#include "import_ops.h"

namespace wo {
namespace map {

enum : int32_t { TYPE_COLOR = 0, TYPE_HEIGHTMAP, TYPE_LANDHEIGHTMAP, TYPE_LANDMASK, TYPE_BIOME, TYPE_KOPPEN, TYPE_COUNT };
WO_IMP_HD inline bool type_is_grey(int32_t t) { return t == TYPE_HEIGHTMAP || t == TYPE_LANDHEIGHTMAP || t == TYPE_LANDMASK; }
WO_IMP_HD inline bool type_needs_koppen(int32_t t) { return t == TYPE_BIOME || t == TYPE_KOPPEN; }

constexpr uint32_t NO_SIDE = 0xFFFFFFFFu;
constexpr int64_t SMALL_BOX = 256;       // pixel boxes up to this size are walked by the side's own lane, larger ones by a workgroup

// Math.max / Math.min of two Numbers: NaN if either is; max(+0, -0) = +0, min(+0, -0) = -0
WO_IMP_HD inline double js_max(double a, double b) {
    if (a != a || b != b) return a + b;
    if (a == 0.0 && b == 0.0) return (imp::hi_word(a) < 0) ? b : a;
    return a > b ? a : b;
}
WO_IMP_HD inline double js_min(double a, double b) {
    if (a != a || b != b) return a + b;
    if (a == 0.0 && b == 0.0) return (imp::hi_word(a) < 0) ? a : b;
    return a < b ? a : b;
}

struct LonLat { double lon, lat; };

WO_IMP_HD inline LonLat lonlat_of(float x, float y, float z) {
    return LonLat{imp::fd_atan2((double)x, (double)z), imp::fd_asin(js_max(-1.0, js_min(1.0, (double)y)))};
}
// generateTriangleCenters (js/sphere-mesh.js:206-219) for triangle t, then its longitude and latitude
WO_IMP_HD inline void triangle_center(const int32_t* triangles, const float* r_xyz, int64_t t, float c[3]) {
    const int64_t a = triangles[3 * t], b = triangles[3 * t + 1], d = triangles[3 * t + 2];
    for (int k = 0; k < 3; ++k) {
        double s = (double)r_xyz[3 * a + k] + (double)r_xyz[3 * b + k];
        s = s + (double)r_xyz[3 * d + k];
        c[k] = (float)(s / 3.0);
    }
}
WO_IMP_HD inline LonLat lonlat_of_center(const int32_t* triangles, const float* r_xyz, int64_t t) {
    float c[3];
    triangle_center(triangles, r_xyz, t, c);
    return lonlat_of(c[0], c[1], c[2]);
}

struct Tri { float x[3], y[3]; };

// the one or two map triangles of a side from the longitudes and latitudes of its three vertices; returns how many
WO_IMP_HD inline int side_triangles(const LonLat v[3], Tri out[2]) {
    const double PI = 3.141592653589793, sx = 2.0 / PI;
    double lon[3] = {v[0].lon, v[1].lon, v[2].lon};
    const double maxLon = js_max(js_max(lon[0], lon[1]), lon[2]), minLon = js_min(js_min(lon[0], lon[1]), lon[2]);
    const bool wraps = (maxLon - minLon) > PI;
    if (wraps)
        for (int k = 0; k < 3; ++k) if (lon[k] < 0.0) lon[k] += 2.0 * PI;
    for (int k = 0; k < 3; ++k) {
        const float y = (float)js_max(-1.0, js_min(1.0, v[k].lat * sx));
        out[0].x[k] = (float)js_max(-2.0, js_min(2.0, lon[k] * sx));
        out[0].y[k] = y;
        if (wraps) {
            out[1].x[k] = (float)js_max(-2.0, js_min(2.0, (lon[k] - 2.0 * PI) * sx));
            out[1].y[k] = y;
        }
    }
    return wraps ? 2 : 1;
}

WO_IMP_HD inline double pixel_xc(int64_t i, int32_t W) { return -2.0 + 4.0 * ((double)i + 0.5) / (double)W; }
WO_IMP_HD inline double pixel_yc(int64_t j, int32_t H) { return 1.0 - 2.0 * ((double)j + 0.5) / (double)H; }

WO_IMP_HD inline double edge_fn(double ax, double ay, double bx, double by, double px, double py) {
    return (bx - ax) * (py - ay) - (by - ay) * (px - ax);
}
WO_IMP_HD inline double tri_area2(const Tri& t) { return edge_fn(t.x[0], t.y[0], t.x[1], t.y[1], t.x[2], t.y[2]); }
// area2 is tri_area2(t), neither 0 nor NaN
WO_IMP_HD inline bool tri_covers(const Tri& t, double area2, double xc, double yc) {
    const double e0 = edge_fn(t.x[0], t.y[0], t.x[1], t.y[1], xc, yc);
    const double e1 = edge_fn(t.x[1], t.y[1], t.x[2], t.y[2], xc, yc);
    const double e2 = edge_fn(t.x[2], t.y[2], t.x[0], t.y[0], xc, yc);
    return area2 > 0.0 ? (e0 >= 0.0 && e1 >= 0.0 && e2 >= 0.0) : (e0 <= 0.0 && e1 <= 0.0 && e2 <= 0.0);
}

// The pixels whose centres can lie in the triangle's bounding box, one pixel wider on every side than the arithmetic asks for (the
// exact test is tri_covers).  Returns false for a triangle that covers nothing.  Positions lie in [-2, 2] x [-1, 1].
struct Box { int32_t i0, i1, j0, j1; };      // inclusive
WO_IMP_HD inline bool tri_box(const Tri& t, double area2, int32_t W, int32_t H, Box& b) {
    if (!(area2 > 0.0 || area2 < 0.0)) return false;
    const double minx = fmin(fmin((double)t.x[0], (double)t.x[1]), (double)t.x[2]), maxx = fmax(fmax((double)t.x[0], (double)t.x[1]), (double)t.x[2]);
    const double miny = fmin(fmin((double)t.y[0], (double)t.y[1]), (double)t.y[2]), maxy = fmax(fmax((double)t.y[0], (double)t.y[1]), (double)t.y[2]);
    int64_t i0 = (int64_t)floor((minx + 2.0) * (double)W / 4.0 - 0.5) - 1, i1 = (int64_t)ceil((maxx + 2.0) * (double)W / 4.0 - 0.5) + 1;
    int64_t j0 = (int64_t)floor((1.0 - maxy) * (double)H / 2.0 - 0.5) - 1, j1 = (int64_t)ceil((1.0 - miny) * (double)H / 2.0 - 0.5) + 1;
    if (i0 < 0) i0 = 0;
    if (j0 < 0) j0 = 0;
    if (i1 > W - 1) i1 = W - 1;
    if (j1 > H - 1) j1 = H - 1;
    if (i0 > i1 || j0 > j1) return false;
    b = Box{(int32_t)i0, (int32_t)i1, (int32_t)j0, (int32_t)j1};
    return true;
}
WO_IMP_HD inline int64_t box_pixels(const Box& b) { return (int64_t)(b.i1 - b.i0 + 1) * (int64_t)(b.j1 - b.j0 + 1); }

// the longitudes and latitudes of side s's vertices from the two tables
WO_IMP_HD inline void side_vertices(const int32_t* triangles, const int32_t* halfedges, const LonLat* t_ll, const LonLat* r_ll, int64_t s, LonLat v[3]) {
    v[0] = t_ll[s / 3];
    v[1] = t_ll[halfedges[s] / 3];
    v[2] = r_ll[triangles[s]];
}

// The equirectangular projection as the shared raster (raster.hip) and the height pass (relief.hip) take it: the two tables, the size
// and the functions above under the names that cube::Projection (cube_ops.h) gives its own.  A side yields at most PIECES triangles:
// its triangle and, where it wraps, the seam copy.
struct Projection {
    static constexpr int PIECES = 2;
    using Side = Tri[PIECES];                                 // a side's vertices, as side_triangles leaves them
    using Word = uint32_t;                                    // the per-pixel word of the side map
    const LonLat* t_ll;
    const LonLat* r_ll;
    int32_t W, H;
    WO_IMP_HD int64_t pixels() const { return (int64_t)W * H; }
    // fetches side s; returns how many pieces it has
    WO_IMP_HD int vertices(const int32_t* triangles, const int32_t* halfedges, int64_t s, Side& v) const {
        LonLat ll[3];
        side_vertices(triangles, halfedges, t_ll, r_ll, s, ll);
        return side_triangles(ll, v);
    }
    // piece k of a side: its triangle, tri_area2 of it and its clipped box; false where nothing is drawn.  The map has one face, 0.
    WO_IMP_HD bool piece(const Side& v, int k, Tri& t, double& area2, Box& b, int32_t& f) const {
        t = v[k];
        area2 = tri_area2(t);
        f = 0;
        return tri_box(t, area2, W, H, b);
    }
    WO_IMP_HD void center(int32_t i, int32_t j, double& xc, double& yc) const { xc = pixel_xc(i, W); yc = pixel_yc(j, H); }
    WO_IMP_HD int64_t index(int32_t, int32_t i, int32_t j) const { return (int64_t)j * W + i; }      // in the side map
    // what side s leaves, under a minimum, at a pixel centre that its triangle covers: its index
    WO_IMP_HD Word word(const Side&, const Tri&, double, double, double, uint32_t s) const { return s; }
};

// ---- colours ----------------------------------------------------------------------------------------------------------------
struct Rgb { float r, g, b; };
WO_IMP_HD inline Rgb rgb_of(double r, double g, double b) { return Rgb{(float)r, (float)g, (float)b}; }

// js/color-map.js:7-12
WO_IMP_HD inline double elev_to_height_km(double elev) {
    if (elev <= 0.0) return elev * 10.0;
    const double t = js_min(elev, 1.0), t2 = t * t;
    return 6.0 * t2 * t2 * (5.0 - 4.0 * t);
}
// js/color-map.js:116-125
WO_IMP_HD inline void elevation_to_color(double e, double c[3]) {
    double t;
    if (e < -0.50) { c[0] = 0.04; c[1] = 0.06; c[2] = 0.30; return; }
    if (e < -0.10) { t = (e + 0.50) / 0.40; c[0] = 0.04 + t * 0.07; c[1] = 0.06 + t * 0.14; c[2] = 0.30 + t * 0.18; return; }
    if (e < 0.00) { t = (e + 0.10) / 0.10; c[0] = 0.11 + t * 0.19; c[1] = 0.20 + t * 0.22; c[2] = 0.48 + t * 0.12; return; }
    if (e < 0.03) { t = e / 0.03; c[0] = 0.72 + t * 0.08; c[1] = 0.68 - t * 0.02; c[2] = 0.46 - t * 0.10; return; }
    if (e < 0.25) { t = (e - 0.03) / 0.22; c[0] = 0.20 - t * 0.06; c[1] = 0.54 - t * 0.12; c[2] = 0.12 + t * 0.08; return; }
    if (e < 0.50) { t = (e - 0.25) / 0.25; c[0] = 0.14 + t * 0.30; c[1] = 0.42 - t * 0.14; c[2] = 0.20 - t * 0.06; return; }
    if (e < 0.75) { t = (e - 0.50) / 0.25; c[0] = 0.44 + t * 0.16; c[1] = 0.28 + t * 0.12; c[2] = 0.14 + t * 0.18; return; }
    t = js_min(1.0, (e - 0.75) / 0.20);
    c[0] = 0.60 + t * 0.35; c[1] = 0.40 + t * 0.50; c[2] = 0.32 + t * 0.60;
}
// js/planet-mesh.js:64-80
WO_IMP_HD inline double heightmap_shade(double e) { return js_max(0.0, js_min(1.0, (elev_to_height_km(e) + 5.0) / 11.0)); }
WO_IMP_HD inline double land_heightmap_shade(double e) { return e <= 0.0 ? 0.0 : js_max(0.0, js_min(1.0, elev_to_height_km(e) / 6.0)); }
WO_IMP_HD inline double land_mask_shade(double e) { return e > 0.0 ? 1.0 : 0.0; }

// js/koppen.js:19-51, the colour column (an id outside the table takes class 0: js/planet-mesh.js:175-178)
WO_IMP_HD inline void koppen_color(int32_t id, double c[3]) {
    const double T[31][3] = {
        {0.29, 0.44, 0.65}, {0.00, 0.00, 1.00}, {0.00, 0.47, 1.00}, {0.27, 0.67, 0.98}, {1.00, 0.00, 0.00}, {1.00, 0.59, 0.59}, {0.96, 0.65, 0.00},
        {1.00, 0.86, 0.39}, {0.78, 1.00, 0.31}, {0.39, 1.00, 0.31}, {0.20, 0.78, 0.00}, {1.00, 1.00, 0.00}, {0.78, 0.78, 0.00}, {0.59, 0.59, 0.00},
        {0.59, 1.00, 0.59}, {0.39, 0.78, 0.39}, {0.20, 0.59, 0.20}, {0.00, 1.00, 1.00}, {0.22, 0.78, 1.00}, {0.00, 0.49, 0.49}, {0.00, 0.27, 0.37},
        {0.90, 0.50, 1.00}, {0.70, 0.35, 0.85}, {0.50, 0.20, 0.65}, {0.35, 0.10, 0.45}, {0.67, 0.69, 1.00}, {0.43, 0.47, 0.78}, {0.29, 0.31, 0.78},
        {0.20, 0.00, 0.53}, {0.70, 0.70, 0.70}, {0.41, 0.41, 0.41}};
    const int k = (id >= 0 && id <= 30) ? id : 0;
    c[0] = T[k][0]; c[1] = T[k][1]; c[2] = T[k][2];
}

// js/color-map.js:14-114: biomeColor(koppenId, elevation)
WO_IMP_HD inline void biome_color(int32_t id, double elevation, double c[3]) {
    if (id == 0 || elevation <= 0.0) { elevation_to_color(elevation, c); return; }
    const double B[31][3] = {
        {0.30, 0.50, 0.20}, {0.05, 0.30, 0.05}, {0.08, 0.33, 0.07}, {0.42, 0.50, 0.18}, {0.82, 0.72, 0.50}, {0.60, 0.55, 0.48}, {0.72, 0.62, 0.30},
        {0.55, 0.52, 0.32}, {0.18, 0.42, 0.12}, {0.12, 0.38, 0.10}, {0.10, 0.28, 0.10}, {0.45, 0.48, 0.22}, {0.40, 0.45, 0.20}, {0.35, 0.40, 0.20},
        {0.20, 0.44, 0.14}, {0.15, 0.40, 0.12}, {0.12, 0.32, 0.10}, {0.12, 0.36, 0.08}, {0.10, 0.32, 0.08}, {0.06, 0.22, 0.08}, {0.05, 0.18, 0.07},
        {0.38, 0.38, 0.18}, {0.35, 0.35, 0.17}, {0.08, 0.22, 0.08}, {0.06, 0.18, 0.07}, {0.14, 0.36, 0.10}, {0.12, 0.32, 0.09}, {0.07, 0.22, 0.08},
        {0.05, 0.18, 0.07}, {0.35, 0.32, 0.22}, {0.78, 0.80, 0.84}};             // entry 0 is the fallback of an id outside 1 .. 30
    const int k = (id >= 1 && id <= 30) ? id : 0;
    const double hKm = elev_to_height_km(elevation);
    double alpineLine, snowLine;                                                  // altitudeThresholds (:57-67)
    if (id <= 0) { alpineLine = 0.0; snowLine = 0.0; }
    else if (id <= 3) { alpineLine = 3.5; snowLine = 5.5; }
    else if (id <= 7) { alpineLine = 3.0; snowLine = 5.0; }
    else if (id <= 16) { alpineLine = 2.0; snowLine = 3.5; }
    else if (id <= 18 || id == 21 || id == 22 || id == 25 || id == 26) { alpineLine = 1.5; snowLine = 3.0; }
    else if (id <= 28) { alpineLine = 0.8; snowLine = 2.0; }
    else if (id == 29) { alpineLine = 0.4; snowLine = 1.5; }
    else { alpineLine = 0.0; snowLine = 0.5; }
    double r = B[k][0], g = B[k][1], b = B[k][2];
    if (hKm < 0.2) {
        const double dark = 0.93 + 0.07 * (hKm / 0.2);
        r *= dark; g *= dark; b *= dark;
    }
    if (alpineLine > 0.0 && hKm > 0.2 && hKm < alpineLine) {
        const double t = (hKm - 0.2) / (alpineLine - 0.2);
        const double darken = 1.0 - t * 0.15;
        r *= darken; g *= darken; b *= darken;
    }
    if (alpineLine > 0.0 && hKm > alpineLine) {
        const double rockZone = snowLine > alpineLine ? snowLine - alpineLine : 2.0;
        const double rockT = js_min(1.0, (hKm - alpineLine) / rockZone);
        const double s = rockT * rockT;
        r = r + (0.42 - r) * s;
        g = g + (0.38 - g) * s;
        b = b + (0.32 - b) * s;
    }
    if (snowLine > 0.0 && hKm > snowLine) {
        const double snowT = js_min(1.0, (hKm - snowLine) / 2.5);
        const double s = snowT * snowT;
        r = r + (0.92 - r) * s;
        g = g + (0.93 - g) * s;
        b = b + (0.96 - b) * s;
    }
    c[0] = r; c[1] = g; c[2] = b;
}

// the region colour of every type but `biome`, and the raw (unsmoothed) colour of `biome`; koppen is not read by the other four
WO_IMP_HD inline Rgb region_color(int32_t type, float elevation, int32_t koppenId) {
    const double e = (double)elevation;
    double c[3];
    switch (type) {
        case TYPE_HEIGHTMAP: c[0] = c[1] = c[2] = heightmap_shade(e); break;
        case TYPE_LANDHEIGHTMAP: c[0] = c[1] = c[2] = land_heightmap_shade(e); break;
        case TYPE_LANDMASK: c[0] = c[1] = c[2] = land_mask_shade(e); break;
        case TYPE_BIOME: biome_color(koppenId, e, c); break;
        case TYPE_KOPPEN: koppen_color(koppenId, c); break;
        default: elevation_to_color(e, c); break;
    }
    return rgb_of(c[0], c[1], c[2]);
}
// smoothBiomeColors' second loop for region r (raw: 3 floats per region)
WO_IMP_HD inline Rgb biome_smooth(const float* raw, const int32_t* off, const int32_t* adj, int32_t r) {
    const int32_t start = off[r], end = off[r + 1], count = end - start;
    const int64_t o = 3 * (int64_t)r;
    if (count == 0) return Rgb{raw[o], raw[o + 1], raw[o + 2]};
    const double alpha = 0.35;
    double avgR = 0.0, avgG = 0.0, avgB = 0.0;
    for (int32_t i = start; i < end; ++i) {
        const int64_t n = 3 * (int64_t)adj[i];
        avgR += (double)raw[n]; avgG += (double)raw[n + 1]; avgB += (double)raw[n + 2];
    }
    avgR /= (double)count; avgG /= (double)count; avgB /= (double)count;
    return rgb_of((double)raw[o] * (1.0 - alpha) + avgR * alpha, (double)raw[o + 1] * (1.0 - alpha) + avgG * alpha, (double)raw[o + 2] * (1.0 - alpha) + avgB * alpha);
}

// q = floor(c * 255 + 0.5) on the f32 value clamped to [0, 1]; NaN gives 0
WO_IMP_HD inline int32_t quantise(float c) {
    double v = (double)c;
    if (!(v > 0.0)) return 0;
    if (v > 1.0) v = 1.0;
    return (int32_t)floor(v * 255.0 + 0.5);
}
// R | G << 8 | B << 16 | 255 << 24: the four bytes of an RGBA pixel in memory order
WO_IMP_HD inline uint32_t pack_rgba(const Rgb& c, const uint8_t* lut) {
    return (uint32_t)lut[quantise(c.r)] | ((uint32_t)lut[quantise(c.g)] << 8) | ((uint32_t)lut[quantise(c.b)] << 16) | 0xFF000000u;
}

// ---- host only: the gamma table and the background (pow is the host libm's; every value is floored to a byte) -----------------
// LUT[k] = (v <= 0.0031308 ? v * 12.92 : 1.055 * pow(v, 1 / 2.4) - 0.055) * 255 + 0.5 | 0 at v = k / 255 (:1908-1910)
inline void gamma_lut(uint8_t lut[256]) {
    for (int k = 0; k < 256; ++k) {
        const double v = (double)k / 255.0;
        lut[k] = (uint8_t)(int32_t)((v <= 0.0031308 ? v * 12.92 : 1.055 * std::pow(v, 1.0 / 2.4) - 0.055) * 255.0 + 0.5);
    }
}
// three r160's SRGBToLinear
inline double srgb_to_linear(double c) { return c < 0.04045 ? c * 0.0773993808 : std::pow(c * 0.9478672986 + 0.0521327014, 2.4); }
// the pixel nothing covers: (0, 0, 0) for the grey types, 0x1a1a2e through SRGBToLinear, the quantiser and the table otherwise
inline uint32_t background_rgba(int32_t type, const uint8_t* lut) {
    if (type_is_grey(type)) return 0xFF000000u;
    const Rgb c = rgb_of(srgb_to_linear(0x1a / 255.0), srgb_to_linear(0x1a / 255.0), srgb_to_linear(0x2e / 255.0));
    return pack_rgba(c, lut);
}

}  // namespace map
}  // namespace wo
