// Relief export: a smooth height per pixel, its 16-bit encoding and the normals of the displaced surface, for the equirectangular
// map and the cube map.  The per-pixel bodies shared by the device kernels (relief.hip) and the test-only CPU emulator
// (tests/emu_relief), so that both compile the very same arithmetic.  The library compiles with -ffp-contract=off; everything is
// double arithmetic on f32 inputs with + - * /, sqrt, floor and the fd_sin / fd_cos of import_ops.h.  Ours: the reference exports
// neither, so this header is the contract.
//
// The surface.  The globe mesh (globe_ops.h) is one flat triangle per side s between v0 = t_xyz[s / 3], v1 = t_xyz[halfedges[s] / 3]
//   and v2 = r_xyz[triangles[s]], with the elevations E0 = t_elevation[s / 3], E1 = t_elevation[halfedges[s] / 3] (globe::
//   triangle_elevation, stored f32) and E2 = r_elevation[triangles[s]].  The raster (raster.hip) decides which side
//   covers a pixel (the side map); the height of the pixel is that side's elevation interpolated at the pixel centre.
// Height, equirectangular.  t is the map::Tri of the winning side that was rastered: side_triangles' k = 0, or for a wrapping side
//   k = 0 if that triangle has a usable area2 and covers the centre, else k = 1.  With area2 = tri_area2(t) and e0, e1, e2 the edge
//   functions of tri_covers at the centre (e0 along v0 v1, e1 along v1 v2, e2 along v2 v0):
//       h = ((e1 * E0 + e2 * E1) + e0 * E2) / area2        in double, stored as f32.
//   Affine in the map plane, also for vertices that the clamp moved.
// Height, cube face f.  The triangle of cube::side_on_face(v, f) with its positions NOT rounded to f32: a_k = sc / ma, b_k = tc / ma in
//   double by the face table, ma_k the major-axis component of vertex k (a float, taken as a double); area2 and the edge functions
//   as above on those; b0 = e1 / area2, b1 = e2 / area2, b2 = e0 / area2, w_k = b_k / ma_k:
//       h = ((w0 * E0 + w1 * E1) + w2 * E2) / ((w0 + w1) + w2)        in double, stored as f32.
//   Perspective-correct: the elevation at which the ray through the pixel centre meets the flat 3-D triangle (v0, v1, v2), so a
//   side drawn on two faces gives the same surface on both.  The raster decides coverage on the f32 positions, whose rounding
//   (2^-24 of a position times the slope of the side) would otherwise be the largest error of h against that 3-D statement.  A
//   centre within that rounding of an edge can therefore get a weight of -1e-8: h is held to [min E, max E] of its side, which it
//   could leave by no more than that (fminf / fmaxf pass over a NaN elevation; h is a NaN then).
// Uncovered pixels get the quiet NaN 0x7FC00000.  A NaN elevation propagates through the arithmetic.
// 16 bit.  HEIGHT: shade = map::heightmap_shade(h); LAND_HEIGHT: shade = map::land_heightmap_shade(h); q = floor(shade * 65535 + 0.5)
//   in double; a NaN h gives 0.  No gamma table: heights are data, the encoding is linear in the reference's shade.
// Direction of a pixel.  Cube: cube::cube_direction divided by its length (one sqrt, three divisions).  Map, W x H around centerLon:
//   lat = yc * (pi / 2), lon = xc * (pi / 2) + centerLon (the inverse of the raster's x = wrap_lon(lon, centerLon) * 2 / pi), d =
//   (cos lat * sin lon, sin lat, cos lat * cos lon): the reference's frame, lon = atan2(x, z).  One RowDir per row (cos lat, sin lat)
//   and one ColDir per column (sin lon, cos lon), not one evaluation per pixel.
// Neighbours.  Map: columns wrap modulo W; beyond the first or last row the pixel itself stands in.  Cube: a step off the face takes
//   the extended coordinate pixel_c(-1, S) or pixel_c(S, S), the direction cube_direction gives for it, the face f' of that
//   direction's major axis (unique: one extended coordinate exceeds 1 in magnitude, the other does not), a' = sc / ma, b' = tc / ma
//   on f' by the face table in double, and the pixel clamp(floor((a' + 1) * S / 2), 0, S - 1), likewise for b'.  Only the four axis
//   neighbours are ever asked for.
// Normal.  R(h) = 1 + strength * (h > 0 ? h * V : h * V * 0.3), V = globe::V.  With FLAT_OCEAN, h <= 0 counts as 0.  A NaN neighbour
//   takes the centre's h; a NaN centre gives the flat normal.  P(q) = dhat(q) * R(h(q)) with dhat(q) the direction of the pixel
//   actually sampled (across a cube edge the neighbour's own centre): every difference is an honest secant.  Tu = P(right) - P(left),
//   Tv = P(up) - P(down), N = Tu x Tv.  The gnomonic stencil is not symmetric about the pixel, so on a perfect sphere N leans away
//   from dhat by O(1 / S^2): N0, the same product with every R set to the centre's, is that lean and nothing else, and the normal is
//       n = (N - N0) + |N0| dhat,
//   expressed in the pixel's frame (right, up, dhat) as t = ((N - N0) . right, (N - N0) . up, (N - N0) . dhat + |N0|), negated if
//   t.z < 0, divided by its length; t = (0, 0, 1) if it is zero or has a NaN.  A constant field has N == N0 in every bit, so its
//   normal is exactly flat.  Tangent space: t.  Object space: right * t.x + up * t.y + dhat * t.z.
// Frames, right-handed and orthonormal (image right, image up, outward).  Map: east = (cos lon, 0, -sin lon), north = (-sin lat
//   sin lon, cos lat, -sin lat cos lon), dhat.  Cube: right = face_right(f) (the face table's d/da) less its component along dhat,
//   divided by its length; up = dhat x right, which points towards decreasing b.
// Bytes: floor((c * 0.5 + 0.5) * 255 + 0.5) per component clamped to [0, 255], alpha 255; R | G << 8 | B << 16 | A << 24.
#pragma once
#include <cmath>
#include <cstdint>

#include "cube_ops.h"
#include "globe_ops.h"
#include "map_layer_ops.h"
#include "map_ops.h"

namespace wo {
namespace relief {

namespace M = wo::map;
namespace Q = wo::cube;

enum : int32_t { KIND_HEIGHT = 0, KIND_LAND_HEIGHT = 1, KIND_COUNT };            // WO_RELIEF_HEIGHT, WO_RELIEF_LAND_HEIGHT
enum : int32_t { SPACE_TANGENT = 0, SPACE_OBJECT = 1, SPACE_COUNT };             // WO_RELIEF_NORMAL_*
enum : int32_t { FLAG_FLAT_OCEAN = 1, FLAG_ALL = 1 };                            // WO_RELIEF_FLAT_OCEAN

constexpr uint32_t NAN_BITS = 0x7FC00000u;
WO_IMP_HD inline float quiet_nan() { return M::f32_of_bits(NAN_BITS); }

// ---- heights --------------------------------------------------------------------------------------------------------------------
struct Edges { double e0, e1, e2; };
WO_IMP_HD inline Edges edges_at(const M::Tri& t, double xc, double yc) {
    return Edges{M::edge_fn(t.x[0], t.y[0], t.x[1], t.y[1], xc, yc), M::edge_fn(t.x[1], t.y[1], t.x[2], t.y[2], xc, yc), M::edge_fn(t.x[2], t.y[2], t.x[0], t.y[0], xc, yc)};
}
WO_IMP_HD inline float height_planar(const M::Tri& t, double area2, double xc, double yc, const float E[3]) {
    const Edges e = edges_at(t, xc, yc);
    return (float)(((e.e1 * (double)E[0] + e.e2 * (double)E[1]) + e.e0 * (double)E[2]) / area2);
}
// a, b: the unrounded face coordinates of the three vertices
WO_IMP_HD inline float height_perspective(const double a[3], const double b[3], double xc, double yc, const double ma[3], const float E[3]) {
    const double area2 = M::edge_fn(a[0], b[0], a[1], b[1], a[2], b[2]);
    const double e0 = M::edge_fn(a[0], b[0], a[1], b[1], xc, yc), e1 = M::edge_fn(a[1], b[1], a[2], b[2], xc, yc), e2 = M::edge_fn(a[2], b[2], a[0], b[0], xc, yc);
    const double w0 = (e1 / area2) / ma[0], w1 = (e2 / area2) / ma[1], w2 = (e0 / area2) / ma[2];
    float h = (float)(((w0 * (double)E[0] + w1 * (double)E[1]) + w2 * (double)E[2]) / ((w0 + w1) + w2));
    const float lo = fminf(fminf(E[0], E[1]), E[2]), hi = fmaxf(fmaxf(E[0], E[1]), E[2]);      // pass over a NaN; h is one then anyway
    if (h < lo) h = lo;
    if (h > hi) h = hi;
    return h;
}

// the three elevations of side s
WO_IMP_HD inline void side_elevations(const int32_t* triangles, const int32_t* halfedges, const float* t_elevation, const float* r_elevation, int64_t s, float E[3]) {
    E[0] = t_elevation[s / 3];
    E[1] = t_elevation[halfedges[s] / 3];
    E[2] = r_elevation[triangles[s]];
}

// pixel q of the W x H map, covered by side s (never NO_SIDE)
WO_IMP_HD inline float map_pixel_height(const int32_t* triangles, const int32_t* halfedges, const M::LonLat* t_ll, const M::LonLat* r_ll, const float* t_elevation,
                                        const float* r_elevation, int64_t s, int64_t q, int32_t W, int32_t H) {
    M::LonLat v[3];
    M::side_vertices(triangles, halfedges, t_ll, r_ll, s, v);
    M::Tri tri[2];
    const int n = M::side_triangles(v, tri);
    const double xc = M::pixel_xc(q % W, W), yc = M::pixel_yc(q / W, H);
    int k = 0;
    double area2 = M::tri_area2(tri[0]);
    if (n == 2 && !((area2 > 0.0 || area2 < 0.0) && M::tri_covers(tri[0], area2, xc, yc))) {
        k = 1;
        area2 = M::tri_area2(tri[1]);
    }
    float E[3];
    side_elevations(triangles, halfedges, t_elevation, r_elevation, s, E);
    return height_planar(tri[k], area2, xc, yc, E);
}

// pixel q of the S x 6S cube map, covered by side s (never NO_SIDE)
WO_IMP_HD inline float cube_pixel_height(const int32_t* triangles, const int32_t* halfedges, const float* t_xyz, const float* r_xyz, const float* t_elevation,
                                         const float* r_elevation, int64_t s, int64_t q, int32_t S) {
    const int64_t face = (int64_t)S * S;
    const int32_t f = (int32_t)(q / face);
    const int64_t r = q % face;
    float v[3][3];
    Q::side_vertices(triangles, halfedges, t_xyz, r_xyz, s, v);
    double a[3], b[3], ma[3];
    for (int k = 0; k < 3; ++k) {
        float m, sc, tc;
        Q::face_terms(f, v[k][0], v[k][1], v[k][2], m, sc, tc);
        if (!(m > 0.0f)) return quiet_nan();                  // never: the raster drew s on f
        ma[k] = (double)m;
        a[k] = (double)sc / (double)m;
        b[k] = (double)tc / (double)m;
    }
    float E[3];
    side_elevations(triangles, halfedges, t_elevation, r_elevation, s, E);
    return height_perspective(a, b, Q::pixel_c(r % S, S), Q::pixel_c(r / S, S), ma, E);
}

// the two bodies above under one name, for the height pass that takes its projection as a type (relief.hip: k_relief_heights)
WO_IMP_HD inline float pixel_height(const M::Projection& P, const int32_t* triangles, const int32_t* halfedges, const float* t_elevation, const float* r_elevation, int64_t s,
                                    int64_t q) {
    return map_pixel_height(triangles, halfedges, P.t_ll, P.r_ll, t_elevation, r_elevation, s, q, P.W, P.H);
}
WO_IMP_HD inline float pixel_height(const Q::Projection& P, const int32_t* triangles, const int32_t* halfedges, const float* t_elevation, const float* r_elevation, int64_t s,
                                    int64_t q) {
    return cube_pixel_height(triangles, halfedges, P.t_xyz, P.r_xyz, t_elevation, r_elevation, s, q, P.S);
}

// ---- 16 bit ---------------------------------------------------------------------------------------------------------------------
WO_IMP_HD inline bool kind_ok(int32_t kind) { return kind >= 0 && kind < KIND_COUNT; }
WO_IMP_HD inline uint16_t height16(int32_t kind, float h) {
    if (h != h) return 0;
    const double shade = kind == KIND_LAND_HEIGHT ? M::land_heightmap_shade((double)h) : M::heightmap_shade((double)h);
    return (uint16_t)(int32_t)floor(shade * 65535.0 + 0.5);    // shade lies in [0, 1]
}

// ---- directions -----------------------------------------------------------------------------------------------------------------
constexpr double HALF_PI = 3.141592653589793 / 2.0;
struct RowDir { double cosLat, sinLat; };
struct ColDir { double sinLon, cosLon; };
WO_IMP_HD inline RowDir map_row(int64_t j, int32_t H) {
    const double lat = M::pixel_yc(j, H) * HALF_PI;
    return RowDir{imp::fd_cos(lat), imp::fd_sin(lat)};
}
WO_IMP_HD inline ColDir map_col(int64_t i, int32_t W, double centerLon) {
    const double lon = M::pixel_xc(i, W) * HALF_PI + centerLon;
    return ColDir{imp::fd_sin(lon), imp::fd_cos(lon)};
}
WO_IMP_HD inline void map_direction(const RowDir& r, const ColDir& c, double d[3]) { d[0] = r.cosLat * c.sinLon; d[1] = r.sinLat; d[2] = r.cosLat * c.cosLon; }
WO_IMP_HD inline void map_frame(const RowDir& r, const ColDir& c, double right[3], double up[3]) {
    right[0] = c.cosLon; right[1] = 0.0; right[2] = -c.sinLon;
    up[0] = -r.sinLat * c.sinLon; up[1] = r.cosLat; up[2] = -r.sinLat * c.cosLon;
}

WO_IMP_HD inline double dot3(const double a[3], const double b[3]) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }
WO_IMP_HD inline void cross3(const double a[3], const double b[3], double c[3]) {
    c[0] = a[1] * b[2] - a[2] * b[1];
    c[1] = a[2] * b[0] - a[0] * b[2];
    c[2] = a[0] * b[1] - a[1] * b[0];
}
WO_IMP_HD inline void cube_unit_direction(int32_t f, int64_t i, int64_t j, int32_t S, double d[3]) {
    Q::cube_direction(f, i, j, S, d);
    const double len = sqrt(dot3(d, d));
    d[0] /= len; d[1] /= len; d[2] /= len;
}

// the face table once more, on doubles
WO_IMP_HD inline void face_terms_d(int32_t f, const double d[3], double& ma, double& sc, double& tc) {
    switch (f) {
        case 0: ma = d[0]; sc = -d[2]; tc = -d[1]; break;
        case 1: ma = -d[0]; sc = d[2]; tc = -d[1]; break;
        case 2: ma = d[1]; sc = d[0]; tc = d[2]; break;
        case 3: ma = -d[1]; sc = d[0]; tc = -d[2]; break;
        case 4: ma = d[2]; sc = d[0]; tc = -d[1]; break;
        default: ma = -d[2]; sc = -d[0]; tc = -d[1]; break;
    }
}
// d/da of cube_direction on face f: image right
WO_IMP_HD inline void face_right(int32_t f, double r[3]) {
    r[0] = r[1] = r[2] = 0.0;
    switch (f) {
        case 0: r[2] = -1.0; break;
        case 1: r[2] = 1.0; break;
        case 2: case 3: case 4: r[0] = 1.0; break;
        default: r[0] = -1.0; break;
    }
}
WO_IMP_HD inline void cube_frame(int32_t f, const double d[3], double right[3], double up[3]) {
    double a[3];
    face_right(f, a);
    const double along = dot3(a, d);
    for (int k = 0; k < 3; ++k) right[k] = a[k] - along * d[k];
    const double len = sqrt(dot3(right, right));
    for (int k = 0; k < 3; ++k) right[k] /= len;
    cross3(d, right, up);
}

// ---- neighbours -----------------------------------------------------------------------------------------------------------------
struct FacePixel { int32_t f, i, j; };
WO_IMP_HD inline int32_t face_clamp(double a, int32_t S) {
    const double x = floor((a + 1.0) * (double)S / 2.0);
    return x < 0.0 ? 0 : x > (double)(S - 1) ? S - 1 : (int32_t)x;
}
// the pixel that stands for (i + di, j + dj) of face f; (di, dj) is one of (+-1, 0), (0, +-1)
WO_IMP_HD inline FacePixel cube_neighbor(int32_t f, int32_t i, int32_t j, int32_t di, int32_t dj, int32_t S) {
    const int32_t ni = i + di, nj = j + dj;
    if (ni >= 0 && ni < S && nj >= 0 && nj < S) return FacePixel{f, ni, nj};
    double d[3];
    Q::cube_direction(f, ni, nj, S, d);
    int32_t k = 0;
    for (int32_t c = 1; c < 3; ++c) if (fabs(d[c]) > fabs(d[k])) k = c;
    const int32_t g = 2 * k + (d[k] > 0.0 ? 0 : 1);
    double ma, sc, tc;
    face_terms_d(g, d, ma, sc, tc);
    return FacePixel{g, face_clamp(sc / ma, S), face_clamp(tc / ma, S)};
}

// ---- normals --------------------------------------------------------------------------------------------------------------------
WO_IMP_HD inline bool space_ok(int32_t space) { return space >= 0 && space < SPACE_COUNT; }
WO_IMP_HD inline bool flags_ok(int32_t flags) { return (flags & ~FLAG_ALL) == 0; }
WO_IMP_HD inline bool strength_ok(double s) { return s >= 0.0 && s <= 1.7976931348623157e308; }

WO_IMP_HD inline double radius(double h, double strength, int32_t flags) {
    if ((flags & FLAG_FLAT_OCEAN) && h <= 0.0) h = 0.0;
    return 1.0 + strength * (h > 0.0 ? h * globe::V : h * globe::V * 0.3);
}

// one sample of the stencil: the direction of the pixel sampled and its height
struct Sample { double d[3]; float h; };

WO_IMP_HD inline void secant_normal(const Sample q[4], const double R[4], double N[3]) {          // q: right, left, up, down
    double Tu[3], Tv[3];
    for (int k = 0; k < 3; ++k) {
        Tu[k] = q[0].d[k] * R[0] - q[1].d[k] * R[1];
        Tv[k] = q[2].d[k] * R[2] - q[3].d[k] * R[3];
    }
    cross3(Tu, Tv, N);
}

WO_IMP_HD inline uint32_t normal_byte(double c) {
    const double v = floor((c * 0.5 + 0.5) * 255.0 + 0.5);
    return v > 0.0 ? (v < 255.0 ? (uint32_t)v : 255u) : 0u;
}

// the packed RGBA of a pixel from its own direction, frame and height hc and the four samples right, left, up, down
WO_IMP_HD inline uint32_t normal_rgba(const double d[3], const double right[3], const double up[3], float hc, const Sample q[4], int32_t space, double strength, int32_t flags) {
    double t[3] = {0.0, 0.0, 1.0};
    if (hc == hc) {
        const double Rc = radius((double)hc, strength, flags);
        double R[4], R0[4], N[3], N0[3], D[3];
        for (int k = 0; k < 4; ++k) {
            R[k] = radius((double)(q[k].h == q[k].h ? q[k].h : hc), strength, flags);
            R0[k] = Rc;
        }
        secant_normal(q, R, N);
        secant_normal(q, R0, N0);
        for (int k = 0; k < 3; ++k) D[k] = N[k] - N0[k];
        t[0] = dot3(D, right); t[1] = dot3(D, up); t[2] = dot3(D, d) + sqrt(dot3(N0, N0));
        if (t[2] < 0.0) { t[0] = -t[0]; t[1] = -t[1]; t[2] = -t[2]; }
        const double len = sqrt(dot3(t, t));
        if (len > 0.0 && len <= 1.7976931348623157e308) { t[0] /= len; t[1] /= len; t[2] /= len; }
        else { t[0] = 0.0; t[1] = 0.0; t[2] = 1.0; }
    }
    double n[3] = {t[0], t[1], t[2]};
    if (space == SPACE_OBJECT)
        for (int k = 0; k < 3; ++k) n[k] = (right[k] * t[0] + up[k] * t[1]) + d[k] * t[2];
    return normal_byte(n[0]) | (normal_byte(n[1]) << 8) | (normal_byte(n[2]) << 16) | 0xFF000000u;
}

// pixel (i, j) of the W x H map: heights is the resident height map, rows and cols the two tables
WO_IMP_HD inline uint32_t map_pixel_normal(const float* heights, const RowDir* rows, const ColDir* cols, int32_t W, int32_t H, int32_t i, int32_t j, int32_t space,
                                           double strength, int32_t flags) {
    const int32_t ir = i + 1 == W ? 0 : i + 1, il = i == 0 ? W - 1 : i - 1, ju = j == 0 ? 0 : j - 1, jd = j + 1 == H ? H - 1 : j + 1;
    const int32_t qi[4] = {ir, il, i, i}, qj[4] = {j, j, ju, jd};
    Sample q[4];
    for (int k = 0; k < 4; ++k) {
        map_direction(rows[qj[k]], cols[qi[k]], q[k].d);
        q[k].h = heights[(int64_t)qj[k] * W + qi[k]];
    }
    double d[3], right[3], up[3];
    map_direction(rows[j], cols[i], d);
    map_frame(rows[j], cols[i], right, up);
    return normal_rgba(d, right, up, heights[(int64_t)j * W + i], q, space, strength, flags);
}

// pixel (i, j) of face f of the S x 6S cube map
WO_IMP_HD inline uint32_t cube_pixel_normal(const float* heights, int32_t S, int32_t f, int32_t i, int32_t j, int32_t space, double strength, int32_t flags) {
    const int32_t di[4] = {1, -1, 0, 0}, dj[4] = {0, 0, -1, 1};
    Sample q[4];
    for (int k = 0; k < 4; ++k) {
        const FacePixel n = cube_neighbor(f, i, j, di[k], dj[k], S);
        cube_unit_direction(n.f, n.i, n.j, S, q[k].d);
        q[k].h = heights[Q::pixel_index(n.f, n.i, n.j, S)];
    }
    double d[3], right[3], up[3];
    cube_unit_direction(f, i, j, S, d);
    cube_frame(f, d, right, up);
    return normal_rgba(d, right, up, heights[Q::pixel_index(f, i, j, S)], q, space, strength, flags);
}

}  // namespace relief
}  // namespace wo
