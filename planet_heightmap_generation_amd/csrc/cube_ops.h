// Cube-map export: the per-vertex, per-side and per-pixel bodies shared by the device kernels (cube.hip, raster.hip) and the test-only CPU
// emulator (tests/emu_cube), so that both compile the very same arithmetic.  The library compiles with -ffp-contract=off: no FMA
// changes a result, and nothing here calls libm beyond floor / ceil / fmin / fmax.  Ours: the reference exports no cube map.
//
// The gnomonic projection maps great-circle arcs to straight lines, so the six faces are exactly the reference's globe mesh
// (buildMesh: one flat triangle per side, displaced radially, which moves no vertex's direction) seen from its centre.  There is
// no seam, no wrap and no pole cap: on a closed mesh every pixel is covered.
//
// Faces.  Order +X, -X, +Y, -Y, +Z, -Z, named px nx py ny pz nz: the OpenGL cube-map table.  For a point (x, y, z) and face f with
//   major-axis component ma (signed so that it is positive in front of the face), a = sc / ma and b = tc / ma with
//       face   ma   sc   tc
//       +X     +x   -z   -y
//       -X     -x   +z   -y
//       +Y     +y   +x   +z
//       -Y     -y   +x   -z
//       +Z     +z   +x   -y
//       -Z     -z   -x   -y
//   The division is in double on the f32 inputs; the result is stored as f32, as the map stores its positions, so that map::Tri,
//   tri_area2, tri_covers and edge_fn are reused unchanged (Tri.x = a, Tri.y = b).  The reference's frame has north at +Y and
//   longitude 0 at +Z: pz is centred on the map's centre, and row 0 of the four side faces is north.
// Vertices.  The map's: for side s they are t_xyz[s / 3], t_xyz[halfedges[s] / 3] and r_xyz[triangles[s]], t_xyz from
//   map::triangle_center.  Nothing is normalised.
// Which sides are drawn.  A side is drawn on face f only if all three of its vertices have ma > 0 there; any other side is not
//   drawn on that face (it is neither clipped nor split).  The corner of a face lies atan(sqrt 2) = 54.74 degrees from its centre,
//   so such a side could reach the face only if it spanned more than 90 - 54.74 = 35.26 degrees: the contract holds for meshes whose
//   sides are shorter than that, and the entry point does not check it.  ma > 0 holds on at most one face per axis, so a side is
//   drawn on at most three faces.
// Pixel centres.  The centre of pixel (i, j) of a face of size S: ac = -1 + 2 (i + 0.5) / S, bc = -1 + 2 (j + 0.5) / S in double, in
//   this order of operations.
// Coverage.  map_ops.h's rule: area2 of 0 or NaN covers nothing; otherwise a pixel is covered when all three edge functions are
//   >= 0, or all are <= 0; the LOWEST side index wins; the region is triangles[s], or -1 where nothing covers the pixel.  The rule
//   does not depend on thread order.
// Layout.  The faces are stacked vertically into one S x 6S region map: face f, row j, column i lies at ((f S + j) S + i), indexed
//   in 64 bits.  1 <= S <= 16384; odd sizes are allowed.
// Bounding box.  That of the f32 positions, intersected with [-1, 1]^2 BEFORE any conversion to integer (a vertex near the plane
//   ma = 0 projects to a huge or infinite position), then one pixel wider on every side, as map::tri_box is.
#pragma once
#include <cmath>
#include <cstdint>

#include "map_ops.h"

namespace wo {
namespace cube {

constexpr int32_t FACE_COUNT = 6;
constexpr int32_t MAX_FACE_SIZE = 16384;

WO_IMP_HD inline bool face_size_ok(int32_t S) { return S >= 1 && S <= MAX_FACE_SIZE; }

// the face table: ma, sc and tc of a point on face f
WO_IMP_HD inline void face_terms(int32_t f, float x, float y, float z, float& ma, float& sc, float& tc) {
    switch (f) {
        case 0: ma = x; sc = -z; tc = -y; break;
        case 1: ma = -x; sc = z; tc = -y; break;
        case 2: ma = y; sc = x; tc = z; break;
        case 3: ma = -y; sc = x; tc = -z; break;
        case 4: ma = z; sc = x; tc = -y; break;
        default: ma = -z; sc = -x; tc = -y; break;
    }
}

// the face of axis k (0 x, 1 y, 2 z) in front of which component c lies (c > 0: the positive one)
WO_IMP_HD inline int32_t face_of_axis(int32_t k, float c) { return 2 * k + (c > 0.0f ? 0 : 1); }

// the three vertices of side s: 3 floats each
WO_IMP_HD inline void side_vertices(const int32_t* triangles, const int32_t* halfedges, const float* t_xyz, const float* r_xyz, int64_t s, float v[3][3]) {
    const int64_t it = s / 3, ot = halfedges[s] / 3, br = triangles[s];
    for (int k = 0; k < 3; ++k) {
        v[0][k] = t_xyz[3 * it + k];
        v[1][k] = t_xyz[3 * ot + k];
        v[2][k] = r_xyz[3 * br + k];
    }
}

// the side's triangle on face f; false when the side is not drawn there (a vertex with ma <= 0 or NaN)
WO_IMP_HD inline bool side_on_face(const float v[3][3], int32_t f, map::Tri& t) {
    for (int k = 0; k < 3; ++k) {
        float ma, sc, tc;
        face_terms(f, v[k][0], v[k][1], v[k][2], ma, sc, tc);
        if (!(ma > 0.0f)) return false;
        t.x[k] = (float)((double)sc / (double)ma);
        t.y[k] = (float)((double)tc / (double)ma);
    }
    return true;
}

WO_IMP_HD inline double pixel_c(int64_t i, int32_t S) { return -1.0 + 2.0 * ((double)i + 0.5) / (double)S; }

// The pixels of one face whose centres can lie in the triangle's bounding box, one pixel wider on every side than the arithmetic
// asks for (the exact test is map::tri_covers).  Returns false for a triangle that covers nothing on the face.  fmin / fmax pass
// over a NaN; an area2 that is neither 0 nor NaN has no NaN position.
WO_IMP_HD inline bool tri_box(const map::Tri& t, double area2, int32_t S, map::Box& b) {
    if (!(area2 > 0.0 || area2 < 0.0)) return false;
    double minx = fmin(fmin((double)t.x[0], (double)t.x[1]), (double)t.x[2]), maxx = fmax(fmax((double)t.x[0], (double)t.x[1]), (double)t.x[2]);
    double miny = fmin(fmin((double)t.y[0], (double)t.y[1]), (double)t.y[2]), maxy = fmax(fmax((double)t.y[0], (double)t.y[1]), (double)t.y[2]);
    minx = fmax(minx, -1.0); maxx = fmin(maxx, 1.0);          // the face, before any integer: what is left lies in [-1, 1]
    miny = fmax(miny, -1.0); maxy = fmin(maxy, 1.0);
    if (!(minx <= maxx && miny <= maxy)) return false;
    int64_t i0 = (int64_t)floor((minx + 1.0) * (double)S / 2.0 - 0.5) - 1, i1 = (int64_t)ceil((maxx + 1.0) * (double)S / 2.0 - 0.5) + 1;
    int64_t j0 = (int64_t)floor((miny + 1.0) * (double)S / 2.0 - 0.5) - 1, j1 = (int64_t)ceil((maxy + 1.0) * (double)S / 2.0 - 0.5) + 1;
    if (i0 < 0) i0 = 0;
    if (j0 < 0) j0 = 0;
    if (i1 > S - 1) i1 = S - 1;
    if (j1 > S - 1) j1 = S - 1;
    if (i0 > i1 || j0 > j1) return false;
    b = map::Box{(int32_t)i0, (int32_t)i1, (int32_t)j0, (int32_t)j1};
    return true;
}

// where pixel (i, j) of face f lies in the S x 6S map
WO_IMP_HD inline int64_t pixel_index(int32_t f, int32_t i, int32_t j, int32_t S) { return ((int64_t)f * S + j) * (int64_t)S + i; }

// The gnomonic projection as the shared raster (raster.hip) and the height pass (relief.hip) take it: the centres, the resident
// positions, the face size and the functions above under the names of map::Projection.  A side yields at most PIECES triangles: one
// per axis k, on the face in front of which the side's first vertex lies (ma > 0 holds on at most one face per axis).
struct Projection {
    static constexpr int PIECES = 3;
    using Side = float[3][3];                                 // a side's vertices: 3 floats each
    using Word = uint32_t;                                    // the per-pixel word of the side map
    const float* t_xyz;
    const float* r_xyz;
    int32_t S;
    WO_IMP_HD int64_t pixels() const { return (int64_t)FACE_COUNT * S * S; }
    // fetches side s; returns how many pieces it has
    WO_IMP_HD int vertices(const int32_t* triangles, const int32_t* halfedges, int64_t s, Side& v) const {
        side_vertices(triangles, halfedges, t_xyz, r_xyz, s, v);
        return PIECES;
    }
    // piece k of a side: its face, its triangle there, tri_area2 of it and its clipped box; false where nothing is drawn
    WO_IMP_HD bool piece(const Side& v, int k, map::Tri& t, double& area2, map::Box& b, int32_t& f) const {
        f = face_of_axis(k, v[0][k]);
        if (!side_on_face(v, f, t)) return false;
        area2 = map::tri_area2(t);
        return tri_box(t, area2, S, b);
    }
    WO_IMP_HD void center(int32_t i, int32_t j, double& xc, double& yc) const { xc = pixel_c(i, S); yc = pixel_c(j, S); }
    WO_IMP_HD int64_t index(int32_t f, int32_t i, int32_t j) const { return pixel_index(f, i, j, S); }      // in the side map
    // what side s leaves, under a minimum, at a pixel centre that its triangle covers: its index
    WO_IMP_HD Word word(const Side&, const map::Tri&, double, double, double, uint32_t s) const { return s; }
};

// the direction of the centre of pixel (i, j) of face f: the major axis is +-1, the other two come from ac and bc through the table
WO_IMP_HD inline void cube_direction(int32_t f, int64_t i, int64_t j, int32_t S, double d[3]) {
    const double a = pixel_c(i, S), b = pixel_c(j, S);
    switch (f) {
        case 0: d[0] = 1.0; d[1] = -b; d[2] = -a; break;
        case 1: d[0] = -1.0; d[1] = -b; d[2] = a; break;
        case 2: d[0] = a; d[1] = 1.0; d[2] = b; break;
        case 3: d[0] = a; d[1] = -1.0; d[2] = -b; break;
        case 4: d[0] = a; d[1] = -b; d[2] = 1.0; break;
        default: d[0] = -a; d[1] = -b; d[2] = -1.0; break;
    }
}

}  // namespace cube
}  // namespace wo
