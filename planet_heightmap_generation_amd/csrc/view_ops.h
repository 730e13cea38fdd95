// The globe view: the displaced globe mesh seen through a camera, with a depth per pixel and a Lambert term per facet.  The
// per-vertex, per-side and per-pixel bodies shared by the device kernels (view.hip, raster.hip) and the test-only CPU emulator
// (tests/emu_view), so that both compile the very same arithmetic.  The library compiles with -ffp-contract=off: no FMA changes a
// result.  Everything is double arithmetic on f32 inputs with + - * /, floor / ceil / fmin / fmax and sqrt, which is correctly
// rounded on both sides, as in relief_ops.h; the tangent of the field of view is taken once on the host.  Ours: the reference draws
// this picture with three.js (js/scene.js: a perspective camera of 50 degrees at (0, 0.4, 2.8) that orbits the origin, an ambient
// light and a sun at (5, 3, 4)), whose rasteriser, lighting and tone pipeline are NOT reproduced; this header is the contract.
//
// Camera.  eye[3] in double, finite and not the origin; the target is the origin.  fovY in degrees: 0 < fovY < 180 is a perspective
//   camera, fovY == 0 an orthographic one of half height halfHeight > 0.  The basis, computed once on the host (camera_make) and
//   handed to the kernels as doubles: z = eye / |eye| with |eye| = sqrt((ex ex + ey ey) + ez ez); x = (0, 1, 0) x z = (z.z, 0, -z.x)
//   divided by its length sqrt(z.z z.z + z.x z.x), or (1, 0, 0) when that length is below 1e-12 (the view from a pole); y = z x x.
//   For a vertex v (three f32 taken as doubles): d = v - origin with origin = eye (perspective) or 10 z (orthographic: a plane at a
//   fixed distance of 10, so every vertex of a planet has zc > 0); xr = x . d, yu = y . d, zc = -(z . d), every dot product summed
//   (a0 b0 + a1 b1) + a2 b2.  Screen position: perspective f = 1 / tan(fovY pi / 180 / 2), a = (f xr) / zc, b = -((f yu) / zc);
//   orthographic f = 1 / halfHeight, a = f xr, b = -(f yu); stored as f32 in a map::Tri (Tri.x = a, Tri.y = b), so that tri_area2,
//   tri_covers and edge_fn are reused unchanged: a camera maps a flat triangle to a flat triangle.  Row 0 is the top of the image.
// Pixels.  W x H, each from 1 to 16384, odd sizes allowed.  The centre of pixel (i, j): ac = (2 (i + 0.5) - W) / H, bc = (2 (j + 0.5)
//   - H) / H in double, in this order of operations: b spans [-1, 1], a spans [-W / H, W / H].
// Bounding box.  cube::tri_box's construction: that of the f32 positions, intersected with the image [-W / H, W / H] x [-1, 1] in
//   double BEFORE any conversion to integer, then one pixel wider on every side.
// Vertices.  Exactly the globe mesh's f32 positions (globe_ops.h: the Center records and side_positions), with one parameter:
//   exaggeration >= 0 multiplies globe::V in double (v = V * exaggeration).  1 gives the bits of wo_globe_mesh, 0 the smooth sphere.
// Which sides are drawn.  A side is drawn iff (i) all three zc > 0: a side with a vertex behind the camera is not drawn, neither
//   clipped nor split, as on a cube face; (ii) it faces the camera: with n = (v1 - v0) x (v2 - v0) in the winding side_positions
//   leaves (n . centroid >= 0), in double on the stored f32 positions, perspective n . (eye - v0) > 0, orthographic n . z > 0 (a NaN
//   fails); (iii) area2 of the projected triangle is neither 0 nor NaN.  The mesh is a radial graph over the sphere, so on a closed
//   mesh a side turned away is always hidden by one that is not; the test is part of the contract all the same.
// Depth.  For a pixel centre that a drawn side covers (tri_covers, closed edges) the depth is the side's zc there, stored as f32.
//   With e0, e1, e2 the edge functions of tri_covers over the f32 screen positions (relief_ops.h: edges_at): perspective
//   w0 = (e1 / area2) / zc0, w1 = (e2 / area2) / zc1, w2 = (e0 / area2) / zc2, depth = 1 / ((w0 + w1) + w2) (perspective-correct: the
//   form of relief::height_perspective with zc in the place of ma); orthographic depth = ((e1 zc0 + e2 zc1) + e0 zc2) / area2 (the
//   form of relief::height_planar).
// The winner.  The smallest depth; among equal f32 depths the lowest side index.  As one word: key = bits(depth) << 32 | side under
//   a 64-bit minimum (a positive float's bits order as the float does).  A depth that is not > 0 is not written.  The result
//   depends on pixel and side only, never on the order of arrival.
// Outputs per pixel.  Region: triangles[side], or -1.  Depth: f32, the quiet NaN 0x7FC00000 where nothing covers.  Lambert (with a
//   shading request only): max(0, nhat . lhat) of the winning side as f32, n as above divided component by component by its length
//   sqrt(n . n), lhat the light direction in world space normalised in the same way on the host; a NaN gives 0; 0 where nothing
//   covers.
// Shading of an RGBA pixel.  Each of R, G, B becomes min(255, floor(c * (ambient + diffuse * lambert) + 0.5)) in double; alpha is
//   kept.  ambient and diffuse are finite and >= 0; the defaults 0.55 and 0.45 let a facet that faces the light keep its colour.
//   Uncovered pixels take the request's background word (R | G << 8 | B << 16 | A << 24) as it stands, unshaded.
#pragma once
#include <cmath>
#include <cstdint>

#include "globe_ops.h"
#include "map_ops.h"
#include "relief_ops.h"

namespace wo {
namespace view {

namespace M = wo::map;
namespace G = wo::globe;
namespace R = wo::relief;

constexpr int32_t MAX_SIZE = 16384;
constexpr double ORTHO_DISTANCE = 10.0;
constexpr unsigned long long NO_KEY = ~0ull;
constexpr uint32_t DEFAULT_BACKGROUND = 0xFF080303u;          // the reference's scene colour 0x030308, opaque

WO_IMP_HD inline bool size_ok(int32_t n) { return n >= 1 && n <= MAX_SIZE; }

// ---- camera -------------------------------------------------------------------------------------------------------------------
struct Camera {
    double origin[3];                                         // what a vertex is taken against: the eye, or 10 z
    double x[3], y[3], z[3];
    double f;
    int32_t ortho;
};

WO_IMP_HD inline bool finite3(const double v[3]) { return v[0] - v[0] == 0.0 && v[1] - v[1] == 0.0 && v[2] - v[2] == 0.0; }
// v / |v|; false for a vector that is zero or not finite, or whose length is
WO_IMP_HD inline bool unit3(const double v[3], double out[3]) {
    if (!finite3(v)) return false;
    const double len = sqrt(R::dot3(v, v));
    if (!(len > 0.0) || !(len - len == 0.0)) return false;
    out[0] = v[0] / len; out[1] = v[1] / len; out[2] = v[2] / len;
    return true;
}
// the basis and the origin; f is the caller's (camera_make).  false: the eye is zero or not finite
WO_IMP_HD inline bool camera_basis(const double eye[3], bool ortho, Camera& c) {
    if (!unit3(eye, c.z)) return false;
    const double xl = sqrt(c.z[2] * c.z[2] + c.z[0] * c.z[0]);
    if (xl < 1e-12) { c.x[0] = 1.0; c.x[1] = 0.0; c.x[2] = 0.0; }
    else { c.x[0] = c.z[2] / xl; c.x[1] = 0.0; c.x[2] = -c.z[0] / xl; }
    R::cross3(c.z, c.x, c.y);
    for (int k = 0; k < 3; ++k) c.origin[k] = ortho ? ORTHO_DISTANCE * c.z[k] : eye[k];
    c.ortho = ortho ? 1 : 0;
    return true;
}
// host only (tan is the host libm's).  CAMERA_OK, or which argument is out of range
enum : int { CAMERA_OK = 0, CAMERA_BAD_EYE, CAMERA_BAD_FOV, CAMERA_BAD_HALF_HEIGHT };
inline int camera_make(const double eye[3], double fovY, double halfHeight, Camera& c) {
    const bool ortho = fovY == 0.0;
    if (!camera_basis(eye, ortho, c)) return CAMERA_BAD_EYE;
    if (!ortho && !(fovY > 0.0 && fovY < 180.0)) return CAMERA_BAD_FOV;
    if (ortho && !(halfHeight > 0.0 && halfHeight - halfHeight == 0.0)) return CAMERA_BAD_HALF_HEIGHT;
    c.f = ortho ? 1.0 / halfHeight : 1.0 / std::tan(fovY * 3.141592653589793 / 180.0 / 2.0);
    return CAMERA_OK;
}

// ---- a side -------------------------------------------------------------------------------------------------------------------
struct Side {
    float p[9];                                               // the globe mesh's positions: side_positions' nine floats
    double zc[3];
    float a[3], b[3];                                         // the screen positions
};

// zc and the screen position of one vertex
WO_IMP_HD inline void camera_vertex(const Camera& c, const float v[3], double& zc, float& a, float& b) {
    const double d[3] = {(double)v[0] - c.origin[0], (double)v[1] - c.origin[1], (double)v[2] - c.origin[2]};
    const double xr = R::dot3(c.x, d), yu = R::dot3(c.y, d);
    zc = -R::dot3(c.z, d);
    if (c.ortho) { a = (float)(c.f * xr); b = (float)(-(c.f * yu)); }
    else { a = (float)((c.f * xr) / zc); b = (float)(-((c.f * yu) / zc)); }
}
// n = (v1 - v0) x (v2 - v0) of the stored positions
WO_IMP_HD inline void side_normal(const float p[9], double n[3]) {
    const double e1[3] = {(double)p[3] - (double)p[0], (double)p[4] - (double)p[1], (double)p[5] - (double)p[2]};
    const double e2[3] = {(double)p[6] - (double)p[0], (double)p[7] - (double)p[1], (double)p[8] - (double)p[2]};
    R::cross3(e1, e2, n);
}
WO_IMP_HD inline bool side_faces(const Camera& c, const float p[9]) {
    double n[3];
    side_normal(p, n);
    if (c.ortho) return R::dot3(n, c.z) > 0.0;
    const double t[3] = {c.origin[0] - (double)p[0], c.origin[1] - (double)p[1], c.origin[2] - (double)p[2]};
    return R::dot3(n, t) > 0.0;
}
// the nine floats of side s; v = globe::V * exaggeration
WO_IMP_HD inline void side_floats(const int32_t* triangles, const int32_t* halfedges, const G::Center* centers, const float* r_xyz, const float* r_elevation, double v, int64_t s,
                                  float p[9]) {
    const int64_t br = triangles[s];
    const float r[3] = {r_xyz[3 * br], r_xyz[3 * br + 1], r_xyz[3 * br + 2]};
    G::side_positions(centers[s / 3], centers[halfedges[s] / 3], r, r_elevation[br], v, p);
}
// side s of the mesh through the camera
WO_IMP_HD inline void side_make(const Camera& c, const int32_t* triangles, const int32_t* halfedges, const G::Center* centers, const float* r_xyz, const float* r_elevation,
                                double v, int64_t s, Side& out) {
    side_floats(triangles, halfedges, centers, r_xyz, r_elevation, v, s, out.p);
    for (int k = 0; k < 3; ++k) camera_vertex(c, out.p + 3 * k, out.zc[k], out.a[k], out.b[k]);
}
// rules (i) and (ii), and the projected triangle
WO_IMP_HD inline bool side_triangle(const Camera& c, const Side& v, M::Tri& t) {
    if (!(v.zc[0] > 0.0 && v.zc[1] > 0.0 && v.zc[2] > 0.0)) return false;
    if (!side_faces(c, v.p)) return false;
    for (int k = 0; k < 3; ++k) { t.x[k] = v.a[k]; t.y[k] = v.b[k]; }
    return true;
}

// ---- pixels -------------------------------------------------------------------------------------------------------------------
WO_IMP_HD inline double pixel_a(int64_t i, int32_t W, int32_t H) { return (2.0 * ((double)i + 0.5) - (double)W) / (double)H; }
WO_IMP_HD inline double pixel_b(int64_t j, int32_t H) { return (2.0 * ((double)j + 0.5) - (double)H) / (double)H; }

// The pixels whose centres can lie in the triangle's bounding box, one pixel wider on every side than the arithmetic asks for (the
// exact test is map::tri_covers).  Returns false for a triangle that covers nothing.  fmin / fmax pass over a NaN; an area2 that is
// neither 0 nor NaN has no NaN position.
WO_IMP_HD inline bool tri_box(const M::Tri& t, double area2, int32_t W, int32_t H, M::Box& b) {
    if (!(area2 > 0.0 || area2 < 0.0)) return false;
    double minx = fmin(fmin((double)t.x[0], (double)t.x[1]), (double)t.x[2]), maxx = fmax(fmax((double)t.x[0], (double)t.x[1]), (double)t.x[2]);
    double miny = fmin(fmin((double)t.y[0], (double)t.y[1]), (double)t.y[2]), maxy = fmax(fmax((double)t.y[0], (double)t.y[1]), (double)t.y[2]);
    const double aspect = (double)W / (double)H;
    minx = fmax(minx, -aspect); maxx = fmin(maxx, aspect);    // the image, before any integer
    miny = fmax(miny, -1.0); maxy = fmin(maxy, 1.0);
    if (!(minx <= maxx && miny <= maxy)) return false;
    int64_t i0 = (int64_t)floor((minx * (double)H + (double)W) / 2.0 - 0.5) - 1, i1 = (int64_t)ceil((maxx * (double)H + (double)W) / 2.0 - 0.5) + 1;
    int64_t j0 = (int64_t)floor((miny * (double)H + (double)H) / 2.0 - 0.5) - 1, j1 = (int64_t)ceil((maxy * (double)H + (double)H) / 2.0 - 0.5) + 1;
    if (i0 < 0) i0 = 0;
    if (j0 < 0) j0 = 0;
    if (i1 > W - 1) i1 = W - 1;
    if (j1 > H - 1) j1 = H - 1;
    if (i0 > i1 || j0 > j1) return false;
    b = M::Box{(int32_t)i0, (int32_t)i1, (int32_t)j0, (int32_t)j1};
    return true;
}

// ---- depth and the key --------------------------------------------------------------------------------------------------------
WO_IMP_HD inline float depth_at(bool ortho, const M::Tri& t, double area2, double xc, double yc, const double zc[3]) {
    const R::Edges e = R::edges_at(t, xc, yc);
    if (ortho) return (float)(((e.e1 * zc[0] + e.e2 * zc[1]) + e.e0 * zc[2]) / area2);
    const double w0 = (e.e1 / area2) / zc[0], w1 = (e.e2 / area2) / zc[1], w2 = (e.e0 / area2) / zc[2];
    return (float)(1.0 / ((w0 + w1) + w2));
}
WO_IMP_HD inline unsigned long long depth_key(float depth, uint32_t s) {
    if (!(depth > 0.0f)) return NO_KEY;                       // the minimum leaves the pixel as it is
    return ((unsigned long long)M::f32_bits(depth) << 32) | (unsigned long long)s;
}

// ---- the projection -----------------------------------------------------------------------------------------------------------
// The camera as the shared raster (raster.hip) takes it: the centre records, the resident positions, the elevation, the camera and
// the functions above under the names of map::Projection.  A side yields one triangle.  The per-pixel word is the key.
struct Projection {
    static constexpr int PIECES = 1;
    using Side = view::Side;
    using Word = unsigned long long;                          // what the 64-bit atomicMin takes
    const G::Center* centers;
    const float* r_xyz;
    const float* r_elevation;
    Camera cam;
    double v;                                                 // globe::V * exaggeration
    int32_t W, H;
    WO_IMP_HD int64_t pixels() const { return (int64_t)W * H; }
    WO_IMP_HD int vertices(const int32_t* triangles, const int32_t* halfedges, int64_t s, Side& out) const {
        side_make(cam, triangles, halfedges, centers, r_xyz, r_elevation, v, s, out);
        return PIECES;
    }
    WO_IMP_HD bool piece(const Side& s, int, M::Tri& t, double& area2, M::Box& b, int32_t& f) const {
        f = 0;
        if (!side_triangle(cam, s, t)) return false;
        area2 = M::tri_area2(t);
        return view::tri_box(t, area2, W, H, b);
    }
    WO_IMP_HD void center(int32_t i, int32_t j, double& xc, double& yc) const { xc = pixel_a(i, W, H); yc = pixel_b(j, H); }
    WO_IMP_HD int64_t index(int32_t, int32_t i, int32_t j) const { return (int64_t)j * W + i; }
    // what side s leaves at a pixel centre that its triangle covers
    WO_IMP_HD Word word(const Side& sd, const M::Tri& t, double area2, double xc, double yc, uint32_t s) const {
        return depth_key(depth_at(cam.ortho != 0, t, area2, xc, yc, sd.zc), s);
    }
};

// ---- what a pixel holds -------------------------------------------------------------------------------------------------------
// light: a unit vector
WO_IMP_HD inline float side_lambert(const float p[9], const double light[3]) {
    double n[3];
    side_normal(p, n);
    const double len = sqrt(R::dot3(n, n));
    const double nh[3] = {n[0] / len, n[1] / len, n[2] / len};
    const double d = R::dot3(nh, light);
    return d > 0.0 ? (float)d : 0.0f;
}

struct Pixel { int32_t region; float depth, lambert; };
// shade false: no shading request, lambert is 0 and the light (lx, ly, lz) is not read
WO_IMP_HD inline Pixel pixel_of(const Projection& P, const int32_t* triangles, const int32_t* halfedges, unsigned long long key, bool shade, double lx, double ly, double lz) {
    if (key == NO_KEY) return Pixel{-1, R::quiet_nan(), 0.0f};
    const uint32_t s = (uint32_t)key;
    Pixel out{triangles[s], M::f32_of_bits((uint32_t)(key >> 32)), 0.0f};
    if (shade) {
        const double light[3] = {lx, ly, lz};
        float p[9];
        side_floats(triangles, halfedges, P.centers, P.r_xyz, P.r_elevation, P.v, s, p);
        out.lambert = side_lambert(p, light);
    }
    return out;
}

// ---- shading ------------------------------------------------------------------------------------------------------------------
WO_IMP_HD inline uint32_t shade_channel(uint32_t c, double gain) {
    const double v = floor((double)c * gain + 0.5);
    return v < 255.0 ? (uint32_t)v : 255u;
}
WO_IMP_HD inline uint32_t shade_rgba(uint32_t rgba, float lambert, double ambient, double diffuse) {
    const double gain = ambient + diffuse * (double)lambert;
    return shade_channel(rgba & 0xFFu, gain) | (shade_channel((rgba >> 8) & 0xFFu, gain) << 8) | (shade_channel((rgba >> 16) & 0xFFu, gain) << 16) | (rgba & 0xFF000000u);
}

}  // namespace view
}  // namespace wo
