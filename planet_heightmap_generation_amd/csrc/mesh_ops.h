// The arithmetic of the spherical Delaunay builder, once: the bodies shared by the host builder (mesh_builder.cc) and the device
// builder (mesh.hip), so that both compile the very same double operations (-ffp-contract=off is global) and the stars one side
// computes agree bit for bit with the stars of the other.
//
// Contract:
//   * orient(a, b, c, d) is det[b-a, c-a, d-a] evaluated on the index-sorted tuple, the sign fixed up by the permutation's parity:
//     the floating-point value, and so every decision, is the same from whichever star asks.
//   * The grid: cell edge h = min(0.5, 2 * sqrt(4 pi / V)), G = ceil(2 / h) + 1 cells per axis, origin -1; occupied cells in an
//     open-addressing table of key + 1 (0: empty) under `mix`.  A cell's point ids are ascending: with the fixed order of the
//     cells of a block (z, then y, then x) that defines the order of the candidates, and the Jarvis scan depends on that order
//     where orientations are exactly zero.
//   * star_at_level: nearest candidate (lowest index among equals) first, then Jarvis steps with a strict `> 0`, sequential in
//     candidate order; the star is accepted when every face's circumcap lies inside the searched block (or the level is brute).
//     A face whose outward normal n has n.P <= 0 sees the centre on its outer side: no block certifies it, and the brute level,
//     which has seen every point, refuses the star with FAIL_CENTRE_OUTSIDE: the points lie in a closed hemisphere, their hull is
//     no triangulation of the sphere.
//   * The candidate list is a template parameter with size(), operator[] and push(): a std::vector on the host, a strided slice of
//     LDS or of global scratch on the device.
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define WO_MESH_HD __host__ __device__
#else
#define WO_MESH_HD
#endif

namespace wo {
namespace mesh {

constexpr int MAX_STAR = 48;          // a star of more neighbours is a failure
constexpr int MAX_LEVEL = 6;          // levels 1..5 search a (2 level + 1)^3 block of cells, level 6 is brute
constexpr int STAR_INLINE = 12;       // neighbours kept in the common per-point storage
constexpr int FAIL_CENTRE_OUTSIDE = -4;   // failcode of a brute star with a face that does not have the centre strictly behind it

struct P3 { double x, y, z; };

// the f32 input is up to ~3e-8 off the unit sphere: the radial noise comes out before the hull is built.  false: zero length
WO_MESH_HD inline bool normalise(float fx, float fy, float fz, P3& out) {
    const double x = fx, y = fy, z = fz;
    const double l = sqrt(x * x + y * y + z * z);
    if (!(l > 0.0)) return false;
    out.x = x / l; out.y = y / l; out.z = z / l;
    return true;
}

struct Orient {
    const P3* pts;
    WO_MESH_HD inline double raw(int a, int b, int c, int d) const {
        const P3 &A = pts[a], &B = pts[b], &C = pts[c], &D = pts[d];
        const double bx = B.x - A.x, by = B.y - A.y, bz = B.z - A.z;
        const double cx = C.x - A.x, cy = C.y - A.y, cz = C.z - A.z;
        const double dx = D.x - A.x, dy = D.y - A.y, dz = D.z - A.z;
        return bx * (cy * dz - cz * dy) - by * (cx * dz - cz * dx) + bz * (cx * dy - cy * dx);
    }
    WO_MESH_HD inline double operator()(int a, int b, int c, int d) const {
        int v0 = a, v1 = b, v2 = c, v3 = d;
        int sgn = 1;
        // 4-element sorting network, tracking parity
#define WO_CSWAP(i, j) if (i > j) { int t = i; i = j; j = t; sgn = -sgn; }
        WO_CSWAP(v0, v1) WO_CSWAP(v2, v3) WO_CSWAP(v0, v2) WO_CSWAP(v1, v3) WO_CSWAP(v1, v2)
#undef WO_CSWAP
        return sgn * raw(v0, v1, v2, v3);
    }
};

// cell edge and cells per axis for V points
inline void grid_dims(int V, double& h, int& G) {
    const double spacing = std::sqrt(4.0 * 3.141592653589793 / (double)V);
    h = 2.0 * spacing;
    if (h > 0.5) h = 0.5;
    G = (int)std::ceil(2.0 / h) + 1;
}

// a view of the grid: the tables live with the caller (host vectors or device buffers)
struct GridView {
    double h;                     // cell edge
    int G;                        // cells per axis
    const uint64_t* hkey;         // open-addressing table: key + 1 (0 = empty)
    const int* hval;              // the cell of a slot; nullptr: the cell is the slot itself
    uint64_t hmask;
    const int* cellStart;         // per cell: start into sortedIdx; cellStart[c + 1] is its end
    const int* sortedIdx;         // point ids grouped by cell, ascending inside a cell

    WO_MESH_HD inline int coord(double v) const {
        int c = (int)floor((v + 1.0) / h);
        if (c < 0) c = 0;
        if (c >= G) c = G - 1;
        return c;
    }
    WO_MESH_HD inline uint64_t key(int ix, int iy, int iz) const {
        return (uint64_t)ix + (uint64_t)G * ((uint64_t)iy + (uint64_t)G * (uint64_t)iz);
    }
    WO_MESH_HD static inline uint64_t mix(uint64_t k) {
        k ^= k >> 33; k *= 0xff51afd7ed558ccdULL; k ^= k >> 33; k *= 0xc4ceb9fe1a85ec53ULL; k ^= k >> 33;
        return k;
    }
    // the table is never full, so the probe ends at an empty slot at the latest; the count bounds it all the same
    WO_MESH_HD inline int find(uint64_t k) const {
        uint64_t slot = mix(k) & hmask;
        for (uint64_t n = 0; n <= hmask; ++n) {
            const uint64_t v = hkey[slot];
            if (v == 0) return -1;
            if (v == k + 1) return hval ? hval[slot] : (int)slot;
            slot = (slot + 1) & hmask;
        }
        return -1;
    }
};

// the candidates of p at `level`: every other point (brute), or the points of the block of cells around (cx, cy, cz)
template <class Cand>
WO_MESH_HD inline void gather_candidates(int p, int V, const GridView& g, int cx, int cy, int cz, int level, bool brute, Cand& cand) {
    if (brute) {
        for (int i = 0; i < V; ++i) if (i != p) cand.push(i);
        return;
    }
    for (int dz = -level; dz <= level; ++dz) {
        int iz = cz + dz; if (iz < 0 || iz >= g.G) continue;
        for (int dy = -level; dy <= level; ++dy) {
            int iy = cy + dy; if (iy < 0 || iy >= g.G) continue;
            for (int dx = -level; dx <= level; ++dx) {
                int ix = cx + dx; if (ix < 0 || ix >= g.G) continue;
                int c = g.find(g.key(ix, iy, iz));
                if (c < 0) continue;
                for (int k = g.cellStart[c]; k < g.cellStart[c + 1]; ++k) {
                    int q = g.sortedIdx[k];
                    if (q != p) cand.push(q);
                }
            }
        }
    }
}

WO_MESH_HD inline bool level_is_brute(int level, int G) { return (level == MAX_LEVEL) || ((2 * level + 1) >= G); }

// Star of p from the candidates of one level (neighbours counter-clockwise seen from outside, out[MAX_STAR]).  Returns the degree
// when the star is accepted, -1 when the next level must try; failcode is set when the wrap itself failed.
template <class Cand>
WO_MESH_HD inline int star_at_level(int p, const P3* pts, const GridView& g, int cx, int cy, int cz, int level, bool brute,
                                    const Cand& cand, int* out, int& failcode) {
    const int nc = (int)cand.size();
    if (nc < 3) return -1;
    const P3 P = pts[p];
    const Orient orient{pts};
    // nearest candidate (lowest index on ties) is always a Delaunay neighbour
    int q0 = -1; double best = 1e300;
    for (int i = 0; i < nc; ++i) {
        const int q = cand[i];
        const double dx = pts[q].x - P.x, dy = pts[q].y - P.y, dz = pts[q].z - P.z;
        const double d2 = dx * dx + dy * dy + dz * dz;
        if (d2 < best || (d2 == best && q < q0)) { best = d2; q0 = q; }
    }
    int deg = 0; bool ok = true; bool certified = true;
    // searched block in coordinates (cells cx-level .. cx+level); the grid origin is -1
    const double lox = (cx - level) * g.h - 1.0, hix = (cx + level + 1) * g.h - 1.0;
    const double loy = (cy - level) * g.h - 1.0, hiy = (cy + level + 1) * g.h - 1.0;
    const double loz = (cz - level) * g.h - 1.0, hiz = (cz + level + 1) * g.h - 1.0;
    int q = q0;
    for (;;) {
        if (deg >= MAX_STAR) { ok = false; failcode = -2; break; }
        out[deg++] = q;
        // Jarvis step: r such that every other candidate lies on the origin side of plane (p,q,r)
        int r = -1;
        for (int i = 0; i < nc; ++i) {
            const int s = cand[i];
            if (s == q) continue;
            if (r < 0) { r = s; continue; }
            if (orient(p, q, r, s) > 0.0) r = s;
        }
        // circumcap of (p,q,r): centre direction n = (q-p)x(r-p) (outward).  Every point of the cap is
        // within chord distance |c - p| of the centre c = n/|n|; the face is certified empty when that
        // ball lies inside the searched block of grid cells.
        {
            const P3 &Q = pts[q], &R = pts[r];
            const double ax = Q.x - P.x, ay = Q.y - P.y, az = Q.z - P.z;
            const double bx = R.x - P.x, by = R.y - P.y, bz = R.z - P.z;
            double nx = ay * bz - az * by, ny = az * bx - ax * bz, nz = ax * by - ay * bx;
            const double nl = sqrt(nx * nx + ny * ny + nz * nz);
            if (!(nl > 0.0)) { ok = false; failcode = -3; break; }
            nx /= nl; ny /= nl; nz /= nl;
            if (nx * P.x + ny * P.y + nz * P.z <= 0.0) {
                if (brute) { ok = false; failcode = FAIL_CENTRE_OUTSIDE; break; }
                certified = false;
            } else {
                const double ex = nx - P.x, ey = ny - P.y, ez = nz - P.z;
                const double rad = sqrt(ex * ex + ey * ey + ez * ez) * 1.000001 + 1e-12;
                if (nx - rad < lox || nx + rad > hix || ny - rad < loy || ny + rad > hiy ||
                    nz - rad < loz || nz + rad > hiz) certified = false;
            }
        }
        q = r;
        if (q == q0) break;
    }
    if (!ok) return -1;
    if (brute || certified) return deg;
    return -1;
}

// position of the lowest neighbour: the star is stored rotated to start there
WO_MESH_HD inline int lowest_position(const int* st, int d) {
    int m = 0;
    for (int i = 1; i < d; ++i) if (st[i] < st[m]) m = i;
    return m;
}

// pass 2: does p own the triangle (p, q, r)?  The owner is the lowest vertex.
WO_MESH_HD inline bool owns(int p, int q, int r) { return p < q && p < r; }

// pass 3: the triangle (v, u, w) written from its owner m as (m, a, .) counter-clockwise
WO_MESH_HD inline void owner_of(int v, int u, int w, int& m, int& a) {
    m = v; a = u;
    if (u < m && u < w) { m = u; a = w; }
    else if (w < m && w < u) { m = w; a = v; }
}

WO_MESH_HD inline int next_side(int s) { return (s % 3 == 2) ? s - 2 : s + 1; }

// computeNeighborDist (js/sphere-mesh.js:191-203): the chord between two f32 positions, in double, stored as f32
WO_MESH_HD inline float chord(double x, double y, double z, float qx, float qy, float qz) {
    const double dx = x - (double)qx, dy = y - (double)qy, dz = z - (double)qz;
    return (float)sqrt(dx * dx + dy * dy + dz * dz);
}

}  // namespace mesh
}  // namespace wo
