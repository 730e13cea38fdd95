// Native sphere-mesh producer: Fibonacci points -> spherical Delaunay (3-D convex hull of the
// unit-sphere points, pole included) -> triangles/halfedges -> CSR neighbour graph.
//
// This replaces the reference's input producer for the hot path:
//   generateFibonacciSphere      js/sphere-mesh.js:9-37
//   stereographic Delaunay + addPoleToMesh   js/sphere-mesh.js:41-90,174-186  (delaunator@5.0.1 there)
//   SphereMesh CSR construction  js/sphere-mesh.js:94-146
//   computeNeighborDist          js/sphere-mesh.js:191-203
//
// Design (not a port): the reference triangulates a stereographic projection with a sweep-hull and then
// stitches the projection pole back in.  The planar Delaunay of the projected points plus that pole fan
// is exactly the convex hull of {points} U {pole}; we build that hull directly and in parallel: every
// point computes its own star by gift-wrapping the candidates found in a hashed 3-D grid, with an
// empty-circumcap certificate that widens the search when needed.  All orientation predicates are
// evaluated on the index-sorted 4-tuple so every star sees bit-identical decisions, which makes the
// independently computed stars mutually consistent.  Triangles are wound counter-clockwise seen from
// outside the sphere.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <cstdlib>
#include <atomic>
#include <string>
#include <vector>

#include "host_util.h"
#include "mesh_ops.h"
#include "wo_internal.h"

namespace wo {

// ---------------------------------------------------------------------------------------------
// Points (js/sphere-mesh.js:9-37).  Sequential because the reference draws four LCG values per
// point in a fixed order; evaluation order of every expression follows the JS left-to-right rules.
// ---------------------------------------------------------------------------------------------
void fib_sphere_points(int N, double jitter, double seed, float* xyz /* 3*(N+1) */) {
    ParkMiller rng(seed);
    const double PI = 3.141592653589793;
    const double s = 3.6 / std::sqrt((double)N);
    const double dlong = PI * (3.0 - std::sqrt(5.0));
    const double dz = 2.0 / (double)N;
    double lng = 0.0, z = 1.0 - dz / 2.0;
    for (int k = 0; k < N; ++k) {
        const double r = std::sqrt(1.0 - z * z);
        double latDeg = std::asin(z) * 180.0 / PI;
        double lonDeg = lng * 180.0 / PI;
        if (jitter > 0) {
            double a = rng.next(); double b = rng.next();
            const double jLat = a - b;
            a = rng.next(); b = rng.next();
            const double jLon = a - b;
            const double nextZ = std::max(-1.0, z - dz * 2.0 * PI * r / s);
            latDeg += jitter * jLat * (latDeg - std::asin(nextZ) * 180.0 / PI);
            lonDeg += jitter * jLon * (s / r * 180.0 / PI);
        }
        const double latR = latDeg * PI / 180.0;
        const double lonR = lonDeg * PI / 180.0;
        xyz[3 * k]     = (float)(std::cos(latR) * std::cos(lonR));
        xyz[3 * k + 1] = (float)(std::cos(latR) * std::sin(lonR));
        xyz[3 * k + 2] = (float)(std::sin(latR));
        lng += dlong;
        z -= dz;
    }
    // pole region appended by buildSphere (js/sphere-mesh.js:179-181)
    xyz[3 * N] = 0.f; xyz[3 * N + 1] = 0.f; xyz[3 * N + 2] = 1.f;
}

// ---------------------------------------------------------------------------------------------
// Spherical Delaunay
// ---------------------------------------------------------------------------------------------
namespace {

using mesh::P3;
using mesh::Orient;
using mesh::MAX_STAR;

// the grid's tables; mesh_ops.h's GridView reads them
struct Grid {
    double h;       // cell edge
    int G;          // cells per axis
    std::vector<uint64_t> cellKey;   // sorted unique keys
    std::vector<int> cellStart;      // start into sortedIdx, size = cells+1
    std::vector<int> sortedIdx;      // point ids grouped by cell
    std::vector<uint64_t> hkey;      // open-addressing table: key+1 (0 = empty)
    std::vector<int> hval;
    uint64_t hmask;
    mesh::GridView view() const { return mesh::GridView{h, G, hkey.data(), hval.data(), hmask, cellStart.data(), sortedIdx.data()}; }
};

void radix_sort_pairs(std::vector<uint64_t>& keys, std::vector<int>& vals, int bits) {
    const size_t n = keys.size();
    std::vector<uint64_t> k2(n);
    std::vector<int> v2(n);
    for (int shift = 0; shift < bits; shift += 11) {
        size_t cnt[2049];
        std::memset(cnt, 0, sizeof(cnt));
        for (size_t i = 0; i < n; ++i) cnt[((keys[i] >> shift) & 2047) + 1]++;
        for (int b = 0; b < 2048; ++b) cnt[b + 1] += cnt[b];
        for (size_t i = 0; i < n; ++i) {
            size_t d = cnt[(keys[i] >> shift) & 2047]++;
            k2[d] = keys[i]; v2[d] = vals[i];
        }
        keys.swap(k2); vals.swap(v2);
    }
}

void build_grid(Grid& g, const P3* pts, int V) {
    mesh::grid_dims(V, g.h, g.G);
    std::vector<uint64_t> keys(V);
    std::vector<int> vals(V);
    {
        const mesh::GridView gv = g.view();      // coord and key read h and G only
        parallel_ranges(V, [&](int64_t b, int64_t e, int) {
            for (int64_t i = b; i < e; ++i) {
                keys[i] = gv.key(gv.coord(pts[i].x), gv.coord(pts[i].y), gv.coord(pts[i].z));
                vals[i] = (int)i;
            }
        });
    }
    int bits = 1;
    { uint64_t mx = (uint64_t)g.G * g.G * g.G; while ((1ULL << bits) < mx) ++bits; }
    radix_sort_pairs(keys, vals, bits);
    g.sortedIdx.swap(vals);
    g.cellKey.clear(); g.cellStart.clear();
    for (int i = 0; i < V; ++i) {
        if (i == 0 || keys[i] != keys[i - 1]) { g.cellKey.push_back(keys[i]); g.cellStart.push_back(i); }
    }
    g.cellStart.push_back(V);
    size_t cap = 16;
    while (cap < g.cellKey.size() * 2 + 8) cap <<= 1;
    g.hkey.assign(cap, 0); g.hval.assign(cap, -1); g.hmask = cap - 1;
    for (size_t c = 0; c < g.cellKey.size(); ++c) {
        uint64_t slot = mesh::GridView::mix(g.cellKey[c]) & g.hmask;
        while (g.hkey[slot] != 0) slot = (slot + 1) & g.hmask;
        g.hkey[slot] = g.cellKey[c] + 1; g.hval[slot] = (int)c;
    }
}

// the candidate list of mesh_ops.h on a vector
struct VecCand {
    std::vector<int>& v;
    size_t size() const { return v.size(); }
    int operator[](int i) const { return v[i]; }
    void push(int q) { v.push_back(q); }
};

// Star of p (neighbours counter-clockwise seen from outside).  Returns degree, or <0 on failure.
int star_of(int p, const P3* pts, int V, const mesh::GridView& g, int* out, std::vector<int>& candStore) {
    const P3 P = pts[p];
    const int cx = g.coord(P.x), cy = g.coord(P.y), cz = g.coord(P.z);
    int failcode = -1;
    VecCand cand{candStore};
    for (int level = 1; level <= mesh::MAX_LEVEL; ++level) {
        candStore.clear();
        const bool brute = mesh::level_is_brute(level, g.G);
        mesh::gather_candidates(p, V, g, cx, cy, cz, level, brute, cand);
        const int d = mesh::star_at_level(p, pts, g, cx, cy, cz, level, brute, cand, out, failcode);
        if (d >= 0) return d;
    }
    return failcode;
}

// the normalised points; false: a zero-length point
bool normalise_points(int V, const float* xyz, std::vector<P3>& pts) {
    pts.resize(V);
    for (int i = 0; i < V; ++i)
        if (!mesh::normalise(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], pts[i])) return false;
    return true;
}

}  // namespace

// The stars of the listed points, as sphere_delaunay computes them (the device builder's completion, mesh.hip): degOut[i] is the
// degree of ids[i], 0 for a failed star, and starsOut holds the stars back to back, rotated to their lowest neighbour.
// Returns the number of failed stars, -1 for a zero-length point.
int stars_on_host(int V, const float* xyz, int n, const int* ids, std::vector<int>& degOut, std::vector<int>& starsOut, int* centreOutside) {
    if (centreOutside) *centreOutside = 0;
    std::vector<P3> pts;
    if (!normalise_points(V, xyz, pts)) return -1;
    Grid g;
    build_grid(g, pts.data(), V);
    const mesh::GridView gv = g.view();
    degOut.assign(n, 0);
    std::vector<int> flat((size_t)n * MAX_STAR);
    std::atomic<int> failed{0}, outside{0};
    parallel_ranges(n, [&](int64_t b, int64_t e, int) {
        std::vector<int> cand; cand.reserve(256);
        int st[MAX_STAR];
        for (int64_t i = b; i < e; ++i) {
            const int d = star_of(ids[i], pts.data(), V, gv, st, cand);
            if (d < 3) { failed.fetch_add(1); if (d == mesh::FAIL_CENTRE_OUTSIDE) outside.fetch_add(1); continue; }
            const int m = mesh::lowest_position(st, d);
            degOut[i] = d;
            for (int k = 0; k < d; ++k) flat[(size_t)i * MAX_STAR + k] = st[(m + k) % d];
        }
    }, 64);
    starsOut.clear();
    for (int i = 0; i < n; ++i) starsOut.insert(starsOut.end(), flat.begin() + (size_t)i * MAX_STAR, flat.begin() + (size_t)i * MAX_STAR + degOut[i]);
    if (centreOutside) *centreOutside = outside.load();
    return failed.load();
}

std::string star_failure_message(long long failed, long long centreOutside) {
    if (centreOutside > 0)
        return "sphere_delaunay: the hull of the points does not hold the sphere's centre strictly inside (" + std::to_string(centreOutside) +
               " points have a face that sees it): the points lie in a hemisphere and have no triangulation of the sphere";
    return "sphere_delaunay: star construction failed for " + std::to_string(failed) + " points";
}

// triangles/halfedges sized 3*(2V-4).  Returns 0 on success.
int sphere_delaunay(int V, const float* xyz, int* triangles, int* halfedges, std::string& err) {
    if (V < 4) { err = "sphere_delaunay: need at least 4 points"; return 1; }
    // The float32 inputs sit up to ~3e-8 off the unit sphere, enough to push one of two nearly
    // coincident points (they occur from ~1e6 jittered points up) inside the hull of the others; a planar
    // Delaunay of the projection keeps every point, so we take the radial noise out before building the hull.
    std::vector<P3> pts;
    if (!normalise_points(V, xyz, pts)) { err = "sphere_delaunay: zero-length point"; return 1; }
    Grid g;
    build_grid(g, pts.data(), V);
    const mesh::GridView gv = g.view();

    // pass 1: stars (degree + neighbours, rotated to start at the lowest-index neighbour)
    std::vector<int> deg(V);
    std::vector<int> starBuf((size_t)V * 12);         // common case storage
    std::vector<std::vector<int>> bigStar;            // rare degree > 12
    std::vector<int> bigIndex(V, -1);
    std::atomic<int> failed{0}, outside{0};
    std::vector<std::vector<std::pair<int, std::vector<int>>>> bigLocal(host_threads() + 1);
    parallel_ranges(V, [&](int64_t b, int64_t e, int tid) {
        std::vector<int> cand; cand.reserve(256);
        int st[MAX_STAR];
        for (int64_t p = b; p < e; ++p) {
            int d = star_of((int)p, pts.data(), V, gv, st, cand);
            if (d == mesh::FAIL_CENTRE_OUTSIDE) outside.fetch_add(1);
            if (d < 3) { if (failed.fetch_add(1) == 0) fprintf(stderr, "star fail p=%d code=%d xyz=%.9g %.9g %.9g\n", (int)p, d, pts[p].x, pts[p].y, pts[p].z); deg[p] = 0; continue; }
            const int m = mesh::lowest_position(st, d);
            deg[p] = d;
            if (d <= 12) {
                for (int i = 0; i < d; ++i) starBuf[(size_t)p * 12 + i] = st[(m + i) % d];
            } else {
                std::vector<int> v(d);
                for (int i = 0; i < d; ++i) v[i] = st[(m + i) % d];
                bigLocal[tid].emplace_back((int)p, std::move(v));
            }
        }
    }, 1024);
    if (failed.load() != 0) { err = star_failure_message(failed.load(), outside.load()); return 2; }
    for (auto& l : bigLocal) for (auto& pr : l) { bigIndex[pr.first] = (int)bigStar.size(); bigStar.push_back(std::move(pr.second)); }
    auto star = [&](int p) -> const int* { return bigIndex[p] >= 0 ? bigStar[bigIndex[p]].data() : &starBuf[(size_t)p * 12]; };

    // pass 2: triangle ownership (owner = lowest vertex), ids by (owner, star position)
    std::vector<int64_t> starOff(V + 1, 0);
    for (int p = 0; p < V; ++p) starOff[p + 1] = starOff[p] + deg[p];
    std::vector<int> triOfStar(starOff[V], -1);
    std::vector<int> ownCount(V + 1, 0);
    parallel_ranges(V, [&](int64_t b, int64_t e, int) {
        for (int64_t p = b; p < e; ++p) {
            const int* s = star((int)p); int d = deg[p], c = 0;
            for (int i = 0; i < d; ++i) { int q = s[i], r = s[(i + 1) % d]; if (mesh::owns((int)p, q, r)) ++c; }
            ownCount[p + 1] = c;
        }
    });
    for (int p = 0; p < V; ++p) ownCount[p + 1] += ownCount[p];
    const int T = ownCount[V];
    if (T != 2 * V - 4) { err = "sphere_delaunay: triangle count " + std::to_string(T) + " != 2V-4 (inconsistent stars)"; return 3; }
    parallel_ranges(V, [&](int64_t b, int64_t e, int) {
        for (int64_t p = b; p < e; ++p) {
            const int* s = star((int)p); int d = deg[p]; int t = ownCount[p];
            for (int i = 0; i < d; ++i) {
                int q = s[i], r = s[(i + 1) % d];
                if (mesh::owns((int)p, q, r)) {
                    triangles[3 * t] = (int)p; triangles[3 * t + 1] = q; triangles[3 * t + 2] = r;
                    triOfStar[starOff[p] + i] = t; ++t;
                }
            }
        }
    });
    // pass 3: halfedges.  Side s = (u -> v) of triangle t; its twin is side (v -> u) of the triangle
    // (v, u, w) where w follows u in v's star.
    std::atomic<int> bad{0};
    parallel_ranges(T, [&](int64_t b, int64_t e, int) {
        for (int64_t t = b; t < e; ++t) {
            for (int k = 0; k < 3; ++k) {
                const int u = triangles[3 * t + k], v = triangles[3 * t + (k + 1) % 3];
                const int* sv = star(v); const int dv = deg[v];
                int i = -1;
                for (int j = 0; j < dv; ++j) if (sv[j] == u) { i = j; break; }
                if (i < 0) { bad.fetch_add(1); halfedges[3 * t + k] = -1; continue; }
                const int w = sv[(i + 1) % dv];
                // owner of (v,u,w) and the star position of that triangle in the owner's star
                int m, a;                               // triangle as (m, a, .) counter-clockwise
                mesh::owner_of(v, u, w, m, a);
                const int* sm = star(m); const int dm = deg[m];
                int j2 = -1;
                for (int j = 0; j < dm; ++j) if (sm[j] == a) { j2 = j; break; }
                int t2 = (j2 >= 0) ? triOfStar[starOff[m] + j2] : -1;
                if (t2 < 0) { bad.fetch_add(1); halfedges[3 * t + k] = -1; continue; }
                int side = -1;
                for (int c = 0; c < 3; ++c) if (triangles[3 * t2 + c] == v && triangles[3 * t2 + (c + 1) % 3] == u) side = c;
                if (side < 0) { bad.fetch_add(1); halfedges[3 * t + k] = -1; continue; }
                halfedges[3 * t + k] = 3 * t2 + side;
            }
        }
    });
    if (bad.load() != 0) { err = "sphere_delaunay: " + std::to_string(bad.load()) + " unmatched half-edges (inconsistent stars)"; return 4; }
    return 0;
}

// ---------------------------------------------------------------------------------------------
// CSR from triangles/halfedges, following the circulation rule of js/sphere-mesh.js:102-141:
// row r starts at the lowest-numbered side leaving r and steps s <- next(halfedges[s]).
// ---------------------------------------------------------------------------------------------
using mesh::next_side;

int mesh_csr(int V, int numSides, const int* triangles, const int* halfedges,
             int* adjOffset /*V+1*/, int* adjList /*numSides*/, int* adjTri /*numSides or null*/, std::string& err) {
    if (V < 0 || numSides < 0 || numSides % 3 != 0) { err = "mesh_csr: bad sizes"; return 3; }
    {   // the walks below index r_s[] with triangle corners and follow half-edges: refuse anything out of range first
        std::atomic<int> oob{0};
        parallel_ranges(numSides, [&](int64_t b, int64_t e, int) {
            for (int64_t s = b; s < e; ++s) {
                if (triangles[s] < 0 || triangles[s] >= V) { oob = 1; break; }
                if (halfedges[s] < -1 || halfedges[s] >= numSides) { oob = 2; break; }
            }
        });
        if (oob == 1) { err = "mesh_csr: triangle corner out of range"; return 3; }
        if (oob == 2) { err = "mesh_csr: half-edge index out of range"; return 3; }
    }
    std::vector<int> r_s(V, -1);
    for (int s = numSides - 1; s >= 0; --s) r_s[triangles[s]] = s;   // lowest side wins
    adjOffset[0] = 0;
    std::vector<int> cnt(V, 0);
    std::atomic<int> bad{0};
    parallel_ranges(V, [&](int64_t b, int64_t e, int) {
        for (int64_t r = b; r < e; ++r) {
            int s0 = r_s[r]; if (s0 < 0) continue;
            int s = s0, c = 0;
            do { ++c; int h = halfedges[s]; if (h < 0 || c > 4096) { bad.fetch_add(1); break; } s = next_side(h); } while (s != s0);
            cnt[r] = c;
        }
    });
    if (bad.load()) { err = "mesh_csr: open or malformed half-edge structure"; return 1; }
    for (int r = 0; r < V; ++r) adjOffset[r + 1] = adjOffset[r] + cnt[r];
    if (adjOffset[V] > numSides) { err = "mesh_csr: adjacency larger than side count"; return 2; }
    parallel_ranges(V, [&](int64_t b, int64_t e, int) {
        for (int64_t r = b; r < e; ++r) {
            int s0 = r_s[r]; if (s0 < 0) continue;
            int s = s0, idx = adjOffset[r];
            do {
                adjList[idx] = triangles[next_side(s)];
                if (adjTri) adjTri[idx] = s / 3;
                ++idx;
                s = next_side(halfedges[s]);
            } while (s != s0);
        }
    });
    return 0;
}

void neighbor_dist(int V, const int* adjOffset, const int* adjList, const float* xyz, float* out) {
    parallel_ranges(V, [&](int64_t b, int64_t e, int) {
        for (int64_t r = b; r < e; ++r) {
            const double x = xyz[3 * r], y = xyz[3 * r + 1], z = xyz[3 * r + 2];
            for (int i = adjOffset[r]; i < adjOffset[r + 1]; ++i) {
                const int nb = adjList[i];
                out[i] = mesh::chord(x, y, z, xyz[3 * nb], xyz[3 * nb + 1], xyz[3 * nb + 2]);
            }
        }
    });
}

}  // namespace wo
