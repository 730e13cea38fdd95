// Stand-alone host program for a sanitizer run of the two raster projections (csrc/map_ops.h: map::Projection, csrc/cube_ops.h:
// cube::Projection) as the shared raster of csrc/raster.hip drives them: vertices, every piece, the box, the pixel centres and the
// pixel indices.  The sides are built from zero, signed zero, denormal, huge, infinite and NaN coordinates (and a few ordinary ones),
// at sizes from the smallest to the largest the entry points accept.  Every box must lie within its map or face and every pixel
// index within the side map; at the small sizes the covered pixels are written into a side map of exactly that many words, so a
// write past it is the sanitizer's to find.  CPU only, no GPU call, not loaded into Python.
//
//   g++ -std=c++17 -O1 -g -fno-omit-frame-pointer -ffp-contract=off -fsanitize=address,undefined,float-cast-overflow \
//       -fno-sanitize-recover=undefined tools/sanitize/raster_projection_main.cc -o /tmp/raster_projection_asan && /tmp/raster_projection_asan
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../planet_heightmap_generation_amd/csrc/cube_ops.h"
#include "../../planet_heightmap_generation_amd/csrc/map_ops.h"

namespace M = wo::map;
namespace Q = wo::cube;

static int failures = 0;
static int64_t piecesDrawn = 0, pixelsWalked = 0;
#define CHECK(cond) do { if (!(cond)) { if (++failures <= 20) std::printf("FAILED %s (line %d)\n", #cond, __LINE__); } } while (0)

// the mesh of one side: side 0 has its inner centre in table entry 0, its outer centre (halfedges[0] / 3) in entry 1 and its region
// in entry 0 of the region table; the arrays are exactly as long as the projection may read
static const std::vector<int32_t> kTriangles = {0}, kHalfedges = {3};

// what the two kernels of raster.hip do with one side, on the host: every piece, its box and, for a small box or a small map, its pixels
template <class P>
static void drive(const P& proj, int32_t W, int32_t H, int32_t faces, std::vector<uint32_t>* sideMap) {
    typename P::Side v;
    const int n = proj.vertices(kTriangles.data(), kHalfedges.data(), 0, v);
    CHECK(n >= 0 && n <= P::PIECES);
    for (int k = 0; k < n; ++k) {
        M::Tri t;
        double area2;
        M::Box b;
        int32_t f;
        if (!proj.piece(v, k, t, area2, b, f)) continue;
        ++piecesDrawn;
        CHECK(area2 > 0.0 || area2 < 0.0);
        CHECK(f >= 0 && f < faces);
        CHECK(0 <= b.i0 && b.i0 <= b.i1 && b.i1 <= W - 1 && 0 <= b.j0 && b.j0 <= b.j1 && b.j1 <= H - 1);
        CHECK(proj.index(f, b.i0, b.j0) >= 0 && proj.index(f, b.i1, b.j1) < proj.pixels());
        if (!sideMap && M::box_pixels(b) > M::SMALL_BOX) continue;
        for (int32_t j = b.j0; j <= b.j1; ++j)
            for (int32_t i = b.i0; i <= b.i1; ++i) {
                double xc, yc;
                proj.center(i, j, xc, yc);
                const int64_t q = proj.index(f, i, j);
                CHECK(q >= 0 && q < proj.pixels());
                ++pixelsWalked;
                if (sideMap && M::tri_covers(t, area2, xc, yc)) (*sideMap)[(size_t)q] = 0;
            }
    }
}

int main() {
    const double PI = 3.141592653589793, DEN = 5e-324, HUGE_D = 1e300;
    const float DENF = 1e-45f, HUGE_F = 3e38f;

    // ---- the map: longitudes and latitudes straight into the two tables ------------------------------------------------------------
    std::vector<M::LonLat> pool;
    for (double lon : {0.0, -0.0, DEN, -DEN, 1.0, -3.0, PI, -PI, HUGE_D, -HUGE_D, (double)INFINITY, -(double)INFINITY, (double)NAN})
        for (double lat : {0.0, DEN, 0.5, -PI / 2.0, PI / 2.0, HUGE_D, -(double)INFINITY, (double)NAN}) pool.push_back(M::LonLat{lon, lat});
    for (int32_t W : {2, 4, 6, 50, 64, 250, 2048, 16384, 32768}) {
        const int32_t H = W / 2;
        std::vector<uint32_t> sideMap(W <= 64 ? (size_t)W * H : 0, M::NO_SIDE);
        for (size_t a = 0; a < pool.size(); ++a)
            for (size_t b = 0; b < pool.size(); b += 3)
                for (size_t c = 0; c < pool.size(); c += 5) {
                    const std::vector<M::LonLat> t_ll = {pool[a], pool[(a + b) % pool.size()]}, r_ll = {pool[(a + c) % pool.size()]};
                    drive(M::Projection{t_ll.data(), r_ll.data(), W, H}, W, H, 1, W <= 64 ? &sideMap : nullptr);
                }
    }
    std::printf("map: %lld pieces drawn, %lld pixels walked\n", (long long)piecesDrawn, (long long)pixelsWalked);
    CHECK(piecesDrawn > 0 && pixelsWalked > 0);

    // ---- the cube: positions straight into the two tables ---------------------------------------------------------------------------
    piecesDrawn = pixelsWalked = 0;
    const float C[] = {0.0f, -0.0f, DENF, 1.0f, -1.0f, 0.25f, HUGE_F, -HUGE_F, INFINITY, -INFINITY, NAN};
    const size_t NC = sizeof(C) / sizeof(C[0]);
    std::vector<float> xyz;                                    // every position with coordinates from C
    for (size_t x = 0; x < NC; ++x)
        for (size_t y = 0; y < NC; ++y)
            for (size_t z = 0; z < NC; ++z) { xyz.push_back(C[x]); xyz.push_back(C[y]); xyz.push_back(C[z]); }
    const size_t NV = xyz.size() / 3;
    for (int32_t S : {1, 2, 3, 7, 50, 64, 1024, 4097, 16384}) {
        std::vector<uint32_t> sideMap(S <= 64 ? (size_t)Q::FACE_COUNT * S * S : 0, M::NO_SIDE);
        for (size_t a = 0; a < NV; ++a)
            for (size_t b = 0; b < NV; b += 97)
                for (size_t c = 0; c < NV; c += 61) {
                    const size_t vb = (a + b) % NV, vc = (a + c) % NV;
                    const std::vector<float> t_xyz = {xyz[3 * a], xyz[3 * a + 1], xyz[3 * a + 2], xyz[3 * vb], xyz[3 * vb + 1], xyz[3 * vb + 2]};
                    const std::vector<float> r_xyz = {xyz[3 * vc], xyz[3 * vc + 1], xyz[3 * vc + 2]};
                    drive(Q::Projection{t_xyz.data(), r_xyz.data(), S}, S, S, Q::FACE_COUNT, S <= 64 ? &sideMap : nullptr);
                }
    }
    std::printf("cube: %lld pieces drawn, %lld pixels walked\n", (long long)piecesDrawn, (long long)pixelsWalked);
    CHECK(piecesDrawn > 0 && pixelsWalked > 0);

    std::printf(failures ? "raster_projection_main: %d checks FAILED\n" : "raster_projection_main: all checks passed\n", failures);
    return failures ? 1 : 0;
}
