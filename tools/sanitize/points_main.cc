// Stand-alone host program for a sanitizer run of the point generator's shared bodies (csrc/points_ops.h): the chain-table builder and
// evaluator against the serial f64 loops (the sphere's two chains at the crafted sizes, and chains through zero, through the subnormals
// and into a table overflow), the Park-Miller jump-ahead against serial draws, the large-argument reduction on arguments from 2^20 to
// the largest double, and fib_point over whole spheres into exactly sized buffers.  CPU only, no GPU call, not loaded into Python.
//
//   g++ -std=c++17 -O1 -g -fno-omit-frame-pointer -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       tools/sanitize/points_main.cc -o /tmp/points_asan && /tmp/points_asan
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../planet_heightmap_generation_amd/csrc/points_ops.h"

namespace P = wo::points;

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED %s (line %d)\n", #cond, __LINE__); ++failures; } } while (0)
static uint64_t bits_of(double x) { uint64_t u; std::memcpy(&u, &x, 8); return u; }

static int64_t chain_mismatches(double x0, double c, int32_t N, int* size) {
    std::vector<P::ChainEntry> t(P::CHAIN_CAP);               // exactly the capacity: a write past it is the sanitizer's to find
    const int n = P::build_chain(x0, c, N, t.data());
    *size = n;
    if (n < 0) return -1;
    t.resize((size_t)n);
    t.shrink_to_fit();                                        // the evaluator reads inside [0, n)
    volatile double x = x0;
    int64_t bad = 0;
    for (int32_t k = 0; k < N; ++k) { if (bits_of(P::chain_value(t.data(), n, k)) != bits_of(x)) ++bad; x = x + c; }
    return bad;
}

int main() {
    int size = 0;
    const double dlong = P::FIB_PI * (3.0 - std::sqrt(5.0));
    for (int32_t N : {1, 2, 3, 4, 7, 63, 255, 256, 257, 2000, 5000, 12345, 65536, 999983, 1000000, 1 << 20}) {
        const double dz = 2.0 / (double)N;
        CHECK(chain_mismatches(0.0, dlong, N, &size) == 0);
        CHECK(chain_mismatches(1.0 - dz / 2.0, -dz, N, &size) == 0);
    }
    CHECK(chain_mismatches(-3.0, 0x1p-30, 200000, &size) == 0);
    CHECK(chain_mismatches(1.0, 0x1p-53, 1000, &size) == 0 && size == 2);
    CHECK(chain_mismatches(1.0, 0x1.8p-52, 100000, &size) == 0);
    CHECK(chain_mismatches(5e-324, 5e-324, 250, &size) == 0 && size == 250);
    CHECK(chain_mismatches(5e-324, 5e-324, 257, &size) == -1);
    CHECK(chain_mismatches(0x1p-960, 0x1.4cccccccccccdp-1000, 100000, &size) == 0);

    for (double seed : {1.0, 7.0, 0.5, -3.0, 2147483645.0}) {
        std::vector<P::ChainEntry> a(P::CHAIN_CAP), b(P::CHAIN_CAP);
        P::FibParams F{};
        CHECK(P::fib_setup(1, 0.0, seed, a.data(), b.data(), F) == 0);
        uint64_t s = F.s0;
        int64_t bad = 0;
        for (uint32_t i = 1; i <= 400000; ++i) { s = s * 16807u % 2147483647u; if (P::lcg_jump(F.s0, i) != s) ++bad; }
        CHECK(bad == 0);
        CHECK(P::lcg_jump(F.s0, 0xffffffffu) >= 1);
    }

    double y[2];
    int finite = 0, total = 0;
    for (int e = 20; e <= 1023; ++e)
        for (double m : {1.0, 1.0000000000000002, 1.5707963267948966, 1.9999999999999998}) {
            const double x = std::ldexp(m, e);
            for (double v : {x, -x}) {
                const int32_t n = P::fd_rem_pio2_large(v, y);
                ++total;
                if (n >= -7 && n <= 7 && std::fabs(y[0]) <= 0.7853981633974484 && std::fabs(y[1]) <= std::fabs(y[0])) ++finite;
                const double s = P::fd_sin_big(v), c = P::fd_cos_big(v);
                CHECK(std::fabs(s * s + c * c - 1.0) < 1e-15);
            }
        }
    CHECK(finite == total);
    CHECK(std::isnan(P::fd_sin_big(INFINITY)) && std::isnan(P::fd_cos_big(-INFINITY)) && std::isnan(P::fd_sin_big(NAN)));
    CHECK(P::fd_sin_big(0x1.921fb54442d18p+0 * 0x1p70) == P::fd_sin_big(0x1.921fb54442d18p+70));

    for (int32_t N : {1, 2, 3, 7, 63, 257, 5000, 700000})
        for (double jitter : {0.0, 0.75, 1.0}) {
            std::vector<P::ChainEntry> a(P::CHAIN_CAP), b(P::CHAIN_CAP);
            P::FibParams F{};
            CHECK(P::fib_setup(N, jitter, 1.0, a.data(), b.data(), F) == 0);
            std::vector<float> xyz(3 * (size_t)N);
            int64_t offSphere = 0;
            for (int32_t k = 0; k < N; ++k) {
                float* p = xyz.data() + 3 * (size_t)k;
                P::fib_point(k, F, p);
                const double l = (double)p[0] * p[0] + (double)p[1] * p[1] + (double)p[2] * p[2];
                if (!(std::fabs(l - 1.0) < 1e-6)) ++offSphere;
            }
            CHECK(offSphere == 0);
        }
    std::printf(failures ? "points_main: %d checks FAILED\n" : "points_main: all checks passed\n", failures);
    return failures ? 1 : 0;
}
