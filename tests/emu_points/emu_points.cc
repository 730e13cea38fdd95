// Test-only host emulator of csrc/points_ops.h: the chain tables against the serial f64 loops, the Park-Miller jump-ahead against
// serial draws, the large-argument sine and cosine, and the points of a whole sphere from the same fib_point the device kernel runs.
#include <cstdint>
#include <vector>

#include "../../planet_heightmap_generation_amd/csrc/points_ops.h"

namespace P = wo::points;

static inline uint64_t bits_of(double x) { uint64_t u; memcpy(&u, &x, 8); return u; }

extern "C" {

// steps k in [0, N) of both chains of an N-cell sphere at which the table's value differs from the serial loop's bits;
// -1: a table overflowed.  sizes[0], sizes[1]: entries of the lng and z tables.
int64_t emu_chain_mismatches(int32_t N, int32_t* sizes) {
    std::vector<P::ChainEntry> tl(P::CHAIN_CAP), tz(P::CHAIN_CAP);
    P::FibParams F;
    if (P::fib_setup(N, 0.0, 1.0, tl.data(), tz.data(), F)) return -1;
    sizes[0] = F.nLng; sizes[1] = F.nZ;
    const double dlong = P::FIB_PI * (3.0 - std::sqrt(5.0)), dz = 2.0 / (double)N;
    volatile double lng = 0.0, z = 1.0 - dz / 2.0;         // js/sphere-mesh.js:15,34
    int64_t bad = 0;
    for (int32_t k = 0; k < N; ++k) {
        if (bits_of(P::chain_value(F.lng, F.nLng, k)) != bits_of(lng)) ++bad;
        if (bits_of(P::chain_value(F.z, F.nZ, k)) != bits_of(z)) ++bad;
        lng = lng + dlong;
        z = z - dz;
    }
    return bad;
}

// a chain of the caller's own (x0, c): mismatches against the serial loop, -1 on overflow
int64_t emu_chain_mismatches_of(double x0, double c, int32_t N, int32_t* size) {
    std::vector<P::ChainEntry> t(P::CHAIN_CAP);
    const int n = P::build_chain(x0, c, N, t.data());
    if (n < 0) return -1;
    *size = n;
    volatile double x = x0;
    int64_t bad = 0;
    for (int32_t k = 0; k < N; ++k) { if (bits_of(P::chain_value(t.data(), n, k)) != bits_of(x)) ++bad; x = x + c; }
    return bad;
}

// draws 1 .. n of makeRng(seed) (js/rng.js, serially) against lcg_jump: the number of differing states
int64_t emu_jump_mismatches(double seed, int32_t n) {
    std::vector<P::ChainEntry> tl(P::CHAIN_CAP), tz(P::CHAIN_CAP);
    P::FibParams F;
    P::fib_setup(1, 0.0, seed, tl.data(), tz.data(), F);
    double s = (double)F.s0;                               // the reference's own arithmetic: doubles
    int64_t bad = 0;
    for (int32_t i = 1; i <= n; ++i) {
        s = std::fmod(s * 16807.0, 2147483647.0);
        const uint32_t j = P::lcg_jump(F.s0, (uint32_t)i);
        if ((double)j != s || P::lcg_draw(j) != (s - 1.0) / 2147483646.0) ++bad;
    }
    return bad;
}
uint32_t emu_seed_state(double seed) {
    std::vector<P::ChainEntry> tl(P::CHAIN_CAP), tz(P::CHAIN_CAP);
    P::FibParams F;
    P::fib_setup(1, 0.0, seed, tl.data(), tz.data(), F);
    return F.s0;
}

void emu_sin_big(int64_t n, const double* x, double* out) { for (int64_t i = 0; i < n; ++i) out[i] = P::fd_sin_big(x[i]); }
void emu_cos_big(int64_t n, const double* x, double* out) { for (int64_t i = 0; i < n; ++i) out[i] = P::fd_cos_big(x[i]); }
void emu_sin(int64_t n, const double* x, double* out) { for (int64_t i = 0; i < n; ++i) out[i] = wo::imp::fd_sin(x[i]); }
void emu_cos(int64_t n, const double* x, double* out) { for (int64_t i = 0; i < n; ++i) out[i] = wo::imp::fd_cos(x[i]); }

// 3 (N + 1) floats: the N points and the pole; 1: bad arguments or a table overflow
int emu_fib_points(int32_t N, double jitter, double seed, float* xyz) {
    if (N < 1 || !xyz) return 1;
    std::vector<P::ChainEntry> tl(P::CHAIN_CAP), tz(P::CHAIN_CAP);
    P::FibParams F;
    if (P::fib_setup(N, jitter, seed, tl.data(), tz.data(), F)) return 1;
    for (int32_t k = 0; k < N; ++k) P::fib_point(k, F, xyz + 3 * (int64_t)k);
    xyz[3 * (int64_t)N] = 0.f; xyz[3 * (int64_t)N + 1] = 0.f; xyz[3 * (int64_t)N + 2] = 1.f;
    return 0;
}

// lonR of every stride-th point of a jittered sphere (the arguments the large reduction meets); returns how many
int64_t emu_lonr_samples(int32_t N, double jitter, double seed, int32_t stride, double* out) {
    std::vector<P::ChainEntry> tl(P::CHAIN_CAP), tz(P::CHAIN_CAP);
    P::FibParams F;
    if (P::fib_setup(N, jitter, seed, tl.data(), tz.data(), F)) return -1;
    int64_t n = 0;
    for (int32_t k = 0; k < N; k += stride) {
        const double lng = P::chain_value(F.lng, F.nLng, k), z = P::chain_value(F.z, F.nZ, k);
        const double r = sqrt(1.0 - z * z);
        double lonDeg = lng * 180.0 / P::FIB_PI;
        if (jitter > 0) {
            uint32_t st = P::lcg_jump(F.s0, 4u * (uint32_t)k + 2u);
            st = P::lcg_step(st); const double a2 = P::lcg_draw(st);
            st = P::lcg_step(st); const double b2 = P::lcg_draw(st);
            lonDeg += jitter * (a2 - b2) * (F.s / r * 180.0 / P::FIB_PI);
        }
        out[n++] = lonDeg * P::FIB_PI / 180.0;
    }
    return n;
}

}  // extern "C"
