// Test-only libm perturbation hook of _build/libemu_libm.so (see libm_perturb.h): every wrapped call returns glibc's result
// moved by k double ulps, k = +K (seed 1), -K (seed 2) or drawn from [-K, K] by a hash of the function, its arguments and the
// seed (any other seed).  The hash makes k a function of the call, not of the call order, so threaded callers stay
// deterministic.  K = 0 leaves every result as glibc's.  Per-function call counters show that the hook is reached.
#include <atomic>
#include <cstdint>
#include <cstring>

#include "libm_perturb.h"

namespace {

enum Fn { F_TANH, F_EXP, F_SIN, F_COS, F_ATAN2, F_POW, F_ASIN, F_COUNT };
std::atomic<uint64_t> g_calls[F_COUNT];
uint64_t g_seed = 0;
int64_t g_K = 0;

uint64_t bits_of(double v) { uint64_t u; std::memcpy(&u, &v, 8); return u; }
double of_bits(uint64_t u) { double v; std::memcpy(&v, &u, 8); return v; }

uint64_t mix(uint64_t z) {                              // splitmix64 finaliser
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// the finite doubles in value order as integers (+0 and -0 both map to 0), so that moving by k ulps is an addition
int64_t ordered(double v) {
    const uint64_t u = bits_of(v);
    const int64_t mag = (int64_t)(u & 0x7FFFFFFFFFFFFFFFull);
    return (u >> 63) ? -mag : mag;
}
double from_ordered(int64_t k) {
    const int64_t maxFinite = 0x7FEFFFFFFFFFFFFFll;
    if (k > maxFinite) k = maxFinite;
    if (k < -maxFinite) k = -maxFinite;
    return k >= 0 ? of_bits((uint64_t)k) : of_bits((uint64_t)(-k) | 0x8000000000000000ull);
}

double nudge(Fn fn, double r, double a, double b) {
    g_calls[fn].fetch_add(1, std::memory_order_relaxed);
    if (g_K == 0 || !std::isfinite(r)) return r;
    int64_t k;
    if (g_seed == 1) k = g_K;
    else if (g_seed == 2) k = -g_K;
    else {
        const uint64_t h = mix(mix(mix(g_seed ^ ((uint64_t)fn << 56)) ^ bits_of(a)) ^ bits_of(b));
        k = (int64_t)(h % (uint64_t)(2 * g_K + 1)) - g_K;
    }
    return from_ordered(ordered(r) + k);
}

}  // namespace

namespace wo {
double tanh(double x) { return nudge(F_TANH, std::tanh(x), x, 0); }
double exp(double x) { return nudge(F_EXP, std::exp(x), x, 0); }
double sin(double x) { return nudge(F_SIN, std::sin(x), x, 0); }
double cos(double x) { return nudge(F_COS, std::cos(x), x, 0); }
double atan2(double y, double x) { return nudge(F_ATAN2, std::atan2(y, x), y, x); }
double pow(double x, double y) { return nudge(F_POW, std::pow(x, y), x, y); }
double asin(double x) { return nudge(F_ASIN, std::asin(x), x, 0); }
}  // namespace wo

// seed 1: every result + K ulps, seed 2: - K ulps, otherwise hashed in [-K, K]; resets the call counters
extern "C" void emu_set_libm_perturb(uint64_t seed, int64_t K) {
    g_seed = seed;
    g_K = K < 0 ? -K : K;
    for (auto& c : g_calls) c.store(0);
}

// calls since the last emu_set_libm_perturb, in the order tanh, exp, sin, cos, atan2, pow, asin
extern "C" void emu_libm_calls(uint64_t* out7) {
    for (int i = 0; i < F_COUNT; ++i) out7[i] = g_calls[i].load();
}
