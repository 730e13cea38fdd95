// The Fibonacci sphere's points (js/sphere-mesh.js:9-37) one point at a time: the bodies shared by the device kernel (points.hip) and the
// test-only CPU emulator (tests/emu_points), so that both compile the very same arithmetic.  DESIGN 8.16 has the derivation.
//
// The reference's loop carries three values from point to point, and each has a closed form that reproduces the loop's bits:
//   * the Park-Miller state (js/rng.js:3-6): draw i is s0 * 16807^i mod (2^31 - 1); point k uses draws 4k+1 .. 4k+4 (lcg_jump)
//   * lng += dlong and z -= dz, two chains x <- fl(x + c) in f64.  While x stays in one binade and is a multiple of that binade's ulp,
//     the rounded increment is one constant multiple of the ulp (from the second step inside the binade on: where c falls exactly
//     between two multiples the first result is even, and stays even).  So x_k is piecewise linear over integer mantissas:
//     x_k = (X + (k - k0) * D) * 2^e with |X + j D| < 2^53, exact in int64 and in the conversion.  build_chain (host) walks the chain
//     segment by segment and chain_value (host and device) evaluates entry k.
// The rest is per-point arithmetic in the reference's operation order, on import_ops.h's ports of V8's fdlibm (fd_asin, fd_kernel_sin,
// fd_kernel_cos, fd_rem_pio2).  lonR reaches 2.4e7 rad at 10 M cells, beyond fd_sin / fd_cos's domain, so fd_sin_big / fd_cos_big add
// fdlibm's large-argument reduction (__kernel_rem_pio2 with its table of 2/pi digits) above it and are fd_sin / fd_cos below.
// Plain f64 arithmetic, integer arithmetic and bit manipulation only; the library compiles with -ffp-contract=off.  Every loop is
// bounded.  The tables between BEGIN / END marks are tools/gen_points_tables.py's output (--check compares them).
#pragma once
#include <cstdint>
#include <cstring>
#include <cmath>

#include "import_ops.h"

namespace wo {
namespace points {

using imp::hi_word;
using imp::lo_word;

// ---------------------------------------------------------------------------------------------------------------------------
// Park-Miller jump-ahead
// ---------------------------------------------------------------------------------------------------------------------------
constexpr uint64_t LCG_M = 2147483647u;
WO_IMP_HD inline uint32_t lcg_mul(uint32_t a, uint32_t b) { return (uint32_t)(((uint64_t)a * b) % LCG_M); }
// 16807^n mod (2^31 - 1)
WO_IMP_HD inline uint32_t lcg_pow(uint32_t n) {
    const uint32_t sq[32] = {
        // BEGIN LCG_POW
        16807u, 282475249u, 984943658u, 1457850878u, 1137522503u, 1636807826u, 685118024u, 515204530u,
        897054849u, 2038299453u, 1836275591u, 349037107u, 149796865u, 1186652285u, 2106880871u, 877809922u,
        1682791109u, 1900685356u, 2080563572u, 612544882u, 1295048709u, 1987420232u, 868966365u, 1331238991u,
        1550655590u, 766698560u, 1154667137u, 901595110u, 1008653149u, 1821072732u, 2147466840u, 282475249u
        // END LCG_POW
    };
    uint32_t r = 1;
    for (int b = 0; b < 32; ++b) if ((n >> b) & 1u) r = lcg_mul(r, sq[b]);
    return r;
}
// the state after n draws from state s0 (1 <= s0 < 2^31 - 1), and the draw a state stands for
WO_IMP_HD inline uint32_t lcg_jump(uint32_t s0, uint32_t n) { return lcg_mul(s0, lcg_pow(n)); }
WO_IMP_HD inline uint32_t lcg_step(uint32_t s) { return lcg_mul(s, 16807u); }
WO_IMP_HD inline double lcg_draw(uint32_t s) { return (double)(s - 1u) / 2147483646.0; }

// ---------------------------------------------------------------------------------------------------------------------------
// chain tables: x_0, x_{k+1} = fl(x_k + c)
// ---------------------------------------------------------------------------------------------------------------------------
constexpr int CHAIN_CAP = 256;
// steps k0 .. (the next entry's k0) - 1 hold (X + (k - k0) * D) * 2^e; a single value has D = 0 and X * 2^e = x_k0 (X = 0: e = 0)
struct ChainEntry { int64_t X, D; int32_t k0, e; };

WO_IMP_HD inline double pow2(int32_t e) {                  // 2^e, -1022 <= e <= 1023
    const uint64_t u = (uint64_t)(e + 1023) << 52; double r; memcpy(&r, &u, 8); return r;
}
// X * 2^e of a finite double: |X| < 2^53 (normal: 2^52 <= |X|), e >= -1074
inline void chain_split(double x, int64_t& X, int32_t& e) {
    uint64_t u; memcpy(&u, &x, 8);
    const int32_t be = (int32_t)((u >> 52) & 0x7ff);
    const int64_t m = (int64_t)(u & 0xfffffffffffffull);
    int64_t a;
    if (be == 0) { a = m; e = -1074; } else { a = m | (1ll << 52); e = be - 1075; }
    if (a == 0) e = 0;
    X = (u >> 63) ? -a : a;
}
WO_IMP_HD inline double chain_compose(int64_t X, int32_t e) {
    // exact: |X| < 2^53 converts exactly; the scale is a power of two, applied in two normal factors where e is below -1022
    const double v = (double)X;
    return e >= -1022 ? v * pow2(e) : (v * pow2(e + 60)) * pow2(-60);
}
// x_k from the table: the last entry with k0 <= k (entry 0 has k0 = 0), by binary search
WO_IMP_HD inline double chain_value(const ChainEntry* t, int32_t n, int32_t k) {
    int32_t lo = 0, hi = n - 1;
    for (int it = 0; it < 9 && lo < hi; ++it) {            // n <= 256: at most 8 halvings
        const int32_t mid = (lo + hi + 1) >> 1;
        if (t[mid].k0 <= k) lo = mid; else hi = mid - 1;
    }
    const ChainEntry E = t[lo];
    return chain_compose(E.X + (int64_t)(k - E.k0) * E.D, E.e);
}

// The host walk for steps 0 .. N-1.  Returns the number of entries, or -1 where more than CHAIN_CAP would be needed.
// Three real steps a = x_k, b, d: if they share sign and exponent (and the ulp is a normal double), a is emitted as a single value and a
// linear segment opens at b with D = (d - b) / ulp; it runs while the mantissa stays strictly inside the binade, which is where the
// exact sum lies in the binade too and the rounding is the constant one.  Otherwise a is a single value and the walk goes on from b.
inline int build_chain(double x0, double c, int32_t N, ChainEntry* out) {
    int n = 0;
    int32_t k = 0;
    volatile double cur = x0;                              // volatile: every step is rounded to f64 as the loop's is
    while (k < N) {
        if (n >= CHAIN_CAP) return -1;
        const double a = cur;
        volatile double bv = a + c; const double b = bv;
        volatile double dv = b + c; const double d = dv;
        int64_t Xa, Xb, Xd; int32_t ea, eb, ed;
        chain_split(a, Xa, ea); chain_split(b, Xb, eb); chain_split(d, Xd, ed);
        out[n].X = Xa; out[n].D = 0; out[n].k0 = k; out[n].e = ea; ++n;
        const bool sameSign = (Xa > 0 && Xb > 0 && Xd > 0) || (Xa < 0 && Xb < 0 && Xd < 0);
        const int64_t lowM = 1ll << 52, highM = 1ll << 53;
        int64_t jmax = 0;
        if (sameSign && ea == eb && eb == ed && eb >= -1022 && k + 2 < N) {
            const int64_t A = Xb < 0 ? -Xb : Xb, dA = Xb < 0 ? -(Xd - Xb) : (Xd - Xb);     // the magnitude and its step
            if (dA > 0) jmax = (highM - 1 - A) / dA;
            else if (dA < 0) jmax = A > lowM ? (A - (lowM + 1)) / (-dA) : 0;
            else jmax = N;
            jmax = jmax < (int64_t)(N - 1 - (k + 1)) ? jmax : (int64_t)(N - 1 - (k + 1));
        }
        if (jmax >= 1) {
            if (n >= CHAIN_CAP) return -1;
            out[n].X = Xb; out[n].D = Xd - Xb; out[n].k0 = k + 1; out[n].e = eb; ++n;
            const double last = chain_compose(Xb + jmax * (Xd - Xb), eb);
            volatile double nv = last + c;
            cur = nv;
            k = (int32_t)(k + 2 + jmax);
        } else {
            cur = b;
            k += 1;
        }
    }
    return n;
}

// ---------------------------------------------------------------------------------------------------------------------------
// large-argument trigonometry
// ---------------------------------------------------------------------------------------------------------------------------
// k_rem_pio2.c (__kernel_rem_pio2) for the three 24-bit pieces of one double and prec = 2 (jk = 4), preceded by the last branch of
// e_rem_pio2.c that forms the pieces: y[0] + y[1] = x - n * pi/2, returns n mod 8 (negated for x < 0).  For finite |x| with a high
// word above 0x413921fb; the operation order is V8's (src/base/ieee754.cc).  The work arrays have 20 entries as in fdlibm; jz starts
// at 4 and grows only where the product cancels to zero, which no double does past a few words: it is held below 18.
WO_IMP_HD inline int32_t fd_rem_pio2_large(double x, double* y) {
    const int32_t ipio2[66] = {
        // BEGIN IPIO2
        0xA2F983, 0x6E4E44, 0x1529FC, 0x2757D1, 0xF534DD, 0xC0DB62, 0x95993C, 0x439041, 0xFE5163, 0xABDEBB, 0xC561B7,
        0x246E3A, 0x424DD2, 0xE00649, 0x2EEA09, 0xD1921C, 0xFE1DEB, 0x1CB129, 0xA73EE8, 0x8235F5, 0x2EBB44, 0x84E99C,
        0x7026B4, 0x5F7E41, 0x3991D6, 0x398353, 0x39F49C, 0x845F8B, 0xBDF928, 0x3B1FF8, 0x97FFDE, 0x05980F, 0xEF2F11,
        0x8B5A0A, 0x6D1F6D, 0x367ECF, 0x27CB09, 0xB74F46, 0x3F669E, 0x5FEA2D, 0x7527BA, 0xC7EBE5, 0xF17B3D, 0x0739F7,
        0x8A5292, 0xEA6BFB, 0x5FB11F, 0x8D5D08, 0x560330, 0x46FC7B, 0x6BABF0, 0xCFBC20, 0x9AF436, 0x1DA9E3, 0x91615E,
        0xE61B08, 0x659985, 0x5F14A0, 0x68408D, 0xFFD880, 0x4D7327, 0x310606, 0x1556CA, 0x73A8C9, 0x60E27B, 0xC08C6B
        // END IPIO2
    };
    const double PIo2[8] = {
        // BEGIN PIO2
        0xC90FDAp-23, 0xA22168p-47, 0xC234C4p-71, 0xC6628Bp-95,
        0x80DC1Cp-119, 0xD12902p-143, 0x4E088Ap-167, 0x67CC74p-191
        // END PIO2
    };
    const double zero = 0.0, one = 1.0, two24 = 1.67772160000000000000e+07, twon24 = 5.96046447753906250000e-08;
    const int32_t hx = hi_word(x), ix = hx & 0x7fffffff;
    // e_rem_pio2.c: z = scalbn(|x|, -e0) with e0 = ilogb(x) - 23, then three 24-bit pieces
    const int32_t e0 = (ix >> 20) - 1046;
    double z;
    { const uint64_t u = ((uint64_t)(uint32_t)(ix - (int32_t)((uint32_t)e0 << 20)) << 32) | lo_word(x); memcpy(&z, &u, 8); }
    double tx[3];
    for (int i = 0; i < 2; ++i) { tx[i] = (double)((int32_t)z); z = (z - tx[i]) * two24; }
    tx[2] = z;
    int nx = 3;
    while (nx > 1 && tx[nx - 1] == zero) nx--;

    // k_rem_pio2.c
    const int jk = 4, jp = jk, jx = nx - 1;
    int jv = (e0 - 3) / 24; if (jv < 0) jv = 0;
    int q0 = e0 - 24 * (jv + 1);
    int32_t iq[20];
    double f[20], fq[20], q[20], fw;
    int i, j, k, n, ih, carry;
    for (i = 0; i < 20; ++i) { iq[i] = 0; f[i] = zero; fq[i] = zero; q[i] = zero; }
    j = jv - jx;
    const int m = jx + jk;
    for (i = 0; i <= m; i++, j++) f[i] = (j < 0) ? zero : (double)ipio2[j < 66 ? j : 65];
    for (i = 0; i <= jk; i++) {
        for (j = 0, fw = 0.0; j <= jx; j++) fw += tx[j] * f[jx + i - j];
        q[i] = fw;
    }
    int jz = jk;
    for (int round = 0; round < 16; ++round) {             // fdlibm's "recompute" loop
        for (i = 0, j = jz, z = q[jz]; j > 0; i++, j--) {  // distill q[] into iq[] reversingly
            fw = (double)((int32_t)(twon24 * z));
            iq[i] = (int32_t)(z - two24 * fw);
            z = q[j - 1] + fw;
        }
        z = z * pow2(q0);                                  // scalbn(z, q0): -28 < q0 <= 2, exact
        z -= 8.0 * floor(z * 0.125);                       // trim off integer >= 8
        n = (int32_t)z;
        z -= (double)n;
        ih = 0;
        if (q0 > 0) {                                      // need iq[jz-1] to determine n
            i = (iq[jz - 1] >> (24 - q0)); n += i;
            iq[jz - 1] -= i << (24 - q0);
            ih = iq[jz - 1] >> (23 - q0);
        } else if (q0 == 0) ih = iq[jz - 1] >> 23;
        else if (z >= 0.5) ih = 2;
        if (ih > 0) {                                      // q > 0.5
            n += 1; carry = 0;
            for (i = 0; i < jz; i++) {                     // compute 1 - q
                j = iq[i];
                if (carry == 0) { if (j != 0) { carry = 1; iq[i] = 0x1000000 - j; } }
                else iq[i] = 0xffffff - j;
            }
            if (q0 == 1) iq[jz - 1] &= 0x7fffff;
            else if (q0 == 2) iq[jz - 1] &= 0x3fffff;
            if (ih == 2) {
                z = one - z;
                if (carry != 0) z -= pow2(q0);
            }
        }
        if (z != zero) break;
        j = 0;
        for (i = jz - 1; i >= jk; i--) j |= iq[i];
        if (j != 0) break;
        for (k = 1; k < jk && iq[jk - k] == 0; k++) {}     // k = number of terms needed
        if (jz + k > 17 || jv + jz + k > 65) break;        // never for a double (see above); keeps every index in range
        for (i = jz + 1; i <= jz + k; i++) {               // add q[jz+1] to q[jz+k]
            f[jx + i] = (double)ipio2[jv + i];
            for (j = 0, fw = 0.0; j <= jx; j++) fw += tx[j] * f[jx + i - j];
            q[i] = fw;
        }
        jz += k;
    }
    if (z == 0.0) {                                        // chop off zero terms
        jz -= 1; q0 -= 24;
        while (jz > 0 && iq[jz] == 0) { jz--; q0 -= 24; }
    } else {                                               // break z into 24-bit if necessary
        z = z * pow2(-q0);
        if (z >= two24) {
            fw = (double)((int32_t)(twon24 * z));
            iq[jz] = (int32_t)(z - two24 * fw);
            jz += 1; q0 += 24;
            iq[jz] = (int32_t)fw;
        } else iq[jz] = (int32_t)z;
    }
    fw = pow2(q0);                                         // convert integer "bit" chunk to floating-point value
    for (i = jz; i >= 0; i--) { q[i] = fw * (double)iq[i]; fw *= twon24; }
    for (i = jz; i >= 0; i--) {                            // compute PIo2[0,...,jp] * q[jz,...,0]
        for (fw = 0.0, k = 0; k <= jp && k <= jz - i; k++) fw += PIo2[k] * q[i + k];
        fq[jz - i] = fw;
    }
    for (i = jz, fw = 0.0; i >= 0; i--) fw += fq[i];       // prec == 2
    y[0] = (ih == 0) ? fw : -fw;
    fw = fq[0] - fw;
    for (i = 1; i <= jz; i++) fw += fq[i];
    y[1] = (ih == 0) ? fw : -fw;
    n &= 7;
    if (hx < 0) { y[0] = -y[0]; y[1] = -y[1]; return -n; }
    return n;
}

// y[0] + y[1] = x - n pi/2 for every finite x: fd_rem_pio2 inside its domain, the large reduction above it
WO_IMP_HD inline int32_t rem_pio2_any(double x, double* y) {
    int32_t n;
    if (imp::fd_rem_pio2(x, y, &n)) return n;
    return fd_rem_pio2_large(x, y);
}
// Math.sin / Math.cos of V8 for every double
WO_IMP_HD inline double fd_sin_big(double x) {
    const int32_t ix = hi_word(x) & 0x7fffffff;
    if (ix <= 0x3fe921fb) return imp::fd_kernel_sin(x, 0.0, 0);
    if (ix >= 0x7ff00000) return x - x;
    double y[2];
    const int32_t n = rem_pio2_any(x, y);
    switch (n & 3) {
        case 0: return imp::fd_kernel_sin(y[0], y[1], 1);
        case 1: return imp::fd_kernel_cos(y[0], y[1]);
        case 2: return -imp::fd_kernel_sin(y[0], y[1], 1);
        default: return -imp::fd_kernel_cos(y[0], y[1]);
    }
}
WO_IMP_HD inline double fd_cos_big(double x) {
    const int32_t ix = hi_word(x) & 0x7fffffff;
    if (ix <= 0x3fe921fb) return imp::fd_kernel_cos(x, 0.0);
    if (ix >= 0x7ff00000) return x - x;
    double y[2];
    const int32_t n = rem_pio2_any(x, y);
    switch (n & 3) {
        case 0: return imp::fd_kernel_cos(y[0], y[1]);
        case 1: return -imp::fd_kernel_sin(y[0], y[1], 1);
        case 2: return -imp::fd_kernel_cos(y[0], y[1]);
        default: return imp::fd_kernel_sin(y[0], y[1], 1);
    }
}
// both of one argument: one reduction
WO_IMP_HD inline void fd_sincos_big(double x, double& s, double& c) {
    const int32_t ix = hi_word(x) & 0x7fffffff;
    if (ix <= 0x3fe921fb) { s = imp::fd_kernel_sin(x, 0.0, 0); c = imp::fd_kernel_cos(x, 0.0); return; }
    if (ix >= 0x7ff00000) { s = c = x - x; return; }
    double y[2];
    const int32_t n = rem_pio2_any(x, y);
    const double ks = imp::fd_kernel_sin(y[0], y[1], 1), kc = imp::fd_kernel_cos(y[0], y[1]);
    switch (n & 3) {
        case 0: s = ks; c = kc; break;
        case 1: s = kc; c = -ks; break;
        case 2: s = -ks; c = -kc; break;
        default: s = -kc; c = ks; break;
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// the point body
// ---------------------------------------------------------------------------------------------------------------------------
// what every point of one sphere shares; fib_setup (host) fills it, the tables' pointers are the caller's (host or device)
struct FibParams {
    int32_t N; uint32_t s0; double jitter, s, dz;
    const ChainEntry* lng; const ChainEntry* z; int32_t nLng, nZ;
};
constexpr double FIB_PI = 3.141592653589793;
constexpr int32_t FIB_MAX_N = (1 << 29) - 1;            // 3 (N + 1) floats and 4 k + 4 draws stay far inside int32 / uint32

// Math.max(-1, v): NaN if v is
WO_IMP_HD inline double js_max_m1(double v) { return v != v ? v : (v > -1.0 ? v : -1.0); }

// point k of generateFibonacciSphere(N, jitter, rng) as three f32, js/sphere-mesh.js:15-33 in its operation order
WO_IMP_HD inline void fib_point(int32_t k, const FibParams& P, float* out) {
    const double PI = FIB_PI;
    const double lng = chain_value(P.lng, P.nLng, k), z = chain_value(P.z, P.nZ, k);
    const double r = sqrt(1.0 - z * z);
    double latDeg = imp::fd_asin(z) * 180.0 / PI;
    double lonDeg = lng * 180.0 / PI;
    if (P.jitter > 0) {
        uint32_t st = lcg_jump(P.s0, 4u * (uint32_t)k);
        st = lcg_step(st); const double a1 = lcg_draw(st);
        st = lcg_step(st); const double b1 = lcg_draw(st);
        st = lcg_step(st); const double a2 = lcg_draw(st);
        st = lcg_step(st); const double b2 = lcg_draw(st);
        const double jLat = a1 - b1, jLon = a2 - b2;
        const double nextZ = js_max_m1(z - P.dz * 2.0 * PI * r / P.s);
        latDeg += P.jitter * jLat * (latDeg - imp::fd_asin(nextZ) * 180.0 / PI);
        lonDeg += P.jitter * jLon * (P.s / r * 180.0 / PI);
    }
    const double latR = latDeg * PI / 180.0;
    const double lonR = lonDeg * PI / 180.0;
    double sLat, cLat, sLon, cLon;
    fd_sincos_big(latR, sLat, cLat);
    fd_sincos_big(lonR, sLon, cLon);
    out[0] = (float)(cLat * cLon);
    out[1] = (float)(cLat * sLon);
    out[2] = (float)sLat;
}

// s0 as the reference seeds it (js/rng.js:4; host_util.h's ParkMiller computes the same), the constants of the loop's head and both
// tables into lng[CHAIN_CAP], z[CHAIN_CAP].  Returns 0, or 1 where a table would overflow.
inline int fib_setup(int32_t N, double jitter, double seed, ChainEntry* lng, ChainEntry* z, FibParams& P) {
    const double v = std::abs(std::floor(seed * 9301.0 + 49297.0));
    P.N = N; P.jitter = jitter;
    P.s0 = (uint32_t)(uint64_t)(std::fmod(v, 2147483646.0) + 1.0);
    P.s = 3.6 / std::sqrt((double)N);
    P.dz = 2.0 / (double)N;
    const double dlong = FIB_PI * (3.0 - std::sqrt(5.0));
    P.nLng = build_chain(0.0, dlong, N, lng);
    P.nZ = build_chain(1.0 - P.dz / 2.0, -P.dz, N, z);
    P.lng = lng; P.z = z;
    return (P.nLng < 0 || P.nZ < 0) ? 1 : 0;
}

}  // namespace points
}  // namespace wo
