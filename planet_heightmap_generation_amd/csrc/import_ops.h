// Heightmap import (js/planet-worker.js:682-831): per-cell bodies shared by the device kernels (heightmap.hip) and the
// test-only CPU emulator (tests/emu_import), so that both compile the very same arithmetic.
//
// Contract (bit-identical to the reference):
//   * fd_asin / fd_atan / fd_atan2 are f64 ports of fdlibm's e_asin.c / s_atan.c / e_atan2.c in the form V8 ships them
//     (src/base/ieee754.cc: Math.asin, Math.atan2).  Neither ocml nor glibc promises those bits (glibc differs from V8 for
//     ~6 % of f32-derived asin arguments and ~18 % of atan2 ones), and one ulp in one sampled cell can move the priority
//     flood downstream.  Plain f64 arithmetic and bit manipulation only; the library compiles with -ffp-contract=off, so no
//     FMA changes a result.
//   * sample_heightmap_cell restates sampleHeightmap / sampleBilinear / grayscaleToElevation (:682-727) in the
//     reference's operation order (left-to-right association of the four bilinear products), f64 throughout, f32 store.
//   * classification (:811-831) on the FINAL field with JS comparison semantics (NaN is land, never coast or mountain):
//       ocean_r  e <= 0     mountain_r  e > 0.5     coastline_r  e > 0 and some neighbour has e <= 0
//   * deriveSyntheticPlates (:733-769): r_plate[r] = smallest region id of r's component, cells joined along mesh edges
//     whose endpoints share (e <= 0).  With a symmetric adjacency this is the reference's ascending-r BFS labelling; the
//     device computes it by union-find (cc_find / cc_hook_cell / cc_flatten_cell, ECL-CC style): every hook puts a
//     larger root under a smaller one, so a component's surviving root is its minimum id whatever the interleaving.
#pragma once
#include <cstdint>
#include <cstring>
#include <cmath>

#if defined(__HIPCC__)
#define WO_IMP_HD __host__ __device__
#else
#define WO_IMP_HD
#endif

namespace wo {
namespace imp {

WO_IMP_HD inline int32_t hi_word(double x) { uint64_t u; memcpy(&u, &x, 8); return (int32_t)(uint32_t)(u >> 32); }
WO_IMP_HD inline uint32_t lo_word(double x) { uint64_t u; memcpy(&u, &x, 8); return (uint32_t)u; }
WO_IMP_HD inline double with_lo_zero(double x) { uint64_t u; memcpy(&u, &x, 8); u &= 0xffffffff00000000ull; double r; memcpy(&r, &u, 8); return r; }
WO_IMP_HD inline double fd_fabs(double x) { uint64_t u; memcpy(&u, &x, 8); u &= 0x7fffffffffffffffull; double r; memcpy(&r, &u, 8); return r; }

// e_asin.c
WO_IMP_HD inline double fd_asin(double x) {
    const double one = 1.0, huge = 1.000e+300;
    const double pio2_hi = 1.57079632679489655800e+00, pio2_lo = 6.12323399573676603587e-17, pio4_hi = 7.85398163397448278999e-01;
    const double pS0 = 1.66666666666666657415e-01, pS1 = -3.25565818622400915405e-01, pS2 = 2.01212532134862925881e-01,
                 pS3 = -4.00555345006794114027e-02, pS4 = 7.91534994289814532176e-04, pS5 = 3.47933107596021167570e-05;
    const double qS1 = -2.40339491173441421878e+00, qS2 = 2.02094576023350569471e+00, qS3 = -6.88283971605453293030e-01,
                 qS4 = 7.70381505559019352791e-02;
    double t = 0.0, w, p, q, c, r, s;
    const int32_t hx = hi_word(x), ix = hx & 0x7fffffff;
    if (ix >= 0x3ff00000) {                                  // |x| >= 1
        if (((ix - 0x3ff00000) | (int32_t)lo_word(x)) == 0) return x * pio2_hi + x * pio2_lo;
        return (x - x) / (x - x);                            // |x| > 1 or NaN: NaN
    } else if (ix < 0x3fe00000) {                            // |x| < 0.5
        if (ix < 0x3e400000) {                               // |x| < 2^-27
            if (huge + x > one) return x;
        } else {
            t = x * x;
        }
        p = t * (pS0 + t * (pS1 + t * (pS2 + t * (pS3 + t * (pS4 + t * pS5)))));
        q = one + t * (qS1 + t * (qS2 + t * (qS3 + t * qS4)));
        w = p / q;
        return x + x * w;
    }
    // 1 > |x| >= 0.5
    w = one - fd_fabs(x);
    t = w * 0.5;
    p = t * (pS0 + t * (pS1 + t * (pS2 + t * (pS3 + t * (pS4 + t * pS5)))));
    q = one + t * (qS1 + t * (qS2 + t * (qS3 + t * qS4)));
    s = sqrt(t);
    if (ix >= 0x3FEF3333) {                                  // |x| > 0.975
        w = p / q;
        t = pio2_hi - (2.0 * (s + s * w) - pio2_lo);
    } else {
        w = with_lo_zero(s);
        c = (t - w * w) / (s + w);
        r = p / q;
        p = 2.0 * s * r - (pio2_lo - 2.0 * c);
        q = pio4_hi - 2.0 * w;
        t = pio4_hi - (p - q);
    }
    return hx > 0 ? t : -t;
}

// s_atan.c
WO_IMP_HD inline double fd_atan(double x) {
    const double atanhi[4] = {4.63647609000806093515e-01, 7.85398163397448278999e-01, 9.82793723247329054082e-01, 1.57079632679489655800e+00};
    const double atanlo[4] = {2.26987774529616870924e-17, 3.06161699786838301793e-17, 1.39033110312309984516e-17, 6.12323399573676603587e-17};
    const double aT[11] = {3.33333333333329318027e-01, -1.99999999998764832476e-01, 1.42857142725034663711e-01, -1.11111104054623557880e-01,
                           9.09088713343650656196e-02, -7.69187620504482999495e-02, 6.66107313738753120669e-02, -5.83357013379057348645e-02,
                           4.97687799461593236017e-02, -3.65315727442169155270e-02, 1.62858201153657823623e-02};
    const double one = 1.0, huge = 1.000e+300;
    double w, s1, s2, z;
    int id;
    const int32_t hx = hi_word(x), ix = hx & 0x7fffffff;
    if (ix >= 0x44100000) {                                  // |x| >= 2^66
        if (ix > 0x7ff00000 || (ix == 0x7ff00000 && lo_word(x) != 0)) return x + x;   // NaN
        return hx > 0 ? atanhi[3] + atanlo[3] : -atanhi[3] - atanlo[3];
    }
    if (ix < 0x3fdc0000) {                                   // |x| < 0.4375
        if (ix < 0x3e400000) {                               // |x| < 2^-27
            if (huge + x > one) return x;
        }
        id = -1;
    } else {
        x = fd_fabs(x);
        if (ix < 0x3ff30000) {                               // |x| < 1.1875
            if (ix < 0x3fe60000) { id = 0; x = (2.0 * x - one) / (2.0 + x); }     // 7/16 <= |x| < 11/16
            else                 { id = 1; x = (x - one) / (x + one); }           // 11/16 <= |x| < 19/16
        } else {
            if (ix < 0x40038000) { id = 2; x = (x - 1.5) / (one + 1.5 * x); }     // |x| < 2.4375
            else                 { id = 3; x = -1.0 / x; }                         // 2.4375 <= |x| < 2^66
        }
    }
    z = x * x;
    w = z * z;
    s1 = z * (aT[0] + w * (aT[2] + w * (aT[4] + w * (aT[6] + w * (aT[8] + w * aT[10])))));
    s2 = w * (aT[1] + w * (aT[3] + w * (aT[5] + w * (aT[7] + w * aT[9]))));
    if (id < 0) return x - x * (s1 + s2);
    z = atanhi[id] - ((x * (s1 + s2) - atanlo[id]) - x);
    return hx < 0 ? -z : z;
}

// e_atan2.c (V8's form: |y/x| > 2^60 gives +-pi/2 in every quadrant)
WO_IMP_HD inline double fd_atan2(double y, double x) {
    const double tiny = 1.0e-300, pi_o_4 = 7.8539816339744827900E-01, pi_o_2 = 1.5707963267948965580E+00,
                 pi = 3.1415926535897931160E+00, pi_lo = 1.2246467991473531772E-16;
    double z;
    const int32_t hx = hi_word(x), ix = hx & 0x7fffffff, hy = hi_word(y), iy = hy & 0x7fffffff;
    const uint32_t lx = lo_word(x), ly = lo_word(y);
    if (((uint32_t)ix | ((lx | (0u - lx)) >> 31)) > 0x7ff00000u || ((uint32_t)iy | ((ly | (0u - ly)) >> 31)) > 0x7ff00000u) return x + y;   // NaN
    if ((((uint32_t)hx - 0x3ff00000u) | lx) == 0) return fd_atan(y);                                                                    // x == 1
    int m = ((hy >> 31) & 1) | ((hx >> 30) & 2);             // 2*sign(x) + sign(y)
    if ((iy | (int32_t)ly) == 0) {                           // y == 0
        switch (m) { case 0: case 1: return y; case 2: return pi + tiny; default: return -pi - tiny; }
    }
    if ((ix | (int32_t)lx) == 0) return hy < 0 ? -pi_o_2 - tiny : pi_o_2 + tiny;      // x == 0
    if (ix == 0x7ff00000) {                                  // x is INF
        if (iy == 0x7ff00000) {
            switch (m) { case 0: return pi_o_4 + tiny; case 1: return -pi_o_4 - tiny; case 2: return 3.0 * pi_o_4 + tiny; default: return -3.0 * pi_o_4 - tiny; }
        } else {
            switch (m) { case 0: return 0.0; case 1: return -0.0; case 2: return pi + tiny; default: return -pi - tiny; }
        }
    }
    if (iy == 0x7ff00000) return hy < 0 ? -pi_o_2 - tiny : pi_o_2 + tiny;             // y is INF
    const int32_t k = (iy - ix) >> 20;
    if (k > 60) { z = pi_o_2 + 0.5 * pi_lo; m &= 1; }        // |y/x| > 2^60
    else if (hx < 0 && k < -60) z = 0.0;                     // 0 > |y|/x > -2^-60
    else z = fd_atan(fd_fabs(y / x));
    switch (m) {
        case 0: return z;
        case 1: return -z;
        case 2: return pi - (z - pi_lo);
        default: return (z - pi_lo) - pi;
    }
}

// sampleHeightmap for one cell (:710-727 with sampleBilinear :682-697 and grayscaleToElevation :704-707)
WO_IMP_HD inline float sample_heightmap_cell(float fx_, float fy_, float fz_, const uint8_t* pixels, int32_t imgW, int32_t imgH) {
    const double pi = 3.141592653589793;
    double y = (double)fy_;
    if (!(y != y)) y = y > 1.0 ? 1.0 : y;                   // Math.max(-1, Math.min(1, y)): NaN stays NaN, -0 stays -0
    if (!(y != y)) y = y < -1.0 ? -1.0 : y;
    const double lat = fd_asin(y);
    const double lon = fd_atan2((double)fx_, (double)fz_);
    const double W = (double)imgW, H = (double)imgH;
    const double px = (lon / pi + 1.0) * 0.5 * W;
    double py = (0.5 - lat / pi) * H;
    py = (py != py) ? py : (py < H - 1.0 ? py : H - 1.0);      // Math.max(0, Math.min(py, imgH - 1))
    py = (py != py) ? py : (py > 0.0 ? py : 0.0);
    if (px != px || py != py) return (float)(px + py);     // pixels[NaN] is undefined in JS: the sample is NaN
    const double x0 = floor(px), y0 = floor(py);
    const int64_t x0i = (int64_t)x0, y0i = (int64_t)y0, w = imgW;
    const int64_t x1 = (((x0i + 1) % w) + w) % w;            // horizontal wrap (px == W at lon == pi; x0 >= 0, so this is (x0 + 1) % W)
    const int64_t y1 = (y0i + 1 < imgH - 1) ? y0i + 1 : (int64_t)imgH - 1;
    const int64_t xw = ((x0i % w) + w) % w;
    const double fx = px - x0, fy = py - y0;
    const double v00 = pixels[y0i * w + xw], v10 = pixels[y0i * w + x1], v01 = pixels[y1 * w + xw], v11 = pixels[y1 * w + x1];
    const double v = v00 * (1.0 - fx) * (1.0 - fy) + v10 * fx * (1.0 - fy) + v01 * (1.0 - fx) * fy + v11 * fx * fy;
    if (v < 1.0) return -0.5f;
    return (float)sqrt((v - 1.0) / 254.0);
}

// classification bits of one cell (:811-831) plus the synthetic-plate seed bits (:733-769)
enum : uint8_t { CLS_OCEAN = 1, CLS_MOUNTAIN = 2, CLS_COAST = 4, CLS_SEED = 8, CLS_SEED_OCEAN = 16 };
WO_IMP_HD inline uint8_t classify_cell(const float* e, const int32_t* off, const int32_t* adj, int32_t r) {
    const float v = e[r];
    uint8_t f = 0;
    if (v <= 0.0f) f |= CLS_OCEAN;
    else if (v > 0.5f) f |= CLS_MOUNTAIN;
    if (v > 0.0f) {
        for (int32_t i = off[r]; i < off[r + 1]; ++i)
            if (e[adj[i]] <= 0.0f) { f |= CLS_COAST; break; }
    }
    return f;
}

// ---- union-find over the same-class edges (parent values only ever decrease: racing path-halving stores are benign) ----
#if defined(__HIP_DEVICE_COMPILE__)
__device__ inline int32_t cc_load(int32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ inline void cc_store(int32_t* p, int32_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ inline int32_t cc_cas(int32_t* p, int32_t expect, int32_t want) { return atomicCAS(p, expect, want); }
#else
inline int32_t cc_load(int32_t* p) { return __atomic_load_n(p, __ATOMIC_RELAXED); }
inline void cc_store(int32_t* p, int32_t v) { __atomic_store_n(p, v, __ATOMIC_RELAXED); }
inline int32_t cc_cas(int32_t* p, int32_t expect, int32_t want) { __atomic_compare_exchange_n(p, &expect, want, false, __ATOMIC_RELAXED, __ATOMIC_RELAXED); return expect; }
#endif

// root of r with path halving
WO_IMP_HD inline int32_t cc_find(int32_t* parent, int32_t r) {
    int32_t cur = cc_load(parent + r);
    if (cur != r) {
        int32_t prev = r, next;
        while (cur > (next = cc_load(parent + cur))) {
            cc_store(parent + prev, next);
            prev = cur;
            cur = next;
        }
    }
    return cur;
}
WO_IMP_HD inline bool cc_same_class(const float* e, int32_t a, int32_t b) { return (e[a] <= 0.0f) == (e[b] <= 0.0f); }
// every same-class edge (r, nb) with nb > r: join the two trees, the larger root under the smaller one
WO_IMP_HD inline void cc_hook_cell(int32_t* parent, const float* e, const int32_t* off, const int32_t* adj, int32_t r) {
    int32_t a = -1;
    for (int32_t i = off[r]; i < off[r + 1]; ++i) {
        const int32_t nb = adj[i];
        if (nb <= r || !cc_same_class(e, r, nb)) continue;
        if (a < 0) a = cc_find(parent, r);
        int32_t b = cc_find(parent, nb);
        while (a != b) {
            if (a < b) {
                const int32_t got = cc_cas(parent + b, b, a);
                if (got == b) break;
                b = got;                                     // b was no longer a root: climb
            } else {
                const int32_t got = cc_cas(parent + a, a, b);
                if (got == a) { a = b; break; }
                a = got;
            }
        }
    }
}
// after every hook: each cell's own entry := its root.  The chase stores nothing else: a halving store of another thread
// could otherwise put a non-root back into an entry that was already flattened.
WO_IMP_HD inline void cc_flatten_cell(int32_t* parent, int32_t r) {
    int32_t cur = cc_load(parent + r), next;
    const int32_t old = cur;
    while (cur > (next = cc_load(parent + cur))) cur = next;
    if (cur != old) cc_store(parent + r, cur);
}

}  // namespace imp
}  // namespace wo
