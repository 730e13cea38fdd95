// Heightmap import (js/planet-worker.js:682-831): per-cell bodies shared by the device kernels (heightmap.hip) and the
// test-only CPU emulator (tests/emu_import), so that both compile the very same arithmetic.
//
// Contract (bit-identical to the reference):
//   * fd_asin / fd_atan / fd_atan2 are f64 ports of fdlibm's e_asin.c / s_atan.c / e_atan2.c in the form V8 ships them
//     (src/base/ieee754.cc: Math.asin, Math.atan2).  Neither ocml nor glibc promises those bits (glibc differs from V8 for
//     ~6 % of f32-derived asin arguments and ~18 % of atan2 ones), and one ulp in one sampled cell can move the priority
//     flood downstream.  Plain f64 arithmetic and bit manipulation only; the library compiles with -ffp-contract=off, so no
//     FMA changes a result.
//   * fd_sin / fd_cos / fd_exp (with fd_kernel_sin / fd_kernel_cos / fd_rem_pio2) are the same for s_sin.c / s_cos.c / e_exp.c: Math.sin,
//     Math.cos and Math.exp of the plate generation's host stage (csrc/plates_gen_host.cc: Euler pole angles in [0, 2pi), continent
//     weights exp(x) with |x| <= 1.25).  Supported domain of sin / cos: |x| up to about 2^20 * pi/2 = 1 647 099 (the reduction's
//     special case and medium path); beyond it they return NaN instead of a number fdlibm would not give.  exp: every double.
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

// k_sin.c: sine on [-pi/4, pi/4]; (x, y) is the reduced argument head and tail, iy == 0 says y is exactly 0
WO_IMP_HD inline double fd_kernel_sin(double x, double y, int iy) {
    const double S1 = -1.66666666666666324348e-01, S2 = 8.33333333332248946124e-03, S3 = -1.98412698298579493134e-04,
                 S4 = 2.75573137070700676789e-06, S5 = -2.50507602534068634195e-08, S6 = 1.58969099521155010221e-10;
    const int32_t ix = hi_word(x) & 0x7fffffff;
    if (ix < 0x3e400000) { if ((int)x == 0) return x; }    // |x| < 2^-27
    const double z = x * x, v = z * x;
    const double r = S2 + z * (S3 + z * (S4 + z * (S5 + z * S6)));
    if (iy == 0) return x + v * (S1 + z * r);
    return x - ((z * (0.5 * y - v * r) - y) - v * S1);
}

// k_cos.c: cosine on [-pi/4, pi/4]
WO_IMP_HD inline double fd_kernel_cos(double x, double y) {
    const double one = 1.0;
    const double C1 = 4.16666666666666019037e-02, C2 = -1.38888888888741095749e-03, C3 = 2.48015872894767294178e-05,
                 C4 = -2.75573143513906633035e-07, C5 = 2.08757232129817482790e-09, C6 = -1.13596475577881948265e-11;
    const int32_t ix = hi_word(x) & 0x7fffffff;
    if (ix < 0x3e400000) { if ((int)x == 0) return one; }  // |x| < 2^-27
    const double z = x * x;
    const double r = z * (C1 + z * (C2 + z * (C3 + z * (C4 + z * (C5 + z * C6)))));
    if (ix < 0x3FD33333) return one - (0.5 * z - (z * r - x * y));          // |x| < 0.3
    double qx;
    if (ix > 0x3fe90000) qx = 0.28125;                      // |x| > 0.78125
    else { const uint64_t u = (uint64_t)(uint32_t)(ix - 0x00200000) << 32; memcpy(&qx, &u, 8); }     // x / 4
    const double hz = 0.5 * z - qx, a = one - qx;
    return a - (hz - (z * r - x * y));
}

// e_rem_pio2.c without its last branch: y[0] + y[1] = x - n * pi/2 for |x| up to about 2^20 * pi/2 (high word <= 0x413921fb), which
// takes the special case below 3pi/4 and the medium path with up to three rounds of Cody-Waite subtraction.  Larger
// arguments need the 1584-bit table of k_rem_pio2.c, which is not ported: returns false and the callers give NaN.
WO_IMP_HD inline bool fd_rem_pio2(double x, double* y, int32_t* nOut) {
    const int32_t npio2_hw[32] = {0x3FF921FB, 0x400921FB, 0x4012D97C, 0x401921FB, 0x401F6A7A, 0x4022D97C, 0x4025FDBB, 0x402921FB,
                                  0x402C463A, 0x402F6A7A, 0x4031475C, 0x4032D97C, 0x40346B9C, 0x4035FDBB, 0x40378FDB, 0x403921FB,
                                  0x403AB41B, 0x403C463A, 0x403DD85A, 0x403F6A7A, 0x40407E4C, 0x4041475C, 0x4042106C, 0x4042D97C,
                                  0x4043A28C, 0x40446B9C, 0x404534AC, 0x4045FDBB, 0x4046C6CB, 0x40478FDB, 0x404858EB, 0x404921FB};
    const double half = 0.5, invpio2 = 6.36619772367581382433e-01, pio2_1 = 1.57079632673412561417e+00, pio2_1t = 6.07710050650619224932e-11,
                 pio2_2 = 6.07710050630396597660e-11, pio2_2t = 2.02226624879595063154e-21, pio2_3 = 2.02226624871116645580e-21,
                 pio2_3t = 8.47842766036889956997e-32;
    double z, w, t, r, fn;
    const int32_t hx = hi_word(x), ix = hx & 0x7fffffff;
    if (ix <= 0x3fe921fb) { y[0] = x; y[1] = 0; *nOut = 0; return true; }        // |x| <= pi/4
    if (ix < 0x4002d97c) {                                                          // |x| < 3pi/4: n = +-1
        if (hx > 0) {
            z = x - pio2_1;
            if (ix != 0x3ff921fb) { y[0] = z - pio2_1t; y[1] = (z - y[0]) - pio2_1t; }
            else { z -= pio2_2; y[0] = z - pio2_2t; y[1] = (z - y[0]) - pio2_2t; }   // near pi/2: 33 + 33 + 53 bits of pi
            *nOut = 1;
        } else {
            z = x + pio2_1;
            if (ix != 0x3ff921fb) { y[0] = z + pio2_1t; y[1] = (z - y[0]) + pio2_1t; }
            else { z += pio2_2; y[0] = z + pio2_2t; y[1] = (z - y[0]) + pio2_2t; }
            *nOut = -1;
        }
        return true;
    }
    if (ix > 0x413921fb) return false;
    t = fd_fabs(x);
    const int32_t n = (int32_t)(t * invpio2 + half);
    fn = (double)n;
    r = t - fn * pio2_1;
    w = fn * pio2_1t;                                                               // first round: good to 85 bits
    if (n < 32 && ix != npio2_hw[n - 1]) {
        y[0] = r - w;
    } else {
        const int32_t j = ix >> 20;
        y[0] = r - w;
        int32_t i = j - (int32_t)(((uint32_t)hi_word(y[0]) >> 20) & 0x7ff);
        if (i > 16) {                                                               // second round: good to 118 bits
            t = r; w = fn * pio2_2; r = t - w; w = fn * pio2_2t - ((t - r) - w); y[0] = r - w;
            i = j - (int32_t)(((uint32_t)hi_word(y[0]) >> 20) & 0x7ff);
            if (i > 49) { t = r; w = fn * pio2_3; r = t - w; w = fn * pio2_3t - ((t - r) - w); y[0] = r - w; }   // third: 151 bits
        }
    }
    y[1] = (r - y[0]) - w;
    if (hx < 0) { y[0] = -y[0]; y[1] = -y[1]; *nOut = -n; } else *nOut = n;
    return true;
}

// s_sin.c / s_cos.c in V8's form (Math.sin, Math.cos).  Supported domain: |x| < about 1 647 099 (2^20 * pi/2: high word <= 0x413921fb), which
// holds every argument this library forms (Euler pole angles in [0, 2pi)); infinities and NaN give NaN as in fdlibm,
// finite arguments beyond the domain give NaN as well (fdlibm would go on to k_rem_pio2.c).
WO_IMP_HD inline double fd_sin(double x) {
    const int32_t ix = hi_word(x) & 0x7fffffff;
    if (ix <= 0x3fe921fb) return fd_kernel_sin(x, 0.0, 0);
    if (ix >= 0x7ff00000) return x - x;
    double y[2]; int32_t n;
    if (!fd_rem_pio2(x, y, &n)) return (x - x) / (x - x);
    switch (n & 3) {
        case 0: return fd_kernel_sin(y[0], y[1], 1);
        case 1: return fd_kernel_cos(y[0], y[1]);
        case 2: return -fd_kernel_sin(y[0], y[1], 1);
        default: return -fd_kernel_cos(y[0], y[1]);
    }
}
WO_IMP_HD inline double fd_cos(double x) {
    const int32_t ix = hi_word(x) & 0x7fffffff;
    if (ix <= 0x3fe921fb) return fd_kernel_cos(x, 0.0);
    if (ix >= 0x7ff00000) return x - x;
    double y[2]; int32_t n;
    if (!fd_rem_pio2(x, y, &n)) return (x - x) / (x - x);
    switch (n & 3) {
        case 0: return fd_kernel_cos(y[0], y[1]);
        case 1: return -fd_kernel_sin(y[0], y[1], 1);
        case 2: return -fd_kernel_cos(y[0], y[1]);
        default: return fd_kernel_sin(y[0], y[1], 1);
    }
}

// e_exp.c in V8's form (Math.exp; exp(1) returns Math.E exactly).  Supported domain: every double.
WO_IMP_HD inline double fd_exp(double x) {
    const double one = 1.0, halF[2] = {0.5, -0.5}, o_threshold = 7.09782712893383973096e+02, u_threshold = -7.45133219101941108420e+02,
                 ln2HI[2] = {6.93147180369123816490e-01, -6.93147180369123816490e-01}, ln2LO[2] = {1.90821492927058770002e-10, -1.90821492927058770002e-10},
                 invln2 = 1.44269504088896338700e+00, P1 = 1.66666666666666019037e-01, P2 = -2.77777777770155933842e-03,
                 P3 = 6.61375632143793436117e-05, P4 = -1.65339022054652515390e-06, P5 = 4.13813679705723846039e-08, E = 2.718281828459045;
    const double huge = 1.0e+300, twom1000 = 9.33263618503218878990e-302, two1023 = 8.988465674311579539e307;
    double y, hi = 0.0, lo = 0.0, c, t, twopk;
    int32_t k = 0;
    uint32_t hx = (uint32_t)hi_word(x);
    const int32_t xsb = (int32_t)((hx >> 31) & 1);
    hx &= 0x7fffffff;
    if (hx >= 0x40862E42) {                                  // |x| >= 709.78...
        if (hx >= 0x7ff00000) {
            if (((hx & 0xfffff) | lo_word(x)) != 0) return x + x;      // NaN
            return xsb == 0 ? x : 0.0;                       // exp(+-inf) = {inf, 0}
        }
        if (x > o_threshold) return huge * huge;
        if (x < u_threshold) return twom1000 * twom1000;
    }
    if (hx > 0x3fd62e42) {                                   // |x| > 0.5 ln2
        if (hx < 0x3FF0A2B2) {                               // and |x| < 1.5 ln2
            if (x == 1.0) return E;
            hi = x - ln2HI[xsb]; lo = ln2LO[xsb]; k = 1 - xsb - xsb;
        } else {
            k = (int32_t)(invln2 * x + halF[xsb]);
            t = k;
            hi = x - t * ln2HI[0];
            lo = t * ln2LO[0];
        }
        x = hi - lo;
    } else if (hx < 0x3e300000) {                            // |x| < 2^-28
        if (huge + x > one) return one + x;
    } else {
        k = 0;
    }
    t = x * x;
    { const uint64_t u = (uint64_t)(uint32_t)(0x3ff00000 + ((k >= -1021 ? k : k + 1000) * 1048576)) << 32; memcpy(&twopk, &u, 8); }
    c = x - t * (P1 + t * (P2 + t * (P3 + t * (P4 + t * P5))));
    if (k == 0) return one - ((x * c) / (c - 2.0) - x);
    y = one - ((lo - (x * c) / (2.0 - c)) - hi);
    if (k >= -1021) {
        if (k == 1024) return y * 2.0 * two1023;
        return y * twopk;
    }
    return y * twopk * twom1000;
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
