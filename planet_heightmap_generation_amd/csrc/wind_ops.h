// Seasonal pressure and wind (js/wind.js:394-687): per-cell bodies shared by the device kernels (wind.hip) and the
// test-only CPU emulator (tests/emu_wind), so that both compile the very same arithmetic.
//
// Contract:
//   * Number arithmetic is f64 in the reference's operation order, stores are f32 (the reference's Float32Arrays); the
//     library compiles with -ffp-contract=off.
//   * r_lat / r_lon come from the V8-exact fd_asin / fd_atan2 of import_ops.h: they are outputs and feed the floor of
//     the 36 x 72 binning.  exp / sin / cos (the Gaussians of regionPressure, the rotation of pressureToWind and the
//     cos(dlon) of the disc test) are the platform's: ocml on the device, glibc in the emulator.  They are called
//     UNQUALIFIED so that the emulator's second build can route them through tests/emu/libm_perturb.h.
//   * Everything that runs on the host in the product (the 576 sample centres, the 72-point smoothing, the periodic
//     spline) is plain host code here and calls std:: functions: the emulator runs the same host code.
//   * Order-free parts: the ocean components (union-find of import_ops.h over the edges whose two ends are non-land, a
//     component's label is its smallest cell), the main ocean (largest, ties to the smallest first cell: the reference's
//     `size > mainOceanSize` is strict over ascending first cells) and the two hop-distance fields (any level-synchronous
//     BFS gives the reference's FIFO distances).
//   * elevSum of a disc sample is a sequential f64 sum in bin-then-cell order (cells of a bin ascending): sample kernels
//     must add in that order; +0 terms (cells with e <= 0) may be skipped, which is exact.
#pragma once
#include <cstdint>
#include <cmath>

#include "import_ops.h"
#include "noise.h"

namespace wo {
namespace wind {

constexpr double PI = 3.141592653589793;
constexpr double DEG = PI / 180;
constexpr double RAD = 180 / PI;
constexpr int LAT_BINS = 36, LON_BINS = 72, NUM_BINS = LAT_BINS * LON_BINS;
constexpr int NUM_LON = 72, NUM_DEG = 4, NUM_SAMPLES = 2 * NUM_LON * NUM_DEG;      // season x longitude x {5, 10, 15, 20} degrees
constexpr int ITCZ_SAMPLES = 360;

WO_HD inline double js_max(double a, double b) { return (a != a || b != b) ? (a + b) : (a > b ? a : b); }   // Math.max / Math.min: NaN propagates
WO_HD inline double js_min(double a, double b) { return (a != a || b != b) ? (a + b) : (a < b ? a : b); }

// js/wind.js:75-79
WO_HD inline double smoothstep(double edge0, double edge1, double x) {
    if (edge0 == edge1) return x >= edge1 ? 1 : 0;
    const double t = js_max(0, js_min(1, (x - edge0) / (edge1 - edge0)));
    return t * t * (3 - 2 * t);
}

// js/color-map.js:7-12
WO_HD inline double elev_to_height_km(double elev) {
    if (elev <= 0) return elev * 10;
    const double t = js_min(elev, 1);
    const double t2 = t * t;
    return 6 * t2 * t2 * (5 - 4 * t);
}

// ---- step 0 (:418-443) ----
struct CellGeo {
    float *lat, *lon, *sinLat, *cosLat;
    uint8_t* isLand;
    float *eastX, *eastY, *eastZ, *northX, *northY, *northZ;
};

WO_HD inline void precompute_cell(const float* xyz, const float* e, const CellGeo& G, int32_t r) {
    const double x = xyz[3 * (int64_t)r], y = xyz[3 * (int64_t)r + 1], z = xyz[3 * (int64_t)r + 2];
    G.lat[r] = (float)imp::fd_asin(js_max(-1, js_min(1, y)));
    G.lon[r] = (float)imp::fd_atan2(x, z);
    G.sinLat[r] = (float)y;
    double c = sqrt(1 - y * y);
    if (!(c != 0)) c = 0.01;                                 // `|| 0.01`: 0 and NaN are falsy
    G.cosLat[r] = (float)c;
    G.isLand[r] = e[r] > 0.0f ? 1 : 0;
    double ex = z, ey = 0, ez = -x;
    double elen = sqrt(ex * ex + ez * ez);
    if (elen < 1e-10) { ex = 1; ez = 0; elen = 1; }
    ex /= elen; ez /= elen;
    double nx = y * ez - z * ey, ny = z * ex - x * ez, nz = x * ey - y * ex;
    double nlen = sqrt(nx * nx + ny * ny + nz * nz);
    if (!(nlen != 0)) nlen = 1;
    nx /= nlen; ny /= nlen; nz /= nlen;
    G.eastX[r] = (float)ex; G.eastY[r] = (float)ey; G.eastZ[r] = (float)ez;
    G.northX[r] = (float)nx; G.northY[r] = (float)ny; G.northZ[r] = (float)nz;
}

// ---- geo index (:95-100): the bin of a cell, from the stored f32 latitude and longitude ----
WO_HD inline int32_t clamp_floor(double v, int32_t hi) {      // Math.max(0, Math.min(hi, Math.floor(v))); NaN never reaches here from finite positions
    const double f = floor(v);
    return f < 0 ? 0 : (f > (double)hi ? hi : (int32_t)f);
}
WO_HD inline int32_t bin_of(float lat, float lon) {
    const int32_t latBin = clamp_floor(((double)lat + PI / 2) / PI * LAT_BINS, LAT_BINS - 1);
    const int32_t lonBin = clamp_floor(((double)lon + PI) / (2 * PI) * LON_BINS, LON_BINS - 1);
    return latBin * LON_BINS + lonBin;
}

// one disc sample of computeITCZ (:126-145, :184-192): centre, bin window and the constants of the membership test.
// Host code in the product (std:: functions); index = (season * NUM_LON + i) * NUM_DEG + (deg / 5 - 1)
struct SampleSpec {
    double lon, sinLat0, cosLat0, cosRadius;
    int32_t bMin, bMax, lMin, lMax;
};
struct SampleAcc { double elevSum; int32_t landCount, totalCount; };

inline void make_sample_specs(SampleSpec* out) {
    const double radius = 20 * DEG;
    for (int season = 0; season < 2; ++season)
        for (int i = 0; i < NUM_LON; ++i)
            for (int d = 0; d < NUM_DEG; ++d) {
                const double sign = season == 0 ? 1 : -1;
                const double lon = -PI + (i + 0.5) * (2 * PI / NUM_LON);
                const double lat = (5 + 5 * d) * sign * DEG;
                SampleSpec& S = out[(season * NUM_LON + i) * NUM_DEG + d];
                const double latMin = lat - radius, latMax = lat + radius;
                S.bMin = (int32_t)std::fmax(0, std::floor((latMin + PI / 2) / PI * LAT_BINS));
                S.bMax = (int32_t)std::fmin(LAT_BINS - 1, std::floor((latMax + PI / 2) / PI * LAT_BINS));
                double cosLat = std::cos(lat);
                if (!(cosLat != 0)) cosLat = 0.01;
                const double lonSpan = radius / cosLat;
                S.lMin = (int32_t)std::floor((lon - lonSpan + PI) / (2 * PI) * LON_BINS);
                S.lMax = (int32_t)std::floor((lon + lonSpan + PI) / (2 * PI) * LON_BINS);
                S.lon = lon; S.cosRadius = std::cos(radius); S.sinLat0 = std::sin(lat); S.cosLat0 = std::cos(lat);
            }
}
WO_HD inline int32_t sample_bin(int32_t bi, int32_t li) { return bi * LON_BINS + ((li % LON_BINS) + LON_BINS) % LON_BINS; }
// :149-153
WO_HD inline bool sample_member(const SampleSpec& S, float sinLat1, float cosLat1, float lon1) {
    const double dlon = (double)lon1 - S.lon;
    const double cosDist = S.sinLat0 * (double)sinLat1 + S.cosLat0 * (double)cosLat1 * cos(dlon);
    return cosDist >= S.cosRadius;
}

// ---- ITCZ (:12-71, :193-231): host code in the product ----
struct Spline { double xs[NUM_LON], ys[NUM_LON], b[NUM_LON], c[NUM_LON], d[NUM_LON]; };

inline void build_periodic_spline(const double* xs, const double* ys, Spline& S) {
    const int n = NUM_LON;
    const double period = 2 * PI;
    double h[NUM_LON], alpha[NUM_LON];
    for (int i = 0; i < n; ++i) {
        const int next = (i + 1) % n;
        h[i] = std::fmod(xs[next] - xs[i] + period, period);
        if (h[i] == 0) h[i] = period / n;
    }
    for (int i = 0; i < n; ++i) {
        const int prev = (i - 1 + n) % n, next = (i + 1) % n;
        alpha[i] = (3 / h[i]) * (ys[next] - ys[i]) - (3 / h[prev]) * (ys[i] - ys[prev]);
    }
    for (int i = 0; i < n; ++i) { S.xs[i] = xs[i]; S.ys[i] = ys[i]; S.c[i] = 0; }
    for (int iter = 0; iter < 20; ++iter)
        for (int i = 0; i < n; ++i) {
            const int prev = (i - 1 + n) % n, next = (i + 1) % n;
            S.c[i] = (alpha[i] - h[prev] * S.c[prev] - h[i] * S.c[next]) / (2 * (h[prev] + h[i]));
        }
    for (int i = 0; i < n; ++i) {
        const int next = (i + 1) % n;
        S.b[i] = (ys[next] - ys[i]) / h[i] - h[i] * (S.c[next] + 2 * S.c[i]) / 3;
        S.d[i] = (S.c[next] - S.c[i]) / (3 * h[i]);
    }
}

// :55-71 (fmod is exact on every platform)
WO_HD inline double evaluate_spline(const Spline& S, double lon) {
    const double period = 2 * PI;
    const int n = NUM_LON;
    const double t = fmod(fmod(lon - S.xs[0], period) + period, period) + S.xs[0];
    int seg = 0;
    for (int i = 0; i < n; ++i) {
        const double lo = S.xs[i];
        const double hi = i < n - 1 ? S.xs[i + 1] : S.xs[0] + period;
        if (t >= lo && t < hi) { seg = i; break; }
    }
    const double dx = t - S.xs[seg];
    return S.ys[seg] + S.b[seg] * dx + S.c[seg] * dx * dx + S.d[seg] * dx * dx * dx;
}

// computeITCZ after its samples (:193-231) for both seasons, and the 360 visualisation points (:656-665)
inline void itcz_finish(const SampleAcc* acc, Spline* splines /* [2] */, float* itczLons, float* itczLatsSummer, float* itczLatsWinter) {
    for (int season = 0; season < 2; ++season) {
        const double sign = season == 0 ? 1 : -1;
        double lons[NUM_LON], lats[NUM_LON], tmp[NUM_LON];
        for (int i = 0; i < NUM_LON; ++i) {
            lons[i] = -PI + (i + 0.5) * (2 * PI / NUM_LON);
            double landSum = 0, elevSum = 0; int samples = 0;
            for (int d = 0; d < NUM_DEG; ++d) {
                const SampleAcc& A = acc[(season * NUM_LON + i) * NUM_DEG + d];
                const double landFrac = A.totalCount == 0 ? 0 : (double)A.landCount / A.totalCount;
                const double avgElev = A.totalCount == 0 ? 0 : A.elevSum / A.totalCount;
                landSum += landFrac; elevSum += avgElev; ++samples;
            }
            const double avgLand = landSum / samples, avgElev = elevSum / samples;
            const double landPull = js_min(1, avgLand * 2);
            const double itczDeg = 5 + landPull * 15 - elev_to_height_km(avgElev) * 1.5;
            const double clampedDeg = js_max(5, js_min(20, itczDeg));
            lats[i] = clampedDeg * sign * DEG;
        }
        for (int pass = 0; pass < 3; ++pass) {
            for (int i = 0; i < NUM_LON; ++i) {
                const int p = (i - 1 + NUM_LON) % NUM_LON, n = (i + 1) % NUM_LON;
                tmp[i] = 0.25 * lats[p] + 0.5 * lats[i] + 0.25 * lats[n];
            }
            for (int i = 0; i < NUM_LON; ++i) lats[i] = tmp[i];
        }
        const double clampMin = (sign > 0 ? 5 : -20) * DEG, clampMax = (sign > 0 ? 20 : -5) * DEG;
        for (int i = 0; i < NUM_LON; ++i) lats[i] = js_max(clampMin, js_min(clampMax, lats[i]));
        build_periodic_spline(lons, lats, splines[season]);
    }
    for (int i = 0; i < ITCZ_SAMPLES; ++i) {
        const double lon = -PI + (i + 0.5) * (2 * PI / ITCZ_SAMPLES);
        itczLons[i] = (float)lon;
        itczLatsSummer[i] = (float)evaluate_spline(splines[0], lon);
        itczLatsWinter[i] = (float)evaluate_spline(splines[1], lon);
    }
}

// ---- continentality (:476-594) ----
inline double avg_edge_km(int32_t N) { return (PI * 6371) / std::sqrt((double)N); }
inline int32_t js_round_passes(double v) { const double r = std::floor(v + 0.5); return r < 1 ? 1 : (int32_t)r; }   // Math.max(1, Math.round(v)), v > 0

// plateIsOcean.has(id): binary search in the ascending list of ocean plate ids
WO_HD inline bool id_in_sorted(const int32_t* ids, int32_t n, int32_t id) {
    int32_t lo = 0, hi = n;
    while (lo < hi) { const int32_t mid = lo + ((hi - lo) >> 1); if (ids[mid] < id) lo = mid + 1; else hi = mid; }
    return lo < n && ids[lo] == id;
}

// union-find hook over the edges (r, nb), nb > r, whose two ends are non-land (:485-503)
WO_IMP_HD inline void cc_hook_ocean_cell(int32_t* parent, const uint8_t* isLand, const int32_t* off, const int32_t* adj, int32_t r) {
    if (isLand[r]) return;
    int32_t a = -1;
    for (int32_t i = off[r]; i < off[r + 1]; ++i) {
        const int32_t nb = adj[i];
        if (nb <= r || isLand[nb]) continue;
        if (a < 0) a = imp::cc_find(parent, r);
        int32_t b = imp::cc_find(parent, nb);
        while (a != b) {
            if (a < b) {
                const int32_t got = imp::cc_cas(parent + b, b, a);
                if (got == b) break;
                b = got;
            } else {
                const int32_t got = imp::cc_cas(parent + a, a, b);
                if (got == a) { a = b; break; }
                a = got;
            }
        }
    }
}
// {size, first cell} of a component as one ordered key: larger size wins, then the smaller first cell
WO_HD inline unsigned long long main_ocean_key(int32_t size, int32_t root) { return ((unsigned long long)(uint32_t)size << 32) | (uint32_t)(0x7fffffff - root); }
WO_HD inline int32_t main_ocean_root(unsigned long long key) { return key == 0 ? -1 : 0x7fffffff - (int32_t)(uint32_t)key; }

// :514-525: a land cell that touches the main ocean
WO_HD inline bool coast_seed_cell(const uint8_t* isLand, const int32_t* label, int32_t mainRoot, const int32_t* off, const int32_t* adj, int32_t r) {
    if (!isLand[r]) return false;
    for (int32_t i = off[r]; i < off[r + 1]; ++i) { const int32_t nb = adj[i]; if (!isLand[nb] && label[nb] == mainRoot) return true; }
    return false;
}
// :563-573: a continental-plate cell that touches an oceanic-plate cell
WO_HD inline bool plate_seed_cell(const uint8_t* plateOcean, const int32_t* off, const int32_t* adj, int32_t r) {
    if (plateOcean[r]) return false;
    for (int32_t i = off[r]; i < off[r + 1]; ++i) if (plateOcean[adj[i]]) return true;
    return false;
}
// :543-547, :587-592 (inside[r]: land with a distance, or continental plate with a distance)
WO_HD inline float continentality_cell(int32_t dist, bool inside, double avgEdgeKm) {
    if (!(inside && dist >= 0)) return 0.0f;
    return (float)smoothstep(0, 2000, dist * avgEdgeKm);
}

// ---- regionPressure (:239-301) ----
WO_HD inline double gauss(double v) { return exp(-0.5 * (v * v)); }
WO_HD inline float region_pressure_cell(float latF, float lonF, const Spline& S, int seasonSign, float contF, float elevF, const uint8_t* P, const uint8_t* M,
                                        float pxF, float pyF, float pzF) {
    const double lat = latF, lon = lonF, landFrac = contF, elevation = elevF;
    const double itczLat = evaluate_spline(S, lon);
    const double latDeg = lat * RAD;
    double p = 1013;
    const double dItcz = (lat - itczLat) * RAD;
    p -= 15 * gauss(dItcz / 8);
    const double shiftDeg = seasonSign * 5;
    const double nhSubHigh = 30 + shiftDeg, shSubHigh = -(30 - shiftDeg);
    const double highIntensity = 12 * (1 - 0.3 * landFrac);
    p += highIntensity * gauss((latDeg - nhSubHigh) / 10);
    p += highIntensity * gauss((latDeg - shSubHigh) / 10);
    p -= 10 * gauss((latDeg - 60) / 10);
    p -= 10 * gauss((latDeg + 60) / 10);
    p += 8 * gauss((latDeg - 85) / 8);
    p += 8 * gauss((latDeg + 85) / 8);
    const double continentalScale = smoothstep(0.2, 0.5, landFrac);
    if (continentalScale > 0.001) {
        const double absLatDeg = fabs(lat) * RAD;
        const double latFactor = absLatDeg < 15 ? 0
            : absLatDeg < 30 ? 0.75 * smoothstep(15, 30, absLatDeg)
            : absLatDeg < 45 ? 0.75 + 0.25 * smoothstep(30, 45, absLatDeg)
            : absLatDeg < 60 ? 1
            : absLatDeg < 90 ? smoothstep(90, 60, absLatDeg)
            : 0;
        const bool summerHemisphere = (seasonSign > 0 && lat > 0) || (seasonSign < 0 && lat < 0);
        if (summerHemisphere) p -= 10 * latFactor * continentalScale;
        else p += 14 * latFactor * continentalScale;
    }
    p -= 3 * elev_to_height_km(js_max(0, elevation));
    const double px = pxF, py = pyF, pz = pzF;
    p += fbm(P, M, px * 2, py * 2, pz * 2, 3) * 2;
    return (float)p;
}

// ---- computeGradients (:306-339) ----
struct Frames { const float *eastX, *eastY, *eastZ, *northX, *northY, *northZ; };
WO_HD inline void gradient_cell(const int32_t* off, const int32_t* adj, const float* xyz, const float* pressure, const Frames& T, float* gradE, float* gradN, int32_t r) {
    const double px = xyz[3 * (int64_t)r], py = xyz[3 * (int64_t)r + 1], pz = xyz[3 * (int64_t)r + 2];
    const double ex = T.eastX[r], ey = T.eastY[r], ez = T.eastZ[r];
    const double nx = T.northX[r], ny = T.northY[r], nz = T.northZ[r];
    const double pHere = pressure[r];
    double sumEP = 0, sumEE = 0, sumNP = 0, sumNN = 0;
    for (int32_t ni = off[r]; ni < off[r + 1]; ++ni) {
        const int64_t nb = adj[ni];
        const double dx = (double)xyz[3 * nb] - px, dy = (double)xyz[3 * nb + 1] - py, dz = (double)xyz[3 * nb + 2] - pz;
        const double de = dx * ex + dy * ey + dz * ez;
        const double dn = dx * nx + dy * ny + dz * nz;
        const double dp = (double)pressure[nb] - pHere;
        sumEP += de * dp; sumEE += de * de; sumNP += dn * dp; sumNN += dn * dn;
    }
    gradE[r] = sumEE > 1e-12 ? (float)(sumEP / sumEE) : 0.0f;
    gradN[r] = sumNN > 1e-12 ? (float)(sumNP / sumNN) : 0.0f;
}

// ---- pressureToWind (:343-378) ----
WO_HD inline void wind_cell(const float* gradE, const float* gradN, const float* sinLatF, float* windE, float* windN, float* speed, int32_t r) {
    const double sin5 = sin(5 * DEG);
    const double pgfE = -(double)gradE[r], pgfN = -(double)gradN[r];
    const double sinLat = sinLatF[r];
    const double absSinLat = fabs(sinLat);
    const double geoAngle = 70 * DEG * smoothstep(0, sin5, absSinLat);
    const double frictionAngle = 20 * DEG;
    const double sign = sinLat >= 0 ? -1 : 1;
    const double totalAngle = sign * (geoAngle - frictionAngle);
    const double cosA = cos(totalAngle), sinA = sin(totalAngle);
    const double we = (pgfE * cosA - pgfN * sinA) * 0.6;
    const double wn = (pgfE * sinA + pgfN * cosA) * 0.6;
    windE[r] = (float)we;
    windN[r] = (float)wn;
    speed[r] = (float)sqrt(we * we + wn * wn);
}

// ---- percentile(speed, 0.95) (js/climate-util.js:103-110): the value at index floor(n * p) of the ascending order, by a
// three-digit histogram select over an order-preserving key (negative values below positive ones, NaN above everything) ----
constexpr int SEL_PASSES = 3, SEL_BINS = 2048;
WO_HD inline uint32_t sel_key(float f) { union { float f; uint32_t u; } v; v.f = f; return (v.u & 0x80000000u) ? ~v.u : (v.u | 0x80000000u); }
WO_HD inline float sel_value(uint32_t k) { union { float f; uint32_t u; } v; v.u = (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k; return v.f; }
WO_HD inline int sel_shift(int pass) { return pass == 0 ? 21 : pass == 1 ? 10 : 0; }
WO_HD inline uint32_t sel_digit(uint32_t key, int pass) { return pass == 0 ? key >> 21 : pass == 1 ? (key >> 10) & 2047u : key & 1023u; }
// does key agree with the digits chosen in the earlier passes?
WO_HD inline bool sel_matches(uint32_t key, uint32_t prefix, int pass) { return pass == 0 || (key >> sel_shift(pass - 1)) == (prefix >> sel_shift(pass - 1)); }
struct SelState { uint32_t prefix; uint32_t k; };            // digits chosen so far (in place), rank still to skip inside them
// after a pass's histogram: pick its digit
WO_HD inline void sel_pick(SelState& S, const uint32_t* hist, int pass) {
    const int bins = pass == 2 ? 1024 : SEL_BINS;
    uint32_t k = S.k;
    int d = 0;
    for (; d < bins - 1; ++d) { if (k < hist[d]) break; k -= hist[d]; }
    S.prefix |= (uint32_t)d << sel_shift(pass);
    S.k = k;
}
inline uint32_t percentile_index(int32_t n, double p) { return (uint32_t)std::floor((double)n * p); }
// `work[k] || 1`
WO_HD inline float max_speed_of(uint32_t key) { const float v = sel_value(key); return (v != v || v == 0.0f) ? 1.0f : v; }

// :637-639, :644-646
WO_HD inline float normalise_speed_cell(float speed, float maxSpeed) { return (float)js_min(1, (double)speed / (double)maxSpeed); }
WO_HD inline float pressure_dev_cell(float pressure) { return (float)((double)pressure - 1013); }

}  // namespace wind
}  // namespace wo
