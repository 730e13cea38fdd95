// Ocean surface currents (js/ocean.js:204-382): per-cell bodies shared by the device kernels (ocean.hip) and the test-only
// CPU emulator (tests/emu_ocean), so that both compile the very same arithmetic.  One body per loop of the reference.
//
// Contract (the bar is bit equality on all eight outputs; the stage calls no libm function except sqrt):
//   * f32 rounding at every store.  Every store into one of the reference's Float32Arrays rounds to f32 and the next read
//     sees the rounded value.  `currentE[r] = baseE`, the two `currentE[r] *= ...` and the circumpolar blend are four
//     separate roundings; `currentN[r] += ...` and `-= ...` each read the f32 back.  The bodies replay them one by one in
//     double with a (float) at each store.  The library compiles with -ffp-contract=off.
//   * Sums are double, in adjacency order.  landDir* is a double sum of (double)xyz[nb] - (double)xyz[r]; the masked
//     smooth adds (double)field[nb] over the ocean neighbours in row order and divides by the integer count in double.
//   * Divisions stay divisions: lat / DEG with DEG = pi / 180 in double, wDist / coastThreshold in double.  Nothing is
//     multiplied by a reciprocal.
//   * JS semantics: % on doubles is fmod; Math.round is floor(x + 0.5) (wind_ops.h: js_round_passes); percentile(arr, 0.95)
//     is the element at index floor(n * 0.95) of the ascending ocean speeds that are > 0, and 1 when that element is 0
//     (or NaN) or when n == 0.
//   * smoothstep is wind_ops.h's (the reference imports it from js/wind.js).
//   * Order-free parts: the two hop-distance fields (any level-synchronous BFS gives the reference's FIFO distances; the
//     order of the seed list does not matter).  Distances are only compared with coastThreshold and with
//     warmthRange = 2 * coastThreshold, so a field built to depth warmthRange - 1 with -1 beyond it gives the same
//     outputs as the complete one (tests/test_ocean.py holds the emulator to that).  r_coastDist of the reference is
//     never read and is not built.
#pragma once
#include <cstdint>
#include <cmath>

#include "wind_ops.h"

namespace wo {
namespace ocean {

namespace W = wo::wind;

constexpr int CIRC_BINS = 72;                                 // hasCircumpolarChannel: NUM_BINS
constexpr int SEED_NONE = 0, SEED_WEST = 1, SEED_EAST = 2;
constexpr int FIELD_SHIFT = 30;                               // a frontier entry: (field << 30) | cell, cells < 2^30
constexpr int32_t CELL_MASK = (1 << FIELD_SHIFT) - 1;

// K fields of one cell side by side, so that a neighbour's group is one 4 * K byte load
template <int K> struct alignas(4 * K) Group { float v[K]; };

// the scalars of a call (:207, :247-249, :338, :354)
struct Params { int32_t coastThreshold, warmthRange, currentPasses, warmthPasses; };
inline Params params_for(int32_t N) {
    Params P;
    const double t = std::floor(std::sqrt((double)N) * 0.035 + 0.5);
    P.coastThreshold = t < 5 ? 5 : (int32_t)t;
    P.warmthRange = P.coastThreshold * 2;
    const double avgEdgeKm = W::avg_edge_km(N);
    P.currentPasses = W::js_round_passes(125 / avgEdgeKm) < 2 ? 2 : W::js_round_passes(125 / avgEdgeKm);
    P.warmthPasses = W::js_round_passes(900 / avgEdgeKm) < 3 ? 3 : W::js_round_passes(900 / avgEdgeKm);
    return P;
}

// ---- the coast seed test with the west / east split (:21-55) ----
WO_HD inline int coast_seed_cell(const uint8_t* isOcean, const int32_t* off, const int32_t* adj, const float* xyz, const float* eastX, const float* eastY,
                                 const float* eastZ, int32_t r) {
    if (!isOcean[r]) return SEED_NONE;
    double landDirX = 0, landDirY = 0, landDirZ = 0;
    bool hasLandNeighbor = false;
    const double px = xyz[3 * (int64_t)r], py = xyz[3 * (int64_t)r + 1], pz = xyz[3 * (int64_t)r + 2];
    for (int32_t ni = off[r]; ni < off[r + 1]; ++ni) {
        const int64_t nb = adj[ni];
        if (!isOcean[nb]) {
            hasLandNeighbor = true;
            landDirX += (double)xyz[3 * nb] - px;
            landDirY += (double)xyz[3 * nb + 1] - py;
            landDirZ += (double)xyz[3 * nb + 2] - pz;
        }
    }
    if (!hasLandNeighbor) return SEED_NONE;
    const double normalE = landDirX * (double)eastX[r] + landDirY * (double)eastY[r] + landDirZ * (double)eastZ[r];
    if (normalE < -0.2) return SEED_WEST;
    if (normalE > 0.2) return SEED_EAST;
    return normalE <= 0 ? SEED_WEST : SEED_EAST;
}

// ---- the circumpolar bin of a cell (:97-104): 0 .. 71 in the northern band, 72 .. 143 in the southern one, -1 in neither ----
WO_HD inline int32_t circumpolar_bin(bool isOcean, float latF, float lonF) {
    if (!isOcean) return -1;
    const double lat = latF;
    int32_t half;
    if (!(lat < 60 * W::DEG - 5 * W::DEG || lat > 60 * W::DEG + 5 * W::DEG)) half = 0;
    else if (!(lat < -60 * W::DEG - 5 * W::DEG || lat > -60 * W::DEG + 5 * W::DEG)) half = 1;
    else return -1;
    double bin = floor((((double)lonF + W::PI) / (2 * W::PI)) * CIRC_BINS);
    bin = fmod(fmod(bin, (double)CIRC_BINS) + CIRC_BINS, (double)CIRC_BINS);
    if (!(bin >= 0 && bin < CIRC_BINS)) return -1;            // NaN: the reference's store to binHasOcean[NaN] does nothing
    return half * CIRC_BINS + (int32_t)bin;
}

// ---- makeItczLookup (js/climate-util.js:29-42) over the 360 stored latitudes ----
WO_HD inline double itcz_lookup(const float* itczLats, double lon) {
    const int n = W::ITCZ_SAMPLES;
    const double step = (2 * W::PI) / n;
    const double lonStart = -W::PI + step * 0.5;
    double fi = (lon - lonStart) / step;
    fi = fmod(fmod(fi, (double)n) + n, (double)n);
    if (!(fi >= 0 && fi < n)) return fi - fi;                 // only a NaN gets here (fmod of a NaN or infinite longitude): itczLats[NaN] is undefined, the sum NaN
    const int i0 = (int)floor(fi);
    const int i1 = (i0 + 1) % n;
    const double frac = fi - i0;
    return (double)itczLats[i0] * (1 - frac) + (double)itczLats[i1] * frac;
}

// ---- the band and deflection body of steps 3-4 (:266-333) for one season; land cells hold 0 and are not passed here ----
WO_HD inline void current_cell(float latF, float lonF, int32_t wDist, int32_t eDist, int32_t coastThreshold, bool circumpolarNH, bool circumpolarSH,
                               double seasonalShiftDeg, const float* itczLats, float& outE, float& outN) {
    const double lat = latF;
    const double absLatDeg = fabs(lat) / W::DEG;
    const double lon = lonF;
    const double hemisphereSign = lat >= 0 ? 1 : -1;
    const double bandLatDeg = fabs(lat / W::DEG - seasonalShiftDeg);
    const double itczLat = itcz_lookup(itczLats, lon);
    const double distFromItcz = fabs(lat - itczLat) / W::DEG;
    double baseE;
    if (distFromItcz < 3) baseE = 1 - 2 * W::smoothstep(0, 3, distFromItcz);
    else if (bandLatDeg < 30) baseE = -1;
    else if (bandLatDeg < 35) baseE = -1 + 2 * W::smoothstep(30, 35, bandLatDeg);
    else if (bandLatDeg < 58) baseE = 1;
    else if (bandLatDeg < 65) baseE = 1 - 1.5 * W::smoothstep(58, 65, bandLatDeg);
    else baseE = -0.5;
    float currentE = (float)baseE;
    float currentN = 0.0f;
    if (wDist >= 0 && wDist < coastThreshold) {
        const double t = 1 - (double)wDist / (double)coastThreshold;
        const double strength = t * t * 2.0;
        currentN = (float)((double)currentN + hemisphereSign * strength);
        currentE = (float)((double)currentE * (1 - t * t * 0.7));
    }
    if (eDist >= 0 && eDist < coastThreshold) {
        const double t = 1 - (double)eDist / (double)coastThreshold;
        const double strength = t * t * 0.8;
        currentN = (float)((double)currentN - hemisphereSign * strength);
        currentE = (float)((double)currentE * (1 - t * t * 0.5));
    }
    const bool isCircumpolar = (lat > 0 && circumpolarNH) || (lat < 0 && circumpolarSH);
    if (isCircumpolar && absLatDeg >= 55 && absLatDeg <= 75) {
        const double cStrength = 1 - fabs(absLatDeg - 65) / 10;
        currentE = (float)((double)currentE * (1 - cStrength) + 1.5 * cStrength);
        currentN = (float)((double)currentN * (1 - cStrength * 0.8));
    }
    outE = currentE;
    outN = currentN;
}

// ---- classifyWarmth (:120-164) for one ocean cell ----
WO_HD inline float warmth_cell(float latF, int32_t wDist, int32_t eDist, int32_t fadeRange, double seasonalShiftDeg) {
    const double bandLatDeg = fabs((double)latF / W::DEG - seasonalShiftDeg);
    double cellSign;
    if (bandLatDeg < 28) cellSign = 1;
    else if (bandLatDeg < 35) cellSign = 1 - 2 * W::smoothstep(28, 35, bandLatDeg);
    else if (bandLatDeg < 55) cellSign = -1;
    else if (bandLatDeg < 65) cellSign = -1 + 2 * W::smoothstep(55, 65, bandLatDeg);
    else cellSign = 1;
    double warm = 0;
    if (wDist >= 0 && wDist < fadeRange) {
        const double t = 1 - (double)wDist / (double)fadeRange;
        warm += cellSign * t * t;
    }
    if (eDist >= 0 && eDist < fadeRange) {
        const double t = 1 - (double)eDist / (double)fadeRange;
        warm -= cellSign * t * t;
    }
    return (float)W::js_max(-1, W::js_min(1, warm));
}

// ---- the masked smooth (:173-186) on K fields of a cell at once: land copies through, an ocean cell averages itself and
// its ocean neighbours (each field its own double sum in row order, one shared count) ----
template <int K>
WO_HD inline Group<K> smooth_ocean_cell(const int32_t* off, const int32_t* adj, const uint8_t* isOcean, const Group<K>* field, int32_t r) {
    const Group<K> self = field[r];
    if (!isOcean[r]) return self;
    double sum[K];
    for (int k = 0; k < K; ++k) sum[k] = self.v[k];
    int32_t count = 1;
    for (int32_t ni = off[r]; ni < off[r + 1]; ++ni) {
        const int32_t nb = adj[ni];
        if (isOcean[nb]) {
            const Group<K> g = field[nb];
            for (int k = 0; k < K; ++k) sum[k] += (double)g.v[k];
            ++count;
        }
    }
    Group<K> out;
    for (int k = 0; k < K; ++k) out.v[k] = (float)(sum[k] / count);
    return out;
}

// ---- the speed and its normalisation (:358-369) ----
WO_HD inline double speed_of(float currentE, float currentN) { return sqrt((double)currentE * (double)currentE + (double)currentN * (double)currentN); }
// does the cell enter oceanSpeeds?  (spd > 0 on the double; its f32 store is > 0 as well: spd is at least the larger
// component's magnitude, an f32)
WO_HD inline bool speed_counts(bool isOcean, double spd) { return isOcean && spd > 0; }
WO_HD inline uint32_t percentile_rank(uint32_t n) { return (uint32_t)floor((double)n * 0.95); }
// percentile(oceanSpeeds, 0.95) from the selected key: `n === 0` gives 1, `work[k] || 1` otherwise
WO_HD inline float p95_of(uint32_t n, uint32_t key) { return n == 0 ? 1.0f : W::max_speed_of(key); }
// Math.min(1, r_speed[r] / p95): wind_ops.h's normalise_speed_cell

}  // namespace ocean
}  // namespace wo
