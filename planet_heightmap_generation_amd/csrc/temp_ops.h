// Seasonal temperature (js/temperature.js:69-237) and the Koppen classification (js/koppen.js:67-288): per-cell bodies shared by
// the device kernels (temp.hip) and the test-only CPU emulator (tests/emu_temperature), so that both compile the very same
// arithmetic.  One body per loop of the reference.
//
// Contract of computeTemperature (the bar is a per-cell bound, not bit equality: the per-cell code calls libm):
//   * Double arithmetic on f32 loads, in the reference's operation order.  Every store into one of the reference's Float32Arrays
//     rounds to f32 once and the next read sees the rounded value: coastal / tmp of diffuseOceanWarmth (after every pass), temp
//     after the per-cell loop, temp after the smoothField pass (the mean is rounded BEFORE the normalisation reads it), temp
//     after the normalisation.  The library compiles with -ffp-contract=off.
//   * Sums are double, in adjacency order.  Divisions stay divisions (lat / DEG, x / maxDist, sum / count, (t + 45) / 90).
//   * pow(t, 1.4) of the three curves is the platform's: ocml on the device, glibc in the emulator, V8's in the reference.  It is
//     called UNQUALIFIED so that the emulator's second build can route it through tests/emu/libm_perturb.h; the bound that
//     follows from it is derived in tests/test_temperature_libm.py.  Nothing else of the stage calls libm.
//   * tAnn and T_annual (:189-191) do not depend on the season: annual_curve is computed once per cell and handed to both
//     seasons, which is what the reference computes twice from identical operands.
//   * Reuse: smoothstep, js_max / js_min, elev_to_height_km, avg_edge_km and js_round_passes are wind_ops.h's, the ITCZ lookup is
//     ocean_ops.h's itcz_lookup (makeItczLookup), smoothField is erode_ops.h's smooth_field_cell, the warmth seed and the
//     single-field pass are climate_ops.h's warmth_seed_cell / warmth_diffuse_cell.  The emulator runs diffuseOceanWarmth season
//     by season with those; warmth_diffuse_pair_cell below is the same pass on both seasons of a cell at once (each season its own
//     double sum and its own sum / count, the neighbours in the same order), so both give the same bits.
//   * oceanWarmthPasses = max(4, Math.round(1400 / avgEdgeKm)) comes from warmth_passes(N) on the host: 4 at 64 cells, 7 at
//     10 001, 70 at 1 000 001.
//   * Out of contract: the reference's null-tolerant branches (a missing r_precip, r_oceanWarmth, r_oceanSpeed or
//     r_plateContinentality: the entry point refuses instead) and NaN inputs.
//
// Contract of classifyKoppen: class equality on every cell given the same inputs.  No libm; the multiplications, the divisions
// (/ 6, / 2, / 10, 2 / 6) and the comparisons are double, in the reference's order.  The reference builds its C and D codes as
// strings ('C' + pattern + letter) and looks them up; here koppen_c / koppen_d give the ids.  All nine C codes exist and letter
// 'd' needs Tcold < -38 while band C has Tcold >= 0, and all twelve D codes exist: the reference's two fallbacks ('Cfb', 'Df' +
// letter) are unreachable and are not coded.
#pragma once
#include <cstdint>
#include <cmath>

#include "climate_ops.h"
#include "erode_ops.h"
#include "ocean_ops.h"
#include "wind_ops.h"

namespace wo {
namespace temp {

namespace W = wo::wind;
namespace O = wo::ocean;

using G2 = O::Group<2>;                                       // summer, winter of one cell

constexpr double T_MIN = -45, T_MAX = 45, T_RANGE = T_MAX - T_MIN;
constexpr int32_t SMOOTH_PASSES = 1;                          // js/temperature.js:76

// js/temperature.js:100-101
inline int32_t warmth_passes(int32_t N) { const int32_t r = W::js_round_passes(1400 / W::avg_edge_km(N)); return r < 4 ? 4 : r; }

// branch census (tests/test_temperature.py, tests/test_koppen.py): the emulator counts, the device does not
enum Branch : int {
    B_OCEAN = 0, B_COAST_WARM, B_COAST_NONE, B_INLAND,        // ocean / land with |cw| > 0.001 / land with |cw| <= 0.001 the diffusion reaches / land with plateCont >= 0.95
    B_P_HIGH, B_P_LOW, B_P_MID, B_LAPSE, B_NO_LAPSE, B_LOCAL_SUMMER, B_LOCAL_WINTER,
    K_FRAC_HIGH, K_FRAC_LOW, K_FRAC_MID, K_DESERT, K_STEPPE, K_PATTERN_S, K_PATTERN_W, K_PATTERN_F, K_LETTER_A, K_LETTER_B, K_LETTER_C, K_LETTER_D,
    B_COUNT
};
struct NoCensus { WO_HD void hit(int) const {} };

// ---- diffuseOceanWarmth (:19-54), one pass on both seasons of cell r ----
WO_HD inline G2 warmth_diffuse_pair_cell(const int32_t* off, const int32_t* adj, const G2* coastal, const float* r_plateContinentality, int32_t r) {
    const G2 self = coastal[r];
    if ((double)r_plateContinentality[r] >= 0.95) return self;
    double sumS = self.v[0], sumW = self.v[1];
    int32_t count = 1;
    for (int32_t ni = off[r]; ni < off[r + 1]; ++ni) {
        const G2 g = coastal[adj[ni]];
        sumS += (double)g.v[0]; sumW += (double)g.v[1];
        ++count;
    }
    return G2{{(float)(sumS / count), (float)(sumW / count)}};
}

// ---- the curve 28 - 47 * pow(max(0, distDeg - 13) / 77, 1.4) of :121-134 and :189-191 ----
WO_HD inline double zonal_curve(double distDeg) {
    const double tropicalHW = 13;
    const double maxDist = 90 - tropicalHW;
    const double t = W::js_max(0, distDeg - tropicalHW) / maxDist;
    return 28 - 47 * pow(t, 1.4);
}
// T_annual of :189-191: the same for both seasons of a cell
WO_HD inline double annual_curve(float latF) { return zonal_curve(fabs((double)latF) / W::DEG); }

struct CellIn {
    float lat, lon, elev, cont, plateCont;
    bool land;
};

// ---- the per-cell loop (:106-212) for one season ----
template <class C>
WO_HD inline float temperature_cell(const CellIn& I, bool summer, const float* itczLats, float precip, float oceanWarmth, float oceanSpeed, float coastalWarmth,
                                    double T_annual, double temperatureOffset, const C& census) {
    const double lat = I.lat, lon = I.lon;
    const double elev = I.elev, cont = I.cont, pCont = I.plateCont;
    // 1. base temperature from the thermal equator
    const double itczLat = O::itcz_lookup(itczLats, lon);
    const double distItcz = fabs(lat - itczLat) / W::DEG;
    const double T_itcz = zonal_curve(distItcz);
    const double flatItczLat = (summer ? 5 : -5) * W::DEG;
    const double distFlat = fabs(lat - flatItczLat) / W::DEG;
    const double T_flat = zonal_curve(distFlat);
    const double absLatDeg = fabs(lat) / W::DEG;
    const double blend = W::smoothstep(45, 90, absLatDeg);
    double T = T_itcz * (1 - blend) + T_flat * blend;
    // 2. elevation lapse rate
    const double moisture = precip;
    const double lapse = 4.5 + 4.8 * (1 - moisture);
    const bool lapsed = I.land && elev > 0;
    census.hit(lapsed ? B_LAPSE : B_NO_LAPSE);
    if (lapsed) T -= lapse * W::elev_to_height_km(elev);
    // 5. ocean current influence
    if (!I.land) {
        census.hit(B_OCEAN);
        const double warmth = oceanWarmth, speed = oceanSpeed;
        T += warmth * W::js_min(1, speed * 2) * 16;
    } else {
        const double cw = coastalWarmth;
        if (fabs(cw) > 0.001) {
            census.hit(B_COAST_WARM);
            T += cw * (1 - W::smoothstep(0, 0.95, pCont)) * 20;
        } else census.hit(pCont >= 0.95 ? B_INLAND : B_COAST_NONE);
    }
    // 6. cloud cover moderation
    const double p = precip;
    if (p > 0.5) {
        census.hit(B_P_HIGH);
        const double mod = W::smoothstep(0.5, 1.0, p) * 0.15;
        T *= (1 - mod);
    } else if (p < 0.3) {
        census.hit(B_P_LOW);
        const double amp = W::smoothstep(0.3, 0.0, p) * 0.15;
        T *= (1 + amp);
    } else census.hit(B_P_MID);
    // 7. maritime / continental moderation
    const double distAnn = absLatDeg;
    const double T_ann_adj = lapsed ? T_annual - lapse * W::elev_to_height_km(elev) : T_annual;
    const double deviation = T - T_ann_adj;
    const double seasonalBoost = 12 * W::smoothstep(10, 55, distAnn) * (1 - W::smoothstep(75, 90, distAnn));
    const bool isLocalSummer = summer ? (lat >= 0) : (lat < 0);
    census.hit(isLocalSummer ? B_LOCAL_SUMMER : B_LOCAL_WINTER);
    const double seasonSign = isLocalSummer ? 1 : -1;
    const double boostedDeviation = deviation + seasonSign * seasonalBoost;
    const double maritimeFactor = 0.50 + cont * 0.70;
    T = T_ann_adj + boostedDeviation * maritimeFactor;
    T += temperatureOffset;
    return (float)T;
}

// ---- the smoothField pass (:218) with the normalisation (:223-225) at its store ----
WO_HD inline float normalise_cell(float t) { return (float)W::js_max(0, W::js_min(1, ((double)t - T_MIN) / T_RANGE)); }
WO_HD inline float smooth_normalise_cell(const Fields& F, const float* src, int32_t r) { return normalise_cell(smooth_field_cell(F, src, r)); }

// ---- classifyKoppen (js/koppen.js:76-285): the ids are the indices of KOPPEN_CLASSES (:19-51) ----
constexpr int KOPPEN_CLASSES = 31;
enum Koppen : uint8_t { K_OCEAN = 0, K_AF = 1, K_AM = 2, K_AW = 3, K_BWH = 4, K_BWK = 5, K_BSH = 6, K_BSK = 7, K_ET = 29, K_EF = 30 };
// pattern f, s, w by letter a, b, c(, d)
WO_HD inline uint8_t koppen_c(int pattern, int letter) { return (uint8_t)(8 + 3 * pattern + letter); }      // Cfa 8 .. Cfc 10, Csa 11 .. Csc 13, Cwa 14 .. Cwc 16
WO_HD inline uint8_t koppen_d(int pattern, int letter) { return (uint8_t)(17 + 4 * pattern + letter); }     // Dfa 17 .. Dfd 20, Dsa 21 .. Dsd 24, Dwa 25 .. Dwd 28

template <class C>
WO_HD inline uint8_t koppen_cell(float elevation, float tSummer, float tWinter, float pSummer, float pWinter, const C& census) {
    if (elevation <= 0) return K_OCEAN;
    const double Ts = -45 + W::js_max(0, W::js_min(1, (double)tSummer)) * 90;
    const double Tw = -45 + W::js_max(0, W::js_min(1, (double)tWinter)) * 90;
    const double Thot = W::js_max(Ts, Tw);
    const double Tcold = W::js_min(Ts, Tw);
    const double Tann = (Ts + Tw) / 2;
    const double Tshoulder = Thot - (Thot - Tcold) * (2.0 / 6);
    const bool localSummerIsSim = Ts >= Tw;
    const double Ps = W::js_max(0, (double)pSummer) * 1000;
    const double Pw = W::js_max(0, (double)pWinter) * 1000;
    const double Pann = Ps + Pw;
    const double PsummerLocal = localSummerIsSim ? Ps : Pw;
    const double PwinterLocal = localSummerIsSim ? Pw : Ps;
    const double PsMonthLocal = PsummerLocal / 6;
    const double PwMonthLocal = PwinterLocal / 6;
    const double Pdry = W::js_min(PsMonthLocal, PwMonthLocal);
    // step 1: temperature bands
    if (Thot < 0) return K_EF;
    if (Thot < 10) return K_ET;
    const int band = Tcold >= 18 ? 0 : (Tcold >= 0 ? 1 : 2);      // A, C, D
    // step 2: arid zones
    double Pthresh;
    const double summerFrac = Pann > 0 ? PsummerLocal / Pann : 0.5;
    if (summerFrac >= 0.7) { census.hit(K_FRAC_HIGH); Pthresh = 20 * Tann + 280; }
    else if (summerFrac <= 0.3) { census.hit(K_FRAC_LOW); Pthresh = 20 * Tann; }
    else { census.hit(K_FRAC_MID); Pthresh = 20 * Tann + 140; }
    Pthresh = W::js_max(0, Pthresh);
    if (Pann < Pthresh) {
        const bool isHot = Tann >= 18;
        if (Pann < Pthresh * 0.5) { census.hit(K_DESERT); return isHot ? K_BWH : K_BWK; }
        census.hit(K_STEPPE);
        return isHot ? K_BSH : K_BSK;
    }
    // step 3: precipitation pattern and temperature letter
    int pattern;                                              // 0 f, 1 s, 2 w
    const bool localSummerDrier = PsummerLocal < PwinterLocal;
    if (localSummerDrier && PsMonthLocal < 50 && PsMonthLocal < PwMonthLocal / 2) { census.hit(K_PATTERN_S); pattern = 1; }
    else if (!localSummerDrier && PwMonthLocal < PsMonthLocal / 10) { census.hit(K_PATTERN_W); pattern = 2; }
    else { census.hit(K_PATTERN_F); pattern = 0; }
    int letter;
    if (Thot >= 22) { census.hit(K_LETTER_A); letter = 0; }
    else if (Tshoulder >= 10) { census.hit(K_LETTER_B); letter = 1; }
    else if (Tcold >= -38) { census.hit(K_LETTER_C); letter = 2; }
    else { census.hit(K_LETTER_D); letter = 3; }
    if (band == 0) {
        if (Pdry >= 60) return K_AF;
        if (Pann >= 25 * (100 - Pdry)) return K_AM;
        return K_AW;
    }
    return band == 1 ? koppen_c(pattern, letter) : koppen_d(pattern, letter);
}

}  // namespace temp
}  // namespace wo
