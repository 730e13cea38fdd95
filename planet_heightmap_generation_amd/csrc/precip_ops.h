// Seasonal precipitation (js/precipitation.js:196-684, js/heuristic-precip.js): per-cell bodies shared by the device kernels
// (precip.hip) and the test-only CPU emulator (tests/emu_precip), so that both compile the very same arithmetic.  One body per
// loop of the reference.
//
// Contract (the bar is bit equality on all four outputs; no per-cell code of the stage calls libm):
//   * Double arithmetic on f32 loads, f32 rounding at every store.  Every store into one of the reference's Float32Arrays
//     rounds to f32 and the next read sees the rounded value: r_elevSmoothed after the 0.6 / 0.4 blend, r_heightKm, hWindE/N,
//     r_windE/N, r_wind3dX/Y/Z, r_convergence, moisture, precip (after the mechanisms loop, after step 2c, after every smoothing
//     pass), rainShadow, upWt / dnWt, shadowField / windwardField, src / dst of both propagations, r_westCoast / wcTmp, the
//     heuristic precip and blended (after the blend, after the normalisation, after the cap: three roundings).  The library
//     compiles with -ffp-contract=off.
//   * Sums are double, in adjacency order.  Divisions stay divisions (lat / DEG, sum / weight, blended / maxPrecip).
//   * JS semantics: % on doubles is fmod, Math.round is floor(x + 0.5) (wind_ops.h: js_round_passes), Math.max / Math.min are
//     climate_ops.h's cl_max / cl_min; Math.max(0, x) where a -0 could reach a store is max0 below (+0, as in JS).
//   * Reuse: smoothstep, js_round_passes, avg_edge_km, elev_to_height_km and the selection keys are wind_ops.h's, the ITCZ lookup
//     is ocean_ops.h's itcz_lookup (makeItczLookup), wind_convergence_cell / moisture_seed_cell / moisture_advect_cell are
//     climate_ops.h's, smoothField is erode_ops.h's smooth_field_cell, computeGradients is wind_ops.h's gradient_cell.
//   * Wind-aligned neighbour lists (:520-547) are kept ROW-SHAPED: one f32 weight per adjacency entry and list, in row order,
//     0 where the entry is no member (upDot > 0 / dnDot > 0 decided in double; ocean rows hold 0 throughout).  A member's weight
//     is that double rounded to f32.  The propagation bodies take an entry only when `weight > 0`, so an excluded entry adds
//     nothing to either sum.  A member whose positive double rounds to the f32 0 is skipped as well; in the reference it adds
//     val * 0 = -+0 to a sum that starts at +0 and 0 to the weight, which changes neither (x + -0 = x, +0 + -0 = +0 in
//     round-to-nearest).  The members that remain are visited in row order, which is the order of the compacted lists.  So both
//     forms give the same bits; tests/test_precip.py runs the compacted form as a second route of the emulator against this one.
//     dnDot is -(sum) of a double sum, not a sum of negated terms (the two round alike here, but the form is the reference's).
//   * Propagations (:549-601) gather only val < 0 (shadow) or val > 0 (windward); carried = (sum / weight) * (1 - decay); the
//     store is min(src, carried) / max(src, carried); after the last pass the fold into shadowField / windwardField uses < / >;
//     the merge is shadowField < 0 ? shadowField : windwardField.  Both start from the same seeded rainShadow.
//   * r_coastDistLand = -1 (land the main ocean never reaches): monsoon relief takes maxHops (`>= 0 ? d : maxHops`), the polar
//     front takes maxHops (`< 0 ? maxHops : d`), lee cyclogenesis is off (`>= 0 && < leeCoastHops`), the distance cut-off is
//     off (`> 0`); the moisture seed and the west-coast seed test `!== 0` / `=== 0`.
//   * Percentile.  blended = (float)(0.5 * complex + 0.5 * heur) is non-negative and NaN-free for finite inputs: complex is a
//     smoothed max(0, .) (step 2c multiplies by a factor >= 0.02 or adds rs * 1.2 with rs > 0.01), heur a smoothed max(0.05, .).
//     So its order-preserving key (wind_ops.h: sel_key) orders the values as the numbers do, -0 cannot occur, and the radix
//     select over the raw bits returns what Floyd-Rivest leaves at index floor(N * 0.95).  NaN inputs are out of contract.
//   * Scalars of a call come from params_for(N) on the host.  Three of them are 1 - pow(b, 1 / hops) from the host libm
//     against V8's Math.pow.  tests/golden/precip_pow_v8.npz holds V8's values for hops 1 .. 1024 (0.15, 0.25) and 1 .. 200
//     (0.78); tests/test_precip.py compares the host's with them.  glibc 2.35 differs from V8, by one ulp each time, at
//       pow(0.15, 1/h): h = 5, 18, 420 (shadowHops; 5 is below its floor of 8)
//       pow(0.25, 1/h): h = 4, 8, 40, 83, 321, 431, 979 (windwardHops; 4 is below its floor of 6)
//       pow(0.78, 1/h): h = 27, 98, 169 (maxHops; all above its cap of 20, so depletionBase is always V8's)
//     (the lists POW_DIFF_* below; the test holds them to the fixture).  At a planet size whose shadowHops or windwardHops is in
//     its list the two rain-shadow outputs, and through step 2c the two precipitation outputs, are exact only up to that
//     scalar; precip_pow_differs tells.  shadowHops = round(2500 / avgEdgeKm), windwardHops = round(1500 / avgEdgeKm).
#pragma once
#include <cstdint>
#include <cmath>

#include "climate_ops.h"
#include "ocean_ops.h"
#include "wind_ops.h"

namespace wo {
namespace precip {

namespace W = wo::wind;
namespace O = wo::ocean;

// the scalars of a call (:208-210, :221, :291, :454, :550-551, :577-578, :609, :632; heuristic-precip.js:152)
struct Params {
    int32_t maxHops, elevSmoothPasses, convSmoothPasses, shadowHops, windwardHops, rsSmoothPasses, precipSmoothPasses, wcPasses, leeCoastHops;
    double depletionBase, shadowDecay, windwardDecay, avgEdgeKm, avgEdgeRad;
};
inline int32_t round_at_least(double v, int32_t lo) { const double r = std::floor(v + 0.5); return r < lo ? lo : (int32_t)r; }
inline Params params_for(int32_t N) {
    Params P;
    P.avgEdgeKm = W::avg_edge_km(N);
    P.avgEdgeRad = W::PI / std::sqrt((double)N);
    const int32_t h = round_at_least(2000 / P.avgEdgeKm, 8);
    P.maxHops = h > 20 ? 20 : h;
    P.elevSmoothPasses = round_at_least(200 / P.avgEdgeKm, 2);
    P.convSmoothPasses = round_at_least(400 / P.avgEdgeKm, 3);
    P.shadowHops = round_at_least(2500 / P.avgEdgeKm, 8);
    P.windwardHops = round_at_least(1500 / P.avgEdgeKm, 6);
    P.rsSmoothPasses = round_at_least(150 / P.avgEdgeKm, 2);
    P.precipSmoothPasses = round_at_least(100 / P.avgEdgeKm, 1);
    P.wcPasses = round_at_least(300 / P.avgEdgeKm, 2);
    P.leeCoastHops = round_at_least(200 / P.avgEdgeKm, 2);
    P.depletionBase = 1 - std::pow(0.78, 1.0 / P.maxHops);
    P.shadowDecay = 1 - std::pow(0.15, 1.0 / P.shadowHops);
    P.windwardDecay = 1 - std::pow(0.25, 1.0 / P.windwardHops);
    return P;
}
// hop counts at which glibc's pow differs from V8's Math.pow (tests/test_precip.py: test_pow_fixture holds these lists to the
// fixture); -1 ends a list
constexpr int32_t POW_DIFF_015[] = {5, 18, 420, -1};
constexpr int32_t POW_DIFF_025[] = {4, 8, 40, 83, 321, 431, 979, -1};
constexpr int32_t POW_DIFF_078[] = {27, 98, 169, -1};
inline bool precip_pow_differs(const Params& P) {
    for (const int32_t* q = POW_DIFF_015; *q >= 0; ++q) if (*q == P.shadowHops) return true;
    for (const int32_t* q = POW_DIFF_025; *q >= 0; ++q) if (*q == P.windwardHops) return true;
    for (const int32_t* q = POW_DIFF_078; *q >= 0; ++q) if (*q == P.maxHops) return true;
    return false;
}

// Math.max(0, x) with JS's zero: -0 gives +0
WO_HD inline double max0(double x) { return x > 0 ? x : (x != x ? x : 0.0); }

// branch census (tests/test_precip.py): the emulator counts, the device does not
enum Branch : int {
    B_ITCZ_IN = 0, B_ITCZ_OUT, B_ITCZ_CORE, B_CONV_POS, B_CONV_NOT, B_ORO_WINDWARD, B_ORO_LEEWARD, B_ORO_NONE, B_LOCAL_SUMMER, B_LOCAL_WINTER,
    B_MONSOON_RELIEF, B_MONSOON_NONE, B_MONSOON_NO_COAST, B_LATBAND_IN, B_LATBAND_OUT, B_PRESS_HIGH, B_PRESS_LOW, B_SUPPRESS_POS, B_SUPPRESS_NOT,
    B_POLAR_IN, B_POLAR_OUT, B_POLAR_NO_COAST, B_CONT_DRY, B_CONT_NOT, B_LEE_HIGH, B_LEE_CYCLO, B_LEE_NOT, B_OCEAN_CELL, B_CUT_NEAR, B_CUT_FAR, B_CUT_NONE,
    B_SEED_WINDWARD, B_SEED_SHADOW, B_SEED_LOW, B_SEED_ZERO,
    B_ZONAL0, B_ZONAL1, B_ZONAL2, B_ZONAL3, B_ZONAL4, B_ZONAL5, B_HWIND0, B_HWIND1, B_HWIND2, B_HWIND3,
    B_MED_IN, B_MED_OUT, B_HEUR_WINDWARD, B_HEUR_LEEWARD, B_HEUR_CUT_FAR, B_CAP_IN, B_CAP_BINDS, B_CAP_OUT, B_APPLY_SHADOW, B_APPLY_WINDWARD, B_APPLY_NONE,
    B_COUNT
};
struct NoCensus { WO_HD void hit(int) const {} };

// ---- :225-227, :237-239 ----
WO_HD inline float elev_blend_cell(float smoothed, float e) { return (float)((double)smoothed * 0.6 + (double)e * 0.4); }
WO_HD inline float height_km_cell(float e) { return (float)W::elev_to_height_km(cl_max(0, (double)e)); }

// ---- heuristicWind (js/heuristic-precip.js:51-81) ----
template <class C>
WO_HD inline void heuristic_wind(double distFromItczDeg, bool isNorthOfItcz, double& we, double& wn, const C& census) {
    const double hemiSign = isNorthOfItcz ? 1 : -1;
    if (distFromItczDeg < 5) {
        census.hit(B_HWIND0);
        we = 0;
        wn = -hemiSign * 0.1;
    } else if (distFromItczDeg < 30) {
        census.hit(B_HWIND1);
        const double tradeStrength = W::smoothstep(5, 15, distFromItczDeg) * (1 - W::smoothstep(25, 32, distFromItczDeg));
        we = -tradeStrength * 0.8;
        wn = -hemiSign * tradeStrength * 0.3;
    } else if (distFromItczDeg < 60) {
        census.hit(B_HWIND2);
        const double westStrength = W::smoothstep(30, 40, distFromItczDeg) * (1 - W::smoothstep(55, 65, distFromItczDeg));
        we = westStrength * 0.9;
        wn = hemiSign * westStrength * 0.25;
    } else {
        census.hit(B_HWIND3);
        const double polarStrength = W::smoothstep(60, 70, distFromItczDeg);
        we = -polarStrength * 0.4;
        wn = -hemiSign * polarStrength * 0.15;
    }
}

// ---- computeHeuristicWindField (:86-102), the 50-50 blend (:267-270) and the 3D vectors (:276-281) of one cell and season ----
struct WindOut { float e, n, x, y, z; };
template <class C>
WO_HD inline WindOut blended_wind_cell(float latF, float lonF, const float* itczLats, float rawE, float rawN, const W::Frames& T, int32_t r, const C& census) {
    const double lat = latF;
    const double itczLat = O::itcz_lookup(itczLats, (double)lonF) * 0.3;
    const double signedDist = lat - itczLat;
    const double distDeg = fabs(signedDist) / W::DEG;
    double hwe, hwn;
    heuristic_wind(distDeg, signedDist > 0, hwe, hwn, census);
    const float hWindE = (float)hwe, hWindN = (float)hwn;
    WindOut o;
    o.e = (float)(0.5 * (double)rawE + 0.5 * (double)hWindE);
    o.n = (float)(0.5 * (double)rawN + 0.5 * (double)hWindN);
    const double we = o.e, wn = o.n;
    o.x = (float)(we * (double)T.eastX[r] + wn * (double)T.northX[r]);
    o.y = (float)(we * (double)T.eastY[r] + wn * (double)T.northY[r]);
    o.z = (float)(we * (double)T.eastZ[r] + wn * (double)T.northZ[r]);
    return o;
}

// ---- the mechanisms loop (:307-487), steps (a) to (h), offset and coverage scaling, of one cell and season ----
struct MechIn {
    float lat, lon, elev, moisture, conv, windE, windN, gradE, gradN, pressure, cont, heightKm;
    int32_t coastDist;
    bool isLand, summer;
};
template <class C>
WO_HD inline float mechanisms_cell(const MechIn& I, const float* itczLats, const Params& P, double precipitationOffset, double landCoverage, const C& census) {
    const double lat = I.lat, lon = I.lon;
    const double absLatDeg = fabs(lat) / W::DEG;
    const double elev = I.elev;
    const bool isLand = I.isLand;
    const double moisture = I.moisture;
    double p = moisture;
    // (a)
    const double itczLat = O::itcz_lookup(itczLats, lon);
    const double distFromItcz = fabs(lat - itczLat) / W::DEG;
    const double cont = isLand ? (double)I.cont : 0;
    if (distFromItcz < 15) {
        census.hit(B_ITCZ_IN);
        const double itczStrength = W::smoothstep(15, 0, distFromItcz);
        if (distFromItcz < 5) census.hit(B_ITCZ_CORE);
        const double coreBoost = distFromItcz < 5 ? 1.5 : 1.0;
        p = p * (1 + itczStrength * coreBoost) + itczStrength * 0.3;
    } else census.hit(B_ITCZ_OUT);
    // (b)
    const double conv = I.conv;
    if (conv > 0) {
        census.hit(B_CONV_POS);
        const double convStrength = cl_min(1, (conv / P.avgEdgeRad) * 0.055);
        p = p * (1 + convStrength * 1.2) + convStrength * moisture * 0.4;
    } else census.hit(B_CONV_NOT);
    // (c)
    const double we = I.windE, wn = I.windN;
    const double windDotGrad = we * (double)I.gradE + wn * (double)I.gradN;
    if (isLand && elev > 0) {
        if (windDotGrad > 0) {
            census.hit(B_ORO_WINDWARD);
            const double uplift = cl_min(1, windDotGrad * 15);
            p += uplift * 1.0;
        } else {
            census.hit(B_ORO_LEEWARD);
            const double shadow = cl_min(1, -windDotGrad * 18);
            p *= cl_max(0.02, 1 - shadow * 0.95);
        }
    } else census.hit(B_ORO_NONE);
    // (d)
    const double pDev = I.pressure;
    const bool inLocalSummer = I.summer ? (lat >= 0) : (lat < 0);
    census.hit(inLocalSummer ? B_LOCAL_SUMMER : B_LOCAL_WINTER);
    const double subtropCenter = inLocalSummer ? 30 : 24;
    const double subtropWidth = inLocalSummer ? 16 : 12;
    double subtropPeak = inLocalSummer ? 0.50 : 0.30;
    if (isLand && inLocalSummer) {
        const double polewardWind = lat >= 0 ? wn : -wn;
        if (polewardWind > 0) {
            census.hit(B_MONSOON_RELIEF);
            if (I.coastDist < 0) census.hit(B_MONSOON_NO_COAST);
            const double coastDist = I.coastDist >= 0 ? I.coastDist : P.maxHops;
            const double coastProximity = 1 - W::smoothstep(0, P.maxHops * 0.4, coastDist);
            const double monsoonRelief = W::smoothstep(0, 0.15, polewardWind) * coastProximity;
            subtropPeak *= (1 - monsoonRelief * 0.7);
        } else census.hit(B_MONSOON_NONE);
    }
    const double subtropDist = fabs(absLatDeg - subtropCenter);
    census.hit(subtropDist < subtropWidth ? B_LATBAND_IN : B_LATBAND_OUT);
    const double latBandSuppression = subtropDist < subtropWidth ? W::smoothstep(subtropWidth, 0, subtropDist) * subtropPeak : 0;
    double pressureMod = 0;
    if (pDev > 0) { census.hit(B_PRESS_HIGH); pressureMod = W::smoothstep(0, 12, pDev) * 0.25; }
    else { census.hit(B_PRESS_LOW); pressureMod = -W::smoothstep(0, 15, -pDev) * 0.2; }
    const double totalSuppression = cl_max(0, latBandSuppression + pressureMod);
    if (totalSuppression > 0) { census.hit(B_SUPPRESS_POS); p *= cl_max(0.05, 1 - totalSuppression); }
    else { census.hit(B_SUPPRESS_NOT); p *= (1 - totalSuppression); }
    // (e)
    if (absLatDeg > 40) {
        census.hit(B_POLAR_IN);
        if (I.coastDist < 0) census.hit(B_POLAR_NO_COAST);
        const double polarStrength = W::smoothstep(40, 70, absLatDeg);
        const double coastDist = I.coastDist < 0 ? P.maxHops : I.coastDist;
        const double inlandFade = 1 - W::smoothstep(0, P.maxHops, coastDist);
        const double polarBase = polarStrength * 0.10;
        const double polarCoastal = polarStrength * 0.20 * inlandFade;
        p += polarBase + polarCoastal;
        p *= (1 + polarStrength * 0.15);
    } else census.hit(B_POLAR_OUT);
    // (f)
    if (isLand && cont > 0) {
        census.hit(B_CONT_DRY);
        const double dryness = cont * cont * 0.55;
        p *= cl_max(0.03, 1 - dryness);
    } else census.hit(B_CONT_NOT);
    // (g)
    const double heightKm = I.heightKm;
    if (isLand && heightKm > 1.5) {
        census.hit(B_LEE_HIGH);
        if (windDotGrad < -0.01 && I.coastDist >= 0 && I.coastDist < P.leeCoastHops) {
            census.hit(B_LEE_CYCLO);
            p += 0.15 * cl_min(1, heightKm / 5);
        } else census.hit(B_LEE_NOT);
    }
    if (!isLand) {
        census.hit(B_OCEAN_CELL);
        const double highPressureFade = pDev > 0 ? W::smoothstep(0, 12, pDev) : 0;
        const double oceanBase = 0.15 * (1 - highPressureFade);
        p = cl_max(p, oceanBase);
    }
    // (h)
    if (isLand && I.coastDist > 0) {
        const double distKm = I.coastDist * P.avgEdgeKm;
        if (distKm > 2000) {
            census.hit(B_CUT_FAR);
            const double fade = 1 - W::smoothstep(2000, 3000, distKm);
            p *= cl_max(0.03, fade);
        } else census.hit(B_CUT_NEAR);
    } else census.hit(B_CUT_NONE);
    const double precipMult = 1 + precipitationOffset * 0.5;
    double finalPrecip = p * precipMult;
    if (landCoverage > 0.4) {
        const double t = (landCoverage - 0.4) / 0.6;
        finalPrecip *= 1 - t * t * 0.98;
    }
    return (float)max0(finalPrecip);
}

// ---- the rain-shadow seed (:501-513); 0 where the reference leaves the fresh array untouched ----
template <class C>
WO_HD inline float shadow_seed_cell(bool isLand, float elev, float windE, float windN, float gradE, float gradN, float heightKmF, const C& census) {
    if (!isLand || elev <= 0.0f) return 0.0f;
    const double windDotGrad = (double)windE * (double)gradE + (double)windN * (double)gradN;
    const double heightKm = heightKmF;
    if (heightKm < 0.8) { census.hit(B_SEED_LOW); return 0.0f; }
    const double heightScale = cl_min(1, (heightKm - 0.5) / 2.5);
    if (windDotGrad > 0) { census.hit(B_SEED_WINDWARD); return (float)(cl_min(1, windDotGrad * 20) * heightScale); }
    if (windDotGrad < 0) { census.hit(B_SEED_SHADOW); return (float)(-cl_min(1, -windDotGrad * 18) * heightScale); }
    census.hit(B_SEED_ZERO);
    return 0.0f;
}

// ---- the wind-aligned weights (:528-545) of one adjacency entry (r, nb) of a land row; upMember / dnMember: the double test ----
WO_HD inline void aligned_weights(const float* xyz, const float* wx, const float* wy, const float* wz, int32_t r, int32_t nb, float& upWt, float& dnWt,
                                  bool& upMember, bool& dnMember) {
    const double dx = (double)xyz[3 * (int64_t)r] - (double)xyz[3 * (int64_t)nb];
    const double dy = (double)xyz[3 * (int64_t)r + 1] - (double)xyz[3 * (int64_t)nb + 1];
    const double dz = (double)xyz[3 * (int64_t)r + 2] - (double)xyz[3 * (int64_t)nb + 2];
    const double upDot = (double)wx[nb] * dx + (double)wy[nb] * dy + (double)wz[nb] * dz;
    const double dnDot = -((double)wx[r] * dx + (double)wy[r] * dy + (double)wz[r] * dz);
    upMember = upDot > 0; dnMember = dnDot > 0;
    upWt = upMember ? (float)upDot : 0.0f;
    dnWt = dnMember ? (float)dnDot : 0.0f;
}

// ---- one propagation pass (:555-571, :582-598) on K fields of a cell at once (K = 2: the two seasons).  SHADOW: gathers
// val < 0 and stores min(src, carried); otherwise gathers val > 0 and stores max.  wt: row-shaped weights, one group per entry ----
template <int K, bool SHADOW>
WO_HD inline O::Group<K> propagate_cell(const int32_t* off, const int32_t* adj, const O::Group<K>* wt, const O::Group<K>* src, double keep /* 1 - decay */, int32_t r) {
    double val[K], w[K];
    for (int k = 0; k < K; ++k) { val[k] = 0; w[k] = 0; }
    for (int32_t ni = off[r]; ni < off[r + 1]; ++ni) {
        const O::Group<K> g = src[adj[ni]];
        const O::Group<K> q = wt[ni];
        for (int k = 0; k < K; ++k) {
            const bool take = SHADOW ? g.v[k] < 0.0f : g.v[k] > 0.0f;
            if (take && q.v[k] > 0.0f) { val[k] += (double)g.v[k] * (double)q.v[k]; w[k] += (double)q.v[k]; }
        }
    }
    const O::Group<K> self = src[r];
    O::Group<K> out;
    for (int k = 0; k < K; ++k) {
        if (w[k] > 0) {
            const double carried = (val[k] / w[k]) * keep;
            out.v[k] = (float)(SHADOW ? cl_min((double)self.v[k], carried) : cl_max((double)self.v[k], carried));
        } else out.v[k] = self.v[k];
    }
    return out;
}
// the folds after the last passes (:572-574, :599-601) and the merge (:604-606)
WO_HD inline float shadow_merge_cell(float seed, float shadowSrc, float windwardSrc) {
    float shadowField = seed, windwardField = seed;
    if (shadowSrc < shadowField) shadowField = shadowSrc;
    if (windwardSrc > windwardField) windwardField = windwardSrc;
    return shadowField < 0.0f ? shadowField : windwardField;
}

// ---- step 2c (:616-627) ----
template <class C>
WO_HD inline float apply_shadow_cell(bool isLand, float precip, float rsF, const C& census) {
    if (!isLand) return precip;
    const double rs = rsF;
    if (rs < -0.01) {
        census.hit(B_APPLY_SHADOW);
        const double strength = cl_min(1, -rs * 2.25);
        return (float)((double)precip * cl_max(0.02, 1 - strength * 0.92));
    }
    if (rs > 0.01) { census.hit(B_APPLY_WINDWARD); return (float)((double)precip + rs * 1.2); }
    census.hit(B_APPLY_NONE);
    return precip;
}

// ---- the west-coast seed (js/heuristic-precip.js:131-150) ----
WO_HD inline float west_coast_seed_cell(const int32_t* off, const int32_t* adj, const float* xyz, const uint8_t* isLand, const int32_t* coastDist,
                                        const float* eastX, const float* eastY, const float* eastZ, int32_t r) {
    if (!isLand[r] || coastDist[r] != 0) return 0.0f;
    double oceanDotEast = 0; int32_t count = 0;
    const double px = xyz[3 * (int64_t)r], py = xyz[3 * (int64_t)r + 1], pz = xyz[3 * (int64_t)r + 2];
    const double ex = eastX[r], ey = eastY[r], ez = eastZ[r];
    for (int32_t ni = off[r]; ni < off[r + 1]; ++ni) {
        const int64_t nb = adj[ni];
        if (!isLand[nb]) {
            const double dx = (double)xyz[3 * nb] - px, dy = (double)xyz[3 * nb + 1] - py, dz = (double)xyz[3 * nb + 2] - pz;
            oceanDotEast += dx * ex + dy * ey + dz * ez;
            ++count;
        }
    }
    if (count == 0) return 0.0f;
    return oceanDotEast < 0 ? 1.0f : -1.0f;
}
// ---- one pass of the land-masked smoothing (:154-166): ocean cells 0, land neighbours only ----
WO_HD inline float west_coast_smooth_cell(const int32_t* off, const int32_t* adj, const uint8_t* isLand, const float* src, int32_t r) {
    if (!isLand[r]) return 0.0f;
    double sum = src[r]; int32_t count = 1;
    for (int32_t ni = off[r]; ni < off[r + 1]; ++ni) {
        const int32_t nb = adj[ni];
        if (isLand[nb]) { sum += (double)src[nb]; ++count; }
    }
    return (float)(sum / count);
}

// ---- zonalBase (:16-37) ----
template <class C>
WO_HD inline double zonal_base(double distDeg, const C& census) {
    if (distDeg < 5) { census.hit(B_ZONAL0); return 1.0; }
    if (distDeg < 10) { census.hit(B_ZONAL1); return 1.0 - 0.65 * W::smoothstep(5, 10, distDeg); }
    if (distDeg < 33) { census.hit(B_ZONAL2); return 0.35 - 0.33 * W::smoothstep(10, 28, distDeg); }
    if (distDeg < 55) { census.hit(B_ZONAL3); return 0.02 + 0.48 * W::smoothstep(33, 55, distDeg); }
    if (distDeg < 70) { census.hit(B_ZONAL4); return 0.5 - 0.2 * W::smoothstep(55, 70, distDeg); }
    census.hit(B_ZONAL5);
    return 0.3 - 0.2 * W::smoothstep(70, 90, distDeg);
}

// ---- the per-cell product of the heuristic model (:183-259) of one cell and season ----
template <class C>
WO_HD inline float heuristic_cell(float latF, float lonF, const float* itczLats, bool summer, bool isLand, float contF, float elevF, float gradE, float gradN,
                                  float westCoast, int32_t coastDist, double avgEdgeKm, const C& census) {
    const double lat = latF, lon = lonF;
    const double itczLat = O::itcz_lookup(itczLats, lon) * 0.3;
    const double signedDist = lat - itczLat;
    const double distFromItczDeg = fabs(signedDist) / W::DEG;
    const bool isNorthOfItcz = signedDist > 0;
    const double zonal = zonal_base(distFromItczDeg, census);
    const double absLatDeg = fabs(lat) / W::DEG;
    const bool inSummerHemi = summer ? (lat >= 0) : (lat < 0);
    double seasonMod = inSummerHemi ? 1.1 : 0.9;
    if (inSummerHemi && absLatDeg > 22 && absLatDeg < 45) {
        census.hit(B_MED_IN);
        const double medSuppress = W::smoothstep(22, 30, absLatDeg) * (1 - W::smoothstep(38, 45, absLatDeg));
        const double wc = westCoast;
        const double strength = 0.15 + wc * 0.20;
        seasonMod *= (1 - medSuppress * cl_max(0, strength));
    } else census.hit(B_MED_OUT);
    double contMod = 1.0;
    const double cont = isLand ? (double)contF : 0;
    if (cont > 0) contMod = 1.0 - cont * cont * 0.65;
    double oroMod = 1.0;
    if (isLand && elevF > 0.0f) {
        double we, wn;
        heuristic_wind(distFromItczDeg, isNorthOfItcz, we, wn, NoCensus());
        const double windDotGrad = we * (double)gradE + wn * (double)gradN;
        if (windDotGrad > 0) {
            census.hit(B_HEUR_WINDWARD);
            const double uplift = cl_min(1, windDotGrad * 15);
            oroMod = 1.0 + uplift * 0.6;
        } else {
            census.hit(B_HEUR_LEEWARD);
            const double heightKm = W::elev_to_height_km(cl_max(0, (double)elevF));
            const double heightScale = cl_min(1, heightKm / 3);
            const double shadow = cl_min(1, -windDotGrad * 18);
            oroMod = cl_max(0.3, 1.0 - shadow * 0.7 * heightScale);
        }
    }
    double distMod = 1.0;
    if (isLand && coastDist > 0) {
        const double distKm = coastDist * avgEdgeKm;
        if (distKm > 2000) { census.hit(B_HEUR_CUT_FAR); distMod = cl_max(0.03, 1 - W::smoothstep(2000, 3000, distKm)); }
    }
    return (float)cl_max(0.05, zonal * seasonMod * contMod * oroMod * distMod);
}

// ---- blend and normalise (:648-676) ----
WO_HD inline float blend_cell(float complex, float heur) { return (float)(0.5 * (double)complex + 0.5 * (double)heur); }
WO_HD inline uint32_t percentile_rank(uint32_t n) { return (uint32_t)floor((double)n * 0.95); }
template <class C>
WO_HD inline float normalise_cell(float blended, float maxPrecip, bool isLand, float contF, const C& census) {
    float b = (float)cl_min(1, (double)blended / (double)maxPrecip);
    if (isLand && (double)contF > 0.5) {
        census.hit(B_CAP_IN);
        const double t = W::smoothstep(0.5, 1.0, (double)contF);
        const double cap = 1.0 - t * 0.80;
        if (cap < (double)b) census.hit(B_CAP_BINDS);
        b = (float)cl_min((double)b, cap);
    } else census.hit(B_CAP_OUT);
    return b;
}

}  // namespace precip
}  // namespace wo
