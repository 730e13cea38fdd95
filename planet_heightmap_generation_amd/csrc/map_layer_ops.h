// The map view's layers and its centre meridian (the reference's buildMapMesh, js/planet-mesh.js:200-382): the bodies shared by the
// device kernels (map.hip) and the test-only CPU emulator (tests/emu_map_layers), beside those of map_ops.h and under its rules
// (double arithmetic on the f32 inputs, stored as f32, js_max / js_min, -ffp-contract=off).
//
// Centre meridian (:244-249).  Every vertex longitude goes through wrapLon: l = lon - centerLon; l > pi: l -= 2 pi; otherwise
//   l < -pi: l += 2 pi.  In double, before the `wraps` test of side_triangles, which with everything after it is unchanged.  The
//   reference wraps once, so centerLon is held to [-pi, pi] by the entry point.  centerLon == 0 changes no bit: l - 0 is exact
//   and neither branch fires.
// Layers.  One colour function per region on one or two fields: continentalityColor (:135-158), temperatureColor (:162-172),
//   precipitationColor (:96-116), rainShadowColor (:120-131), oceanCurrentColor (:506-529; ocean is elevation <= 0) and, for the
//   pressure, wind speed and generic layers, debugValueToColor (:83-93) over the layer's range.  Math.pow(x, 0.6) of
//   oceanCurrentColor is the platform's pow: ocml on the device, glibc in the emulator, V8's in the reference.
// Range (:231-237).  dbgMin and dbgMax start at 0 and move with `<` and `>`: NaN never enters, -0 never replaces +0.  So only
//   values < 0 can be the minimum and only values > 0 the maximum, and inside one sign the order of floats is the order of their
//   bit patterns as unsigned integers: both bounds are a maximum over uint32 words that start at 0 (the bits of +0).  Exact, so
//   any reduction tree gives the same bits.
// What the map view does not define is taken from map_ops.h: the quantiser, the gamma table, alpha 255, and for the pixels nothing
//   covers the 0x1a1a2e background of the coloured types.  That is OUR DECISION: the map view has no exporter of its own.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>

#include "map_ops.h"

namespace wo {
namespace map {

// the reference's debugLayer names (LAYER_DEBUG: any other array, coloured over its own range), as WO_MAP_LAYER_* of worogen.h
enum : int32_t {
    LAYER_DEBUG = 0, LAYER_CONTINENTALITY, LAYER_TEMP_SUMMER, LAYER_TEMP_WINTER, LAYER_PRECIP_SUMMER, LAYER_PRECIP_WINTER, LAYER_RAINSHADOW_SUMMER,
    LAYER_RAINSHADOW_WINTER, LAYER_OCEANCURRENT_SUMMER, LAYER_OCEANCURRENT_WINTER, LAYER_PRESSURE_SUMMER, LAYER_PRESSURE_WINTER, LAYER_WINDSPEED_SUMMER,
    LAYER_WINDSPEED_WINTER, LAYER_COUNT
};
WO_IMP_HD inline bool layer_is_ocean_current(int32_t l) { return l == LAYER_OCEANCURRENT_SUMMER || l == LAYER_OCEANCURRENT_WINTER; }
// debugValueToColor over the values' range
WO_IMP_HD inline bool layer_needs_range(int32_t l) { return l == LAYER_DEBUG || (l >= LAYER_PRESSURE_SUMMER && l <= LAYER_WINDSPEED_WINTER); }

// ---- centre meridian ----------------------------------------------------------------------------------------------------------
WO_IMP_HD inline double wrap_lon(double lon, double centerLon) {
    const double PI = 3.141592653589793;
    double l = lon - centerLon;
    if (l > PI) l -= 2.0 * PI;
    else if (l < -PI) l += 2.0 * PI;
    return l;
}
WO_IMP_HD inline LonLat lonlat_of_centered(float x, float y, float z, double centerLon) {
    return LonLat{wrap_lon(imp::fd_atan2((double)x, (double)z), centerLon), imp::fd_asin(js_max(-1.0, js_min(1.0, (double)y)))};
}
WO_IMP_HD inline LonLat lonlat_of_center_centered(const int32_t* triangles, const float* r_xyz, int64_t t, double centerLon) {
    float c[3];
    triangle_center(triangles, r_xyz, t, c);
    return lonlat_of_centered(c[0], c[1], c[2], centerLon);
}
// what the entry point accepts: finite and within [-pi, pi]
WO_IMP_HD inline bool center_lon_ok(double c) { return c >= -3.141592653589793 && c <= 3.141592653589793; }

// ---- range --------------------------------------------------------------------------------------------------------------------
// The two bounds as uint32 words, both reduced by max from 0: [0] the bits of the minimum (a negative float, or +0), [1] those
// of the maximum (a positive float, or +0).
struct RangeBits { uint32_t lo, hi; };
WO_IMP_HD inline uint32_t f32_bits(float v) { uint32_t u; memcpy(&u, &v, 4); return u; }
WO_IMP_HD inline float f32_of_bits(uint32_t u) { float v; memcpy(&v, &u, 4); return v; }
WO_IMP_HD inline void range_take(RangeBits& r, float v) {
    const uint32_t u = f32_bits(v);
    if (v < 0.0f && u > r.lo) r.lo = u;
    if (v > 0.0f && u > r.hi) r.hi = u;
}

// ---- colours (c: the three channels in double, rounded to f32 by the caller) --------------------------------------------------
// js/planet-mesh.js:83-93
WO_IMP_HD inline void debug_value_color(double v, double minV, double maxV, double c[3]) {
    double range = js_max(imp::fd_fabs(minV), imp::fd_fabs(maxV));
    if (range == 0.0 || range != range) range = 1.0;                              // `|| 1`: 0 and NaN are falsy
    const double t = js_max(-1.0, js_min(1.0, v / range));
    if (t < 0.0) {
        const double s = -t;
        c[0] = 1.0 - s * 0.7; c[1] = 1.0 - s * 0.7; c[2] = 1.0;
    } else {
        const double s = t;
        c[0] = 1.0; c[1] = 1.0 - s * 0.75; c[2] = 1.0 - s * 0.75;
    }
}
// js/planet-mesh.js:96-116
WO_IMP_HD inline void precipitation_color(double value, double c[3]) {
    const double t = js_max(0.0, js_min(1.0, value));
    if (t < 0.25) { const double s = t / 0.25; c[0] = 0.76 - s * 0.16; c[1] = 0.60 - s * 0.05; c[2] = 0.42 - s * 0.12; }
    else if (t < 0.5) { const double s = (t - 0.25) / 0.25; c[0] = 0.60 - s * 0.30; c[1] = 0.55 + s * 0.20; c[2] = 0.30 - s * 0.05; }
    else if (t < 0.75) { const double s = (t - 0.5) / 0.25; c[0] = 0.30 - s * 0.15; c[1] = 0.75 - s * 0.10; c[2] = 0.25 + s * 0.40; }
    else { const double s = (t - 0.75) / 0.25; c[0] = 0.15 - s * 0.05; c[1] = 0.65 - s * 0.35; c[2] = 0.65 + s * 0.20; }
}
// js/planet-mesh.js:120-131
WO_IMP_HD inline void rain_shadow_color(double value, double c[3]) {
    if (value > 0.01) { const double t = js_min(1.0, value / 0.5); c[0] = 0.55 - t * 0.40; c[1] = 0.55 - t * 0.10; c[2] = 0.58 + t * 0.37; }
    else if (value < -0.01) { const double t = js_min(1.0, -value / 0.5); c[0] = 0.55 + t * 0.35; c[1] = 0.55 - t * 0.35; c[2] = 0.58 - t * 0.45; }
    else { c[0] = 0.55; c[1] = 0.55; c[2] = 0.58; }
}
// js/planet-mesh.js:135-158
WO_IMP_HD inline void continentality_color(double value, double c[3]) {
    const double t = js_max(0.0, js_min(1.0, value));
    if (t < 0.15) { const double s = t / 0.15; c[0] = 0.05 + s * 0.10; c[1] = 0.10 + s * 0.20; c[2] = 0.40 + s * 0.20; }
    else if (t < 0.4) { const double s = (t - 0.15) / 0.25; c[0] = 0.15 - s * 0.05; c[1] = 0.30 + s * 0.45; c[2] = 0.60 - s * 0.35; }
    else if (t < 0.7) { const double s = (t - 0.4) / 0.3; c[0] = 0.10 + s * 0.80; c[1] = 0.75 - s * 0.05; c[2] = 0.25 - s * 0.15; }
    else if (t < 0.9) { const double s = (t - 0.7) / 0.2; c[0] = 0.90 + s * 0.05; c[1] = 0.70 - s * 0.40; c[2] = 0.10 - s * 0.05; }
    else { const double s = (t - 0.9) / 0.1; c[0] = 0.95 - s * 0.25; c[1] = 0.30 - s * 0.20; c[2] = 0.05; }
}
// js/planet-mesh.js:162-172
WO_IMP_HD inline void temperature_color(double value, double c[3]) {
    const double T = -45.0 + js_max(0.0, js_min(1.0, value)) * 90.0;
    if (T < -38.0) { c[0] = 0.78; c[1] = 0.78; c[2] = 0.78; }
    else if (T < 0.0) { c[0] = 0.00; c[1] = 0.00; c[2] = 0.50; }
    else if (T < 10.0) { c[0] = 0.53; c[1] = 0.81; c[2] = 0.92; }
    else if (T < 18.0) { c[0] = 1.00; c[1] = 1.00; c[2] = 0.00; }
    else if (T < 22.0) { c[0] = 1.00; c[1] = 0.65; c[2] = 0.00; }
    else if (T < 32.0) { c[0] = 1.00; c[1] = 0.00; c[2] = 0.00; }
    else if (T < 40.0) { c[0] = 0.55; c[1] = 0.00; c[2] = 0.00; }
    else { c[0] = 0.20; c[1] = 0.00; c[2] = 0.00; }
}
// js/planet-mesh.js:506-529
WO_IMP_HD inline void ocean_current_color(double warmth, double speed, bool isOcean, double c[3]) {
    if (!isOcean) { c[0] = 0.45; c[1] = 0.45; c[2] = 0.45; return; }
    const double intensity = pow(js_min(1.0, speed * 3.0), 0.6);
    const double base = 0.12;
    if (warmth > 0.05) {
        const double w = js_min(1.0, warmth * 1.5);
        const double t = base + (1.0 - base) * w * intensity;
        c[0] = t; c[1] = base * 0.4 + t * 0.1; c[2] = base * 0.3;
    } else if (warmth < -0.05) {
        const double w = js_min(1.0, -warmth * 1.5);
        const double t = base + (1.0 - base) * w * intensity;
        c[0] = base * 0.3; c[1] = base * 0.5 + t * 0.15; c[2] = t;
    } else {
        const double t = base + intensity * 0.45;
        c[0] = t * 0.55; c[1] = t * 0.7; c[2] = t * 0.65;
    }
}

// The colour of a region in `layer`.  a: the layer's field (the warmth of an ocean-current layer); b: the speed, and
// elevation: both read by the ocean-current layers only; range: read by the layers of layer_needs_range only.
WO_IMP_HD inline Rgb layer_color(int32_t layer, float a, float b, float elevation, RangeBits range) {
    double c[3];
    const double v = (double)a;
    switch (layer) {
        case LAYER_CONTINENTALITY: continentality_color(v, c); break;
        case LAYER_TEMP_SUMMER: case LAYER_TEMP_WINTER: temperature_color(v, c); break;
        case LAYER_PRECIP_SUMMER: case LAYER_PRECIP_WINTER: precipitation_color(v, c); break;
        case LAYER_RAINSHADOW_SUMMER: case LAYER_RAINSHADOW_WINTER: rain_shadow_color(v, c); break;
        case LAYER_OCEANCURRENT_SUMMER: case LAYER_OCEANCURRENT_WINTER: ocean_current_color(v, (double)b, elevation <= 0.0f, c); break;
        default: debug_value_color(v, (double)f32_of_bits(range.lo), (double)f32_of_bits(range.hi), c); break;
    }
    return rgb_of(c[0], c[1], c[2]);
}

}  // namespace map
}  // namespace wo
