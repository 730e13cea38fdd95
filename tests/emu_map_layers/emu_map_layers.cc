// Test-only CPU emulator: the bodies of csrc/map_layer_ops.h (centre meridian, layer colours, range) compiled for the host, behind
// a C interface that tests/map_layers_common.py loads with ctypes.  Brute force like tests/emu_map: the raster walks every side's
// whole pixel box, sides dealt round-robin to a few host threads that take the minimum per pixel; the range is a plain loop in
// index order.  It shares no scheduling with the kernels of csrc/map.hip.
#include <atomic>
#include <cstdint>
#include <thread>
#include <vector>

#include "../../planet_heightmap_generation_amd/csrc/map_layer_ops.h"

using namespace wo::map;

namespace {

void tables(int32_t N, const float* xyz, int32_t numSides, const int32_t* triangles, double centerLon, std::vector<LonLat>& r_ll, std::vector<LonLat>& t_ll) {
    r_ll.resize(N);
    t_ll.resize(numSides / 3);
    for (int32_t r = 0; r < N; ++r) r_ll[r] = lonlat_of_centered(xyz[3 * (int64_t)r], xyz[3 * (int64_t)r + 1], xyz[3 * (int64_t)r + 2], centerLon);
    for (int32_t t = 0; t < numSides / 3; ++t) t_ll[t] = lonlat_of_center_centered(triangles, xyz, t, centerLon);
}

RangeBits range_of(int32_t n, const float* v) {
    RangeBits r{0u, 0u};
    for (int32_t i = 0; i < n; ++i) range_take(r, v[i]);
    return r;
}

}  // namespace

extern "C" {

// as emu_geometry of tests/emu_map, around a centre meridian
int32_t emu_geometry_centered(int32_t N, const float* xyz, int32_t numSides, const int32_t* triangles, const int32_t* halfedges, double centerLon, float* positions,
                              int32_t* triRegions, int32_t* triSides) {
    std::vector<LonLat> r_ll, t_ll;
    tables(N, xyz, numSides, triangles, centerLon, r_ll, t_ll);
    int32_t count = 0;
    for (int32_t s = 0; s < numSides; ++s) {
        LonLat v[3];
        side_vertices(triangles, halfedges, t_ll.data(), r_ll.data(), s, v);
        Tri tri[2];
        const int n = side_triangles(v, tri);
        for (int k = 0; k < n; ++k, ++count) {
            for (int c = 0; c < 3; ++c) { positions[6 * (int64_t)count + 2 * c] = tri[k].x[c]; positions[6 * (int64_t)count + 2 * c + 1] = tri[k].y[c]; }
            triRegions[count] = triangles[s];
            triSides[count] = s;
        }
    }
    return count;
}

void emu_raster_centered(int32_t N, const float* xyz, int32_t numSides, const int32_t* triangles, const int32_t* halfedges, int32_t W, double centerLon, int32_t* regionMap,
                         int64_t* counts) {
    const int32_t H = W / 2;
    const int64_t pixels = (int64_t)W * H;
    std::vector<LonLat> r_ll, t_ll;
    tables(N, xyz, numSides, triangles, centerLon, r_ll, t_ll);
    std::vector<std::atomic<uint32_t>> sideMap(pixels);
    for (auto& s : sideMap) s.store(NO_SIDE, std::memory_order_relaxed);
    const int workers = 8;
    std::vector<std::thread> pool;
    for (int w = 0; w < workers; ++w)
        pool.emplace_back([&, w] {
            for (int64_t s = w; s < numSides; s += workers) {
                LonLat v[3];
                side_vertices(triangles, halfedges, t_ll.data(), r_ll.data(), s, v);
                Tri tri[2];
                const int n = side_triangles(v, tri);
                for (int k = 0; k < n; ++k) {
                    const double area2 = tri_area2(tri[k]);
                    Box b;
                    if (!tri_box(tri[k], area2, W, H, b)) continue;
                    for (int32_t j = b.j0; j <= b.j1; ++j)
                        for (int32_t i = b.i0; i <= b.i1; ++i) {
                            if (!tri_covers(tri[k], area2, pixel_xc(i, W), pixel_yc(j, H))) continue;
                            auto& cell = sideMap[(int64_t)j * W + i];
                            uint32_t cur = cell.load(std::memory_order_relaxed);
                            while ((uint32_t)s < cur && !cell.compare_exchange_weak(cur, (uint32_t)s, std::memory_order_relaxed)) {}
                        }
                }
            }
        });
    for (auto& t : pool) t.join();
    int64_t covered = 0;
    for (int64_t i = 0; i < pixels; ++i) {
        const uint32_t s = sideMap[i].load(std::memory_order_relaxed);
        regionMap[i] = s == NO_SIDE ? -1 : triangles[s];
        covered += s != NO_SIDE;
    }
    if (counts) { counts[0] = covered; counts[1] = pixels - covered; }
}

// the range of n values as the two floats dbgMin, dbgMax
void emu_range(int32_t n, const float* v, float* out) {
    const RangeBits r = range_of(n, v);
    out[0] = f32_of_bits(r.lo); out[1] = f32_of_bits(r.hi);
}

// One colour per element, 3 floats each.  b and e (the speed and the elevation) may be NULL for every layer but the ocean currents.
// range: dbgMin, dbgMax for the layers coloured over a range, NULL: the range of a.
void emu_layer_colors(int32_t layer, int32_t n, const float* a, const float* b, const float* e, const float* range, float* out) {
    RangeBits R{0u, 0u};
    if (layer_needs_range(layer)) R = range ? RangeBits{f32_bits(range[0]), f32_bits(range[1])} : range_of(n, a);
    for (int32_t r = 0; r < n; ++r) {
        const Rgb c = layer_color(layer, a[r], b ? b[r] : 0.0f, e ? e[r] : 0.0f, R);
        out[3 * (int64_t)r] = c.r; out[3 * (int64_t)r + 1] = c.g; out[3 * (int64_t)r + 2] = c.b;
    }
}

void emu_layer_rgba(int32_t layer, int32_t N, const float* a, const float* b, const float* e, int64_t pixels, const int32_t* regionMap, uint32_t* out) {
    uint8_t lut[256];
    gamma_lut(lut);
    const RangeBits R = layer_needs_range(layer) ? range_of(N, a) : RangeBits{0u, 0u};
    std::vector<uint32_t> packed(N);
    for (int32_t r = 0; r < N; ++r) packed[r] = pack_rgba(layer_color(layer, a[r], b ? b[r] : 0.0f, e ? e[r] : 0.0f, R), lut);
    const uint32_t bg = background_rgba(TYPE_COLOR, lut);
    for (int64_t i = 0; i < pixels; ++i) out[i] = regionMap[i] < 0 ? bg : packed[regionMap[i]];
}

}  // extern "C"
