// One colour per region, for the map export and the globe mesh alike (view_colors.h).  The colour functions are map_ops.h's,
// map_layer_ops.h's and globe_ops.h's, the tints pick_ops.h's; a kernel here is one of them over every region, written through a
// sink: an f32 triple at rgb + 3 r (the globe: the values the reference hands to three.js) or one RGBA8 word at rgba[r], packed
// through the quantiser and the gamma table (the map).  The editor's tint is applied before the sink, on the f32 channels, when a
// highlight state is set and the region's class byte is not 0.
//
// Launches of view_region_colors (on the planet's stream, no host round trip between them):
//   a map type             k_view_type_colors [1]; `biome`: k_view_biome_raw [1] (the untinted f32 triples) and k_view_biome_smooth [1]
//   a map layer            k_view_range [1] for the layers coloured over their range (the bounds as two uint32 words in device memory:
//                          block_ops.h's block_max_to_global), then k_view_layer_colors [1], which reads the bounds from device memory
//   the plate view         k_view_plate_slots [0-1] (the table's row of every seed), k_view_plate_colors [1]
// Memory (device_mem.h): the raw triples, the range words, the plate slots and the uploads are temporaries of the caller's arena.
#include <hip/hip_runtime.h>

#include <atomic>
#include <string>

#include "block_ops.h"
#include "device.h"
#include "globe_ops.h"
#include "map_layer_ops.h"
#include "map_ops.h"
#include "ocean_block.h"
#include "pick_ops.h"
#include "precip_block.h"
#include "view_colors.h"
#include "wind_block.h"

namespace M = wo::map;

namespace wo {

struct SinkRgb {
    float* __restrict__ rgb;
    __device__ void put(int32_t r, const M::Rgb& c) const { rgb[3 * (int64_t)r] = c.r; rgb[3 * (int64_t)r + 1] = c.g; rgb[3 * (int64_t)r + 2] = c.b; }
};
struct SinkRgba {
    uint32_t* __restrict__ rgba;
    const uint8_t* __restrict__ lut;
    __device__ void put(int32_t r, const M::Rgb& c) const { rgba[r] = M::pack_rgba(c, lut); }
};

// cls: the highlight state's class bytes, nullptr without a state
__device__ inline M::Rgb view_tinted(const M::Rgb& c, const uint8_t* __restrict__ cls, int32_t r) { return cls && cls[r] ? pick::tint(c, cls[r]) : c; }

template <class Sink>
__global__ __launch_bounds__(WO_BLOCK) void k_view_type_colors(int32_t type, const float* __restrict__ e, const uint8_t* __restrict__ koppen, const uint8_t* __restrict__ cls, Sink sink, int32_t N) {
    const int32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r < N) sink.put(r, view_tinted(M::region_color(type, e[r], koppen ? (int32_t)koppen[r] : 0), cls, r));
}
__global__ __launch_bounds__(WO_BLOCK) void k_view_biome_raw(const float* __restrict__ e, const uint8_t* __restrict__ koppen, float* __restrict__ raw, int32_t N) {
    const int32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r < N) SinkRgb{raw}.put(r, M::region_color(M::TYPE_BIOME, e[r], (int32_t)koppen[r]));
}
template <class Sink>
__global__ __launch_bounds__(WO_BLOCK) void k_view_biome_smooth(const float* __restrict__ raw, const int32_t* __restrict__ off, const int32_t* __restrict__ adj, const uint8_t* __restrict__ cls, Sink sink,
                                                                int32_t N) {
    const int32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r < N) sink.put(r, view_tinted(M::biome_smooth(raw, off, adj, r), cls, r));
}

// The range of a layer's values (map_layer_ops.h: RangeBits): range[0], range[1] were cleared; every bound is a maximum over uint32
// words.  Sixteen bytes per load where v is aligned for it, four loads in flight per thread, the last N % 4 values one by one.
__global__ __launch_bounds__(WO_BLOCK) void k_view_range(const float* __restrict__ v, int32_t N, uint32_t* __restrict__ range) {
    __shared__ uint32_t blockR[2];
    if (threadIdx.x < 2) blockR[threadIdx.x] = 0u;
    __syncthreads();
    M::RangeBits r{0u, 0u};
    const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (int64_t)gridDim.x * blockDim.x;
    const int64_t groups = (reinterpret_cast<uintptr_t>(v) & 15u) ? 0 : (int64_t)N / 4;
    const float4* __restrict__ v4 = reinterpret_cast<const float4*>(v);
    int64_t g = tid;
    for (; g + 3 * stride < groups; g += 4 * stride) {
        const float4 q0 = v4[g], q1 = v4[g + stride], q2 = v4[g + 2 * stride], q3 = v4[g + 3 * stride];
        M::range_take(r, q0.x); M::range_take(r, q0.y); M::range_take(r, q0.z); M::range_take(r, q0.w);
        M::range_take(r, q1.x); M::range_take(r, q1.y); M::range_take(r, q1.z); M::range_take(r, q1.w);
        M::range_take(r, q2.x); M::range_take(r, q2.y); M::range_take(r, q2.z); M::range_take(r, q2.w);
        M::range_take(r, q3.x); M::range_take(r, q3.y); M::range_take(r, q3.z); M::range_take(r, q3.w);
    }
    for (; g < groups; g += stride) {
        const float4 q = v4[g];
        M::range_take(r, q.x); M::range_take(r, q.y); M::range_take(r, q.z); M::range_take(r, q.w);
    }
    for (int64_t i = 4 * groups + tid; i < N; i += stride) M::range_take(r, v[i]);
    const uint32_t w[2] = {r.lo, r.hi};
    block_max_to_global<2>(w, blockR, range);
}

// b and e are read by the ocean-current layers only, range by the layers coloured over their range
template <class Sink>
__global__ __launch_bounds__(WO_BLOCK) void k_view_layer_colors(int32_t layer, const float* __restrict__ a, const float* __restrict__ b, const float* __restrict__ e, const uint32_t* __restrict__ range,
                                                                const uint8_t* __restrict__ cls, Sink sink, int32_t N) {
    const int32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= N) return;
    const bool current = M::layer_is_ocean_current(layer);
    const M::RangeBits R = M::layer_needs_range(layer) ? M::RangeBits{range[0], range[1]} : M::RangeBits{0u, 0u};
    sink.put(r, view_tinted(M::layer_color(layer, a[r], current ? b[r] : 0.0f, current ? e[r] : 0.0f, R), cls, r));
}

// slot[seed] = the last row of the table with that seed (the reference's object keeps the last assignment); slot was filled with -1
__global__ __launch_bounds__(WO_BLOCK) void k_view_plate_slots(const int32_t* __restrict__ seeds, int32_t numPlates, int32_t* slot) {
    const int32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < numPlates) atomicMax(slot + seeds[i], i);             // view_resolve checked 0 <= seeds[i] < N
}
template <class Sink>
__global__ __launch_bounds__(WO_BLOCK) void k_view_plate_colors(const int32_t* __restrict__ r_plate, const int32_t* __restrict__ slot, const float* __restrict__ plateColors, const uint8_t* __restrict__ cls,
                                                                Sink sink, int32_t N) {
    const int32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r < N) sink.put(r, view_tinted(globe::plate_color(r_plate[r], N, slot, plateColors), cls, r));
}

// where a named layer's values live: the block, and the reference's result key of the field (two for the ocean-current layers)
struct LayerSource { const BlockDesc* block; const char *a, *b; const char* hint; };
static LayerSource layer_source(int32_t layer) {
    switch (layer) {
        case M::LAYER_CONTINENTALITY: return {&wind_desc(), "r_continentality", nullptr, "wo_wind_upload r_continentality"};
        case M::LAYER_TEMP_SUMMER: return {&temp_desc(), "r_temperature_summer", nullptr, "wo_temperature_upload r_temperature_summer"};
        case M::LAYER_TEMP_WINTER: return {&temp_desc(), "r_temperature_winter", nullptr, "wo_temperature_upload r_temperature_winter"};
        case M::LAYER_PRECIP_SUMMER: return {&precip_desc(), "r_precip_summer", nullptr, "wo_precip_upload r_precip_summer"};
        case M::LAYER_PRECIP_WINTER: return {&precip_desc(), "r_precip_winter", nullptr, "wo_precip_upload r_precip_winter"};
        case M::LAYER_RAINSHADOW_SUMMER: return {&precip_desc(), "r_rainshadow_summer", nullptr, "wo_precip_upload r_rainshadow_summer"};
        case M::LAYER_RAINSHADOW_WINTER: return {&precip_desc(), "r_rainshadow_winter", nullptr, "wo_precip_upload r_rainshadow_winter"};
        case M::LAYER_OCEANCURRENT_SUMMER: return {&ocean_desc(), "r_ocean_warmth_summer", "r_ocean_speed_summer", "wo_ocean_upload r_ocean_warmth_summer r_ocean_speed_summer"};
        case M::LAYER_OCEANCURRENT_WINTER: return {&ocean_desc(), "r_ocean_warmth_winter", "r_ocean_speed_winter", "wo_ocean_upload r_ocean_warmth_winter r_ocean_speed_winter"};
        case M::LAYER_PRESSURE_SUMMER: return {&wind_desc(), "r_pressure_summer", nullptr, "wo_wind_upload r_pressure_summer"};
        case M::LAYER_PRESSURE_WINTER: return {&wind_desc(), "r_pressure_winter", nullptr, "wo_wind_upload r_pressure_winter"};
        case M::LAYER_WINDSPEED_SUMMER: return {&wind_desc(), "r_wind_speed_summer", nullptr, "wo_wind_upload r_wind_speed_summer"};
        case M::LAYER_WINDSPEED_WINTER: return {&wind_desc(), "r_wind_speed_winter", nullptr, "wo_wind_upload r_wind_speed_winter"};
        default: return {nullptr, nullptr, nullptr, nullptr};
    }
}

bool view_resolve(const char* fn, wo_planet* p, const ViewRequest& q, ViewPlan& plan, const std::function<bool()>& geometry) {
    const std::string F = std::string(fn) + ": ";
    plan = ViewPlan{};
    plan.request = q;
    if (q.source == VIEW_TYPE && (q.id < 0 || q.id >= M::TYPE_COUNT)) { set_error(F + "unknown map type " + std::to_string(q.id)); return false; }
    if (q.source == VIEW_LAYER && (q.id < 0 || q.id >= M::LAYER_COUNT)) { set_error(F + "unknown map layer " + std::to_string(q.id)); return false; }
    if (q.source == VIEW_PLATES && q.colors) {
        if (!q.r_plate) { set_error(F + "the plate view reads r_plate, it is NULL"); return false; }
        if (q.numPlates < 0) { set_error(F + "numPlates is " + std::to_string(q.numPlates)); return false; }
        if (!q.plateSeeds || !q.plateColors) { set_error(F + "the plate view needs a colour table, " + (q.plateSeeds ? "plateColors" : "plateSeeds") + " is NULL"); return false; }
        for (int32_t i = 0; i < q.numPlates; ++i)
            if ((uint32_t)q.plateSeeds[i] >= (uint32_t)p->N) { set_error(F + "plateSeeds[" + std::to_string(i) + "] = " + std::to_string(q.plateSeeds[i]) + " is no region of the planet, which has " + std::to_string(p->N)); return false; }
    }
    if (!geometry()) return false;
    if (!q.colors) return true;
    if (q.source == VIEW_TYPE) {
        if (q.values) { set_error(F + "a map type reads the elevation, values must be NULL"); return false; }
        if (M::type_needs_koppen(q.id) && !(plan.koppen = koppen_classes(p))) { set_error(F + "no Koppen result on this planet (call wo_classify_koppen first)"); return false; }
    }
    if (q.source == VIEW_LAYER) {
        if (q.id == M::LAYER_DEBUG && !q.values) { set_error(F + "WO_MAP_LAYER_DEBUG takes its values from the caller, values is NULL"); return false; }
        if (M::layer_is_ocean_current(q.id) && q.values) { set_error(F + "an ocean-current layer reads two fields, values must be NULL (wo_ocean_upload sets the warmth and the speed)"); return false; }
        if (!q.values) {                                      // the resident field(s)
            const LayerSource S = layer_source(q.id);
            plan.block = S.block;
            plan.fa = S.block->index(S.a);
            plan.fb = S.b ? S.block->index(S.b) : -1;
            if (!block_require(p, fn, *S.block, bit(plan.fa) | (plan.fb >= 0 ? bit(plan.fb) : 0u), S.hint)) return false;
        }
    }
    return true;
}

template <class Sink>
static void view_launch(wo_planet* p, DeviceArena& T, const ViewPlan& plan, const float* e, Sink sink, ViewFamilies fam) {
    const ViewRequest& q = plan.request;
    const int32_t N = p->N, g = blocks_for(N);
    hipStream_t s = p->ctx->stream;
    const uint8_t* cls = highlight_classes(p);
    if (q.source == VIEW_PLATES) {
        int32_t* slot = T.dev<int32_t>((size_t)N);
        WO_HIP(hipMemsetAsync(slot, 0xFF, (size_t)N * 4, s));
        const int32_t* d_plate = up(T, q.r_plate, (size_t)N, s);
        if (q.numPlates > 0) {
            const int32_t* d_seeds = up(T, q.plateSeeds, (size_t)q.numPlates, s);
            launch(p, fam.colors, k_view_plate_slots, blocks_for(q.numPlates), WO_BLOCK, d_seeds, q.numPlates, slot);
        }
        const float* d_colors = q.numPlates > 0 ? up(T, q.plateColors, 3 * (size_t)q.numPlates, s) : nullptr;
        launch(p, fam.colors, k_view_plate_colors<Sink>, g, WO_BLOCK, d_plate, (const int32_t*)slot, d_colors, cls, sink, N);
    } else if (q.source == VIEW_LAYER) {
        const auto resident = [&](int f) { return (const float*)plan.block->slot(plan.block->get(p), f, (size_t)N).ptr; };
        const float* a = q.values ? up(T, q.values, (size_t)N, s) : resident(plan.fa);
        const float* b = plan.fb >= 0 ? resident(plan.fb) : nullptr;
        uint32_t* range = T.dev<uint32_t>(2);
        if (M::layer_needs_range(q.id)) {
            WO_HIP(hipMemsetAsync(range, 0, 8, s));
            launch(p, fam.range, k_view_range, blocks_for(((int64_t)N + 15) / 16, 1024), WO_BLOCK, a, N, range);      // 16 values per thread and turn
        }
        launch(p, fam.colors, k_view_layer_colors<Sink>, g, WO_BLOCK, q.id, a, b, e, (const uint32_t*)range, cls, sink, N);
    } else if (q.id == M::TYPE_BIOME) {
        float* raw = T.dev<float>(3 * (size_t)N);
        launch(p, fam.colors, k_view_biome_raw, g, WO_BLOCK, e, plan.koppen, raw, N);
        launch(p, fam.colors, k_view_biome_smooth<Sink>, g, WO_BLOCK, (const float*)raw, (const int32_t*)p->d_off, (const int32_t*)p->d_adj, cls, sink, N);
    } else {
        launch(p, fam.colors, k_view_type_colors<Sink>, g, WO_BLOCK, q.id, e, plan.koppen, cls, sink, N);
    }
}

void view_region_colors(wo_planet* p, DeviceArena& T, const ViewPlan& plan, const float* e, const ViewSink& sink, ViewFamilies families) {
    if (sink.rgb) view_launch(p, T, plan, e, SinkRgb{sink.rgb}, families);
    else view_launch(p, T, plan, e, SinkRgba{sink.rgba, sink.lut}, families);
}

bool sides_ok(const char* fn, wo_planet* p, int32_t numSides, const int32_t* triangles, const int32_t* halfedges) {
    const std::string F = std::string(fn) + ": ";
    const int32_t N = p->N;
    if (!triangles || !halfedges) { set_error(F + "null pointer"); return false; }
    if (numSides < 3 || numSides % 3 != 0 || numSides >= (1 << 30)) { set_error(F + "numSides is " + std::to_string(numSides) + ", it must be a multiple of 3 from 3 to 2^30 - 3"); return false; }
    std::atomic<int64_t> badCorner{-1}, badEdge{-1};
    parallel_ranges(numSides, [&](int64_t b, int64_t e, int) {
        for (int64_t s = b; s < e; ++s) {
            if ((uint32_t)triangles[s] >= (uint32_t)N) badCorner.store(s);
            if ((uint32_t)halfedges[s] >= (uint32_t)numSides) badEdge.store(s);
        }
    });
    if (badEdge.load() >= 0) { set_error(F + "half-edge out of range: halfedges[" + std::to_string(badEdge.load()) + "] = " + std::to_string(halfedges[badEdge.load()]) + ", the mesh has " + std::to_string(numSides) + " sides"); return false; }
    if (badCorner.load() >= 0) { set_error(F + "corner out of range: triangles[" + std::to_string(badCorner.load()) + "] = " + std::to_string(triangles[badCorner.load()]) + ", the planet has " + std::to_string(N) + " regions"); return false; }
    return true;
}

}  // namespace wo
