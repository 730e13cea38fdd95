// Per-launch profiling (wo_profile_*: an event pair around every launch, summed per kernel family) and the stage timings and
// statistics of the last call (wo_last_stage_timing, wo_last_erode_stats).
#include <hip/hip_runtime.h>

#include "../../include/worogen.h"
#include "device.h"
#include "erode_block.h"

namespace wo {

const char* const kFamilyNames[FAM_COUNT] = {
    "coast_flags", "smooth_elevation", "sharpen_ridges", "soil_creep", "warp_terrain", "noise_eval", "synthetic_terrain",
    "ocean_from_elevation", "sort_keys", "sort_radix", "rank_scatter", "receivers", "flow_climb",
    "flow_final", "solve_setup", "solve_round", "solve_final", "thermal_excess", "thermal_apply",
    "glac_index", "ice_receivers", "ice_round", "carve_setup", "carve_round", "moraine_fjord", "glacial_blend", "solve_patch", "elev_collisions", "elev_uplift_fused", "plate_grid", "plate_project", "smooth_field", "flood_eval", "flood_apply", "flood_misc", "climate_sweeps", "basin_layout", "basin_sort", "solve_basin", "flow_tiles", "misc", "event_pair_empty", "event_pair_noop_kernel", "event_pair_two_noop_kernels",
    "map_lonlat", "map_fill", "map_sides", "map_big_boxes", "map_resolve", "map_region_colors", "map_pixels",
    "map_range", "map_layer_colors",
    "globe_tables", "globe_region_colors", "globe_range", "globe_mesh", "globe_line_count", "globe_line_scan", "globe_line_write",
    "overlay_bins", "overlay_arrows",
    "pick", "pick_reduce", "highlight",
    "cube_centers", "cube_fill", "cube_sides", "cube_big_boxes", "cube_resolve",
    "relief_tri_elevation", "relief_heights", "relief_height16", "relief_tables", "relief_normals",
    "rivers", "rivers_climb", "rivers_lines",
    "view_tables", "view_fill", "view_sides", "view_big_boxes", "view_resolve", "view_shade",
    "outline_classify", "outline_flags", "outline_succ", "outline_rank", "outline_rings", "outline_positions"};

hipEvent_t profile_event(wo_planet* p) {
    if (!p->eventPool.empty()) { hipEvent_t e = p->eventPool.back(); p->eventPool.pop_back(); return e; }
    hipEvent_t e; WO_HIP(hipEventCreate(&e)); return e;
}
void profile_resolve(wo_planet* p) {
    if (p->pending.empty()) return;
    WO_HIP(hipStreamSynchronize(p->ctx->stream));
    if (p->erode && p->erode->side.built) WO_HIP(hipStreamSynchronize(p->erode->side.stream));
    for (auto& pe : p->pending) {
        float ms = 0; WO_HIP(hipEventElapsedTime(&ms, pe.a, pe.b));
        p->famMs[pe.fam] += ms; p->famLaunches[pe.fam] += 1;
        p->eventPool.push_back(pe.a); p->eventPool.push_back(pe.b);
    }
    p->pending.clear();
}

// The stage brackets of an earlier call, never asked for: their events back to the pool
void release_stage_brackets(wo_planet* p) {
    for (auto& b : p->stageBrackets) { p->eventPool.push_back(b.a); p->eventPool.push_back(b.b); }
    p->stageBrackets.clear(); p->stageSeen.clear(); p->stagePending = false;
}

}  // namespace wo

using namespace wo;

extern "C" {

// What an event pair measures around nothing, around a kernel that does nothing, and around two of them back to back: every family's time is a sum
// of such pairs, one per launch, so for launches of a few microseconds (the radix sort's: 5-25 us) the pair itself is a visible share of the figure.
// Reported as three families of their own; 2 x (one kernel) - (two kernels) is what a pair adds to the kernel it brackets (bench.py takes it off, and says so).
__global__ void k_profile_noop() {}
static void profile_calibrate(wo_planet* p) {
    hipStream_t s = p->ctx->stream;
    for (int k = 0; k < 8; ++k) hipLaunchKernelGGL(k_profile_noop, dim3(1), dim3(64), 0, s);      // (code object loaded, queues warm)
    WO_HIP(hipStreamSynchronize(s));
    auto pair = [&](int fam, int kernels) {
        hipEvent_t a = profile_event(p), b = profile_event(p);
        WO_HIP(hipEventRecord(a, s));
        for (int q = 0; q < kernels; ++q) hipLaunchKernelGGL(k_profile_noop, dim3(1), dim3(64), 0, s);
        WO_HIP(hipEventRecord(b, s));
        p->pending.push_back({fam, a, b});
    };
    for (int k = 0; k < 64; ++k) { pair(FAM_EVENT_PAIR, 0); pair(FAM_EVENT_PAIR_NOOP, 1); pair(FAM_EVENT_PAIR_NOOP2, 2); }
    profile_resolve(p);
}
int wo_profile_enable(wo_planet* p, int32_t on) {
    if (!check_planet(p, "wo_profile_enable")) return 1;
    WO_TRY if (!on) profile_resolve(p); p->profiling = on != 0; if (on) profile_calibrate(p); return 0; WO_CATCH("wo_profile_enable")
}
int wo_profile_reset(wo_planet* p) {
    if (!check_planet(p, "wo_profile_reset")) return 1;
    WO_TRY
    profile_resolve(p);
    for (int i = 0; i < FAM_COUNT; ++i) { p->famMs[i] = 0; p->famLaunches[i] = 0; }
    return 0;
    WO_CATCH("wo_profile_reset")
}
int wo_profile_report(wo_planet* p, int32_t cap, const char** names, double* total_ms, int64_t* launches, int32_t* count) {
    if (!check_planet(p, "wo_profile_report") || !count) return 1;
    WO_TRY
    profile_resolve(p);
    int32_t n = 0;
    for (int i = 0; i < FAM_COUNT && n < cap; ++i) {
        if (p->famLaunches[i] == 0) continue;
        if (names) names[n] = kFamilyNames[i];
        if (total_ms) total_ms[n] = p->famMs[i];
        if (launches) launches[n] = p->famLaunches[i];
        ++n;
    }
    *count = n;
    return 0;
    WO_CATCH("wo_profile_report")
}
static void stage_timing_resolve(wo_planet* p) {
    if (!p->stagePending) return;
    p->stagePending = false;
    WO_HIP(hipStreamSynchronize(p->ctx->stream));
    std::map<std::string, double> acc;
    for (auto& b : p->stageBrackets) {
        float ms = 0; WO_HIP(hipEventElapsedTime(&ms, b.a, b.b));
        acc[b.name] += ms;
        p->eventPool.push_back(b.a); p->eventPool.push_back(b.b);
    }
    p->stageBrackets.clear();
    p->stageTiming.clear();
    for (auto& n : p->stageSeen) { const auto& c = n.second; p->stageTiming.push_back({n.first, acc[n.first] * (c.second > 0 ? (double)c.first / (double)c.second : 1.0)}); }
    p->stageSeen.clear();
}
int wo_last_stage_timing(wo_planet* p, int32_t cap, const char** stages, double* ms, int32_t* count) {
    if (!p || !count) return 1;
    try { stage_timing_resolve(p); } catch (const wo::HipError& e) { wo::set_error(std::string("wo_last_stage_timing: ") + e.msg); return 1; }
    int32_t n = 0;
    for (auto& st : p->stageTiming) { if (n >= cap) break; if (stages) stages[n] = st.first.c_str(); if (ms) ms[n] = st.second; ++n; }
    *count = n;
    return 0;
}
int wo_last_erode_stats(wo_planet* p, int32_t cap, const char** names, double* values, int32_t* count) {
    if (!p || !count) return 1;
    int32_t n = 0;
    for (auto& st : p->erodeStats) { if (n >= cap) break; if (names) names[n] = st.first.c_str(); if (values) values[n] = st.second; ++n; }
    *count = n;
    return 0;
}

}  // extern "C"
