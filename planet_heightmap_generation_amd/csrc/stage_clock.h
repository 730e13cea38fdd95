// Timing helpers of the stage drivers: StageClock (event brackets around the stages of a call on the device, wo_last_stage_timing)
// and HostLap (stderr laps of a host-side stage, WO_FLOOD_TIMING).
#pragma once
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <map>
#include <string>
#include <vector>

#include "device.h"

namespace wo {

// Stage timings (wo_last_stage_timing, the reference's _postTiming).  A pair of event records costs ~10 us of stream time, and the
// composite loop has five stages per iteration (a 1.6 ms iteration: 8 ms of a 460 ms step went into timing it), so inside the loop
// only every 8th iteration is bracketed (`on`) and a stage's sum is scaled by occurrences / bracketed occurrences; stages outside
// the loop (setup, floods) are always bracketed.  WO_STAGE_TIMING=all, or per-launch profiling, brackets every iteration.
struct StageClock {
    wo_planet* p; std::vector<std::pair<std::string, std::pair<hipEvent_t, hipEvent_t>>> ev;
    std::map<std::string, std::pair<int64_t, int64_t>> seen;      // stage -> {occurrences, bracketed}
    bool on = true, open = false;
    explicit StageClock(wo_planet* pl) : p(pl) {}
    void begin(const char* name) {
        auto& c = seen[name]; ++c.first;
        open = on;
        if (!on) return;
        ++c.second;
        hipEvent_t a = profile_event(p), b = profile_event(p); WO_HIP(hipEventRecord(a, p->ctx->stream)); ev.push_back({name, {a, b}});
    }
    void end() { if (open) WO_HIP(hipEventRecord(ev.back().second.second, p->ctx->stream)); open = false; }
    void finish() {
        // the brackets are handed to the planet as they are; wo_last_stage_timing turns them into milliseconds when somebody asks
        release_stage_brackets(p);          // (an earlier call's, never asked for)
        std::vector<std::string> order;
        for (auto& e : ev) {
            if (std::find(order.begin(), order.end(), e.first) == order.end()) order.push_back(e.first);
            p->stageBrackets.push_back({e.first, e.second.first, e.second.second});
        }
        for (auto& n : order) p->stageSeen.push_back({n, seen[n]});
        ev.clear();
        p->stageTiming.clear();
        p->stagePending = true;
    }
    // a call that ends by exception (RedoWithChecks, a failed exchange) never reaches finish(): its events go back to the pool
    ~StageClock() { for (auto& e : ev) { p->eventPool.push_back(e.second.first); p->eventPool.push_back(e.second.second); } }
};

// WO_FLOOD_TIMING: one stderr line per step of a host-side stage, "[tag] what  ms since the previous line"
struct HostLap {
    const char* tag; int width; bool on;
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    void operator()(const char* what) {
        if (!on) return;
        const auto now = std::chrono::steady_clock::now();
        std::fprintf(stderr, "[%s] %-*s %8.1f ms\n", tag, width, what, std::chrono::duration<double, std::milli>(now - t0).count());
        t0 = now;
    }
};

}  // namespace wo
