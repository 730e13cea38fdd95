// Stand-alone host program for a sanitizer run of the failure path of the erosion block's one build helper (csrc/erode_block.h:
// build_group, regrow_group) on a machine WITHOUT a device: there hipMalloc fails, so a group's builder throws at its first
// allocation.  After the throw the group must not count as built, no arena may hold anything (wo::memory_in_use reads 0 bytes),
// the next attempt must run the builder again and end the same way, and the regrown group must be left at capacity 0.  With a
// device the allocations succeed: the program frees them, says that the failure path was not exercised and exits 0.  First, with
// or without a device: a builder that has set a view and THEN throws (what a later allocation of a group does when memory runs
// out).  The view must not survive it: the fresh arena has freed what it pointed at, and the next regrow would hand it to the
// block's arena to release.  No kernel is launched; not loaded into Python.
//
//   g++ -std=c++17 -O1 -g -fno-omit-frame-pointer -fsanitize=address,undefined -fno-sanitize-recover=undefined -D__HIP_PLATFORM_AMD__ \
//       -I/opt/rocm/include tools/sanitize/erode_block_main.cc -L/opt/rocm/lib -lamdhip64 -Wl,-rpath,/opt/rocm/lib \
//       -o /tmp/erode_block_asan && /tmp/erode_block_asan
#include <cstdint>
#include <cstdio>
#include <string>

#include "../../planet_heightmap_generation_amd/csrc/erode_block.h"

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { ++failures; std::printf("FAILED %s (line %d)\n", #cond, __LINE__); } } while (0)

static int64_t live_bytes() { const wo::MemoryInUse& m = wo::memory_in_use(); return m.deviceBytes.load() + m.pinnedBytes.load(); }

int main() {
    constexpr size_t N = 5000;
    int runs = 0;
    bool threw = false;
    {   // a throw after a view was set: the group is back in its initial state, the next attempt runs its builder again
        wo_erode_block b;
        auto& C = b.carve;
        int32_t somewhere = 0;
        int half = 0;
        auto halfway = [&](wo::DeviceArena&) { ++half; C.deps = &somewhere; C.depCnt = &somewhere; throw wo::HipError{"out of memory half-way"}; };
        for (int attempt = 1; attempt <= 2; ++attempt) {
            std::string msg;
            try { wo::regrow_group(b, C, 1024, halfway); } catch (const wo::HipError& e) { msg = e.msg; }
            CHECK(msg == "out of memory half-way");                // (and not the arena's refusal to release a buffer that is not its own)
            CHECK(half == attempt && !C.built && C.cap == 0 && !C.deps && !C.depCnt && live_bytes() == 0);
        }
        auto& T = b.tiles;
        try { wo::build_group(b, T, [&](wo::DeviceArena&) { T.lr = &somewhere; throw wo::HipError{"half-way"}; }); } catch (const wo::HipError&) {}
        CHECK(!T.built && !T.lr);
    }
    {
        wo_erode_block b;
        auto& T = b.tiles;
        auto tiles = [&](wo::DeviceArena& a) { ++runs; T.parent = a.dev<int32_t>(N); T.inflow = a.dev<uint32_t>(N); T.lr = a.dev<int32_t>(N); };
        for (int attempt = 1; attempt <= 2; ++attempt) {
            try { wo::build_group(b, T, tiles); } catch (const wo::HipError& e) { threw = true; if (attempt == 1) std::printf("builder threw: %s\n", e.msg.c_str()); }
            CHECK(runs == attempt || !threw);                  // a failed attempt does not keep the next one from starting again
            if (!threw) break;
            CHECK(!T.built && live_bytes() == 0);
        }
        if (threw) {
            // the pinned side of the arena, and a builder that gives up by itself after its allocations would have been made
            try { wo::build_group(b, b.scratch, [&](wo::DeviceArena& a) { b.scratch.h_patchTotals = a.pinned<int32_t>(4096); }); } catch (const wo::HipError&) {}
            CHECK(!b.scratch.built && live_bytes() == 0);
            try { wo::build_group(b, b.redo, [&](wo::DeviceArena&) { throw wo::HipError{"gave up"}; }); } catch (const wo::HipError&) {}
            CHECK(!b.redo.built && live_bytes() == 0);
            // the regrown group: a failed regrow leaves capacity 0, and a second one too
            auto& C = b.carve;
            for (int attempt = 1; attempt <= 2; ++attempt) {
                bool regrowThrew = false;
                try { wo::regrow_group(b, C, 1024, [&](wo::DeviceArena& a) { C.deps = a.dev<int32_t>(1024 * wo::WO_CARVE_DEPS); C.recs = a.dev<wo::CarveRec>(1024); }); }
                catch (const wo::HipError&) { regrowThrew = true; }
                CHECK(regrowThrew && !C.built && C.cap == 0 && !C.recs && live_bytes() == 0);
            }
        } else {
            CHECK(T.built && runs == 1 && live_bytes() == (int64_t)(3 * N * 4));
            wo::build_group(b, T, tiles);                      // built: the builder does not run again
            CHECK(runs == 1);
        }
    }                                                          // the block goes: its arena frees what it holds
    CHECK(live_bytes() == 0);
    if (!threw) std::printf("erode_block_main: a device is present, the allocations succeeded: the failure path was NOT exercised\n");
    std::printf(failures ? "erode_block_main: %d checks FAILED\n" : "erode_block_main: all checks passed\n", failures);
    return failures ? 1 : 0;
}
