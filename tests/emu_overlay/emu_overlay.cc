// Test-only CPU emulator: the bodies of csrc/overlay_ops.h (the bin and d2 of a region, the 64-bit key, the arrow) compiled for the
// host, behind a C interface that tests/overlay_common.py loads with ctypes.  The winners come in two forms: the reference's
// sequential loop over a Float32Array of minima, and the minimum of the keys.  Plain loops in index order: the compaction is a
// counter.  It shares no scheduling with the kernels of csrc/overlay.hip.
#include <cstdint>
#include <vector>

#include "../../planet_heightmap_generation_amd/csrc/overlay_ops.h"

using namespace wo::overlay;

extern "C" {

// the bin (-1: none) and d2 of every region; e is read with skipLand only
void emu_overlay_candidates(int32_t N, const float* xyz, const float* e, int32_t skipLand, int32_t* idx, double* d2) {
    for (int32_t r = 0; r < N; ++r) {
        Bin b{-1, 0.0};
        if (takes_part(skipLand != 0, skipLand ? e[r] : 0.0f)) b = bin_of(xyz[3 * (int64_t)r], xyz[3 * (int64_t)r + 1], xyz[3 * (int64_t)r + 2]);
        idx[r] = b.idx; d2[r] = b.d2;
    }
}

// the reference's loop (js/planet-mesh.js:1322-1345) over candidates (idx[r] in [0, bins) or negative, d2[r])
void emu_overlay_pick_loop(int32_t n, const int32_t* idx, const double* d2, int32_t bins, int32_t* winners) {
    std::vector<float> gridDist2(bins, 1e9f);
    for (int32_t i = 0; i < bins; ++i) winners[i] = -1;
    for (int32_t r = 0; r < n; ++r) {
        if (idx[r] < 0) continue;
        if (d2[r] < (double)gridDist2[idx[r]]) {
            gridDist2[idx[r]] = (float)d2[r];
            winners[idx[r]] = r;
        }
    }
}

// the minimum of the keys, taken in descending index order to share nothing with the loop
void emu_overlay_pick_keys(int32_t n, const int32_t* idx, const double* d2, int32_t bins, int32_t* winners) {
    std::vector<unsigned long long> keys(bins, EMPTY_KEY);
    for (int32_t r = n - 1; r >= 0; --r) {
        if (idx[r] < 0) continue;
        const unsigned long long k = key_of(d2[r], r);
        if (k < keys[idx[r]]) keys[idx[r]] = k;
    }
    for (int32_t i = 0; i < bins; ++i) winners[i] = winner_of_key(keys[i]);
}

// the arrows of the kept bins in ascending bin order; speed and warmth are read by the ocean form only; any output may be NULL;
// returns the number of arrows
int64_t emu_overlay_arrows(int32_t kind, const float* xyz, const int32_t* winners, const float* a, const float* b, const float* speed, const float* warmth, double centerLon,
                           float* globePos, float* globeCol, float* mapPos, float* mapCol) {
    int64_t n = 0;
    for (int32_t i = 0; i < BINS; ++i) {
        const int32_t r = winners[i];
        if (r < 0) continue;
        Source src{a[r], b[r], 0.0f, 0.0f};
        if (kind == KIND_OCEAN) { src.speed = speed[r]; src.warmth = warmth[r]; }
        if (is_slow(kind, speed_of(kind, src))) continue;
        const int64_t o = n * ARROW_FLOATS;
        arrow(kind, xyz + 3 * (int64_t)r, src, centerLon, globePos ? globePos + o : nullptr, globeCol ? globeCol + o : nullptr, mapPos ? mapPos + o : nullptr,
              mapCol ? mapCol + o : nullptr);
        ++n;
    }
    return n;
}

}  // extern "C"
