// Test-only CPU emulator of the ocean-current stage: drives the bodies of csrc/ocean_ops.h cell by cell in the loop order of
// the reference (js/ocean.js:204-382): per season the band loop, the masked smooth of currentE and then of currentN (one
// field at a time), classifyWarmth and its smooth, the speeds, the percentile (a sort) and the normalisation.  The
// distance fields come from a plain FIFO queue (orderSeed 0), or from a level-synchronous walk whose seed list and
// frontiers are shuffled by `orderSeed`, which stands for the interleaving of the device's threads; `maxDepth` < 0 runs
// them to exhaustion as the reference does, otherwise cells farther than maxDepth stay at -1 as on the device.
// Never linked into the product.
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../planet_heightmap_generation_amd/csrc/ocean_ops.h"

namespace O = wo::ocean;
namespace W = wo::wind;

namespace {

struct Rng {                                                  // splitmix64
    uint64_t s;
    uint64_t next() { uint64_t z = (s += 0x9E3779B97F4A7C15ull); z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31); }
};
void shuffle(std::vector<int32_t>& v, uint64_t seed) {
    Rng g{seed};
    for (size_t i = v.size(); i > 1; --i) std::swap(v[i - 1], v[g.next() % i]);
}

void bfs(int32_t N, const int32_t* off, const int32_t* adj, const uint8_t* isOcean, std::vector<int32_t> seeds, int32_t maxDepth, uint64_t orderSeed, int32_t* dist) {
    for (int32_t r = 0; r < N; ++r) dist[r] = -1;
    if (orderSeed == 0) {                                     // bfsDistance (:58-80)
        std::vector<int32_t> queue;
        for (int32_t s : seeds) { dist[s] = 0; queue.push_back(s); }
        for (size_t head = 0; head < queue.size(); ++head) {
            const int32_t r = queue[head], d = dist[r] + 1;
            if (maxDepth >= 0 && d > maxDepth) continue;
            for (int32_t ni = off[r]; ni < off[r + 1]; ++ni) {
                const int32_t nb = adj[ni];
                if (isOcean[nb] && dist[nb] == -1) { dist[nb] = d; queue.push_back(nb); }
            }
        }
        return;
    }
    std::vector<int32_t> cur = std::move(seeds), next;
    for (int32_t s : cur) dist[s] = 0;
    for (int32_t level = 1; !cur.empty() && (maxDepth < 0 || level <= maxDepth); ++level) {
        shuffle(cur, orderSeed + (uint64_t)level);
        next.clear();
        for (int32_t r : cur)
            for (int32_t ni = off[r]; ni < off[r + 1]; ++ni) {
                const int32_t nb = adj[ni];
                if (isOcean[nb] && dist[nb] == -1) { dist[nb] = level; next.push_back(nb); }
            }
        cur.swap(next);
    }
}

void smooth(int32_t N, const int32_t* off, const int32_t* adj, const uint8_t* isOcean, float* field, int32_t passes) {
    std::vector<float> tmp(N);
    const O::Group<1>* f = reinterpret_cast<const O::Group<1>*>(field);
    for (int32_t p = 0; p < passes; ++p) {
        for (int32_t r = 0; r < N; ++r) tmp[r] = O::smooth_ocean_cell<1>(off, adj, isOcean, f, r).v[0];
        std::memcpy(field, tmp.data(), (size_t)N * 4);
    }
}

}  // namespace

extern "C" {

// out: the eight result arrays in the order of ocean.py's RESULT_FIELDS.  info: circumpolarNH, circumpolarSH, coastThreshold,
// warmthRange, currentPasses, warmthPasses, oceanCells summer / winter; p95: summer, winter.  dist2 (may be NULL): 2 x N,
// the west and the east distance field.
void emu_ocean(int32_t N, const int32_t* off, const int32_t* adj, const float* xyz, const float* lat, const float* lon, const uint8_t* isLand,
               const float* eastX, const float* eastY, const float* eastZ, const float* itczSummer, const float* itczWinter, int32_t maxDepth,
               uint64_t orderSeed, void** out, int32_t* info, float* p95, int32_t* dist2) {
    std::vector<uint8_t> isOcean(N);
    for (int32_t r = 0; r < N; ++r) isOcean[r] = isLand[r] ? 0 : 1;
    // step 1: the seeds and the two distance fields
    std::vector<int32_t> west, east, wDist(N), eDist(N);
    for (int32_t r = 0; r < N; ++r) {
        const int s = O::coast_seed_cell(isOcean.data(), off, adj, xyz, eastX, eastY, eastZ, r);
        if (s == O::SEED_WEST) west.push_back(r);
        else if (s == O::SEED_EAST) east.push_back(r);
    }
    if (orderSeed) { shuffle(west, orderSeed * 5 + 1); shuffle(east, orderSeed * 7 + 3); }
    bfs(N, off, adj, isOcean.data(), west, maxDepth, orderSeed, wDist.data());
    bfs(N, off, adj, isOcean.data(), east, maxDepth, orderSeed ? orderSeed + 1000 : 0, eDist.data());
    if (dist2) { std::memcpy(dist2, wDist.data(), (size_t)N * 4); std::memcpy(dist2 + N, eDist.data(), (size_t)N * 4); }
    // step 2: circumpolar channels
    uint8_t bins[2 * O::CIRC_BINS] = {0};
    for (int32_t r = 0; r < N; ++r) { const int32_t b = O::circumpolar_bin(isOcean[r] != 0, lat[r], lon[r]); if (b >= 0) bins[b] = 1; }
    bool circ[2] = {true, true};
    for (int h = 0; h < 2; ++h) for (int i = 0; i < O::CIRC_BINS; ++i) if (!bins[h * O::CIRC_BINS + i]) circ[h] = false;
    const O::Params P = O::params_for(N);
    info[0] = circ[0]; info[1] = circ[1]; info[2] = P.coastThreshold; info[3] = P.warmthRange; info[4] = P.currentPasses; info[5] = P.warmthPasses;
    for (int s = 0; s < 2; ++s) {
        float *currentE = (float*)out[4 * s], *currentN = (float*)out[4 * s + 1], *speed = (float*)out[4 * s + 2], *warmth = (float*)out[4 * s + 3];
        const double shift = s == 0 ? 5 : -5;
        const float* itcz = s == 0 ? itczSummer : itczWinter;
        for (int32_t r = 0; r < N; ++r) {
            currentE[r] = 0.0f; currentN[r] = 0.0f;
            if (isOcean[r]) O::current_cell(lat[r], lon[r], wDist[r], eDist[r], P.coastThreshold, circ[0], circ[1], shift, itcz, currentE[r], currentN[r]);
        }
        smooth(N, off, adj, isOcean.data(), currentE, P.currentPasses);
        smooth(N, off, adj, isOcean.data(), currentN, P.currentPasses);
        for (int32_t r = 0; r < N; ++r) if (!isOcean[r]) { currentE[r] = 0.0f; currentN[r] = 0.0f; }
        for (int32_t r = 0; r < N; ++r) warmth[r] = isOcean[r] ? O::warmth_cell(lat[r], wDist[r], eDist[r], P.warmthRange, shift) : 0.0f;
        smooth(N, off, adj, isOcean.data(), warmth, P.warmthPasses);
        std::vector<float> oceanSpeeds;
        for (int32_t r = 0; r < N; ++r) {
            const double spd = O::speed_of(currentE[r], currentN[r]);
            speed[r] = (float)spd;
            if (O::speed_counts(isOcean[r] != 0, spd)) oceanSpeeds.push_back((float)spd);
        }
        std::sort(oceanSpeeds.begin(), oceanSpeeds.end());
        const uint32_t n = (uint32_t)oceanSpeeds.size();
        const float q = O::p95_of(n, n ? W::sel_key(oceanSpeeds[O::percentile_rank(n)]) : 0u);
        for (int32_t r = 0; r < N; ++r) speed[r] = W::normalise_speed_cell(speed[r], q);
        info[6 + s] = (int32_t)n;
        p95[s] = q;
    }
}

}  // extern "C"
