// Test-only CPU emulator of the wind stage: drives the bodies of csrc/wind_ops.h cell by cell in the order of the stage in
// csrc/wind.hip, with glibc's libm (libemu_wind.so) or the perturbation hook of tests/emu (libemu_wind_libm.so).
// The order-free parts (union-find hooks, BFS claims inside a level) run in an order drawn from `orderSeed` (0: ascending),
// which stands for the interleaving of the device's threads.  The bin sort is a plain stable counting sort and the disc
// samples add in bin-then-cell order, as the reference does.  Never linked into the product.
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <numeric>
#include <vector>

#include "../../planet_heightmap_generation_amd/csrc/erode_ops.h"
#include "../../planet_heightmap_generation_amd/csrc/wind_ops.h"

namespace W = wo::wind;

namespace {

struct Rng {                                                  // splitmix64
    uint64_t s;
    uint64_t next() { uint64_t z = (s += 0x9E3779B97F4A7C15ull); z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31); }
};
void shuffle(std::vector<int32_t>& v, uint64_t seed) {
    if (seed == 0) return;
    Rng g{seed};
    for (size_t i = v.size(); i > 1; --i) std::swap(v[i - 1], v[g.next() % i]);
}

void components(int32_t N, const int32_t* off, const int32_t* adj, const uint8_t* isLand, uint64_t orderSeed, std::vector<int32_t>& label, int32_t& mainRoot) {
    label.resize(N);
    std::vector<int32_t> order(N), size(N, 0);
    std::iota(order.begin(), order.end(), 0);
    for (int32_t r = 0; r < N; ++r) label[r] = r;
    shuffle(order, orderSeed);
    for (int32_t r : order) W::cc_hook_ocean_cell(label.data(), isLand, off, adj, r);
    shuffle(order, orderSeed * 3 + 1);
    for (int32_t r : order) wo::imp::cc_flatten_cell(label.data(), r);
    for (int32_t r = 0; r < N; ++r) if (!isLand[r]) ++size[label[r]];
    unsigned long long key = 0;
    for (int32_t r : order) if (!isLand[r] && label[r] == r) key = std::max(key, W::main_ocean_key(size[r], r));
    mainRoot = W::main_ocean_root(key);
}

// level-synchronous BFS over the cells with mask == want, frontier processed in a drawn order; returns the level count
int32_t bfs(int32_t N, const int32_t* off, const int32_t* adj, const std::vector<uint8_t>& seed, const uint8_t* mask, uint8_t want, uint64_t orderSeed, int32_t* dist) {
    std::vector<int32_t> cur, next;
    for (int32_t r = 0; r < N; ++r) { dist[r] = seed[r] ? 0 : -1; if (seed[r]) cur.push_back(r); }
    int32_t level = 0;
    for (; !cur.empty(); ++level) {
        shuffle(cur, orderSeed ? orderSeed + level : 0);
        next.clear();
        for (int32_t r : cur)
            for (int32_t j = off[r]; j < off[r + 1]; ++j) {
                const int32_t nb = adj[j];
                if (mask[nb] == want && dist[nb] == -1) { dist[nb] = level + 1; next.push_back(nb); }
            }
        cur.swap(next);
    }
    return level;
}

void smooth(int32_t N, const int32_t* off, const int32_t* adj, std::vector<float>& f, int32_t passes) {
    wo::Fields F{};
    F.N = N; F.off = off; F.adj = adj;
    std::vector<float> tmp(N);
    for (int32_t p = 0; p < passes; ++p) {
        for (int32_t r = 0; r < N; ++r) tmp[r] = wo::smooth_field_cell(F, f.data(), r);
        f.swap(tmp);
    }
}

float percentile95(const float* v, int32_t n) {
    W::SelState S{0u, W::percentile_index(n, 0.95)};
    std::vector<uint32_t> hist(W::SEL_BINS);
    for (int pass = 0; pass < W::SEL_PASSES; ++pass) {
        std::fill(hist.begin(), hist.end(), 0u);
        for (int32_t r = 0; r < n; ++r) { const uint32_t k = W::sel_key(v[r]); if (W::sel_matches(k, S.prefix, pass)) ++hist[W::sel_digit(k, pass)]; }
        W::sel_pick(S, hist.data(), pass);
    }
    return W::max_speed_of(S.prefix);
}

void plate_ocean_flags(int32_t N, const int32_t* plate, const int32_t* oceanIds, int32_t nOcean, std::vector<uint8_t>& flags) {
    std::vector<int32_t> ids(oceanIds, oceanIds + nOcean);
    std::sort(ids.begin(), ids.end());
    ids.erase(std::unique(ids.begin(), ids.end()), ids.end());
    flags.resize(N);
    for (int32_t r = 0; r < N; ++r) flags[r] = W::id_in_sorted(ids.data(), (int32_t)ids.size(), plate[r]) ? 1 : 0;
}

}  // namespace

extern "C" {

// 95th percentile as computeWind takes it (`|| 1` included)
float emu_wind_percentile(const float* v, int32_t n) { return percentile95(v, n); }

// the order-free parts alone: ocean labels (-1 on land), the main ocean's label, both distance fields
void emu_wind_graph(int32_t N, const int32_t* off, const int32_t* adj, const float* e, const int32_t* plate, const int32_t* oceanIds, int32_t nOcean,
                    uint64_t orderSeed, int32_t* labelOut, int32_t* mainRootOut, int32_t* coastDist, int32_t* plateDist) {
    std::vector<uint8_t> isLand(N), plateOcean, seed(N);
    for (int32_t r = 0; r < N; ++r) isLand[r] = e[r] > 0.0f ? 1 : 0;
    std::vector<int32_t> label;
    int32_t mainRoot;
    components(N, off, adj, isLand.data(), orderSeed, label, mainRoot);
    for (int32_t r = 0; r < N; ++r) labelOut[r] = isLand[r] ? -1 : label[r];
    *mainRootOut = mainRoot;
    for (int32_t r = 0; r < N; ++r) seed[r] = W::coast_seed_cell(isLand.data(), label.data(), mainRoot, off, adj, r);
    bfs(N, off, adj, seed, isLand.data(), 1, orderSeed, coastDist);
    plate_ocean_flags(N, plate, oceanIds, nOcean, plateOcean);
    for (int32_t r = 0; r < N; ++r) seed[r] = W::plate_seed_cell(plateOcean.data(), off, adj, r);
    bfs(N, off, adj, seed, plateOcean.data(), 0, orderSeed, plateDist);
}

// the whole stage.  out: 24 arrays in the order of wind.py's RESULT_FIELDS; levels2: BFS levels (coast, plates)
void emu_wind(int32_t N, const int32_t* off, const int32_t* adj, const float* xyz, const float* e, const int32_t* plate, const int32_t* oceanIds,
              int32_t nOcean, double seed, uint64_t orderSeed, void** out, int32_t* levels2) {
    float* season[2][4];
    for (int s = 0; s < 2; ++s) for (int k = 0; k < 4; ++k) season[s][k] = (float*)out[s * 4 + k];
    float *itczLons = (float*)out[8], *itczS = (float*)out[9], *itczW = (float*)out[10];
    float *lat = (float*)out[11], *lon = (float*)out[12], *sinLat = (float*)out[13];
    uint8_t* isLand = (uint8_t*)out[14];
    float *cont = (float*)out[15], *plateCont = (float*)out[17];
    int32_t* coastDist = (int32_t*)out[16];
    std::vector<float> cosLat(N);
    W::CellGeo G{lat, lon, sinLat, cosLat.data(), isLand, (float*)out[18], (float*)out[19], (float*)out[20], (float*)out[21], (float*)out[22], (float*)out[23]};
    for (int32_t r = 0; r < N; ++r) W::precompute_cell(xyz, e, G, r);
    // geo index: stable counting sort by bin
    std::vector<int32_t> bin(N), binOffset(W::NUM_BINS + 1, 0), cells(N);
    for (int32_t r = 0; r < N; ++r) { bin[r] = W::bin_of(lat[r], lon[r]); ++binOffset[bin[r] + 1]; }
    for (int b = 0; b < W::NUM_BINS; ++b) binOffset[b + 1] += binOffset[b];
    { std::vector<int32_t> fill(binOffset.begin(), binOffset.end() - 1); for (int32_t r = 0; r < N; ++r) cells[fill[bin[r]]++] = r; }
    // disc samples
    std::vector<W::SampleSpec> specs(W::NUM_SAMPLES);
    std::vector<W::SampleAcc> acc(W::NUM_SAMPLES);
    W::make_sample_specs(specs.data());
    for (int i = 0; i < W::NUM_SAMPLES; ++i) {
        const W::SampleSpec& S = specs[i];
        W::SampleAcc A{0.0, 0, 0};
        for (int32_t bi = S.bMin; bi <= S.bMax; ++bi)
            for (int32_t li = S.lMin; li <= S.lMax; ++li) {
                const int32_t b = W::sample_bin(bi, li);
                for (int32_t k = binOffset[b]; k < binOffset[b + 1]; ++k) {
                    const int32_t r = cells[k];
                    if (!W::sample_member(S, sinLat[r], cosLat[r], lon[r])) continue;
                    ++A.totalCount;
                    if (isLand[r]) ++A.landCount;
                    A.elevSum += W::js_max(0, (double)e[r]);
                }
            }
        acc[i] = A;
    }
    W::Spline splines[2];
    W::itcz_finish(acc.data(), splines, itczLons, itczS, itczW);
    // continentality
    std::vector<int32_t> label, plateDist(N);
    int32_t mainRoot;
    components(N, off, adj, isLand, orderSeed, label, mainRoot);
    std::vector<uint8_t> seedFlag(N), plateOcean;
    for (int32_t r = 0; r < N; ++r) seedFlag[r] = W::coast_seed_cell(isLand, label.data(), mainRoot, off, adj, r);
    levels2[0] = bfs(N, off, adj, seedFlag, isLand, 1, orderSeed, coastDist);
    plate_ocean_flags(N, plate, oceanIds, nOcean, plateOcean);
    for (int32_t r = 0; r < N; ++r) seedFlag[r] = W::plate_seed_cell(plateOcean.data(), off, adj, r);
    levels2[1] = bfs(N, off, adj, seedFlag, plateOcean.data(), 0, orderSeed, plateDist.data());
    const double avgEdgeKm = W::avg_edge_km(N);
    const int32_t contPasses = W::js_round_passes(100 / avgEdgeKm), pressPasses = W::js_round_passes(75 / avgEdgeKm);
    std::vector<float> f(N);
    for (int32_t r = 0; r < N; ++r) f[r] = W::continentality_cell(coastDist[r], isLand[r] == 1, avgEdgeKm);
    smooth(N, off, adj, f, contPasses);
    std::memcpy(cont, f.data(), (size_t)N * 4);
    for (int32_t r = 0; r < N; ++r) f[r] = W::continentality_cell(plateDist[r], plateOcean[r] == 0, avgEdgeKm);
    smooth(N, off, adj, f, contPasses);
    std::memcpy(plateCont, f.data(), (size_t)N * 4);
    // the seasons
    uint8_t t[1024];
    wo::noise_tables(seed, t, t + 512);
    W::Frames T{G.eastX, G.eastY, G.eastZ, G.northX, G.northY, G.northZ};
    std::vector<float> gradE(N), gradN(N);
    for (int s = 0; s < 2; ++s) {
        for (int32_t r = 0; r < N; ++r)
            f[r] = W::region_pressure_cell(lat[r], lon[r], splines[s], s == 0 ? 1 : -1, cont[r], e[r], t, t + 512, xyz[3 * (int64_t)r], xyz[3 * (int64_t)r + 1], xyz[3 * (int64_t)r + 2]);
        smooth(N, off, adj, f, pressPasses);
        for (int32_t r = 0; r < N; ++r) W::gradient_cell(off, adj, xyz, f.data(), T, gradE.data(), gradN.data(), r);
        for (int32_t r = 0; r < N; ++r) W::wind_cell(gradE.data(), gradN.data(), sinLat, season[s][1], season[s][2], season[s][3], r);
        const float maxSpeed = percentile95(season[s][3], N);
        for (int32_t r = 0; r < N; ++r) { season[s][3][r] = W::normalise_speed_cell(season[s][3][r], maxSpeed); season[s][0][r] = W::pressure_dev_cell(f[r]); }
    }
}

}  // extern "C"
