// Seasonal pressure and wind on the device (js/wind.js:394-687), on the planet's resident mesh and stream.  The per-cell
// bodies and the exactness contract are in wind_ops.h; the results stay on the device in the planet's wind block.
//
// Launch sequence (every buffer is allocated before it; two host round trips: the 576 disc samples come back for the ITCZ
// spline, a few hundred flops of host arithmetic, and each BFS level brings its frontier length back):
//   precompute      k_wind_precompute             lat / lon / sin / cos / isLand / tangent frames, and the cell's bin
//   geo index       radix_sort_pairs (radix.hip)  stable sort of the cells by bin: a bin lists its cells in ascending id
//                   k_wind_bin_offsets            bin -> first position, from the sorted keys (no atomics)
//   ITCZ            k_wind_sample                 one wave per disc sample: the lanes test membership, the adds of elevSum
//                                                 are replayed in lane order (the reference's bin-then-cell order)
//   continentality  k_wind_cc_*                   ocean components by union-find, their sizes, the main ocean
//                   k_wind_bfs_seed / _level      hop distance through land from the main ocean's coast, and through the
//                                                 continental plates from the oceanic ones (level-synchronous, claims by CAS)
//                   k_wind_continentality, k_smooth_field
//   per season      k_wind_pressure, k_smooth_field, k_wind_gradient, k_wind_vectors,
//                   k_wind_sel_hist / _pick x 3   the 95th percentile of the speed as a histogram select
//                   k_wind_finish                 normalised speed and pressure - 1013
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../include/worogen.h"
#include "block_ops.h"
#include "device.h"
#include "wind_block.h"
#include "wind_ops.h"

namespace W = wo::wind;

namespace wo {

#define WIND_CELLS(r, n) const int32_t r = blockIdx.x * blockDim.x + threadIdx.x; if (r < (n))

__global__ __launch_bounds__(WO_BLOCK) void k_wind_precompute(const float* __restrict__ xyz, const float* __restrict__ e, W::CellGeo G, uint32_t* __restrict__ key,
                                                              int32_t* __restrict__ val, int32_t N) {
    WIND_CELLS(r, N) {
        W::precompute_cell(xyz, e, G, r);
        key[r] = (uint32_t)W::bin_of(G.lat[r], G.lon[r]);
        val[r] = r;
    }
}

// sorted keys -> binOffset[0 .. NUM_BINS]: position i opens every bin in (key[i - 1], key[i]]; the end closes the rest
__global__ __launch_bounds__(WO_BLOCK) void k_wind_bin_offsets(const uint32_t* __restrict__ key, int32_t N, int32_t* __restrict__ binOffset) {
    const int32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i > N) return;
    const int32_t lo = i == 0 ? 0 : (int32_t)std::min<uint32_t>(key[i - 1], W::NUM_BINS - 1) + 1;
    const int32_t hi = i == N ? W::NUM_BINS : (int32_t)std::min<uint32_t>(key[i], W::NUM_BINS - 1);
    for (int32_t b = lo; b <= hi; ++b) binOffset[b] = i;
}

// one wave per disc sample (:126-163)
__global__ __launch_bounds__(64) void k_wind_sample(const W::SampleSpec* __restrict__ specs, const int32_t* __restrict__ binOffset, const int32_t* __restrict__ cells,
                                                    const float* __restrict__ sinLat, const float* __restrict__ cosLat, const float* __restrict__ lon,
                                                    const uint8_t* __restrict__ isLand, const float* __restrict__ e, W::SampleAcc* __restrict__ acc) {
    const W::SampleSpec S = specs[blockIdx.x];
    const int lane = threadIdx.x;
    double elevSum = 0;
    int32_t landCount = 0, totalCount = 0;
    for (int32_t bi = S.bMin; bi <= S.bMax; ++bi)
        for (int32_t li = S.lMin; li <= S.lMax; ++li) {
            const int32_t bin = W::sample_bin(bi, li);
            const int32_t start = binOffset[bin], end = binOffset[bin + 1];
            for (int32_t k0 = start; k0 < end; k0 += 64) {
                const int32_t k = k0 + lane;
                bool member = false, land = false;
                float ev = 0.0f;
                if (k < end) {
                    const int32_t r = cells[k];
                    member = W::sample_member(S, sinLat[r], cosLat[r], lon[r]);
                    if (member) { land = isLand[r] != 0; ev = e[r]; }
                }
                totalCount += (int32_t)__popcll(__ballot(member));
                landCount += (int32_t)__popcll(__ballot(land));
                unsigned long long add = __ballot(member && !(ev <= 0.0f));      // Math.max(0, e) is +0 for e <= 0: adding it changes nothing
                while (add) {
                    const int src = __ffsll((long long)add) - 1;
                    elevSum += (double)__shfl(ev, src);
                    add &= add - 1;
                }
            }
        }
    if (lane == 0) { acc[blockIdx.x].elevSum = elevSum; acc[blockIdx.x].landCount = landCount; acc[blockIdx.x].totalCount = totalCount; }
}

// ---- ocean components ----
__global__ __launch_bounds__(WO_BLOCK) void k_wind_cc_init(int32_t* __restrict__ parent, int32_t* __restrict__ compSize, const int32_t* __restrict__ plate,
                                                           const int32_t* __restrict__ oceanIds, int32_t nOcean, uint8_t* __restrict__ plateOcean, int32_t N) {
    WIND_CELLS(r, N) { parent[r] = r; compSize[r] = 0; plateOcean[r] = W::id_in_sorted(oceanIds, nOcean, plate[r]) ? 1 : 0; }
}
__global__ __launch_bounds__(WO_BLOCK) void k_wind_cc_hook(int32_t* parent, const uint8_t* __restrict__ isLand, const int32_t* __restrict__ off,
                                                           const int32_t* __restrict__ adj, int32_t N) {
    WIND_CELLS(r, N) W::cc_hook_ocean_cell(parent, isLand, off, adj, r);
}
__global__ __launch_bounds__(WO_BLOCK) void k_wind_cc_flatten(int32_t* parent, int32_t N) {
    WIND_CELLS(r, N) imp::cc_flatten_cell(parent, r);
}
// component sizes: one add per wave for the lanes that share the first lane's label (neighbouring ids mostly do)
__global__ __launch_bounds__(WO_BLOCK) void k_wind_cc_size(const int32_t* __restrict__ label, const uint8_t* __restrict__ isLand, int32_t* compSize, int32_t N) {
    const int32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    const int32_t l = (r < N && !isLand[r]) ? label[r] : -1;
    const unsigned long long have = __ballot(l >= 0);
    if (!have) return;
    const int leader = __ffsll((long long)have) - 1;
    const int32_t first = __shfl(l, leader);
    const unsigned long long same = __ballot(l == first);
    const int lane = threadIdx.x & 63;
    if (lane == leader) atomicAdd(&compSize[first], (int32_t)__popcll(same));
    else if (l >= 0 && l != first) atomicAdd(&compSize[l], 1);
}
__global__ __launch_bounds__(WO_BLOCK) void k_wind_cc_main(const int32_t* __restrict__ label, const uint8_t* __restrict__ isLand, const int32_t* __restrict__ compSize,
                                                           unsigned long long* mainKey, int32_t N) {
    WIND_CELLS(r, N) if (!isLand[r] && label[r] == r) atomicMax(mainKey, W::main_ocean_key(compSize[r], r));
}

// level 0 of a distance field: mode 0 coast (land cells that touch the main ocean), mode 1 plates
__global__ __launch_bounds__(WO_BLOCK) void k_wind_bfs_seed(int32_t mode, const uint8_t* __restrict__ isLand, const int32_t* __restrict__ label,
                                                            const unsigned long long* __restrict__ mainKey, const uint8_t* __restrict__ plateOcean,
                                                            const int32_t* __restrict__ off, const int32_t* __restrict__ adj, int32_t* __restrict__ dist,
                                                            int32_t* __restrict__ list, int32_t* counter, int32_t N) {
    const int32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    bool seed = false;
    if (r < N) {
        seed = mode == 0 ? W::coast_seed_cell(isLand, label, W::main_ocean_root(*mainKey), off, adj, r) : W::plate_seed_cell(plateOcean, off, adj, r);
        dist[r] = seed ? 0 : -1;
    }
    wave_append(seed, r, list, counter);
}
// one level: frontier cells claim their unreached neighbours inside the region (mask[nb] == want) by CAS -1 -> level
__global__ __launch_bounds__(WO_BLOCK) void k_wind_bfs_level(const int32_t* __restrict__ cur, int32_t n, const uint8_t* __restrict__ mask, uint8_t want,
                                                             const int32_t* __restrict__ off, const int32_t* __restrict__ adj, int32_t* dist, int32_t level,
                                                             int32_t* __restrict__ next, int32_t* nextCount, int32_t* zeroCount) {
    const int32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i == 0) *zeroCount = 0;
    const int32_t r = i < n ? cur[i] : 0;
    const int32_t b = i < n ? off[r] : 0, deg = i < n ? off[r + 1] - b : 0;
    for (int32_t k = 0; __any(k < deg); ++k) {                // the wave stays together for wave_append
        bool claim = false; int32_t nb = -1;
        if (k < deg) {
            nb = adj[b + k];
            claim = mask[nb] == want && dist[nb] == -1 && atomicCAS(&dist[nb], -1, level) == -1;
        }
        wave_append(claim, nb, next, nextCount);
    }
}

__global__ __launch_bounds__(WO_BLOCK) void k_wind_continentality(const int32_t* __restrict__ dist, const uint8_t* __restrict__ mask, uint8_t want, double avgEdgeKm,
                                                                  float* __restrict__ out, int32_t N) {
    WIND_CELLS(r, N) out[r] = W::continentality_cell(dist[r], mask[r] == want, avgEdgeKm);
}

// ---- per season ----
__global__ __launch_bounds__(WO_BLOCK) void k_wind_pressure(const uint8_t* __restrict__ tables, const W::Spline* __restrict__ spline, int32_t seasonSign,
                                                            const float* __restrict__ lat, const float* __restrict__ lon, const float* __restrict__ cont,
                                                            const float* __restrict__ e, const float* __restrict__ xyz, float* __restrict__ out, int32_t N) {
    __shared__ uint8_t sP[512], sM[512];
    __shared__ W::Spline S;
    for (int i = threadIdx.x; i < 512; i += blockDim.x) { sP[i] = tables[i]; sM[i] = tables[512 + i]; }
    for (int i = threadIdx.x; i < (int)(sizeof(W::Spline) / sizeof(double)); i += blockDim.x) reinterpret_cast<double*>(&S)[i] = reinterpret_cast<const double*>(spline)[i];
    __syncthreads();
    WIND_CELLS(r, N)
        out[r] = W::region_pressure_cell(lat[r], lon[r], S, seasonSign, cont[r], e[r], sP, sM, xyz[3 * (int64_t)r], xyz[3 * (int64_t)r + 1], xyz[3 * (int64_t)r + 2]);
}
__global__ __launch_bounds__(WO_BLOCK) void k_wind_gradient(const int32_t* __restrict__ off, const int32_t* __restrict__ adj, const float* __restrict__ xyz,
                                                            const float* __restrict__ pressure, W::Frames T, float* __restrict__ gradE, float* __restrict__ gradN, int32_t N) {
    WIND_CELLS(r, N) W::gradient_cell(off, adj, xyz, pressure, T, gradE, gradN, r);
}
__global__ __launch_bounds__(WO_BLOCK) void k_wind_vectors(const float* __restrict__ gradE, const float* __restrict__ gradN, const float* __restrict__ sinLat,
                                                           float* __restrict__ windE, float* __restrict__ windN, float* __restrict__ speed, int32_t N) {
    WIND_CELLS(r, N) W::wind_cell(gradE, gradN, sinLat, windE, windN, speed, r);
}

// histogram of one digit over the values that agree with the digits already chosen (LDS counts, one flush per block)
__global__ __launch_bounds__(WO_BLOCK) void k_wind_sel_hist(const float* __restrict__ v, int32_t N, int32_t pass, const W::SelState* __restrict__ state, uint32_t* hist) {
    __shared__ uint32_t s[W::SEL_BINS];
    for (int i = threadIdx.x; i < W::SEL_BINS; i += blockDim.x) s[i] = 0;
    __syncthreads();
    const uint32_t prefix = state->prefix;
    for (int32_t r = blockIdx.x * blockDim.x + threadIdx.x; r < N; r += gridDim.x * blockDim.x) {
        const uint32_t key = W::sel_key(v[r]);
        if (W::sel_matches(key, prefix, pass)) atomicAdd(&s[W::sel_digit(key, pass)], 1u);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < W::SEL_BINS; i += blockDim.x) if (s[i]) atomicAdd(&hist[i], s[i]);
}
// one thread: choose the digit, clear the histogram for the next pass; after the last pass the selected value
__global__ void k_wind_sel_pick(W::SelState* state, uint32_t* hist, int32_t pass, float* maxSpeed) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    W::SelState S = *state;
    W::sel_pick(S, hist, pass);
    *state = S;
    for (int i = 0; i < W::SEL_BINS; ++i) hist[i] = 0;
    if (pass == W::SEL_PASSES - 1) *maxSpeed = W::max_speed_of(S.prefix);
}
__global__ __launch_bounds__(WO_BLOCK) void k_wind_finish(float* __restrict__ speed, const float* __restrict__ maxSpeed, const float* __restrict__ pressure,
                                                          float* __restrict__ pressureDev, int32_t N) {
    const float m = *maxSpeed;
    WIND_CELLS(r, N) { speed[r] = W::normalise_speed_cell(speed[r], m); pressureDev[r] = W::pressure_dev_cell(pressure[r]); }
}

void wind_alloc(wo_planet* p) {
    if (p->wind) return;
    std::unique_ptr<wo_wind_block> block(new wo_wind_block());          // the planet gets the block once it is complete
    wo_wind_block* B = block.get(); DeviceArena& a = B->mem;
    const size_t N = (size_t)p->N;
    for (auto& s : B->season) for (auto& f : s) f = a.dev<float>(N);
    B->lat = a.dev<float>(N); B->lon = a.dev<float>(N); B->sinLat = a.dev<float>(N); B->cosLat = a.dev<float>(N); B->isLand = a.dev<uint8_t>(N);
    B->cont = a.dev<float>(N); B->plateCont = a.dev<float>(N); B->coastDist = a.dev<int32_t>(N);
    for (auto& f : B->frame) f = a.dev<float>(N);
    B->e = a.dev<float>(N); B->tmpA = a.dev<float>(N); B->tmpB = a.dev<float>(N); B->gradE = a.dev<float>(N); B->gradN = a.dev<float>(N);
    B->label = a.dev<int32_t>(N); B->compSize = a.dev<int32_t>(N); B->plateDist = a.dev<int32_t>(N); B->plate = a.dev<int32_t>(N); B->plateOcean = a.dev<uint8_t>(N);
    for (int i = 0; i < 2; ++i) { B->keys[i] = a.dev<uint32_t>(N); B->vals[i] = a.dev<int32_t>(N); B->frontier[i] = a.dev<int32_t>(N); }
    const size_t words = radix_scratch_words(p->N);
    B->sortScratch = a.dev<uint32_t>(words);
    WO_HIP(hipMemsetAsync(B->sortScratch, 0, words * 4, p->ctx->stream));
    B->binOffset = a.dev<int32_t>((size_t)W::NUM_BINS + 1);
    B->counts = a.dev<int32_t>(3); B->mainKey = a.dev<unsigned long long>(1);
    B->specs = a.dev<W::SampleSpec>(W::NUM_SAMPLES); B->acc = a.dev<W::SampleAcc>(W::NUM_SAMPLES); B->splines = a.dev<W::Spline>(2);
    B->selHist = a.dev<uint32_t>(W::SEL_BINS); B->selState = a.dev<W::SelState>(1); B->maxSpeed = a.dev<float>(1);
    B->h_acc = a.pinned<W::SampleAcc>(W::NUM_SAMPLES);
    B->h_count = a.pinned<int32_t>(16);
    std::vector<W::SampleSpec> specs(W::NUM_SAMPLES);
    W::make_sample_specs(specs.data());
    WO_HIP(hipMemcpy(B->specs, specs.data(), sizeof(W::SampleSpec) * W::NUM_SAMPLES, hipMemcpyHostToDevice));
    p->wind = block.release();
}

void wind_free(wo_planet* p) { delete p->wind; p->wind = nullptr; }

void stage_itcz(wo_planet* p, float* dst) {
    WO_HIP(hipMemcpyAsync(dst, p->wind->itcz[1], sizeof(float) * 2 * W::ITCZ_SAMPLES, hipMemcpyHostToDevice, p->ctx->stream));
}

// computeGradients on a device-resident field (precip.hip)
void gradient_resident(wo_planet* p, const float* field, const W::Frames& T, float* gradE, float* gradN) {
    launch(p, FAM_CLIMATE, k_wind_gradient, blocks_for(p->N), WO_BLOCK, (const int32_t*)p->d_off, (const int32_t*)p->d_adj, (const float*)p->d_xyz, field, T, gradE, gradN, p->N);
}

// one distance field; returns the number of levels after the seeds
static int32_t wind_bfs(wo_planet* p, int32_t mode, const uint8_t* mask, uint8_t want, int32_t* dist) {
    auto* B = p->wind;
    const int32_t N = p->N, g = blocks_for(N);
    hipStream_t s = p->ctx->stream;
    WO_HIP(hipMemsetAsync(B->counts, 0, 3 * sizeof(int32_t), s));
    launch(p, FAM_CLIMATE, k_wind_bfs_seed, g, WO_BLOCK, mode, (const uint8_t*)B->isLand, (const int32_t*)B->label, (const unsigned long long*)B->mainKey,
           (const uint8_t*)B->plateOcean, (const int32_t*)p->d_off, (const int32_t*)p->d_adj, dist, B->frontier[0], B->counts, N);
    int32_t level = 0;
    for (;; ++level) {
        const int c = level % 3;
        WO_HIP(hipMemcpyAsync(B->h_count, B->counts + c, sizeof(int32_t), hipMemcpyDeviceToHost, s));
        WO_HIP(hipStreamSynchronize(s));
        const int32_t n = *B->h_count;
        if (n < 0 || n > N) throw HipError{"wind BFS: frontier length out of range"};
        if (n == 0) break;
        launch(p, FAM_CLIMATE, k_wind_bfs_level, blocks_for(n), WO_BLOCK, (const int32_t*)B->frontier[level & 1], n, mask, want, (const int32_t*)p->d_off,
               (const int32_t*)p->d_adj, dist, level + 1, B->frontier[(level + 1) & 1], B->counts + (level + 1) % 3, B->counts + (level + 2) % 3);
    }
    return level;
}

static void wind_run(wo_planet* p, double seed) {
    auto* B = p->wind;
    const int32_t N = p->N, g = blocks_for(N);
    hipStream_t s = p->ctx->stream;
    B->have = 0;
    // step 0 and the geo index
    W::CellGeo G{B->lat, B->lon, B->sinLat, B->cosLat, B->isLand, B->frame[0], B->frame[1], B->frame[2], B->frame[3], B->frame[4], B->frame[5]};
    launch(p, FAM_CLIMATE, k_wind_precompute, g, WO_BLOCK, (const float*)p->d_xyz, (const float*)B->e, G, B->keys[0], B->vals[0], N);
    const int sorted = radix_sort_pairs(p, FAM_CLIMATE, B->keys, B->vals, N, 0, 16, nullptr, B->sortScratch, N, B->sortFlip);   // bins < 2^12; an even number of passes (radix.hip)
    launch(p, FAM_CLIMATE, k_wind_bin_offsets, blocks_for((int64_t)N + 1), WO_BLOCK, (const uint32_t*)B->keys[sorted], N, B->binOffset);
    launch(p, FAM_CLIMATE, k_wind_sample, W::NUM_SAMPLES, 64, (const W::SampleSpec*)B->specs, (const int32_t*)B->binOffset, (const int32_t*)B->vals[sorted],
           (const float*)B->sinLat, (const float*)B->cosLat, (const float*)B->lon, (const uint8_t*)B->isLand, (const float*)B->e, B->acc);
    WO_HIP(hipMemcpyAsync(B->h_acc, B->acc, sizeof(W::SampleAcc) * W::NUM_SAMPLES, hipMemcpyDeviceToHost, s));
    // continentality (queued behind the samples; the host finishes the ITCZ meanwhile)
    WO_HIP(hipMemsetAsync(B->mainKey, 0, sizeof(unsigned long long), s));
    launch(p, FAM_CLIMATE, k_wind_cc_init, g, WO_BLOCK, B->label, B->compSize, (const int32_t*)B->plate, (const int32_t*)B->oceanIds, B->nOceanIds,
           B->plateOcean, N);
    launch(p, FAM_CLIMATE, k_wind_cc_hook, g, WO_BLOCK, B->label, (const uint8_t*)B->isLand, (const int32_t*)p->d_off, (const int32_t*)p->d_adj, N);
    launch(p, FAM_CLIMATE, k_wind_cc_flatten, g, WO_BLOCK, B->label, N);
    launch(p, FAM_CLIMATE, k_wind_cc_size, g, WO_BLOCK, (const int32_t*)B->label, (const uint8_t*)B->isLand, B->compSize, N);
    launch(p, FAM_CLIMATE, k_wind_cc_main, g, WO_BLOCK, (const int32_t*)B->label, (const uint8_t*)B->isLand, (const int32_t*)B->compSize, B->mainKey, N);
    B->bfsLevels[0] = wind_bfs(p, 0, B->isLand, 1, B->coastDist);          // its first synchronisation also completes the copy of the samples
    W::Spline splines[2];
    W::itcz_finish(B->h_acc, splines, B->itcz[0], B->itcz[1], B->itcz[2]);
    WO_HIP(hipMemcpyAsync(B->splines, splines, sizeof(splines), hipMemcpyHostToDevice, s));
    B->bfsLevels[1] = wind_bfs(p, 1, B->plateOcean, 0, B->plateDist);     // synchronises: `splines` may leave scope afterwards
    const double avgEdgeKm = W::avg_edge_km(N);
    const int32_t contPasses = W::js_round_passes(100 / avgEdgeKm), pressPasses = W::js_round_passes(75 / avgEdgeKm);
    auto smoothed_into = [&](float* src, float* dst, int32_t passes) {      // src is scratch; the result lands in dst
        float* r = smooth_field_resident(p, src, dst, passes);
        if (r != dst) WO_HIP(hipMemcpyAsync(dst, r, (size_t)N * 4, hipMemcpyDeviceToDevice, s));
    };
    launch(p, FAM_CLIMATE, k_wind_continentality, g, WO_BLOCK, (const int32_t*)B->coastDist, (const uint8_t*)B->isLand, (uint8_t)1, avgEdgeKm, B->tmpA, N);
    smoothed_into(B->tmpA, B->cont, contPasses);
    launch(p, FAM_CLIMATE, k_wind_continentality, g, WO_BLOCK, (const int32_t*)B->plateDist, (const uint8_t*)B->plateOcean, (uint8_t)0, avgEdgeKm, B->tmpA, N);
    smoothed_into(B->tmpA, B->plateCont, contPasses);
    // the seasons
    uint8_t t[1024];
    noise_tables(seed, t, t + 512);
    WO_HIP(hipMemcpyAsync(p->d_tables, t, 1024, hipMemcpyHostToDevice, s));
    WO_HIP(hipStreamSynchronize(s));                                        // `t` is pageable
    W::Frames T{B->frame[0], B->frame[1], B->frame[2], B->frame[3], B->frame[4], B->frame[5]};
    const W::SelState sel0{0u, W::percentile_index(N, 0.95)};
    WO_HIP(hipMemsetAsync(B->selHist, 0, sizeof(uint32_t) * W::SEL_BINS, s));
    for (int season = 0; season < 2; ++season) {
        float** out = B->season[season];
        launch(p, FAM_CLIMATE, k_wind_pressure, g, WO_BLOCK, (const uint8_t*)p->d_tables, (const W::Spline*)(B->splines + season), season == 0 ? 1 : -1,
               (const float*)B->lat, (const float*)B->lon, (const float*)B->cont, (const float*)B->e, (const float*)p->d_xyz, B->tmpA, N);
        const float* pressure = smooth_field_resident(p, B->tmpA, B->tmpB, pressPasses);
        launch(p, FAM_CLIMATE, k_wind_gradient, g, WO_BLOCK, (const int32_t*)p->d_off, (const int32_t*)p->d_adj, (const float*)p->d_xyz, pressure, T, B->gradE, B->gradN, N);
        launch(p, FAM_CLIMATE, k_wind_vectors, g, WO_BLOCK, (const float*)B->gradE, (const float*)B->gradN, (const float*)B->sinLat, out[1], out[2], out[3], N);
        WO_HIP(hipMemcpyAsync(B->selState, &sel0, sizeof(sel0), hipMemcpyHostToDevice, s));
        for (int pass = 0; pass < W::SEL_PASSES; ++pass) {
            launch(p, FAM_CLIMATE, k_wind_sel_hist, blocks_for(N, 1024), WO_BLOCK, (const float*)out[3], N, pass, (const W::SelState*)B->selState, B->selHist);
            launch(p, FAM_CLIMATE, k_wind_sel_pick, 1, 64, B->selState, B->selHist, pass, B->maxSpeed);
        }
        launch(p, FAM_CLIMATE, k_wind_finish, g, WO_BLOCK, out[3], (const float*)B->maxSpeed, pressure, out[0], N);
    }
    WO_HIP(hipStreamSynchronize(s));                                        // sel0 is read by the copies above
    B->have = wind_desc().all();
}

}  // namespace wo

using namespace wo;

// the downloadable fields: the reference's result keys in the order it sets them (js/wind.js:649-683; wind_block.h: WindField)
static const char* const kWindFields[WF_COUNT] = {
    "r_pressure_summer", "r_wind_east_summer", "r_wind_north_summer", "r_wind_speed_summer",
    "r_pressure_winter", "r_wind_east_winter", "r_wind_north_winter", "r_wind_speed_winter",
    "itczLons", "itczLatsSummer", "itczLatsWinter", "r_lat", "r_lon", "r_sinLat", "r_isLand",
    "r_continentality", "r_coastDistLand", "r_plateContinentality", "r_eastX", "r_eastY", "r_eastZ", "r_northX", "r_northY", "r_northZ"};
// where field f lives and how large it is (the ITCZ arrays are host arrays of the block)
static Slot wind_slot(StageBlock* b, int f, size_t N) {
    auto* B = static_cast<wo_wind_block*>(b);
    if (f >= WF_ITCZ0 && f < WF_LAT) return Slot{B->itcz[f - WF_ITCZ0], sizeof(float) * W::ITCZ_SAMPLES, true};
    if (f < WF_ITCZ0) return Slot{B->season[f / WS_STRIDE][f % WS_STRIDE], N * 4, false};
    switch (f) {
        case WF_LAT: return Slot{B->lat, N * 4, false};             case WF_LON: return Slot{B->lon, N * 4, false};
        case WF_SINLAT: return Slot{B->sinLat, N * 4, false};       case WF_ISLAND: return Slot{B->isLand, N, false};
        case WF_CONT: return Slot{B->cont, N * 4, false};           case WF_COASTDIST: return Slot{B->coastDist, N * 4, false};
        case WF_PLATECONT: return Slot{B->plateCont, N * 4, false};
        default: return Slot{B->frame[f - WF_FRAME0], N * 4, false};
    }
}
static StageBlock* wind_of(const wo_planet* p) { return p->wind; }
const BlockDesc& wo::wind_desc() {
    static const BlockDesc D{"wind", "wo_compute_wind", kWindFields, WF_COUNT, wind_of, wind_alloc, wind_slot};
    return D;
}

extern "C" {

int wo_compute_wind(wo_planet* p, int32_t numRegions, const float* r_elevation, const int32_t* r_plate, const int32_t* oceanPlates, int32_t nOceanPlates,
                    double seed, double axialTilt, int32_t* bfsLevels2) {
    if (!check_planet(p, "wo_compute_wind")) return 1;
    if (numRegions != p->N) { set_error("wo_compute_wind: numRegions is " + std::to_string(numRegions) + ", the planet has " + std::to_string(p->N)); return 1; }
    if (!r_plate) { set_error("wo_compute_wind: null r_plate"); return 1; }
    if (nOceanPlates < 0 || (nOceanPlates > 0 && !oceanPlates)) { set_error("wo_compute_wind: ocean plate list of negative length, or null with a positive length"); return 1; }
    if (!(axialTilt == axialTilt)) { set_error("wo_compute_wind: axialTilt is NaN"); return 1; }   // the reference converts it and never reads it again (js/wind.js:397)
    WO_TRY
        wind_alloc(p);
        auto* B = p->wind;
        B->have = 0;
        hipStream_t s = p->ctx->stream;
        const size_t N = (size_t)p->N;
        std::vector<int32_t> ids(oceanPlates, oceanPlates + nOceanPlates);
        std::sort(ids.begin(), ids.end());
        ids.erase(std::unique(ids.begin(), ids.end()), ids.end());
        if ((int64_t)ids.size() > B->oceanIdCap || !B->oceanIds) { B->mem.release(B->oceanIds); B->oceanIdCap = 0; B->oceanIds = B->mem.dev<int32_t>(ids.size()); B->oceanIdCap = (int64_t)ids.size(); }
        B->nOceanIds = (int32_t)ids.size();
        if (!ids.empty()) WO_HIP(hipMemcpyAsync(B->oceanIds, ids.data(), ids.size() * 4, hipMemcpyHostToDevice, s));
        WO_HIP(hipMemcpyAsync(B->plate, r_plate, N * 4, hipMemcpyHostToDevice, s));
        // the elevation is snapshotted: later calls on the planet may change the resident field while the wind block is read
        if (r_elevation) WO_HIP(hipMemcpyAsync(B->e, r_elevation, N * 4, hipMemcpyHostToDevice, s));
        else WO_HIP(hipMemcpyAsync(B->e, p->d_e, N * 4, hipMemcpyDeviceToDevice, s));
        WO_HIP(hipStreamSynchronize(s));                      // `ids` is pageable and leaves scope
        wind_run(p, seed);
        if (bfsLevels2) { bfsLevels2[0] = B->bfsLevels[0]; bfsLevels2[1] = B->bfsLevels[1]; }
        return 0;
    WO_CATCH("wo_compute_wind")
}

int wo_wind_download(wo_planet* p, const char* field, void* out, int64_t outBytes) { return block_download(p, "wo_wind_download", wind_desc(), field, out, outBytes); }
int wo_wind_upload(wo_planet* p, const char* field, const void* data, int64_t bytes) { return block_upload(p, "wo_wind_upload", wind_desc(), field, data, bytes); }

int wo_compute_gradients(wo_planet* p, int32_t numRegions, const float* r_pressure, const float* east3, const float* north3, float* r_gradE, float* r_gradN) {
    if (!check_planet(p, "wo_compute_gradients")) return 1;
    if (numRegions != p->N) { set_error("wo_compute_gradients: numRegions is " + std::to_string(numRegions) + ", the planet has " + std::to_string(p->N)); return 1; }
    if (!r_pressure || !east3 || !north3 || !r_gradE || !r_gradN) { set_error("wo_compute_gradients: null pointer"); return 1; }
    WO_TRY
        const size_t N = (size_t)p->N;
        hipStream_t s = p->ctx->stream;
        DeviceArena B;
        float* d = B.dev<float>(9 * N);                       // pressure, east x/y/z, north x/y/z, gradE, gradN
        WO_HIP(hipMemcpyAsync(d, r_pressure, N * 4, hipMemcpyHostToDevice, s));
        WO_HIP(hipMemcpyAsync(d + N, east3, 3 * N * 4, hipMemcpyHostToDevice, s));
        WO_HIP(hipMemcpyAsync(d + 4 * N, north3, 3 * N * 4, hipMemcpyHostToDevice, s));
        W::Frames T{d + N, d + 2 * N, d + 3 * N, d + 4 * N, d + 5 * N, d + 6 * N};
        launch(p, FAM_CLIMATE, k_wind_gradient, blocks_for(p->N), WO_BLOCK, (const int32_t*)p->d_off, (const int32_t*)p->d_adj, (const float*)p->d_xyz,
               (const float*)d, T, d + 7 * N, d + 8 * N, p->N);
        WO_HIP(hipMemcpyAsync(r_gradE, d + 7 * N, N * 4, hipMemcpyDeviceToHost, s));
        WO_HIP(hipMemcpyAsync(r_gradN, d + 8 * N, N * 4, hipMemcpyDeviceToHost, s));
        WO_HIP(hipStreamSynchronize(s));
        return 0;
    WO_CATCH("wo_compute_gradients")
}

}  // extern "C"
