// Seasonal precipitation on the device (js/precipitation.js:196-684, js/heuristic-precip.js), on the planet's resident mesh and
// stream.  The per-cell bodies and the exactness contract are in precip_ops.h; the stage reads the planet's wind block
// (wind_block.h), the two warmth fields of its ocean block (ocean_block.h) and the elevation, and leaves its four results on the
// device in the planet's precipitation block.
//
// Launch sequence (every pass count depends on N only, so both seasons run the same passes; no host round trip until the few
// scalars of `info` come back).  Launches per call at 10 k / 1 M cells in brackets:
//   elevation       k_smooth_field x elevSmoothPasses [2 / 10], k_precip_prepare (the 0.6 / 0.4 blend, r_heightKm) [1],
//                   k_wind_gradient [1]
//   winds           k_precip_wind: heuristic wind, the 50-50 blend and the 3D vectors of both seasons [1]
//   per season      k_wind_convergence [1], k_smooth_field x convSmoothPasses [3 / 20], k_moisture_seed [1],
//                   k_moisture_advect x maxHops [10 / 20]
//   mechanisms      k_precip_mech: steps (a) to (h) and the rain-shadow seed of both seasons [1]
//   rain shadow     k_precip_weights: the row-shaped wind-aligned weights of both lists and seasons, the list lengths [1]
//                   k_precip_propagate<true> x shadowHops [12 / 125], k_precip_propagate<false> x windwardHops [7 / 75]: both
//                   seasons per launch as one float2 per cell and per adjacency entry
//                   k_precip_merge [1], per season k_smooth_field x rsSmoothPasses [2 / 7], k_precip_apply [1],
//                   per season k_smooth_field x precipSmoothPasses [1 / 5]
//   heuristic       k_precip_wc_seed [1], k_precip_wc_smooth x wcPasses [2 / 15], k_precip_heur [1], per season k_smooth_field x
//                   precipSmoothPasses [1 / 5]
//   blend           k_precip_blend [1], k_ocean_sel_hist / _pick x 3 (ocean_block.h; both seasons per launch) [6],
//                   k_precip_finish [1]
// Temporaries live in an arena on the call's stack; the block holds the four results, the ITCZ latitudes and the control words.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstring>
#include <memory>
#include <string>

#include "../../include/worogen.h"
#include "block_ops.h"
#include "device.h"
#include "ocean_block.h"
#include "precip_block.h"
#include "precip_ops.h"
#include "wind_block.h"

namespace P = wo::precip;

namespace wo {

using G2 = O::Group<2>;
struct SeasonWind { float *e, *n, *x, *y, *z; };
struct MechArgs {
    const float *lat, *lon, *elev, *cont, *heightKm, *gradE, *gradN;
    const int32_t* coastDist;
    const uint8_t* isLand;
    const float *moisture[2], *conv[2], *windE[2], *windN[2], *pressure[2];
    float* precip[2];
    G2* seed;
};

__device__ inline void load_itcz(const float* __restrict__ itcz, float* sItcz) {
    for (int i = threadIdx.x; i < 2 * W::ITCZ_SAMPLES; i += blockDim.x) sItcz[i] = itcz[i];
    __syncthreads();
}

__global__ __launch_bounds__(WO_BLOCK) void k_precip_prepare(const float* __restrict__ smoothed, const float* __restrict__ e, float* __restrict__ blended,
                                                             float* __restrict__ heightKm, int32_t N) {
    const int32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= N) return;
    const float ev = e[r];
    blended[r] = P::elev_blend_cell(smoothed[r], ev);
    heightKm[r] = P::height_km_cell(ev);
}

__global__ __launch_bounds__(WO_BLOCK) void k_precip_wind(const float* __restrict__ lat, const float* __restrict__ lon, const float* __restrict__ itcz,
                                                          const float* __restrict__ rawES, const float* __restrict__ rawNS, const float* __restrict__ rawEW,
                                                          const float* __restrict__ rawNW, W::Frames T, SeasonWind S, SeasonWind Wn, int32_t N) {
    __shared__ float sItcz[2 * W::ITCZ_SAMPLES];
    load_itcz(itcz, sItcz);
    const int32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= N) return;
    const float la = lat[r], lo = lon[r];
    const P::WindOut a = P::blended_wind_cell(la, lo, sItcz, rawES[r], rawNS[r], T, r, P::NoCensus());
    const P::WindOut b = P::blended_wind_cell(la, lo, sItcz + W::ITCZ_SAMPLES, rawEW[r], rawNW[r], T, r, P::NoCensus());
    S.e[r] = a.e; S.n[r] = a.n; S.x[r] = a.x; S.y[r] = a.y; S.z[r] = a.z;
    Wn.e[r] = b.e; Wn.n[r] = b.n; Wn.x[r] = b.x; Wn.y[r] = b.y; Wn.z[r] = b.z;
}

__global__ __launch_bounds__(WO_BLOCK) void k_precip_mech(MechArgs A, const float* __restrict__ itcz, P::Params Q, double precipitationOffset, double landCoverage, int32_t N) {
    __shared__ float sItcz[2 * W::ITCZ_SAMPLES];
    load_itcz(itcz, sItcz);
    const int32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= N) return;
    const bool land = A.isLand[r] != 0;
    const float elev = A.elev[r], gE = A.gradE[r], gN = A.gradN[r], hk = A.heightKm[r];
    G2 seed;
    for (int s = 0; s < 2; ++s) {
        const float wE = A.windE[s][r], wN = A.windN[s][r];
        const P::MechIn I{A.lat[r], A.lon[r], elev, A.moisture[s][r], A.conv[s][r], wE, wN, gE, gN, A.pressure[s][r], A.cont[r], hk, A.coastDist[r], land, s == 0};
        A.precip[s][r] = P::mechanisms_cell(I, sItcz + s * W::ITCZ_SAMPLES, Q, precipitationOffset, landCoverage, P::NoCensus());
        seed.v[s] = P::shadow_seed_cell(land, elev, wE, wN, gE, gN, hk, P::NoCensus());
    }
    A.seed[r] = seed;
}

// the row-shaped weights of both lists and both seasons: one thread per cell walks its row (ocean rows hold 0); the members
// are counted per wave
__global__ __launch_bounds__(WO_BLOCK) void k_precip_weights(const int32_t* __restrict__ off, const int32_t* __restrict__ adj, const float* __restrict__ xyz,
                                                             const uint8_t* __restrict__ isLand, SeasonWind S, SeasonWind Wn, G2* __restrict__ up, G2* __restrict__ dn,
                                                             PrecipCtl* ctl, int32_t N) {
    const int32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t c[4] = {0u, 0u, 0u, 0u};
    if (r < N) {
        const bool land = isLand[r] != 0;
        for (int32_t ni = off[r]; ni < off[r + 1]; ++ni) {
            G2 u{{0.0f, 0.0f}}, d{{0.0f, 0.0f}};
            if (land) {
                const int32_t nb = adj[ni];
                bool um, dm;
                P::aligned_weights(xyz, S.x, S.y, S.z, r, nb, u.v[0], d.v[0], um, dm);
                c[0] += um; c[1] += dm;
                P::aligned_weights(xyz, Wn.x, Wn.y, Wn.z, r, nb, u.v[1], d.v[1], um, dm);
                c[2] += um; c[3] += dm;
            }
            up[ni] = u; dn[ni] = d;
        }
    }
    for (int k = 0; k < 4; ++k) {
        const uint32_t v = wave_sum(c[k]);
        if ((threadIdx.x & 63) == 0 && v) atomicAdd(&ctl->lists[k], v);
    }
}

// one pass of a propagation on both seasons of every cell
template <bool SHADOW>
__global__ __launch_bounds__(WO_BLOCK) void k_precip_propagate(int32_t tile, const int32_t* __restrict__ off, const int32_t* __restrict__ adj, const G2* __restrict__ wt,
                                                               const G2* __restrict__ src, G2* __restrict__ dst, double keep, int32_t N) {
    const int32_t r = ocean_xcd_cell(tile);
    if (r < N) dst[r] = P::propagate_cell<2, SHADOW>(off, adj, wt, src, keep, r);
}

__global__ __launch_bounds__(WO_BLOCK) void k_precip_merge(const G2* __restrict__ seed, const G2* __restrict__ shadow, const G2* __restrict__ windward,
                                                           float* __restrict__ rsS, float* __restrict__ rsW, int32_t N) {
    const int32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= N) return;
    const G2 a = seed[r], b = shadow[r], c = windward[r];
    rsS[r] = P::shadow_merge_cell(a.v[0], b.v[0], c.v[0]);
    rsW[r] = P::shadow_merge_cell(a.v[1], b.v[1], c.v[1]);
}

__global__ __launch_bounds__(WO_BLOCK) void k_precip_apply(const uint8_t* __restrict__ isLand, float* __restrict__ precipS, float* __restrict__ precipW,
                                                           const float* __restrict__ rsS, const float* __restrict__ rsW, int32_t N) {
    const int32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= N) return;
    const bool land = isLand[r] != 0;
    precipS[r] = P::apply_shadow_cell(land, precipS[r], rsS[r], P::NoCensus());
    precipW[r] = P::apply_shadow_cell(land, precipW[r], rsW[r], P::NoCensus());
}

__global__ __launch_bounds__(WO_BLOCK) void k_precip_wc_seed(const int32_t* __restrict__ off, const int32_t* __restrict__ adj, const float* __restrict__ xyz,
                                                             const uint8_t* __restrict__ isLand, const int32_t* __restrict__ coastDist, const float* __restrict__ eastX,
                                                             const float* __restrict__ eastY, const float* __restrict__ eastZ, float* __restrict__ out, int32_t N) {
    const int32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r < N) out[r] = P::west_coast_seed_cell(off, adj, xyz, isLand, coastDist, eastX, eastY, eastZ, r);
}
__global__ __launch_bounds__(WO_BLOCK) void k_precip_wc_smooth(int32_t tile, const int32_t* __restrict__ off, const int32_t* __restrict__ adj,
                                                               const uint8_t* __restrict__ isLand, const float* __restrict__ src, float* __restrict__ dst, int32_t N) {
    const int32_t r = ocean_xcd_cell(tile);
    if (r < N) dst[r] = P::west_coast_smooth_cell(off, adj, isLand, src, r);
}

__global__ __launch_bounds__(WO_BLOCK) void k_precip_heur(const float* __restrict__ lat, const float* __restrict__ lon, const float* __restrict__ itcz,
                                                          const uint8_t* __restrict__ isLand, const float* __restrict__ cont, const float* __restrict__ elev,
                                                          const float* __restrict__ gradE, const float* __restrict__ gradN, const float* __restrict__ westCoast,
                                                          const int32_t* __restrict__ coastDist, double avgEdgeKm, float* __restrict__ outS, float* __restrict__ outW, int32_t N) {
    __shared__ float sItcz[2 * W::ITCZ_SAMPLES];
    load_itcz(itcz, sItcz);
    const int32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= N) return;
    const bool land = isLand[r] != 0;
    const float la = lat[r], lo = lon[r], c = cont[r], e = elev[r], gE = gradE[r], gN = gradN[r], wc = westCoast[r];
    const int32_t cd = coastDist[r];
    outS[r] = P::heuristic_cell(la, lo, sItcz, true, land, c, e, gE, gN, wc, cd, avgEdgeKm, P::NoCensus());
    outW[r] = P::heuristic_cell(la, lo, sItcz + W::ITCZ_SAMPLES, false, land, c, e, gE, gN, wc, cd, avgEdgeKm, P::NoCensus());
}

__global__ __launch_bounds__(WO_BLOCK) void k_precip_blend(const float* __restrict__ precipS, const float* __restrict__ precipW, const float* __restrict__ heurS,
                                                           const float* __restrict__ heurW, float* __restrict__ outS, float* __restrict__ outW, PrecipCtl* ctl, int32_t N) {
    const int32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r == 0) { ctl->cells[0] = (uint32_t)N; ctl->cells[1] = (uint32_t)N; }
    if (r >= N) return;
    outS[r] = P::blend_cell(precipS[r], heurS[r]);
    outW[r] = P::blend_cell(precipW[r], heurW[r]);
}

__global__ __launch_bounds__(WO_BLOCK) void k_precip_finish(float* __restrict__ outS, float* __restrict__ outW, const uint8_t* __restrict__ isLand,
                                                            const float* __restrict__ cont, const PrecipCtl* __restrict__ ctl, int32_t N) {
    const float pS = ctl->p95[0], pW = ctl->p95[1];
    const int32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= N) return;
    const bool land = isLand[r] != 0;
    const float c = cont[r];
    outS[r] = P::normalise_cell(outS[r], pS, land, c, P::NoCensus());
    outW[r] = P::normalise_cell(outW[r], pW, land, c, P::NoCensus());
}

void precip_free(wo_planet* p) { delete p->precip; p->precip = nullptr; }

static void precip_alloc(wo_planet* p) {
    if (p->precip) return;
    std::unique_ptr<wo_precip_block> block(new wo_precip_block());      // the planet gets the block once it is complete
    wo_precip_block* B = block.get(); DeviceArena& a = B->mem;
    for (auto& o : B->out) o = a.dev<float>((size_t)p->N);
    B->itcz = a.dev<float>((size_t)2 * W::ITCZ_SAMPLES);
    B->ctl = a.dev<PrecipCtl>(1);
    B->h_ctl = a.pinned<PrecipCtl>(1);
    p->precip = block.release();
}

// smoothField on x with scratch y: afterwards x is the view that holds the result and y the other buffer
static void smooth_swap(wo_planet* p, float*& x, float*& y, int32_t passes) {
    float* r = smooth_field_resident(p, x, y, passes);
    if (r != x) std::swap(x, y);
}

static void precip_run(wo_planet* p, const float* r_elevation, double precipitationOffset, double landCoverage) {
    auto* B = p->precip;
    auto* Wb = p->wind;
    auto* Ob = p->ocean;
    const int32_t N = p->N, g = blocks_for(N), tile = xcd_tile(N), xg = xcd_grid(N);
    const size_t n = (size_t)N, E = (size_t)p->E;
    hipStream_t s = p->ctx->stream;
    B->have = 0;
    const P::Params Q = P::params_for(N);
    const int32_t* off = p->d_off; const int32_t* adj = p->d_adj; const float* xyz = p->d_xyz;
    const uint8_t* isLand = Wb->isLand;
    DeviceArena T;                                            // the temporaries of this call
    PrecipCtl* ctl = B->ctl;
    WO_HIP(hipMemsetAsync(ctl, 0, sizeof(PrecipCtl), s));
    stage_itcz(p, B->itcz);
    // the elevation, its smoothed blend and that field's gradient, the heights
    const float* e = stage_elevation(p, T, r_elevation);
    float *sa = T.dev<float>(n), *sb = T.dev<float>(n);      // smoothing scratch
    float *es = T.dev<float>(n), *gradE = T.dev<float>(n), *gradN = T.dev<float>(n), *heightKm = T.dev<float>(n);
    WO_HIP(hipMemcpyAsync(sa, e, n * 4, hipMemcpyDeviceToDevice, s));
    smooth_swap(p, sa, sb, Q.elevSmoothPasses);
    launch(p, FAM_CLIMATE, k_precip_prepare, g, WO_BLOCK, (const float*)sa, (const float*)e, es, heightKm, N);
    const W::Frames F{Wb->frame[0], Wb->frame[1], Wb->frame[2], Wb->frame[3], Wb->frame[4], Wb->frame[5]};
    gradient_resident(p, es, F, gradE, gradN);
    // the blended winds of both seasons
    SeasonWind wind[2];
    for (auto& w : wind) w = SeasonWind{T.dev<float>(n), T.dev<float>(n), T.dev<float>(n), T.dev<float>(n), T.dev<float>(n)};
    launch(p, FAM_CLIMATE, k_precip_wind, g, WO_BLOCK, (const float*)Wb->lat, (const float*)Wb->lon, (const float*)B->itcz, (const float*)Wb->season[0][1],
           (const float*)Wb->season[0][2], (const float*)Wb->season[1][1], (const float*)Wb->season[1][2], F, wind[0], wind[1], N);
    // convergence and advected moisture
    float* conv[2] = {T.dev<float>(n), T.dev<float>(n)};
    float* moist[2] = {T.dev<float>(n), T.dev<float>(n)};
    for (int k = 0; k < 2; ++k) {
        wind_convergence_resident(p, wind[k].x, wind[k].y, wind[k].z, conv[k]);
        smooth_swap(p, conv[k], sa, Q.convSmoothPasses);
        float* r = advect_moisture_resident(p, heightKm, isLand, wind[k].e, wind[k].n, wind[k].x, wind[k].y, wind[k].z, Ob->out[ocean_field(k, OF_WARMTH)], Wb->coastDist, Q.maxHops,
                                            Q.depletionBase, moist[k], sa);
        if (r != moist[k]) std::swap(moist[k], sa);
    }
    // the mechanisms and the rain-shadow seed
    float* precip[2] = {T.dev<float>(n), T.dev<float>(n)};
    G2* seed = T.dev<G2>(n);
    MechArgs A{Wb->lat, Wb->lon, e, Wb->cont, heightKm, gradE, gradN, Wb->coastDist, isLand, {moist[0], moist[1]}, {conv[0], conv[1]}, {wind[0].e, wind[1].e},
               {wind[0].n, wind[1].n}, {Wb->season[0][0], Wb->season[1][0]}, {precip[0], precip[1]}, seed};
    launch(p, FAM_CLIMATE, k_precip_mech, g, WO_BLOCK, A, (const float*)B->itcz, Q, precipitationOffset, landCoverage, N);
    // the propagations
    G2 *up = T.dev<G2>(E), *dn = T.dev<G2>(E);
    launch(p, FAM_CLIMATE, k_precip_weights, g, WO_BLOCK, off, adj, xyz, isLand, wind[0], wind[1], up, dn, ctl, N);
    G2* buf[4] = {T.dev<G2>(n), T.dev<G2>(n), T.dev<G2>(n), T.dev<G2>(n)};
    const G2* shadow = seed;
    for (int32_t it = 0; it < Q.shadowHops; ++it) {
        G2* dst = buf[it & 1];
        launch(p, FAM_CLIMATE, k_precip_propagate<true>, xg, WO_BLOCK, tile, off, adj, (const G2*)up, shadow, dst, 1 - Q.shadowDecay, N);
        shadow = dst;
    }
    const G2* windward = seed;
    for (int32_t it = 0; it < Q.windwardHops; ++it) {
        G2* dst = buf[2 + (it & 1)];
        launch(p, FAM_CLIMATE, k_precip_propagate<false>, xg, WO_BLOCK, tile, off, adj, (const G2*)dn, windward, dst, 1 - Q.windwardDecay, N);
        windward = dst;
    }
    float **rain = B->out + PF_PRECIP0, **rs = B->out + PF_SHADOW0;      // both seasons of r_precip_*, of r_rainshadow_*
    launch(p, FAM_CLIMATE, k_precip_merge, g, WO_BLOCK, (const G2*)seed, shadow, windward, rs[0], rs[1], N);
    for (int k = 0; k < 2; ++k) {
        float* r = smooth_field_resident(p, rs[k], sa, Q.rsSmoothPasses);
        if (r != rs[k]) WO_HIP(hipMemcpyAsync(rs[k], r, n * 4, hipMemcpyDeviceToDevice, s));
    }
    launch(p, FAM_CLIMATE, k_precip_apply, g, WO_BLOCK, isLand, precip[0], precip[1], (const float*)rs[0], (const float*)rs[1], N);
    for (int k = 0; k < 2; ++k) smooth_swap(p, precip[k], sa, Q.precipSmoothPasses);
    // the heuristic model (the convergence and moisture buffers are free by now)
    float *wc = conv[0], *wcTmp = conv[1];
    launch(p, FAM_CLIMATE, k_precip_wc_seed, g, WO_BLOCK, off, adj, xyz, isLand, (const int32_t*)Wb->coastDist, (const float*)Wb->frame[0], (const float*)Wb->frame[1],
           (const float*)Wb->frame[2], wc, N);
    for (int32_t pass = 0; pass < Q.wcPasses; ++pass) {
        launch(p, FAM_CLIMATE, k_precip_wc_smooth, xg, WO_BLOCK, tile, off, adj, isLand, (const float*)wc, wcTmp, N);
        std::swap(wc, wcTmp);
    }
    float* heur[2] = {moist[0], moist[1]};
    launch(p, FAM_CLIMATE, k_precip_heur, g, WO_BLOCK, (const float*)Wb->lat, (const float*)Wb->lon, (const float*)B->itcz, isLand, (const float*)Wb->cont, (const float*)e,
           (const float*)gradE, (const float*)gradN, (const float*)wc, (const int32_t*)Wb->coastDist, Q.avgEdgeKm, heur[0], heur[1], N);
    for (int k = 0; k < 2; ++k) smooth_swap(p, heur[k], sa, Q.precipSmoothPasses);
    // blend, percentile, normalise
    launch(p, FAM_CLIMATE, k_precip_blend, g, WO_BLOCK, (const float*)precip[0], (const float*)precip[1], (const float*)heur[0], (const float*)heur[1], rain[0], rain[1], ctl, N);
    for (int pass = 0; pass < W::SEL_PASSES; ++pass) {
        launch(p, FAM_CLIMATE, k_ocean_sel_hist<PrecipCtl>, 2 * blocks_for(N, 1024), WO_BLOCK, (const float*)rain[0], (const float*)rain[1], (const uint8_t*)nullptr, N, pass, ctl);
        launch(p, FAM_CLIMATE, k_ocean_sel_pick<PrecipCtl>, 2, 64, ctl, pass);
    }
    launch(p, FAM_CLIMATE, k_precip_finish, g, WO_BLOCK, rain[0], rain[1], isLand, (const float*)Wb->cont, (const PrecipCtl*)ctl, N);
    WO_HIP(hipMemcpyAsync(B->h_ctl, ctl, PRECIP_CTL_HEAD, hipMemcpyDeviceToHost, s));
    WO_HIP(hipStreamSynchronize(s));                          // also before T frees the temporaries
    const PrecipCtl& H = *B->h_ctl;
    wo_precip_info I{};
    I.maxHops = Q.maxHops; I.elevSmoothPasses = Q.elevSmoothPasses; I.convSmoothPasses = Q.convSmoothPasses; I.shadowHops = Q.shadowHops; I.windwardHops = Q.windwardHops;
    I.rsSmoothPasses = Q.rsSmoothPasses; I.precipSmoothPasses = Q.precipSmoothPasses; I.wcPasses = Q.wcPasses; I.leeCoastHops = Q.leeCoastHops;
    for (int k = 0; k < 4; ++k) I.listLengths[k] = (int32_t)H.lists[k];
    I.depletionBase = Q.depletionBase; I.shadowDecay = Q.shadowDecay; I.windwardDecay = Q.windwardDecay;
    I.p95[0] = H.p95[0]; I.p95[1] = H.p95[1];
    B->info = I;
    B->have = precip_desc().all();
}

}  // namespace wo

using namespace wo;

// the reference's result keys (js/precipitation.js:640-641, :678)
static const char* const kPrecipFields[PF_COUNT] = {"r_precip_summer", "r_precip_winter", "r_rainshadow_summer", "r_rainshadow_winter"};
// the fields of the wind block the stage reads: pressure, east and north wind of both seasons, the ITCZ arrays, the geography
static constexpr uint32_t kWindForPrecip = wind_both(WS_PRESSURE) | wind_both(WS_EAST) | wind_both(WS_NORTH) | WF_ITCZ_ALL | bit(WF_LAT) | bit(WF_LON) | bit(WF_ISLAND) |
                                           bit(WF_CONT) | bit(WF_COASTDIST) | (63u << WF_FRAME0);
static constexpr uint32_t kOceanForPrecip = ocean_both(OF_WARMTH);      // r_ocean_warmth_summer, r_ocean_warmth_winter
static StageBlock* precip_of(const wo_planet* p) { return p->precip; }
const BlockDesc& wo::precip_desc() {
    static const BlockDesc D{"precipitation", "wo_compute_precipitation", kPrecipFields, PF_COUNT, precip_of, precip_alloc, out_slot<wo_precip_block>};
    return D;
}

extern "C" {

int wo_compute_precipitation(wo_planet* p, int32_t numRegions, const float* r_elevation, double precipitationOffset, double landCoverage, wo_precip_info* info) {
    if (!check_planet(p, "wo_compute_precipitation")) return 1;
    if (numRegions != p->N) { set_error("wo_compute_precipitation: numRegions is " + std::to_string(numRegions) + ", the planet has " + std::to_string(p->N)); return 1; }
    if (!(precipitationOffset == precipitationOffset) || !(landCoverage == landCoverage)) { set_error("wo_compute_precipitation: precipitationOffset or landCoverage is NaN"); return 1; }
    if (!block_require(p, "wo_compute_precipitation", wind_desc(), kWindForPrecip,
                       "wo_wind_upload r_lat r_lon r_isLand r_continentality r_coastDistLand, the six frame arrays, the three ITCZ arrays and r_wind_east_* r_wind_north_* "
                       "r_pressure_* of both seasons")) return 1;
    if (!block_require(p, "wo_compute_precipitation", ocean_desc(), kOceanForPrecip, "wo_ocean_upload r_ocean_warmth_summer r_ocean_warmth_winter")) return 1;
    WO_TRY
        precip_alloc(p);
        precip_run(p, r_elevation, precipitationOffset, landCoverage);
        if (info) *info = p->precip->info;
        return 0;
    WO_CATCH("wo_compute_precipitation")
}

int wo_precip_download(wo_planet* p, const char* field, void* out, int64_t outBytes) { return block_download(p, "wo_precip_download", precip_desc(), field, out, outBytes); }
int wo_precip_upload(wo_planet* p, const char* field, const void* data, int64_t bytes) { return block_upload(p, "wo_precip_upload", precip_desc(), field, data, bytes); }

}  // extern "C"
