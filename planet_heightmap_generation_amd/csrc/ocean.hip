// Ocean surface currents on the device (js/ocean.js:204-382), on the planet's resident mesh and stream.  The per-cell bodies
// and the exactness contract are in ocean_ops.h; the stage reads the planet's wind block (wind_block.h) and leaves its eight
// results on the device in the planet's ocean block.
//
// Launch sequence (every buffer is allocated before it; no host round trip until the few scalars of `info` come back):
//   mask            k_ocean_mask          r_isOcean, and the 2 x 72 circumpolar bin flags
//   distance fields k_ocean_seed          coast seeds, west or east: level 0 of both fields, one frontier whose entries carry
//                                         the field in the top bits
//                   k_ocean_level         one launch per level for BOTH fields, warmthRange - 1 launches known beforehand; a
//                                         fixed grid reads the frontier length on the device (claims by CAS -1 -> level)
//   currents        k_ocean_band          steps 3-4 for both seasons into one float4 per cell (E, N summer, E, N winter);
//                                         every workgroup folds the bin flags into the two circumpolar flags
//                   k_ocean_smooth<4>     the masked smooth of all four arrays in one gather per pass
//                   k_ocean_speed         de-interleaves the currents, the raw speeds, the count of ocean speeds > 0
//   percentile      k_ocean_sel_hist / _pick x 3   (ocean_block.h, shared with precip.hip) both seasons per launch, over the cells with isOcean && speed > 0; the rank
//                                         comes from the device's count, a whole wave scans the counters
//   warmth          k_ocean_warmth, k_ocean_smooth<2>   classifyWarmth of both seasons as one float2 per cell
//   finish          k_ocean_finish        normalised speeds, de-interleaved warmth
// Scratch: the two distance fields live in the wind block's sort values (vals[0], vals[1]); the two group buffers of the
// ocean block (16 bytes per cell each) hold the frontiers first, then the float4 currents, then the float2 warmths.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstring>
#include <memory>
#include <string>

#include "../../include/worogen.h"
#include "block_ops.h"
#include "device.h"
#include "ocean_block.h"
#include "ocean_ops.h"
#include "wind_block.h"

namespace wo {

__global__ __launch_bounds__(WO_BLOCK) void k_ocean_mask(const uint8_t* __restrict__ isLand, const float* __restrict__ lat, const float* __restrict__ lon,
                                                         uint8_t* __restrict__ isOcean, uint32_t* __restrict__ bins, int32_t N) {
    const int32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= N) return;
    const bool ocean = isLand[r] == 0;
    isOcean[r] = ocean ? 1 : 0;
    const int32_t b = O::circumpolar_bin(ocean, lat[r], lon[r]);
    if (b >= 0 && b < 2 * O::CIRC_BINS) bins[b] = 1u;
}

// level 0 of both fields: a coast cell seeds the west or the east one
__global__ __launch_bounds__(WO_BLOCK) void k_ocean_seed(const uint8_t* __restrict__ isOcean, const int32_t* __restrict__ off, const int32_t* __restrict__ adj,
                                                         const float* __restrict__ xyz, const float* __restrict__ eastX, const float* __restrict__ eastY,
                                                         const float* __restrict__ eastZ, int32_t* __restrict__ distW, int32_t* __restrict__ distE,
                                                         int32_t* __restrict__ list, int32_t* counter, int32_t N) {
    const int32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    int seed = O::SEED_NONE;
    if (r < N) {
        seed = O::coast_seed_cell(isOcean, off, adj, xyz, eastX, eastY, eastZ, r);
        distW[r] = seed == O::SEED_WEST ? 0 : -1;
        distE[r] = seed == O::SEED_EAST ? 0 : -1;
    }
    wave_append(seed != O::SEED_NONE, ((seed == O::SEED_EAST ? 1 : 0) << O::FIELD_SHIFT) | r, list, counter);
}

// one level of both fields: a frontier entry claims the unreached ocean neighbours of its cell in its own field.  A
// (field, cell) pair is claimed once in a call, so a frontier never holds more than 2 N entries (`cap`).
__global__ __launch_bounds__(WO_BLOCK) void k_ocean_level(const int32_t* __restrict__ cur, int32_t* __restrict__ next, int32_t* counts, int32_t curIdx, int32_t nextIdx,
                                                          int32_t zeroIdx, int32_t cap, const uint8_t* __restrict__ isOcean, const int32_t* __restrict__ off,
                                                          const int32_t* __restrict__ adj, int32_t* distW, int32_t* distE, int32_t level) {
    if (blockIdx.x == 0 && threadIdx.x == 0) counts[zeroIdx] = 0;
    int32_t n = counts[curIdx];
    if (n > cap) n = cap;
    for (int32_t base = blockIdx.x * blockDim.x; base < n; base += gridDim.x * blockDim.x) {      // block-uniform trips: the waves stay whole for wave_append
        const int32_t i = base + threadIdx.x;
        const bool valid = i < n;
        const int32_t entry = valid ? cur[i] : 0;
        const int32_t field = entry >> O::FIELD_SHIFT, r = entry & O::CELL_MASK;
        int32_t* dist = field ? distE : distW;
        const int32_t b = valid ? off[r] : 0, deg = valid ? off[r + 1] - b : 0;
        for (int32_t k = 0; __any(k < deg); ++k) {
            bool claim = false; int32_t nb = 0;
            if (k < deg) {
                nb = adj[b + k];
                claim = isOcean[nb] && dist[nb] == -1 && atomicCAS(&dist[nb], -1, level) == -1;
            }
            wave_append(claim, (field << O::FIELD_SHIFT) | nb, next, counts + nextIdx);
        }
    }
}

// steps 3-4 of both seasons; land cells hold 0
__global__ __launch_bounds__(WO_BLOCK) void k_ocean_band(const float* __restrict__ lat, const float* __restrict__ lon, const uint8_t* __restrict__ isOcean,
                                                         const int32_t* __restrict__ distW, const int32_t* __restrict__ distE, const float* __restrict__ itcz,
                                                         OceanCtl* ctl, int32_t coastThreshold, O::Group<4>* __restrict__ out, int32_t N) {
    __shared__ float sItcz[2 * W::ITCZ_SAMPLES];
    __shared__ int sCirc[2];
    for (int i = threadIdx.x; i < 2 * W::ITCZ_SAMPLES; i += blockDim.x) sItcz[i] = itcz[i];
    if (threadIdx.x < 2) sCirc[threadIdx.x] = 1;
    __syncthreads();
    for (int i = threadIdx.x; i < 2 * O::CIRC_BINS; i += blockDim.x) if (!ctl->bins[i]) sCirc[i / O::CIRC_BINS] = 0;      // every writer writes 0
    __syncthreads();
    const bool nh = sCirc[0] != 0, sh = sCirc[1] != 0;
    if (blockIdx.x == 0 && threadIdx.x == 0) { ctl->circ[0] = nh; ctl->circ[1] = sh; }
    const int32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= N) return;
    O::Group<4> g{{0.0f, 0.0f, 0.0f, 0.0f}};
    if (isOcean[r]) {
        const float la = lat[r], lo = lon[r];
        const int32_t w = distW[r], e = distE[r];
        O::current_cell(la, lo, w, e, coastThreshold, nh, sh, 5, sItcz, g.v[0], g.v[1]);
        O::current_cell(la, lo, w, e, coastThreshold, nh, sh, -5, sItcz + W::ITCZ_SAMPLES, g.v[2], g.v[3]);
    }
    out[r] = g;
}

// one pass of the masked smooth on the K fields of every cell
template <int K>
__global__ __launch_bounds__(WO_BLOCK) void k_ocean_smooth(int32_t tile, const int32_t* __restrict__ off, const int32_t* __restrict__ adj,
                                                           const uint8_t* __restrict__ isOcean, const O::Group<K>* __restrict__ src, O::Group<K>* __restrict__ dst, int32_t N) {
    const int32_t r = ocean_xcd_cell(tile);
    if (r < N) dst[r] = O::smooth_ocean_cell<K>(off, adj, isOcean, src, r);
}

// the A/B form of the smoothing (test hook ocean_split_smooth): the K fields of a group as K separate arrays and back
template <int K>
__global__ __launch_bounds__(WO_BLOCK) void k_ocean_split(const O::Group<K>* __restrict__ in, O::Group<1>* __restrict__ f0, O::Group<1>* __restrict__ f1,
                                                          O::Group<1>* __restrict__ f2, O::Group<1>* __restrict__ f3, int32_t N) {
    const int32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= N) return;
    const O::Group<K> g = in[r];
    O::Group<1>* f[4] = {f0, f1, f2, f3};
    for (int k = 0; k < K; ++k) f[k][r].v[0] = g.v[k];
}
template <int K>
__global__ __launch_bounds__(WO_BLOCK) void k_ocean_join(const O::Group<1>* __restrict__ f0, const O::Group<1>* __restrict__ f1, const O::Group<1>* __restrict__ f2,
                                                         const O::Group<1>* __restrict__ f3, O::Group<K>* __restrict__ out, int32_t N) {
    const int32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= N) return;
    const O::Group<1>* f[4] = {f0, f1, f2, f3};
    O::Group<K> g;
    for (int k = 0; k < K; ++k) g.v[k] = f[k][r].v[0];
    out[r] = g;
}

// the currents leave the group buffer; raw speeds; how many ocean speeds are > 0
__global__ __launch_bounds__(WO_BLOCK) void k_ocean_speed(const O::Group<4>* __restrict__ cur, const uint8_t* __restrict__ isOcean, float* __restrict__ eS, float* __restrict__ nS,
                                                          float* __restrict__ spS, float* __restrict__ eW, float* __restrict__ nW, float* __restrict__ spW,
                                                          uint32_t* oceanCells, int32_t N) {
    const int32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    bool cS = false, cW = false;
    if (r < N) {
        const O::Group<4> g = cur[r];
        const bool ocean = isOcean[r] != 0;
        const double s = O::speed_of(g.v[0], g.v[1]), w = O::speed_of(g.v[2], g.v[3]);
        eS[r] = g.v[0]; nS[r] = g.v[1]; spS[r] = (float)s;
        eW[r] = g.v[2]; nW[r] = g.v[3]; spW[r] = (float)w;
        cS = O::speed_counts(ocean, s); cW = O::speed_counts(ocean, w);
    }
    const unsigned long long mS = __ballot(cS), mW = __ballot(cW);
    if ((threadIdx.x & 63) == 0) {
        if (mS) atomicAdd(&oceanCells[0], (uint32_t)__popcll(mS));
        if (mW) atomicAdd(&oceanCells[1], (uint32_t)__popcll(mW));
    }
}

__global__ __launch_bounds__(WO_BLOCK) void k_ocean_warmth(const float* __restrict__ lat, const uint8_t* __restrict__ isOcean, const int32_t* __restrict__ distW,
                                                           const int32_t* __restrict__ distE, int32_t warmthRange, O::Group<2>* __restrict__ out, int32_t N) {
    const int32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= N) return;
    O::Group<2> g{{0.0f, 0.0f}};
    if (isOcean[r]) {
        const float la = lat[r];
        const int32_t w = distW[r], e = distE[r];
        g.v[0] = O::warmth_cell(la, w, e, warmthRange, 5);
        g.v[1] = O::warmth_cell(la, w, e, warmthRange, -5);
    }
    out[r] = g;
}

__global__ __launch_bounds__(WO_BLOCK) void k_ocean_finish(float* __restrict__ spS, float* __restrict__ spW, const O::Group<2>* __restrict__ warm, float* __restrict__ warmS,
                                                           float* __restrict__ warmW, const OceanCtl* __restrict__ ctl, int32_t N) {
    const float pS = ctl->p95[0], pW = ctl->p95[1];
    const int32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= N) return;
    spS[r] = W::normalise_speed_cell(spS[r], pS);
    spW[r] = W::normalise_speed_cell(spW[r], pW);
    const O::Group<2> g = warm[r];
    warmS[r] = g.v[0]; warmW[r] = g.v[1];
}

void ocean_free(wo_planet* p) { delete p->ocean; p->ocean = nullptr; }

void ocean_alloc(wo_planet* p) {
    if (p->ocean) return;
    std::unique_ptr<wo_ocean_block> block(new wo_ocean_block());        // the planet gets the block once it is complete
    wo_ocean_block* B = block.get(); DeviceArena& a = B->mem;
    const size_t N = (size_t)p->N;
    for (auto& o : B->out) o = a.dev<float>(N);
    B->isOcean = a.dev<uint8_t>(N);
    for (auto& g : B->group) g = a.dev<uint8_t>(16 * N);
    B->itcz = a.dev<float>((size_t)2 * W::ITCZ_SAMPLES);
    B->ctl = a.dev<OceanCtl>(1);
    B->h_ctl = a.pinned<OceanCtl>(1);
    p->ocean = block.release();
}

// `passes` passes of the masked smooth from a into b and back; returns the buffer that holds the result
template <int K>
static O::Group<K>* ocean_smooth(wo_planet* p, const uint8_t* isOcean, O::Group<K>* a, O::Group<K>* b, int32_t passes) {
    const int32_t tile = xcd_tile(p->N);
    for (int32_t pass = 0; pass < passes; ++pass) {
        launch(p, FAM_CLIMATE, k_ocean_smooth<K>, xcd_grid(p->N), WO_BLOCK, tile, (const int32_t*)p->d_off, (const int32_t*)p->d_adj, isOcean, (const O::Group<K>*)a, b, p->N);
        std::swap(a, b);
    }
    return a;
}

// the same passes field by field, as the reference runs them: K single-field sweeps per pass over the wind block's scratch
// arrays.  The same bits (the bodies add each field on its own either way); kept for the A/B of DESIGN section 8.3.
template <int K>
static O::Group<K>* ocean_smooth_split(wo_planet* p, const uint8_t* isOcean, O::Group<K>* a, int32_t passes) {
    auto* Wb = p->wind;
    const int32_t N = p->N, g = blocks_for(N);
    O::Group<1>* f[4] = {(O::Group<1>*)Wb->tmpA, (O::Group<1>*)Wb->tmpB, (O::Group<1>*)Wb->gradE, (O::Group<1>*)Wb->gradN};
    O::Group<1>* tmp = (O::Group<1>*)Wb->keys[0];
    launch(p, FAM_CLIMATE, k_ocean_split<K>, g, WO_BLOCK, (const O::Group<K>*)a, f[0], f[1], f[2], f[3], N);
    for (int k = 0; k < K; ++k) {
        O::Group<1>* r = ocean_smooth<1>(p, isOcean, f[k], tmp, passes);
        if (r != f[k]) WO_HIP(hipMemcpyAsync(f[k], r, (size_t)N * 4, hipMemcpyDeviceToDevice, p->ctx->stream));
    }
    launch(p, FAM_CLIMATE, k_ocean_join<K>, g, WO_BLOCK, (const O::Group<1>*)f[0], (const O::Group<1>*)f[1], (const O::Group<1>*)f[2], (const O::Group<1>*)f[3], a, N);
    return a;
}

static void ocean_run(wo_planet* p) {
    auto* B = p->ocean;
    auto* Wb = p->wind;
    const int32_t N = p->N, g = blocks_for(N);
    hipStream_t s = p->ctx->stream;
    B->have = 0;
    const O::Params P = O::params_for(N);
    int32_t *distW = Wb->vals[0], *distE = Wb->vals[1];
    OceanCtl* ctl = B->ctl;
    WO_HIP(hipMemsetAsync(ctl, 0, sizeof(OceanCtl), s));
    stage_itcz(p, B->itcz);
    launch(p, FAM_CLIMATE, k_ocean_mask, g, WO_BLOCK, (const uint8_t*)Wb->isLand, (const float*)Wb->lat, (const float*)Wb->lon, B->isOcean, ctl->bins, N);
    // the two distance fields, to depth warmthRange - 1
    int32_t* frontier[2] = {(int32_t*)B->group[0], (int32_t*)B->group[1]};      // 4 N entries of room each, 2 N needed
    launch(p, FAM_CLIMATE, k_ocean_seed, g, WO_BLOCK, (const uint8_t*)B->isOcean, (const int32_t*)p->d_off, (const int32_t*)p->d_adj, (const float*)p->d_xyz,
           (const float*)Wb->frame[0], (const float*)Wb->frame[1], (const float*)Wb->frame[2], distW, distE, frontier[0], ctl->counts, N);
    const int32_t cap = 2 * N, levelGrid = blocks_for((int64_t)N, 1024);
    for (int32_t level = 1; level < P.warmthRange; ++level)
        launch(p, FAM_CLIMATE, k_ocean_level, levelGrid, WO_BLOCK, (const int32_t*)frontier[(level - 1) & 1], frontier[level & 1], ctl->counts, (level - 1) % 3, level % 3,
               (level + 1) % 3, cap, (const uint8_t*)B->isOcean, (const int32_t*)p->d_off, (const int32_t*)p->d_adj, distW, distE, level);
    // currents
    auto* c4a = (O::Group<4>*)B->group[0]; auto* c4b = (O::Group<4>*)B->group[1];
    launch(p, FAM_CLIMATE, k_ocean_band, g, WO_BLOCK, (const float*)Wb->lat, (const float*)Wb->lon, (const uint8_t*)B->isOcean, (const int32_t*)distW, (const int32_t*)distE,
           (const float*)B->itcz, ctl, P.coastThreshold, c4a, N);
    const O::Group<4>* cur = p->opt.oceanSplitSmooth ? ocean_smooth_split<4>(p, B->isOcean, c4a, P.currentPasses) : ocean_smooth<4>(p, B->isOcean, c4a, c4b, P.currentPasses);
    float **S = B->out + ocean_field(0, 0), **Wn = B->out + ocean_field(1, 0);      // summer's four fields, winter's
    launch(p, FAM_CLIMATE, k_ocean_speed, g, WO_BLOCK, cur, (const uint8_t*)B->isOcean, S[OF_EAST], S[OF_NORTH], S[OF_SPEED], Wn[OF_EAST], Wn[OF_NORTH], Wn[OF_SPEED], ctl->oceanCells, N);
    // percentile of the ocean speeds, both seasons
    for (int pass = 0; pass < W::SEL_PASSES; ++pass) {
        launch(p, FAM_CLIMATE, k_ocean_sel_hist<OceanCtl>, 2 * blocks_for(N, 1024), WO_BLOCK, (const float*)S[OF_SPEED], (const float*)Wn[OF_SPEED], (const uint8_t*)B->isOcean, N, pass, ctl);
        launch(p, FAM_CLIMATE, k_ocean_sel_pick<OceanCtl>, 2, 64, ctl, pass);
    }
    // warmth
    auto* w2a = (O::Group<2>*)B->group[0]; auto* w2b = (O::Group<2>*)B->group[1];
    launch(p, FAM_CLIMATE, k_ocean_warmth, g, WO_BLOCK, (const float*)Wb->lat, (const uint8_t*)B->isOcean, (const int32_t*)distW, (const int32_t*)distE, P.warmthRange, w2a, N);
    const O::Group<2>* warm = p->opt.oceanSplitSmooth ? ocean_smooth_split<2>(p, B->isOcean, w2a, P.warmthPasses) : ocean_smooth<2>(p, B->isOcean, w2a, w2b, P.warmthPasses);
    launch(p, FAM_CLIMATE, k_ocean_finish, g, WO_BLOCK, S[OF_SPEED], Wn[OF_SPEED], warm, S[OF_WARMTH], Wn[OF_WARMTH], (const OceanCtl*)ctl, N);
    WO_HIP(hipMemcpyAsync(B->h_ctl, ctl, OCEAN_CTL_HEAD, hipMemcpyDeviceToHost, s));
    WO_HIP(hipStreamSynchronize(s));
    const OceanCtl& H = *B->h_ctl;
    B->info = wo_ocean_info{(int32_t)H.circ[0], (int32_t)H.circ[1], P.coastThreshold, P.warmthRange, P.currentPasses, P.warmthPasses,
                            {(int32_t)H.oceanCells[0], (int32_t)H.oceanCells[1]}, {H.p95[0], H.p95[1]}};
    B->have = ocean_desc().all();
}

}  // namespace wo

using namespace wo;

// the reference's result keys in the order it sets them (js/ocean.js:374-377, summer then winter)
static const char* const kOceanFields[OF_COUNT] = {"r_ocean_current_east_summer", "r_ocean_current_north_summer", "r_ocean_speed_summer", "r_ocean_warmth_summer",
                                            "r_ocean_current_east_winter", "r_ocean_current_north_winter", "r_ocean_speed_winter", "r_ocean_warmth_winter"};
// the fields of the wind block the stage reads
static constexpr uint32_t kWindForOcean = bit(WF_LAT) | bit(WF_LON) | bit(WF_ISLAND) | (7u << WF_FRAME0) | WF_ITCZ_ALL;
static StageBlock* ocean_of(const wo_planet* p) { return p->ocean; }
const BlockDesc& wo::ocean_desc() {
    static const BlockDesc D{"ocean", "wo_compute_ocean_currents", kOceanFields, OF_COUNT, ocean_of, ocean_alloc, out_slot<wo_ocean_block>};
    return D;
}

extern "C" {

int wo_compute_ocean_currents(wo_planet* p, int32_t numRegions, wo_ocean_info* info) {
    if (!check_planet(p, "wo_compute_ocean_currents")) return 1;
    if (numRegions != p->N) { set_error("wo_compute_ocean_currents: numRegions is " + std::to_string(numRegions) + ", the planet has " + std::to_string(p->N)); return 1; }
    if (p->N >= (1 << O::FIELD_SHIFT)) { set_error("wo_compute_ocean_currents: the planet has 2^30 cells or more"); return 1; }
    if (!block_require(p, "wo_compute_ocean_currents", wind_desc(), kWindForOcean, "wo_wind_upload r_lat r_lon r_isLand r_eastX r_eastY r_eastZ itczLons itczLatsSummer itczLatsWinter")) return 1;
    WO_TRY
        ocean_alloc(p);
        ocean_run(p);
        if (info) *info = p->ocean->info;
        return 0;
    WO_CATCH("wo_compute_ocean_currents")
}

int wo_ocean_download(wo_planet* p, const char* field, void* out, int64_t outBytes) { return block_download(p, "wo_ocean_download", ocean_desc(), field, out, outBytes); }
int wo_ocean_upload(wo_planet* p, const char* field, const void* data, int64_t bytes) { return block_upload(p, "wo_ocean_upload", ocean_desc(), field, data, bytes); }

}  // extern "C"
