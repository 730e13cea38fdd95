// Heightmap import on the device (js/planet-worker.js:682-831): the equirectangular sampler, the synthetic plates
// (connected components of the same-class cells) and the region classification, all on the planet's resident field and
// stream.  The per-cell bodies and the exactness contract are in import_ops.h.
//
// Launch sequence (no hipMalloc / hipFree / device-wide synchronisation inside it; scratch is allocated before it):
//   sample          k_sample_heightmap                      one thread per cell: r_elevation and r_isOcean = e <= 0
//   plates          k_cc_init, k_cc_hook, k_cc_flatten       union-find, min id per component (import_ops.h)
//   lists           k_import_count, k_block_offsets<4>, k_import_scatter
//                   count: per-256-cell-block counts of the four lists; scan: one workgroup turns them into block offsets;
//                   scatter: each block writes its cells in ascending r (block_ops.h: block_place), so every list
//                   comes out ascending, which is the insertion order of the reference's Sets.
// The one synchronisation brings the list lengths back to the host; the copies of the lists follow it.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>

#include "../../include/worogen.h"
#include "block_ops.h"
#include "device.h"
#include "import_ops.h"

namespace wo {

constexpr int IMP_LISTS = 4;            // plateSeeds, mountain_r, coastline_r, ocean_r

__global__ __launch_bounds__(WO_BLOCK) void k_sample_heightmap(const float* __restrict__ xyz, const uint8_t* __restrict__ img, int32_t W, int32_t H,
                                                               float* __restrict__ e, uint8_t* __restrict__ ocean, int32_t N) {
    const int32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= N) return;
    const float v = imp::sample_heightmap_cell(xyz[3 * (int64_t)r], xyz[3 * (int64_t)r + 1], xyz[3 * (int64_t)r + 2], img, W, H);
    e[r] = v;
    ocean[r] = (v <= 0.0f) ? 1 : 0;                          // wo_planet_ocean_from_elevation's mask
}

__global__ __launch_bounds__(WO_BLOCK) void k_cc_init(int32_t* __restrict__ parent, int32_t N) {
    const int32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r < N) parent[r] = r;
}
__global__ __launch_bounds__(WO_BLOCK) void k_cc_hook(int32_t* parent, const float* __restrict__ e, const int32_t* __restrict__ off,
                                                      const int32_t* __restrict__ adj, int32_t N) {
    const int32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r < N) imp::cc_hook_cell(parent, e, off, adj, r);
}
__global__ __launch_bounds__(WO_BLOCK) void k_cc_flatten(int32_t* parent, int32_t N) {
    const int32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r < N) imp::cc_flatten_cell(parent, r);
}

// list membership of one cell's flag byte: 0 seed, 1 mountain, 2 coast, 3 ocean
__device__ inline bool imp_in_list(uint8_t f, int j) {
    const uint8_t bit = j == 0 ? imp::CLS_SEED : j == 1 ? imp::CLS_MOUNTAIN : j == 2 ? imp::CLS_COAST : imp::CLS_OCEAN;
    return (f & bit) != 0;
}

// One block per WO_BLOCK consecutive cells: the flag byte of every cell and the block's four list counts.
// label == nullptr: classification only (no seed bits).
__global__ __launch_bounds__(WO_BLOCK) void k_import_count(const float* __restrict__ e, const int32_t* __restrict__ off, const int32_t* __restrict__ adj,
                                                           const int32_t* __restrict__ label, int32_t N, uint8_t* __restrict__ flags,
                                                           int32_t* __restrict__ blockCounts) {
    __shared__ int32_t waveCnt[IMP_LISTS][BLOCK_WAVES];
    const int32_t r = blockIdx.x * WO_BLOCK + threadIdx.x;
    uint8_t f = 0;
    if (r < N) {
        f = imp::classify_cell(e, off, adj, r);
        if (label && label[r] == r) f |= (f & imp::CLS_OCEAN) ? (imp::CLS_SEED | imp::CLS_SEED_OCEAN) : imp::CLS_SEED;
        flags[r] = f;
    }
    for (int j = 0; j < IMP_LISTS; ++j) {
        const int32_t n = block_place(imp_in_list(f, j), waveCnt[j]).total;
        if (threadIdx.x == 0) blockCounts[(int64_t)blockIdx.x * IMP_LISTS + j] = n;
    }
}

// Each block writes its cells of every list at the block's offset, in ascending r.
__global__ __launch_bounds__(WO_BLOCK) void k_import_scatter(const uint8_t* __restrict__ flags, const int32_t* __restrict__ blockOffsets, int32_t N,
                                                             int32_t* __restrict__ lists, uint8_t* __restrict__ seedOcean) {
    __shared__ int32_t waveCnt[IMP_LISTS][BLOCK_WAVES];
    const int32_t r = blockIdx.x * WO_BLOCK + threadIdx.x;
    const uint8_t f = r < N ? flags[r] : 0;
    for (int j = 0; j < IMP_LISTS; ++j) {
        const bool in = imp_in_list(f, j);
        const int32_t pos = blockOffsets[(int64_t)blockIdx.x * IMP_LISTS + j] + block_place(in, waveCnt[j]).place;
        if (!in) continue;
        lists[(int64_t)j * N + pos] = r;
        if (j == 0) seedOcean[pos] = (f & imp::CLS_SEED_OCEAN) ? 1 : 0;
    }
}

// Built in an arena of its own and handed to the import scratch whole; h_totals, assigned last, says that the buffers are there
static void import_alloc(wo_planet* p) {
    auto& I = p->imp;
    if (I.h_totals) return;
    const size_t N = (size_t)p->N, nB = (N + WO_BLOCK - 1) / WO_BLOCK;
    DeviceArena a;
    I.label = a.dev<int32_t>(N);
    I.flags = a.dev<uint8_t>(N);
    I.lists = a.dev<int32_t>((size_t)IMP_LISTS * N);
    I.seedOcean = a.dev<uint8_t>(N);
    I.blockCounts = a.dev<int32_t>(nB * IMP_LISTS);
    I.totals = a.dev<int32_t>(IMP_LISTS);
    int32_t* h_totals = a.pinned<int32_t>(16);
    I.mem.adopt(a); I.h_totals = h_totals;
}

// count / scan / scatter on the resident field; returns the four list lengths (the one synchronisation)
static void import_lists(wo_planet* p, bool withPlates, int32_t (&len)[IMP_LISTS]) {
    auto& I = p->imp;
    const int32_t N = p->N, nB = (int32_t)((N + WO_BLOCK - 1) / WO_BLOCK);
    hipStream_t s = p->ctx->stream;
    launch(p, FAM_MISC, k_import_count, nB, WO_BLOCK, (const float*)p->d_e, (const int32_t*)p->d_off, (const int32_t*)p->d_adj,
           (const int32_t*)(withPlates ? I.label : nullptr), N, I.flags, I.blockCounts);
    launch(p, FAM_MISC, k_block_offsets<IMP_LISTS>, 1, BLOCK_SCAN_THREADS, I.blockCounts, nB, I.totals);
    launch(p, FAM_MISC, k_import_scatter, nB, WO_BLOCK, (const uint8_t*)I.flags, (const int32_t*)I.blockCounts, N, I.lists, I.seedOcean);
    WO_HIP(hipMemcpyAsync(I.h_totals, I.totals, IMP_LISTS * 4, hipMemcpyDeviceToHost, s));
    WO_HIP(hipStreamSynchronize(s));
    for (int j = 0; j < IMP_LISTS; ++j) len[j] = I.h_totals[j];
}

static bool check_import_planet(wo_planet* p, const char* fn) {
    if (!p || !p->ctx) { set_error(std::string(fn) + ": null planet handle"); return false; }
    const hipError_t e = hipSetDevice(p->ctx->device);
    if (e != hipSuccess) { set_error(std::string(fn) + ": hipSetDevice failed: " + hipGetErrorString(e)); return false; }
    return true;
}

}  // namespace wo

using namespace wo;

extern "C" {

int wo_sample_heightmap(wo_planet* p, const uint8_t* gray, int32_t W, int32_t H, float* r_elevation_out) {
    if (!check_import_planet(p, "wo_sample_heightmap")) return 1;
    if (!gray) { set_error("wo_sample_heightmap: null image"); return 1; }
    if (W <= 0 || H <= 0) { set_error("wo_sample_heightmap: image width and height must be positive"); return 1; }
    const int64_t px = (int64_t)W * (int64_t)H;
    if (px > INT32_MAX) { set_error("wo_sample_heightmap: image of more than 2^31 - 1 pixels"); return 1; }
    WO_TRY
        hipStream_t s = p->ctx->stream;
        auto& I = p->imp;
        if (!I.img || I.imgCap < px) {                       // the old image goes first; the capacity is set once the new one is there
            I.mem.release(I.img); I.imgCap = 0;
            I.img = I.mem.dev<uint8_t>((size_t)px); I.imgCap = px;
        }
        WO_HIP(hipMemcpyAsync(p->imp.img, gray, (size_t)px, hipMemcpyHostToDevice, s));
        launch(p, FAM_MISC, k_sample_heightmap, (int)((p->N + WO_BLOCK - 1) / WO_BLOCK), WO_BLOCK, (const float*)p->d_xyz, (const uint8_t*)p->imp.img,
               W, H, p->d_e, p->d_ocean, p->N);
        p->h_ocean_valid = false;                            // the host copy of the mask is refreshed lazily (planet.hip: refresh_host_ocean)
        if (r_elevation_out) WO_HIP(hipMemcpyAsync(r_elevation_out, p->d_e, (size_t)p->N * 4, hipMemcpyDeviceToHost, s));
        WO_HIP(hipStreamSynchronize(s));                     // the caller's image is borrowed for the call only
        return 0;
    WO_CATCH("wo_sample_heightmap")
}

int wo_synthetic_plates(wo_planet* p, int32_t* r_plate, int32_t* seeds, uint8_t* seedIsOcean, int32_t* nSeeds) {
    if (!check_import_planet(p, "wo_synthetic_plates")) return 1;
    if (!r_plate || !seeds || !nSeeds) { set_error("wo_synthetic_plates: null pointer"); return 1; }
    WO_TRY
        import_alloc(p);
        auto& I = p->imp;
        const int32_t N = p->N, g = (int32_t)((N + WO_BLOCK - 1) / WO_BLOCK);
        hipStream_t s = p->ctx->stream;
        launch(p, FAM_MISC, k_cc_init, g, WO_BLOCK, I.label, N);
        launch(p, FAM_MISC, k_cc_hook, g, WO_BLOCK, I.label, (const float*)p->d_e, (const int32_t*)p->d_off, (const int32_t*)p->d_adj, N);
        launch(p, FAM_MISC, k_cc_flatten, g, WO_BLOCK, I.label, N);
        int32_t len[IMP_LISTS];
        import_lists(p, true, len);
        WO_HIP(hipMemcpyAsync(r_plate, I.label, (size_t)N * 4, hipMemcpyDeviceToHost, s));
        WO_HIP(hipMemcpyAsync(seeds, I.lists, (size_t)len[0] * 4, hipMemcpyDeviceToHost, s));
        if (seedIsOcean) WO_HIP(hipMemcpyAsync(seedIsOcean, I.seedOcean, (size_t)len[0], hipMemcpyDeviceToHost, s));
        WO_HIP(hipStreamSynchronize(s));
        *nSeeds = len[0];
        return 0;
    WO_CATCH("wo_synthetic_plates")
}

int wo_classify_regions(wo_planet* p, int32_t* mountain, int32_t* coastline, int32_t* ocean, int32_t* counts) {
    if (!check_import_planet(p, "wo_classify_regions")) return 1;
    if (!mountain || !coastline || !ocean || !counts) { set_error("wo_classify_regions: null pointer"); return 1; }
    WO_TRY
        import_alloc(p);
        auto& I = p->imp;
        const int64_t N = p->N;
        hipStream_t s = p->ctx->stream;
        int32_t len[IMP_LISTS];
        import_lists(p, false, len);
        int32_t* out[3] = {mountain, coastline, ocean};
        for (int j = 0; j < 3; ++j) WO_HIP(hipMemcpyAsync(out[j], I.lists + (j + 1) * N, (size_t)len[j + 1] * 4, hipMemcpyDeviceToHost, s));
        WO_HIP(hipStreamSynchronize(s));
        for (int j = 0; j < 3; ++j) counts[j] = len[j + 1];
        return 0;
    WO_CATCH("wo_classify_regions")
}

}  // extern "C"
