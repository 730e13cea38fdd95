// buildSuperPlates on the device (js/super-plates.js:16-273): the per-cell passes over the CSR — plate areas (:21-25), the
// plate adjacency graph (:29-39) and the final gather (:177-180).  The plate-level part is native host code
// (super_plates_host.cc).  Nothing here is floating point, and nothing depends on the order in which threads arrive:
//   area[a]          cells of plate a                                     (integer adds)
//   firstSlot[a][b]  the smallest adjList index ni at which a cell of a   (integer min)
//                    has a neighbour in b, 0xFFFFFFFF: never
// Plates are "slots", positions in plateSeeds; slotOf maps plate id -> slot, -1 for an id that is no seed.  The CSR is the
// planet's own (index order): the key is the reference's slot index, which the Morton mirror does not keep.
#include <hip/hip_runtime.h>

#include <chrono>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/worogen.h"
#include "device.h"

namespace wo {

constexpr uint32_t SUPER_NEVER = 0xFFFFFFFFu;
constexpr int SUPER_MAX_BLOCKS = 2048;         // grid-stride: every block flushes its histogram once, so few, long-lived blocks

__device__ __forceinline__ int32_t super_slot(const int32_t* __restrict__ slotOf, int32_t numIds, int32_t id) {
    return (uint32_t)id < (uint32_t)numIds ? slotOf[id] : -1;
}

// Areas: a histogram per block in LDS, flushed with one global atomicAdd per occupied bin.  Pairs: atomicMin of the slot index;
// every boundary cell of a plate pair hits the same word, so a plain load skips the atomic when the word is already at or
// below the key (values only fall: a stale read is only ever too large and costs one spare atomic).  bad: the smallest cell
// whose plate is no seed.
__global__ __launch_bounds__(WO_BLOCK) void k_super_tables(const int32_t* __restrict__ off, const int32_t* __restrict__ adj, const int32_t* __restrict__ plate,
                                                          const int32_t* __restrict__ slotOf, int32_t numIds, int32_t P, int32_t N,
                                                          int32_t* area, uint32_t* firstSlot, uint32_t* bad) {
    __shared__ int32_t hist[WO_SUPER_MAX_PLATES];
    for (int32_t i = threadIdx.x; i < P; i += blockDim.x) hist[i] = 0;
    __syncthreads();
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < N; r += (int64_t)gridDim.x * blockDim.x) {
        const int32_t a = super_slot(slotOf, numIds, plate[r]);
        if (a < 0) { atomicMin(bad, (uint32_t)r); continue; }
        atomicAdd(&hist[a], 1);
        uint32_t* row = firstSlot + (size_t)a * (size_t)P;
        for (int32_t ni = off[r], end = off[r + 1]; ni < end; ++ni) {
            const int32_t b = super_slot(slotOf, numIds, plate[adj[ni]]);
            if (b < 0 || b == a) continue;            // (a neighbour without a slot is reported by its own thread)
            if (row[b] > (uint32_t)ni) atomicMin(&row[b], (uint32_t)ni);
        }
    }
    __syncthreads();
    for (int32_t i = threadIdx.x; i < P; i += blockDim.x) if (hist[i]) atomicAdd(&area[i], hist[i]);
}

__global__ __launch_bounds__(WO_BLOCK) void k_super_gather(const int32_t* __restrict__ plate, const int32_t* __restrict__ slotOf, int32_t numIds,
                                                          const int32_t* __restrict__ plateToSuper, int32_t N, int32_t* __restrict__ superPlate) {
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < N; r += (int64_t)gridDim.x * blockDim.x) {
        const int32_t a = super_slot(slotOf, numIds, plate[r]);
        superPlate[r] = a < 0 ? -1 : plateToSuper[a];
    }
}

// the device buffers of one call
struct SuperDev {
    DeviceArena mem;
    std::vector<int32_t> slotOf;
    int32_t P = 0, numIds = 0;
    int32_t *plate = nullptr, *slot = nullptr, *area = nullptr;
    uint32_t *first = nullptr, *bad = nullptr;
};

static void super_upload(wo_planet* p, SuperDev& D, const int32_t* r_plate, const int32_t* plateSeeds, int32_t P) {
    if (p->mirror.active) throw HipError{"the planet's CSR is redirected to its Morton mirror"};
    if ((int64_t)p->E >= (int64_t)SUPER_NEVER) throw std::invalid_argument("adjOffset[numRegions] >= 2^32 - 1: a slot index does not fit the table");
    super_plate_slots(P, plateSeeds, D.slotOf);
    hipStream_t s = p->ctx->stream;
    D.P = P; D.numIds = (int32_t)D.slotOf.size();
    D.plate = up(D.mem, r_plate, (size_t)p->N, s);
    D.slot = up(D.mem, D.slotOf.data(), D.slotOf.size(), s);
    D.area = D.mem.dev<int32_t>((size_t)P); D.first = D.mem.dev<uint32_t>((size_t)P * P); D.bad = D.mem.dev<uint32_t>(1);
    WO_HIP(hipMemsetAsync(D.area, 0, (size_t)P * 4, s));
    WO_HIP(hipMemsetAsync(D.first, 0xFF, (size_t)P * P * 4, s));
    WO_HIP(hipMemsetAsync(D.bad, 0xFF, 4, s));
}

// launches k_super_tables and brings the tables to the host; an r_plate entry without a slot is an error (the tables are not delivered)
static void super_tables(wo_planet* p, SuperDev& D, const int32_t* r_plate, int32_t* area, uint32_t* firstSlot) {
    hipStream_t s = p->ctx->stream;
    launch(p, FAM_MISC, k_super_tables, blocks_for(p->N, SUPER_MAX_BLOCKS), WO_BLOCK, (const int32_t*)p->d_off, (const int32_t*)p->d_adj, (const int32_t*)D.plate,
           (const int32_t*)D.slot, D.numIds, D.P, p->N, D.area, D.first, D.bad);
    uint32_t bad = SUPER_NEVER;
    WO_HIP(hipMemcpyAsync(&bad, D.bad, 4, hipMemcpyDeviceToHost, s));
    WO_HIP(hipMemcpyAsync(area, D.area, (size_t)D.P * 4, hipMemcpyDeviceToHost, s));
    WO_HIP(hipMemcpyAsync(firstSlot, D.first, (size_t)D.P * D.P * 4, hipMemcpyDeviceToHost, s));
    WO_HIP(hipStreamSynchronize(s));
    if (bad != SUPER_NEVER) throw std::invalid_argument("r_plate[" + std::to_string(bad) + "] = " + std::to_string(r_plate[bad]) + " is not in plateSeeds");
}

}  // namespace wo

using namespace wo;

// invalid arguments found inside the call are status 1, like the ones found before it
#define WO_SUPER_CATCH(fn) } catch (const std::invalid_argument& e) { set_error(std::string(fn) + ": " + e.what()); return 1; WO_CATCH(fn)

extern "C" {

int wo_super_plate_tables(wo_planet* p, const int32_t* r_plate, const int32_t* plateSeeds, int32_t numPlateSeeds, int32_t* area, uint32_t* firstSlot) {
    if (!check_planet(p, "wo_super_plate_tables")) return 1;
    if (!r_plate || !plateSeeds || !area || !firstSlot) { set_error("wo_super_plate_tables: null pointer"); return 1; }
    if (numPlateSeeds < 1) { set_error("wo_super_plate_tables: numPlateSeeds must be positive"); return 1; }
    WO_TRY
        SuperDev D;
        super_upload(p, D, r_plate, plateSeeds, numPlateSeeds);
        super_tables(p, D, r_plate, area, firstSlot);
        return 0;
    WO_SUPER_CATCH("wo_super_plate_tables")
}

int wo_build_super_plates(wo_planet* p, const int32_t* r_plate, const wo_plate_table* plates, const int32_t* plateSeeds, int32_t numPlateSeeds,
                          int32_t* r_superPlate, int32_t* numSuper, double* superPole, double* superOmega, uint8_t* superIsOcean, double* superDensity) {
    if (!check_planet(p, "wo_build_super_plates")) return 1;
    if (!r_plate || !plates || !plateSeeds || !r_superPlate || !numSuper || !superPole || !superOmega || !superIsOcean || !superDensity) {
        set_error("wo_build_super_plates: null pointer"); return 1;
    }
    if (!plates->hasVec || !plates->pole || !plates->omega || !plates->isOcean || !plates->density) { set_error("wo_build_super_plates: null array in the plate table"); return 1; }
    if (numPlateSeeds < 1) { set_error("wo_build_super_plates: numPlateSeeds must be positive"); return 1; }
    WO_TRY
        hipStream_t s = p->ctx->stream;
        const int32_t P = numPlateSeeds;
        std::vector<std::pair<std::string, double>> timing;
        auto t0 = std::chrono::steady_clock::now();
        auto lap = [&](const char* stage) { WO_HIP(hipStreamSynchronize(s)); auto now = std::chrono::steady_clock::now(); timing.push_back({stage, std::chrono::duration<double, std::milli>(now - t0).count()}); t0 = now; };
        SuperDev D;
        super_upload(p, D, r_plate, plateSeeds, P);
        lap("Upload r_plate");
        std::vector<int32_t> area((size_t)P), toSuper((size_t)P);
        std::vector<uint32_t> first((size_t)P * P);
        super_tables(p, D, r_plate, area.data(), first.data());
        lap("Plate areas + adjacency (device)");
        *numSuper = super_plates_group_host(P, plateSeeds, plates->numIds, plates->hasVec, plates->pole, plates->omega, plates->isOcean, plates->density,
                                            area.data(), first.data(), SuperPlateTables{toSuper.data(), superPole, superOmega, superIsOcean, superDensity});
        lap("Components, split, poles (host)");
        int32_t* d_toSuper = up(D.mem, toSuper.data(), (size_t)P, s);
        int32_t* d_super = D.mem.dev<int32_t>((size_t)p->N);
        launch(p, FAM_MISC, k_super_gather, blocks_for(p->N, SUPER_MAX_BLOCKS), WO_BLOCK, (const int32_t*)D.plate, (const int32_t*)D.slot, D.numIds,
               (const int32_t*)d_toSuper, p->N, d_super);
        WO_HIP(hipMemcpyAsync(r_superPlate, d_super, (size_t)p->N * 4, hipMemcpyDeviceToHost, s));
        lap("Gather r_superPlate (device)");
        release_stage_brackets(p);
        p->stageTiming = timing;
        return 0;
    WO_SUPER_CATCH("wo_build_super_plates")
}

}  // extern "C"
