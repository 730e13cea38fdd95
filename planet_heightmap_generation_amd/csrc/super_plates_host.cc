// buildSuperPlates, the plate-level part (js/super-plates.js:41-172 and :182-270): order-defined double arithmetic on at most
// WO_SUPER_MAX_PLATES plates, from the two tables the device stage (super_plates.hip) makes of the cells.
//
// Order is what carries exactness.  The reference keeps plateNeighbors[pid] as a Set, whose iteration order is the order in
// which neighbour plates are first met scanning r ascending and ni ascending (:31-39) — the ascending order of firstSlot.
// That order decides the BFS order of a component (:44-62), so the scan order of its Dijkstras (:105-112, strict <, first
// wins), the farthest seeds (:127-133) and with them the super-plate ids.  Plates are "slots" here: positions in plateSeeds.
#include <algorithm>
#include <cmath>
#include <limits>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/worogen.h"
#include "wo_internal.h"

namespace wo {

void super_plate_slots(int32_t numSeeds, const int32_t* plateSeeds, std::vector<int32_t>& slotOf) {
    if (numSeeds > WO_SUPER_MAX_PLATES)
        throw std::invalid_argument(std::to_string(numSeeds) + " plates: more than WO_SUPER_MAX_PLATES = " + std::to_string(WO_SUPER_MAX_PLATES));
    int32_t top = -1;
    for (int32_t i = 0; i < numSeeds; ++i) {
        if (plateSeeds[i] < 0) throw std::invalid_argument("plateSeeds[" + std::to_string(i) + "] is negative");
        top = std::max(top, plateSeeds[i]);
    }
    slotOf.assign((size_t)top + 1, -1);
    for (int32_t i = 0; i < numSeeds; ++i) {
        if (slotOf[plateSeeds[i]] >= 0) throw std::invalid_argument("plate " + std::to_string(plateSeeds[i]) + " is repeated in plateSeeds");
        slotOf[plateSeeds[i]] = i;
    }
}

// Math.round of a non-negative quotient of small integers
static int32_t js_round(double x) { return (int32_t)std::floor(x + 0.5); }

namespace {
// one component that splits into k > 1 super plates (js/super-plates.js:79-171); everything is indexed by position in `comp`
struct Split {
    const std::vector<int32_t>& comp;
    std::vector<std::vector<int32_t>> localAdj;     // :85-91, positions in comp, in the neighbour Set's order
    std::vector<double> edgeWeight, dist;            // :94-97, :100
    std::vector<uint8_t> visited;

    // :101-120
    void dijkstra_from(const std::vector<int32_t>& starts) {
        const int32_t n = (int32_t)comp.size();
        std::fill(dist.begin(), dist.end(), std::numeric_limits<double>::infinity());
        std::fill(visited.begin(), visited.end(), 0);
        for (int32_t s : starts) dist[s] = 0.0;
        for (int32_t iter = 0; iter < n; ++iter) {
            int32_t cur = -1; double minD = std::numeric_limits<double>::infinity();
            for (int32_t i = 0; i < n; ++i) if (!visited[i] && dist[i] < minD) { minD = dist[i]; cur = i; }
            if (cur == -1) break;
            visited[cur] = 1;
            for (int32_t nb : localAdj[cur]) { const double nd = dist[cur] + edgeWeight[nb]; if (nd < dist[nb]) dist[nb] = nd; }
        }
    }
};
}  // namespace

int32_t super_plates_group_host(int32_t P, const int32_t* plateSeeds, int32_t numIds, const uint8_t* hasVec, const double* pole, const double* omega,
                                const uint8_t* isOcean, const double* density, const int32_t* area, const uint32_t* firstSlot, const SuperPlateTables& out) {
    for (int32_t a = 0; a < P; ++a)
        if (plateSeeds[a] < 0 || plateSeeds[a] >= numIds) throw std::invalid_argument("plateSeeds[" + std::to_string(a) + "] lies outside the plate table");
    auto ocean = [&](int32_t a) { return isOcean[plateSeeds[a]] != 0; };

    // plateNeighbors[a] in the Set's insertion order
    std::vector<std::vector<int32_t>> nbrs((size_t)P);
    for (int32_t a = 0; a < P; ++a) {
        const uint32_t* row = firstSlot + (size_t)a * (size_t)P;
        for (int32_t b = 0; b < P; ++b) if (b != a && row[b] != 0xFFFFFFFFu) nbrs[a].push_back(b);
        std::sort(nbrs[a].begin(), nbrs[a].end(), [&](int32_t x, int32_t y) { return row[x] < row[y]; });
    }

    // 3. connected components of same-kind plates (:41-62)
    std::vector<uint8_t> seen((size_t)P, 0);
    std::vector<std::vector<int32_t>> components;
    for (int32_t a = 0; a < P; ++a) {
        if (seen[a]) continue;
        const bool oc = ocean(a);
        std::vector<int32_t> queue{a};
        seen[a] = 1;
        for (size_t head = 0; head < queue.size(); ++head)
            for (int32_t nb : nbrs[queue[head]]) if (!seen[nb] && ocean(nb) == oc) { seen[nb] = 1; queue.push_back(nb); }
        components.push_back(std::move(queue));        // comp is the queue: every plate is pushed to both when it is popped / entered
    }

    // 4. split large components (:64-172)
    const int32_t target = std::max(2, std::min(20, js_round((double)P / 4.0)));
    int32_t next = 0;
    std::vector<int32_t> where((size_t)P, -1);          // position in the component being split
    for (const auto& comp : components) {
        const int32_t n = (int32_t)comp.size();
        const int32_t k = std::max(1, js_round((double)target * (double)n / (double)P));
        if (k <= 1) {
            for (int32_t a : comp) out.plateToSuper[a] = next;
            ++next;
            continue;
        }
        for (int32_t i = 0; i < n; ++i) where[comp[i]] = i;
        Split S{comp, std::vector<std::vector<int32_t>>((size_t)n), std::vector<double>((size_t)n), std::vector<double>((size_t)n), std::vector<uint8_t>((size_t)n)};
        for (int32_t i = 0; i < n; ++i) {
            for (int32_t nb : nbrs[comp[i]]) if (where[nb] >= 0) S.localAdj[i].push_back(where[nb]);
            S.edgeWeight[i] = std::sqrt((double)(area[comp[i]] != 0 ? area[comp[i]] : 1));
        }
        // farthest-point seeding (:123-136)
        std::vector<int32_t> seeds{0};
        S.dijkstra_from(seeds);
        for (int32_t si = 1; si < k; ++si) {
            int32_t farthest = 0; double maxDist = -1.0;
            for (int32_t i = 0; i < n; ++i) if (S.dist[i] > maxDist) { maxDist = S.dist[i]; farthest = i; }
            seeds.push_back(farthest);
            S.dijkstra_from(seeds);
        }
        // multi-source Dijkstra that carries the seed's super plate (:139-165)
        std::vector<int32_t> assignment((size_t)n, -1);
        std::vector<double> d((size_t)n, std::numeric_limits<double>::infinity());
        std::vector<uint8_t> visited((size_t)n, 0);
        for (size_t si = 0; si < seeds.size(); ++si) { assignment[seeds[si]] = next + (int32_t)si; d[seeds[si]] = 0.0; }
        for (int32_t iter = 0; iter < n; ++iter) {
            int32_t cur = -1; double minD = std::numeric_limits<double>::infinity();
            for (int32_t i = 0; i < n; ++i) if (!visited[i] && d[i] < minD) { minD = d[i]; cur = i; }
            if (cur == -1) break;
            visited[cur] = 1;
            for (int32_t nb : S.localAdj[cur]) {
                const double nd = d[cur] + S.edgeWeight[nb];
                if (nd < d[nb]) { d[nb] = nd; assignment[nb] = assignment[cur]; }
            }
        }
        for (int32_t i = 0; i < n; ++i) { out.plateToSuper[comp[i]] = assignment[i]; where[comp[i]] = -1; }
        next += (int32_t)seeds.size();
    }
    const int32_t numSuper = next;

    // 6. area-weighted Euler poles (:182-235)
    std::vector<double> Lx((size_t)numSuper, 0.0), Ly((size_t)numSuper, 0.0), Lz((size_t)numSuper, 0.0), omegaSum((size_t)numSuper, 0.0), areaSum((size_t)numSuper, 0.0);
    std::vector<int32_t> largest((size_t)numSuper, -1);
    for (int32_t a = 0; a < P; ++a) {
        const int32_t sp = out.plateToSuper[a], id = plateSeeds[a];
        if (!hasVec[id]) continue;
        const double ar = (double)area[a], om = omega[id];
        Lx[sp] += ar * om * pole[3 * (size_t)id]; Ly[sp] += ar * om * pole[3 * (size_t)id + 1]; Lz[sp] += ar * om * pole[3 * (size_t)id + 2];
        omegaSum[sp] += ar * std::fabs(om);
        areaSum[sp] += ar;
        if (largest[sp] < 0 || area[a] > area[largest[sp]]) largest[sp] = a;
    }
    for (int32_t sp = 0; sp < numSuper; ++sp) {
        const double lx = Lx[sp], ly = Ly[sp], lz = Lz[sp];
        const double lLen = std::sqrt(lx * lx + ly * ly + lz * lz);
        double* q = out.pole + 3 * (size_t)sp;
        if (lLen < 1e-8 || areaSum[sp] < 1.0) {
            if (largest[sp] >= 0) {                     // the first largest plate with a vector
                const int32_t id = plateSeeds[largest[sp]];
                q[0] = pole[3 * (size_t)id]; q[1] = pole[3 * (size_t)id + 1]; q[2] = pole[3 * (size_t)id + 2]; out.omega[sp] = omega[id];
            } else { q[0] = 0.0; q[1] = 1.0; q[2] = 0.0; out.omega[sp] = 0.0; }
            continue;
        }
        q[0] = lx / lLen; q[1] = ly / lLen; q[2] = lz / lLen;
        out.omega[sp] = omegaSum[sp] / areaSum[sp];
    }

    // 7. kind by majority area (:237-251), 8. area-weighted density (:253-270)
    std::vector<double> oceanArea((size_t)numSuper, 0.0), totalArea((size_t)numSuper, 0.0), densSum((size_t)numSuper, 0.0), densArea((size_t)numSuper, 0.0);
    for (int32_t a = 0; a < P; ++a) {
        const int32_t sp = out.plateToSuper[a];
        const double ar = (double)area[a], de = density[plateSeeds[a]];
        totalArea[sp] += ar;
        if (ocean(a)) oceanArea[sp] += ar;
        if (!std::isnan(de)) { densSum[sp] += ar * de; densArea[sp] += ar; }
    }
    for (int32_t sp = 0; sp < numSuper; ++sp) {
        out.isOcean[sp] = oceanArea[sp] > totalArea[sp] * 0.5 ? 1 : 0;
        out.density[sp] = densArea[sp] > 0.0 ? densSum[sp] / densArea[sp] : 2.7;
    }
    return numSuper;
}

}  // namespace wo

extern "C" int wo_super_plates_group(int32_t numPlateSeeds, const int32_t* plateSeeds, const wo_plate_table* plates, const int32_t* area,
                                     const uint32_t* firstSlot, int32_t* plateToSuper, int32_t* numSuper, double* superPole, double* superOmega,
                                     uint8_t* superIsOcean, double* superDensity) {
    if (!plateSeeds || !plates || !area || !firstSlot || !plateToSuper || !numSuper || !superPole || !superOmega || !superIsOcean || !superDensity) {
        wo::set_error("wo_super_plates_group: null pointer"); return 1;
    }
    if (!plates->hasVec || !plates->pole || !plates->omega || !plates->isOcean || !plates->density) { wo::set_error("wo_super_plates_group: null array in the plate table"); return 1; }
    if (numPlateSeeds < 1) { wo::set_error("wo_super_plates_group: numPlateSeeds must be positive"); return 1; }
    try {
        std::vector<int32_t> slotOf;
        wo::super_plate_slots(numPlateSeeds, plateSeeds, slotOf);
        *numSuper = wo::super_plates_group_host(numPlateSeeds, plateSeeds, plates->numIds, plates->hasVec, plates->pole, plates->omega, plates->isOcean,
                                                plates->density, area, firstSlot, wo::SuperPlateTables{plateToSuper, superPole, superOmega, superIsOcean, superDensity});
    } catch (const std::invalid_argument& e) { wo::set_error(std::string("wo_super_plates_group: ") + e.what()); return 1; }
      catch (const std::exception& e) { wo::set_error(std::string("wo_super_plates_group: ") + e.what()); return 3; }
    return 0;
}
