// generatePlates (reference: js/plates.js:6-232) and assignOceanLand (js/ocean-land.js:7-238) — native host stages.
//
// Both walk the (coarse, 20 000-cell) mesh in an order fixed by Park-Miller streams: seeds by farthest point with a draw
// among the top three, plates by round-robin frontier growth with sampled candidates, continents by round-robin growth
// over the plate graph.  Nothing here is order-free, so it is serial host code; it takes a few milliseconds and has no
// device part.  The outputs are the reference's bit for bit, which rests on these points:
//   * two independent streams in generatePlates: rng = ParkMiller(seed + 0.5) (a non-integer seed) and the integer
//     stream randInt(n) = floor(ParkMiller(seed)() * n); assignOceanLand draws from ParkMiller(seed + 42);
//   * minDistToSeed is a Float32Array: 1 - dot is formed in double from the f32 coordinates and stored rounded to f32,
//     and the top-three search and the `<` updates compare those f32 values (as doubles);
//   * the seed loop is unrolled by two in the reference (search, pick, fused update-and-search, pick, update): the
//     randInt(validCount) calls fall where the reference's do, and an odd plate count ends in the update-only branch;
//   * Sets keep insertion order (plateSeeds, plateAdj[pid], the ocean components, bordering); objects keyed by plate id
//     are only ever indexed, so they are arrays by slot (position in plateSeeds) here;
//   * Array.prototype.sort is stable in the reference's engine: std::stable_sort, descending score;
//   * Math.cos / Math.sin / Math.exp are V8's fdlibm ports: fd_cos / fd_sin / fd_exp of import_ops.h;
//   * no contraction of double arithmetic (the library compiles with -ffp-contract=off), every expression in the
//     reference's association.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <limits>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/worogen.h"
#include "host_util.h"
#include "import_ops.h"
#include "wo_internal.h"

namespace wo {
namespace {

constexpr double kPi = 3.141592653589793;                  // Math.PI

inline double sqrt_or_1(double x) { const double s = std::sqrt(x); return (s == 0.0 || s != s) ? 1.0 : s; }   // Math.sqrt(x) || 1
inline double js_round(double x) { return std::floor(x + 0.5); }                                              // Math.round: half up
inline double low_plate_t(int32_t numPlates) { return std::max(0.0, std::min(1.0, (80.0 - (double)numPlates) / 60.0)); }

struct Top3 {
    int32_t r0 = -1, r1 = -1, r2 = -1; double d0 = -1, d1 = -1, d2 = -1;
    inline void offer(int32_t r, double d) {
        if (d > d2) {
            if (d > d0) { r2 = r1; d2 = d1; r1 = r0; d1 = d0; r0 = r; d0 = d; }
            else if (d > d1) { r2 = r1; d2 = d1; r1 = r; d1 = d; }
            else { r2 = r; d2 = d; }
        }
    }
    int32_t valid() const { return (r0 != -1) + (r1 != -1) + (r2 != -1); }
    int32_t at(int32_t pick) const { return pick == 0 ? r0 : pick == 1 ? r1 : r2; }
};

void check_csr(int32_t N, const int32_t* off, const int32_t* adj) {
    if (off[0] != 0) throw std::invalid_argument("adjOffset[0] != 0");
    for (int32_t r = 0; r < N; ++r) if (off[r + 1] < off[r]) throw std::invalid_argument("adjOffset is not monotone");
    for (int32_t i = 0; i < off[N]; ++i) if (adj[i] < 0 || adj[i] >= N) throw std::invalid_argument("adjList entry out of range");
}

}  // namespace

// js/plates.js:6-232.  seedsOut / poleOut / omegaOut have room for min(numPlates, N) entries; returns the seed count.
int32_t generate_plates_host(int32_t N, const int32_t* off, const int32_t* adj, const float* xyz, int32_t numPlates, double seed,
                             int32_t* r_plate, int32_t* seedsOut, double* poleOut, double* omegaOut, int64_t* stats) {
    check_csr(N, off, adj);
    ParkMiller rng(seed + 0.5), rngInt(seed);
    auto randInt = [&](int32_t n) { return (int32_t)std::floor(rngInt.next() * (double)n); };
    auto X = [&](int64_t r, int k) { return (double)xyz[3 * r + k]; };
    auto dist1 = [&](int64_t r, double sx, double sy, double sz) { return 1.0 - (X(r, 0) * sx + X(r, 1) * sy + X(r, 2) * sz); };
    std::fill(r_plate, r_plate + N, -1);

    // :13-87 farthest-point seeds, a draw among the three farthest
    std::vector<int32_t> seeds;
    std::vector<uint8_t> isSeed(N, 0);
    std::vector<float> minDist(N);
    auto addSeed = [&](int32_t r) { seeds.push_back(r); isSeed[r] = 1; };
    auto update = [&](int32_t s) {
        const double sx = X(s, 0), sy = X(s, 1), sz = X(s, 2);
        for (int32_t r = 0; r < N; ++r) { const double d = dist1(r, sx, sy, sz); if (d < (double)minDist[r]) minDist[r] = (float)d; }
    };
    const int32_t firstSeed = randInt(N);
    addSeed(firstSeed);
    {
        const double sx = X(firstSeed, 0), sy = X(firstSeed, 1), sz = X(firstSeed, 2);
        for (int32_t r = 0; r < N; ++r) minDist[r] = (float)dist1(r, sx, sy, sz);
        minDist[firstSeed] = 0.0f;
    }
    while ((int32_t)seeds.size() < numPlates && (int32_t)seeds.size() < N) {
        Top3 t;
        for (int32_t r = 0; r < N; ++r) if (!isSeed[r]) t.offer(r, (double)minDist[r]);
        int32_t valid = t.valid();
        if (!valid) break;
        const int32_t s1 = t.at(randInt(valid));
        addSeed(s1);
        if ((int32_t)seeds.size() < numPlates) {
            const double sx = X(s1, 0), sy = X(s1, 1), sz = X(s1, 2);
            Top3 u;                                                        // fused: update from s1 and search for the next seed
            for (int32_t r = 0; r < N; ++r) {
                const double d = dist1(r, sx, sy, sz);
                if (d < (double)minDist[r]) minDist[r] = (float)d;
                if (!isSeed[r]) u.offer(r, (double)minDist[r]);
            }
            valid = u.valid();
            if (!valid) break;
            const int32_t s2 = u.at(randInt(valid));
            addSeed(s2);
            update(s2);
        } else {
            update(s1);                                                    // last seed of an odd count
        }
    }
    const int32_t P = (int32_t)seeds.size();

    // :90-115 growth rate, direction and directional strength per plate
    const double lowT = low_plate_t(numPlates);
    const double rateMin = 0.7 - 0.4 * lowT, rateRange = 2.3 + 2.4 * lowT, dirBase = 0.15 + 0.25 * lowT, dirScale = 0.25 + 0.25 * lowT;
    std::vector<double> rate(P), dirStrength(P), dir(3 * (size_t)P);
    for (int32_t i = 0; i < P; ++i) {
        const int32_t c = seeds[i];
        const double a = rng.next(), b = rng.next();
        rate[i] = rateMin + a * b * rateRange;
        const double px = X(c, 0), py = X(c, 1), pz = X(c, 2);
        const double pLen = sqrt_or_1(px * px + py * py + pz * pz);
        const double nx = px / pLen, ny = py / pLen, nz = pz / pLen;
        const double rx = rng.next() - 0.5, ry = rng.next() - 0.5, rz = rng.next() - 0.5;
        const double d = rx * nx + ry * ny + rz * nz;
        const double tx = rx - d * nx, ty = ry - d * ny, tz = rz - d * nz;
        const double tLen = sqrt_or_1(tx * tx + ty * ty + tz * tz);
        dir[3 * i] = tx / tLen; dir[3 * i + 1] = ty / tLen; dir[3 * i + 2] = tz / tLen;
        dirStrength[i] = std::min(0.85, rng.next() * (dirBase + dirScale / rate[i]));
    }

    // :118-196 round-robin frontier growth
    std::vector<std::vector<int32_t>> frontier(P);
    std::vector<double> area(P, 1.0);
    for (int32_t i = 0; i < P; ++i) { r_plate[seeds[i]] = seeds[i]; frontier[i].push_back(seeds[i]); }
    int64_t remaining = (int64_t)N - P;
    const double compactWeight = 0.3 - 0.22 * lowT;
    const double expectedArea = std::max(1.0, (double)(N - P) / (double)numPlates);
    const double governorMult = 2.0 + 2.0 * lowT;
    const double invN = 1.0 / (double)N;
    const double inf = std::numeric_limits<double>::infinity();
    while (remaining > 0) {
        bool anyProgress = false;
        for (int32_t i = 0; i < P; ++i) {
            std::vector<int32_t>& f = frontier[i];
            if (f.empty()) continue;
            const int32_t pid = seeds[i];
            const double d0 = dir[3 * i], d1 = dir[3 * i + 1], d2 = dir[3 * i + 2];
            const double dirStr = dirStrength[i], dirStrHalf = dirStr * 0.5;
            double steps = std::max(1.0, std::ceil(rate[i] * (0.5 + rng.next())));
            if (area[i] > expectedArea * governorMult) { steps = std::max(1.0, std::ceil(steps * 0.5)); if (stats) ++stats[WO_PGS_GOVERNOR_HALVED]; }
            const double expectedChord = std::sqrt((area[i] != 0.0 ? area[i] : 1.0) * invN / kPi) * 2.0;
            const double compactThreshold = expectedChord * 1.8;
            const double sx = X(pid, 0), sy = X(pid, 1), sz = X(pid, 2);
            for (double s = 0; s < steps && !f.empty(); s += 1.0) {
                size_t bestIdx = 0; double bestScore = -inf;
                const double want = 3.0 + std::floor(dirStr * 5.0);
                const size_t samples = (double)f.size() < want ? f.size() : (size_t)want;
                for (size_t k = 0; k < samples; ++k) {
                    const size_t idx = (size_t)randInt((int32_t)f.size());
                    const int64_t cell = f[idx];
                    const double dx = X(cell, 0) - sx, dy = X(cell, 1) - sy, dz = X(cell, 2) - sz;
                    const double dLenSq = dx * dx + dy * dy + dz * dz;
                    const double dLen = sqrt_or_1(dLenSq);
                    const double alignment = (dx * d0 + dy * d1 + dz * d2) / dLen;
                    const double excess = std::max(0.0, dLenSq * 0.5 - compactThreshold);
                    const double penalty = excess * (compactWeight * 4.0);
                    const double score = alignment * dirStr + rng.next() * (1.0 - dirStrHalf) - penalty;
                    if (score > bestScore) { bestScore = score; bestIdx = idx; }
                }
                const int32_t current = f[bestIdx];
                f[bestIdx] = f.back();
                f.pop_back();
                for (int32_t j = off[current]; j < off[current + 1]; ++j) {
                    const int32_t nb = adj[j];
                    if (r_plate[nb] == -1) { r_plate[nb] = pid; f.push_back(nb); area[i] += 1.0; --remaining; anyProgress = true; }
                }
            }
        }
        if (!anyProgress) break;
    }

    // :199-214 cells the growth could not reach take the plate of their first claimed neighbour (sweeps until none changes)
    for (bool orphans = true; orphans;) {
        orphans = false;
        for (int32_t r = 0; r < N; ++r) {
            if (r_plate[r] != -1) continue;
            for (int32_t j = off[r]; j < off[r + 1]; ++j) {
                const int32_t nb = adj[j];
                if (r_plate[nb] != -1) { r_plate[r] = r_plate[nb]; orphans = true; if (stats) ++stats[WO_PGS_ORPHANS]; break; }
            }
        }
    }

    smooth_reconnect_plates_host(N, off, adj, r_plate, P, seeds.data(), (int32_t)js_round(3.0 - 2.0 * lowT));   // :216

    // :219-229 Euler pole and angular velocity per plate
    for (int32_t i = 0; i < P; ++i) {
        const double theta = rng.next() * 2.0 * kPi;
        const double cosP = 2.0 * rng.next() - 1.0;
        const double sinP = std::sqrt(1.0 - cosP * cosP);
        poleOut[3 * i] = sinP * imp::fd_cos(theta); poleOut[3 * i + 1] = sinP * imp::fd_sin(theta); poleOut[3 * i + 2] = cosP;
        const double mag = 0.5 + rng.next() * 1.5;
        omegaOut[i] = mag * (rng.next() < 0.5 ? -1.0 : 1.0);
        seedsOut[i] = seeds[i];
    }
    return P;
}

// js/ocean-land.js:7-238.  isOceanOut: one flag per seed, in seed order.
void assign_ocean_land_host(int32_t N, const int32_t* off, const int32_t* adj, const int32_t* r_plate, int32_t P, const int32_t* plateIds,
                            const float* xyz, double seed, int32_t numContinents, double variety, double landCoverage,
                            uint8_t* isOceanOut, int64_t* stats) {
    check_csr(N, off, adj);
    ParkMiller rng(seed + 42.0);
    std::vector<int32_t> slotOf(N, -1);
    for (int32_t i = 0; i < P; ++i) {
        const int32_t pid = plateIds[i];
        if (pid < 0 || pid >= N) throw std::invalid_argument("plate seed out of range");
        if (slotOf[pid] != -1) throw std::invalid_argument("repeated plate seed");
        slotOf[pid] = i;
    }
    // a plate id that is not a seed makes the reference throw (its adjacency Set does not exist)
    std::vector<int32_t> slot(N);
    for (int32_t r = 0; r < N; ++r) {
        const int32_t p = r_plate[r];
        if (p < 0 || p >= N || slotOf[p] < 0) throw std::invalid_argument("r_plate holds a plate id that is not in plateSeeds");
        slot[r] = slotOf[p];
    }

    // :15-34 areas and centroids
    std::vector<double> area(P, 0.0), cen(3 * (size_t)P, 0.0);
    for (int32_t r = 0; r < N; ++r) {
        const int32_t s = slot[r];
        area[s] += 1.0;
        cen[3 * s] += (double)xyz[3 * (int64_t)r]; cen[3 * s + 1] += (double)xyz[3 * (int64_t)r + 1]; cen[3 * s + 2] += (double)xyz[3 * (int64_t)r + 2];
    }
    auto or1 = [](double v) { return v != 0.0 ? v : 1.0; };
    for (int32_t s = 0; s < P; ++s) { const double a = or1(area[s]); cen[3 * s] /= a; cen[3 * s + 1] /= a; cen[3 * s + 2] /= a; }

    // :37-51 plate adjacency (neighbour plates in the order they are first seen) and perimeter
    std::vector<std::vector<int32_t>> padj(P);
    std::vector<double> perim(P, 0.0);
    for (int32_t r = 0; r < N; ++r) {
        const int32_t my = slot[r];
        bool boundary = false;
        for (int32_t j = off[r]; j < off[r + 1]; ++j) {
            const int32_t nb = slot[adj[j]];
            if (nb != my) {
                if (std::find(padj[my].begin(), padj[my].end(), nb) == padj[my].end()) padj[my].push_back(nb);   // a plate has few neighbours
                boundary = true;
            }
        }
        if (boundary) perim[my] += 1.0;
    }

    // :54-63 compactness, normalised to the largest
    std::vector<double> compact(P);
    double maxCompact = 0.0;
    for (int32_t s = 0; s < P; ++s) { compact[s] = std::sqrt(or1(area[s])) / or1(perim[s]); if (compact[s] > maxCompact) maxCompact = compact[s]; }
    if (maxCompact > 0.0) for (int32_t s = 0; s < P; ++s) compact[s] /= maxCompact;

    const double targetLand = landCoverage * (double)N;
    struct Cand { int32_t slot; double score; };
    auto byScore = [](const Cand& a, const Cand& b) { return a.score > b.score; };      // (a, b) => b.score - a.score, stable

    // :68-99 continent seeds: farthest plate centroid weighted by size and compactness, a draw among the best three
    const int32_t effectiveNum = std::min(numContinents, P);
    std::vector<int32_t> cont;                            // continent seeds, by slot
    std::vector<uint8_t> chosen(P, 0);
    {
        const int32_t first = (int32_t)std::floor(rng.next() * (double)P);
        cont.push_back(first); chosen[first] = 1;
    }
    const double sqrtMean = std::sqrt((double)N / (double)P);
    for (int32_t s = 1; s < effectiveNum; ++s) {
        std::vector<Cand> cands;
        for (int32_t p = 0; p < P; ++p) {
            if (chosen[p]) continue;
            double minD = std::numeric_limits<double>::infinity();
            for (int32_t e : cont) {
                const double dx = cen[3 * p] - cen[3 * e], dy = cen[3 * p + 1] - cen[3 * e + 1], dz = cen[3 * p + 2] - cen[3 * e + 2];
                const double d = dx * dx + dy * dy + dz * dz;
                if (d < minD) minD = d;
            }
            const double rawArea = sqrtMean / std::sqrt(or1(area[p]));
            const double areaFactor = 1.0 + (rawArea - 1.0) * (1.0 - variety * 0.5);
            const double cf = 0.3 + 0.7 * compact[p];
            cands.push_back({p, minD * areaFactor * cf});
        }
        if (cands.empty()) break;
        std::stable_sort(cands.begin(), cands.end(), byScore);
        const size_t topK = std::min<size_t>(cands.size(), 3);
        const Cand pick = cands[(size_t)std::floor(rng.next() * (double)topK)];
        cont.push_back(pick.slot); chosen[pick.slot] = 1;
    }

    // :102-112 seeds alone past the land budget: drop the largest (the first of equals) until they fit
    double seedArea = 0.0;
    for (int32_t p : cont) seedArea += area[p];
    while (cont.size() > 1 && seedArea > targetLand) {
        size_t maxIdx = 0;
        for (size_t i = 1; i < cont.size(); ++i) if (area[cont[i]] > area[cont[maxIdx]]) maxIdx = i;
        seedArea -= area[cont[maxIdx]];
        chosen[cont[maxIdx]] = 0;
        cont.erase(cont.begin() + (std::ptrdiff_t)maxIdx);
        if (stats) ++stats[WO_PGS_SEEDS_TRIMMED];
    }

    // :115-146 continent of a plate (-1: none), growth targets
    std::vector<int32_t> plateCont(P, -1);
    const int32_t numC = (int32_t)cont.size();
    for (int32_t c = 0; c < numC; ++c) plateCont[cont[c]] = c;
    double landArea = seedArea;
    const double growTarget = targetLand * 0.9;
    std::vector<double> contTarget(numC), contArea(numC);
    for (int32_t c = 0; c < numC; ++c) contArea[c] = area[cont[c]];
    if (variety > 0.0 && numC > 1) {
        std::vector<double> w(numC);
        for (int32_t c = 0; c < numC; ++c) w[c] = imp::fd_exp((rng.next() - 0.5) * variety * 2.5);
        double total = 0.0;
        for (int32_t c = 0; c < numC; ++c) total = total + w[c];
        for (int32_t c = 0; c < numC; ++c) contTarget[c] = growTarget * w[c] / total;
    } else {
        const double equal = growTarget / (double)std::max(numC, 1);
        for (int32_t c = 0; c < numC; ++c) contTarget[c] = equal;
    }

    // :148-180 round-robin growth over the plate graph
    for (bool progress = true; progress && landArea < growTarget;) {
        progress = false;
        for (int32_t c = 0; c < numC && landArea < growTarget; ++c) {
            if (contArea[c] >= contTarget[c]) { if (stats) ++stats[WO_PGS_CONTINENT_AT_TARGET]; continue; }
            std::vector<Cand> cands;
            for (int32_t p = 0; p < P; ++p) {
                if (plateCont[p] != -1) continue;
                bool touchesSelf = false, touchesOther = false;
                int32_t sameCount = 0;
                for (int32_t a : padj[p]) {
                    const int32_t ac = plateCont[a];
                    if (ac == c) { touchesSelf = true; ++sameCount; }
                    else if (ac != -1) { touchesOther = true; break; }
                }
                if (touchesSelf && !touchesOther) cands.push_back({p, (double)sameCount + compact[p] * 3.0 + rng.next() * 0.5});
            }
            if (cands.empty()) continue;
            std::stable_sort(cands.begin(), cands.end(), byScore);
            const size_t topK = std::min<size_t>(cands.size(), 3);
            const Cand pick = cands[(size_t)std::floor(rng.next() * (double)topK)];
            plateCont[pick.slot] = c;
            contArea[c] += area[pick.slot];
            landArea += area[pick.slot];
            progress = true;
        }
    }

    // :183-206 components of ocean plates; the main ocean is the largest (the first of equals)
    std::vector<std::vector<int32_t>> comps;
    std::vector<uint8_t> visited(P, 0);
    for (int32_t p = 0; p < P; ++p) {
        if (plateCont[p] != -1 || visited[p]) continue;
        std::vector<int32_t> comp{p};
        visited[p] = 1;
        for (size_t qi = 0; qi < comp.size(); ++qi)
            for (int32_t a : padj[comp[qi]])
                if (plateCont[a] == -1 && !visited[a]) { visited[a] = 1; comp.push_back(a); }
        comps.push_back(std::move(comp));
    }
    auto compArea = [&](const std::vector<int32_t>& c) { double a = 0.0; for (int32_t p : c) a += area[p]; return a; };
    size_t mainIdx = 0;
    for (size_t i = 1; i < comps.size(); ++i) if (compArea(comps[i]) > compArea(comps[mainIdx])) mainIdx = i;

    // :208-230 an interior sea bordering exactly one continent joins it while the land stays under 1.1 x the target
    const double absorbCap = targetLand * 1.1;
    for (size_t i = 0; i < comps.size(); ++i) {
        if (i == mainIdx) continue;
        std::vector<int32_t> bordering;                   // continents, in the order they are first seen
        for (int32_t op : comps[i]) {
            for (int32_t a : padj[op])
                if (plateCont[a] != -1 && std::find(bordering.begin(), bordering.end(), plateCont[a]) == bordering.end()) bordering.push_back(plateCont[a]);
            if (bordering.size() > 1) break;
        }
        if (bordering.size() == 1) {
            const double ca = compArea(comps[i]);
            if (landArea + ca <= absorbCap) {
                for (int32_t op : comps[i]) plateCont[op] = bordering[0];
                landArea += ca;
                if (stats) ++stats[WO_PGS_SEA_ABSORBED];
            } else if (stats) ++stats[WO_PGS_SEA_REFUSED];
        } else if (bordering.size() > 1 && stats) ++stats[WO_PGS_SEA_TWO_CONTINENTS];
    }
    for (int32_t p = 0; p < P; ++p) isOceanOut[p] = plateCont[p] == -1 ? 1 : 0;           // :233-236
}

}  // namespace wo

extern "C" {

int wo_generate_plates(int32_t numRegions, const int32_t* adjOffset, const int32_t* adjList, const float* r_xyz, int32_t numPlates,
                       double seed, int32_t* r_plate, int32_t* plateSeeds, int32_t* numPlateSeeds, double* pole, double* omega,
                       int64_t* stats) {
    if (numRegions < 1 || !adjOffset || !adjList || !r_xyz || !r_plate || !plateSeeds || !numPlateSeeds || !pole || !omega) {
        wo::set_error("wo_generate_plates: bad arguments"); return 1;
    }
    if (numPlates < 1) { wo::set_error("wo_generate_plates: numPlates must be at least 1"); return 1; }
    if (!(seed == seed) || std::fabs(seed) > 1e12) { wo::set_error("wo_generate_plates: seed must be a finite number"); return 1; }
    if (stats) std::fill(stats, stats + WO_PLATES_GEN_STATS, (int64_t)0);
    try {
        *numPlateSeeds = wo::generate_plates_host(numRegions, adjOffset, adjList, r_xyz, numPlates, seed, r_plate, plateSeeds, pole, omega, stats);
    } catch (const std::invalid_argument& e) { wo::set_error(std::string("wo_generate_plates: ") + e.what()); return 1; }
      catch (const std::exception& e) { wo::set_error(std::string("wo_generate_plates: ") + e.what()); return 3; }
    return 0;
}

int wo_assign_ocean_land(int32_t numRegions, const int32_t* adjOffset, const int32_t* adjList, const int32_t* r_plate,
                         const int32_t* plateSeeds, int32_t numPlateSeeds, const float* r_xyz, double seed, int32_t numContinents,
                         double continentSizeVariety, double landCoverage, uint8_t* plateIsOcean, int64_t* stats) {
    if (numRegions < 1 || !adjOffset || !adjList || !r_plate || !plateSeeds || !r_xyz || !plateIsOcean) {
        wo::set_error("wo_assign_ocean_land: bad arguments"); return 1;
    }
    if (numPlateSeeds < 1 || numPlateSeeds > numRegions) { wo::set_error("wo_assign_ocean_land: numPlateSeeds must lie in 1 .. numRegions"); return 1; }
    if (!(seed == seed) || std::fabs(seed) > 1e12 || !(continentSizeVariety == continentSizeVariety) || !(landCoverage == landCoverage)) {
        wo::set_error("wo_assign_ocean_land: seed, continentSizeVariety and landCoverage must be numbers"); return 1;
    }
    if (stats) std::fill(stats, stats + WO_PLATES_GEN_STATS, (int64_t)0);
    try {
        wo::assign_ocean_land_host(numRegions, adjOffset, adjList, r_plate, numPlateSeeds, plateSeeds, r_xyz, seed, numContinents,
                                   continentSizeVariety, landCoverage, plateIsOcean, stats);
    } catch (const std::invalid_argument& e) { wo::set_error(std::string("wo_assign_ocean_land: ") + e.what()); return 1; }
      catch (const std::exception& e) { wo::set_error(std::string("wo_assign_ocean_land: ") + e.what()); return 3; }
    return 0;
}

int wo_v8_math(int32_t fn, int64_t n, const double* x, double* out) {
    if (fn < 0 || fn > 2 || n < 0 || (n > 0 && (!x || !out))) { wo::set_error("wo_v8_math: bad arguments"); return 1; }
    for (int64_t i = 0; i < n; ++i) out[i] = fn == 0 ? wo::imp::fd_sin(x[i]) : fn == 1 ? wo::imp::fd_cos(x[i]) : wo::imp::fd_exp(x[i]);
    return 0;
}

}  // extern "C"
