// Stand-alone host program for a sanitizer run of the plate-generation stages (csrc/plates_gen_host.cc): builds the coarse mesh
// with the library's own mesh producer and calls wo_generate_plates and wo_assign_ocean_land on three cases of the test table
// (an odd plate count, the seed trim, interior seas), plus the argument refusals.  CPU only, no GPU call, not loaded into Python.
//
//   cd planet_heightmap_generation_amd/csrc && g++ -std=c++17 -O1 -g -fno-omit-frame-pointer -ffp-contract=off -fsanitize=address,undefined \
//       -fno-sanitize-recover=undefined ../../tools/sanitize/plates_gen_main.cc api_host.cc mesh_builder.cc noise_host.cc plates_host.cc \
//       plates_gen_host.cc -lpthread -o /tmp/plates_gen_asan && /tmp/plates_gen_asan
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../include/worogen.h"

#define CHECK(call) do { if ((call) != 0) { std::fprintf(stderr, "%s failed: %s\n", #call, wo_last_error()); return 1; } } while (0)

static int run_case(double seed, int32_t P, int32_t numContinents, double variety, double coverage) {
    const int32_t N = 20000, V = N + 1, ns = 3 * (2 * V - 4);
    std::vector<float> xyz(3 * (size_t)V);
    CHECK(wo_fib_sphere_points(N, 0.75, seed + 137, xyz.data()));
    std::vector<int32_t> tri(ns), he(ns), off(V + 1), adj(ns);
    CHECK(wo_sphere_delaunay(V, xyz.data(), tri.data(), he.data()));
    CHECK(wo_sphere_reference_closure(V, tri.data(), he.data()));
    CHECK(wo_mesh_csr(V, ns, tri.data(), he.data(), off.data(), adj.data(), nullptr));
    adj.resize(off[V]);                                  // exact size: an index past the list is a heap overflow the sanitizer sees
    std::vector<int32_t> r_plate(V), seeds(P);
    std::vector<double> pole(3 * (size_t)P), omega(P);
    int32_t n = 0; int64_t st1[WO_PLATES_GEN_STATS], st2[WO_PLATES_GEN_STATS];
    CHECK(wo_generate_plates(V, off.data(), adj.data(), xyz.data(), P, seed, r_plate.data(), seeds.data(), &n, pole.data(), omega.data(), st1));
    seeds.resize(n);
    std::vector<uint8_t> isOcean(n);
    CHECK(wo_assign_ocean_land(V, off.data(), adj.data(), r_plate.data(), seeds.data(), n, xyz.data(), seed, numContinents, variety, coverage, isOcean.data(), st2));
    int oceans = 0; for (uint8_t f : isOcean) oceans += f;
    std::printf("seed %g P %d: %d seeds, %d oceanic; governor %lld orphans %lld trimmed %lld at-target %lld absorbed %lld refused %lld two-continents %lld\n",
                seed, P, n, oceans, (long long)st1[WO_PGS_GOVERNOR_HALVED], (long long)st1[WO_PGS_ORPHANS], (long long)st2[WO_PGS_SEEDS_TRIMMED],
                (long long)st2[WO_PGS_CONTINENT_AT_TARGET], (long long)st2[WO_PGS_SEA_ABSORBED], (long long)st2[WO_PGS_SEA_REFUSED], (long long)st2[WO_PGS_SEA_TWO_CONTINENTS]);
    // refusals: no out-of-range read before the message
    std::vector<int32_t> bad(adj); bad[5] = V;
    if (wo_generate_plates(V, off.data(), bad.data(), xyz.data(), P, seed, r_plate.data(), seeds.data(), &n, pole.data(), omega.data(), nullptr) == 0) return 1;
    if (wo_generate_plates(V, off.data(), adj.data(), xyz.data(), 0, seed, r_plate.data(), seeds.data(), &n, pole.data(), omega.data(), nullptr) == 0) return 1;
    if (n > 1 && wo_assign_ocean_land(V, off.data(), adj.data(), r_plate.data(), seeds.data(), n - 1, xyz.data(), seed, 4, 0, 0.3, isOcean.data(), nullptr) == 0) return 1;
    return 0;
}

int main() {
    if (run_case(5, 7, 12, 1.0, 0.1)) return 1;          // odd count ("last seed" branch), many continents on little land
    if (run_case(29, 50, 60, 0.5, 0.6)) return 1;        // every plate a continent seed: trim, seas between two continents
    if (run_case(1, 1, 4, 0.0, 0.3)) return 1;           // one plate: the growth stops early, the orphan sweep fills the rest
    std::puts("plates_gen: three cases and the refusals ran clean");
    return 0;
}
