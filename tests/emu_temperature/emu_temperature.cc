// Test-only CPU emulator of the temperature stage and the Koppen classification: drives the bodies of csrc/temp_ops.h cell by
// cell in the loop order of the reference (js/temperature.js:69-237): one season after the other, diffuseOceanWarmth of a season
// with climate_ops.h's single-field bodies, the per-cell loop, the smoothField pass, then the normalisation as a loop of its own.
// `pair` != 0 runs the diffusion as the kernels do, both seasons of a cell at once.  Never linked into the product.
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../planet_heightmap_generation_amd/csrc/temp_ops.h"

namespace T = wo::temp;

namespace {
struct Count { uint64_t* c; void hit(int i) const { ++c[i]; } };
}  // namespace

extern "C" {

int32_t emu_temperature_branch_count() { return T::B_COUNT; }
int32_t emu_temperature_passes(int32_t N) { return T::warmth_passes(N); }

// itcz: itczLatsSummer, itczLatsWinter; precip / warmth / speed / out: [0] summer, [1] winter.  census: T::B_COUNT counters (added
// to), may be NULL.  Returns oceanWarmthPasses.
int32_t emu_temperature(int32_t N, const int32_t* off, const int32_t* adj, const float* elev, const float* lat, const float* lon, const uint8_t* isLand,
                        const float* cont, const float* plateCont, const float* const* itcz, const float* const* precip, const float* const* warmth,
                        const float* const* speed, double temperatureOffset, int32_t pair, float* const* out, uint64_t* census) {
    std::vector<uint64_t> own(T::B_COUNT, 0);
    const Count C{census ? census : own.data()};
    const int32_t passes = T::warmth_passes(N);
    const wo::ClimateMesh M{N, off, adj, nullptr};
    wo::Fields F{};
    F.N = N; F.off = off; F.adj = adj;
    std::vector<float> coastal[2];
    if (pair) {
        std::vector<T::G2> a(N), b(N);
        for (int32_t r = 0; r < N; ++r) a[r] = T::G2{{wo::warmth_seed_cell(warmth[0], isLand, r), wo::warmth_seed_cell(warmth[1], isLand, r)}};
        for (int32_t p = 0; p < passes; ++p) {
            for (int32_t r = 0; r < N; ++r) b[r] = T::warmth_diffuse_pair_cell(off, adj, a.data(), plateCont, r);
            a.swap(b);
        }
        for (int s = 0; s < 2; ++s) { coastal[s].resize(N); for (int32_t r = 0; r < N; ++r) coastal[s][r] = a[r].v[s]; }
    }
    for (int s = 0; s < 2; ++s) {
        if (!pair) {
            std::vector<float>& c = coastal[s];
            c.resize(N);
            std::vector<float> tmp(N);
            for (int32_t r = 0; r < N; ++r) c[r] = wo::warmth_seed_cell(warmth[s], isLand, r);
            for (int32_t p = 0; p < passes; ++p) {
                for (int32_t r = 0; r < N; ++r) tmp[r] = wo::warmth_diffuse_cell(M, c.data(), plateCont, r);
                c.swap(tmp);
            }
        }
        std::vector<float> temp(N), tmp(N);
        for (int32_t r = 0; r < N; ++r) {
            const T::CellIn I{lat[r], lon[r], elev[r], cont[r], plateCont[r], isLand[r] != 0};
            temp[r] = T::temperature_cell(I, s == 0, itcz[s], precip[s][r], warmth[s][r], speed[s][r], coastal[s][r], T::annual_curve(I.lat), temperatureOffset, C);
        }
        for (int32_t p = 0; p < T::SMOOTH_PASSES; ++p) {
            for (int32_t r = 0; r < N; ++r) tmp[r] = wo::smooth_field_cell(F, temp.data(), r);
            temp.swap(tmp);
        }
        for (int32_t r = 0; r < N; ++r) out[s][r] = T::normalise_cell(temp[r]);
    }
    return passes;
}

void emu_koppen(int32_t N, const float* elev, const float* tSummer, const float* tWinter, const float* pSummer, const float* pWinter, uint8_t* out, uint64_t* census) {
    std::vector<uint64_t> own(T::B_COUNT, 0);
    const Count C{census ? census : own.data()};
    for (int32_t r = 0; r < N; ++r) out[r] = T::koppen_cell(elev[r], tSummer[r], tWinter[r], pSummer[r], pWinter[r], C);
}

}  // extern "C"
