// Stand-alone host program for a sanitizer run of the outline's shared bodies (csrc/outline_ops.h): on an octahedron and on an
// icosahedron subdivided three times it drives classify, the boundary flags, succ as slots, the doubling rounds on two buffers and
// the ring scatter, every array exactly as long as the device's, and holds the rings to a serial walk along succ.  Fields: no ring at
// all, one cell, every cell a class of its own, and a spiral band.  CPU only, no GPU call, not loaded into Python.
//
//   g++ -std=c++17 -O1 -g -fno-omit-frame-pointer -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       tools/sanitize/outline_main.cc -o /tmp/outline_asan && /tmp/outline_asan
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <map>
#include <utility>
#include <vector>

#include "../../planet_heightmap_generation_amd/csrc/outline_ops.h"

namespace O = wo::outline;

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED %s (line %d)\n", #cond, __LINE__); ++failures; } } while (0)

struct Mesh { std::vector<float> xyz; std::vector<int32_t> tri, he; int32_t cells() const { return (int32_t)xyz.size() / 3; } };

static void normalise(std::vector<float>& xyz) {
    for (size_t i = 0; i < xyz.size(); i += 3) {
        const double l = std::sqrt((double)xyz[i] * xyz[i] + (double)xyz[i + 1] * xyz[i + 1] + (double)xyz[i + 2] * xyz[i + 2]);
        for (int k = 0; k < 3; ++k) xyz[i + k] = (float)(xyz[i + k] / l);
    }
}

static void link(Mesh& m) {
    std::map<std::pair<int32_t, int32_t>, int32_t> sideOf;
    const int32_t n = (int32_t)m.tri.size();
    for (int32_t s = 0; s < n; ++s) sideOf[{m.tri[s], m.tri[O::next_side(s)]}] = s;
    m.he.assign(n, -1);
    for (int32_t s = 0; s < n; ++s) {
        const auto twin = sideOf.find({m.tri[O::next_side(s)], m.tri[s]});
        CHECK(twin != sideOf.end());
        if (twin != sideOf.end()) m.he[s] = twin->second;
    }
    for (int32_t s = 0; s < n; ++s) CHECK(m.he[s] >= 0 && m.he[m.he[s]] == s);
}

static Mesh octahedron() {
    Mesh m;
    m.xyz = {1, 0, 0, -1, 0, 0, 0, 1, 0, 0, -1, 0, 0, 0, 1, 0, 0, -1};
    m.tri = {0, 2, 4, 2, 1, 4, 1, 3, 4, 3, 0, 4, 2, 0, 5, 1, 2, 5, 3, 1, 5, 0, 3, 5};
    link(m);
    return m;
}

static Mesh icosphere(int levels) {
    const float t = (float)((1.0 + std::sqrt(5.0)) / 2.0);
    Mesh m;
    m.xyz = {-1, t, 0, 1, t, 0, -1, -t, 0, 1, -t, 0, 0, -1, t, 0, 1, t, 0, -1, -t, 0, 1, -t, t, 0, -1, t, 0, 1, -t, 0, -1, -t, 0, 1};
    m.tri = {0, 11, 5, 0, 5, 1, 0, 1, 7, 0, 7, 10, 0, 10, 11, 1, 5, 9, 5, 11, 4, 11, 10, 2, 10, 7, 6, 7, 1, 8,
             3, 9, 4, 3, 4, 2, 3, 2, 6, 3, 6, 8, 3, 8, 9, 4, 9, 5, 2, 4, 11, 6, 2, 10, 8, 6, 7, 9, 8, 1};
    for (int l = 0; l < levels; ++l) {
        std::map<std::pair<int32_t, int32_t>, int32_t> mid;
        const auto midpoint = [&](int32_t a, int32_t b) {
            const std::pair<int32_t, int32_t> key{a < b ? a : b, a < b ? b : a};
            const auto it = mid.find(key);
            if (it != mid.end()) return it->second;
            const int32_t v = (int32_t)m.xyz.size() / 3;
            for (int k = 0; k < 3; ++k) m.xyz.push_back((m.xyz[3 * a + k] + m.xyz[3 * b + k]) / 2);
            mid[key] = v;
            return v;
        };
        std::vector<int32_t> next;
        for (size_t f = 0; f < m.tri.size(); f += 3) {
            const int32_t a = m.tri[f], b = m.tri[f + 1], c = m.tri[f + 2];
            const int32_t ab = midpoint(a, b), bc = midpoint(b, c), ca = midpoint(c, a);
            for (int32_t v : {a, ab, ca, b, bc, ab, c, ca, bc, ab, bc, ca}) next.push_back(v);
        }
        m.tri.swap(next);
    }
    normalise(m.xyz);
    link(m);
    return m;
}

struct Result { std::vector<int32_t> sides, ringStart, ringClass, ringOfSide; int32_t longest = 0, rounds = 0; };

// the device's steps, every array exactly as long as the device allocates it
static Result trace(const Mesh& m, const std::vector<int32_t>& cls, int32_t onlyClass) {
    const int32_t n = (int32_t)m.tri.size();
    const int32_t *tri = m.tri.data(), *he = m.he.data();
    std::vector<int32_t> slotOf(n, -1), sideOf;
    for (int32_t s = 0; s < n; ++s)
        if (O::is_boundary(tri, he, cls.data(), onlyClass, s)) { slotOf[s] = (int32_t)sideOf.size(); sideOf.push_back(s); }
    sideOf.shrink_to_fit();
    const int32_t M = (int32_t)sideOf.size();
    Result r;
    r.ringStart.push_back(0);
    if (M == 0) return r;
    std::vector<int32_t> succSlot(M);
    std::vector<O::Rank> a(M), b(M);
    for (int32_t i = 0; i < M; ++i) {
        const int32_t s = sideOf[i], t = O::succ_side(tri, he, cls.data(), s);
        CHECK(slotOf[t] >= 0 && O::pred_side(tri, he, cls.data(), t) == s && he[s] / 3 == t / 3);
        succSlot[i] = slotOf[t] >= 0 ? slotOf[t] : i;
        a[i] = O::rank_start(i, succSlot[i]);
    }
    r.rounds = O::rank_rounds(M);
    for (int32_t k = 0; k < r.rounds; ++k) {
        for (int32_t i = 0; i < M; ++i) b[i] = O::rank_round(a[i], a[a[i].jump], (int32_t)1 << k);
        a.swap(b);
    }
    std::vector<int32_t> ringOfSlot(M, -1), ringLen;
    int32_t at = 0;
    for (int32_t i = 0; i < M; ++i) {
        if (a[i].least != i) continue;
        const int32_t len = a[succSlot[i]].dist + 1;
        ringOfSlot[i] = (int32_t)ringLen.size();
        r.ringStart.back() = at;
        r.ringStart.push_back(0);
        r.ringClass.push_back(cls[tri[sideOf[i]]]);
        ringLen.push_back(len);
        at += len;
        if (len > r.longest) r.longest = len;
    }
    r.ringStart.back() = M;
    CHECK(at == M);
    r.sides.assign(M, -1);
    r.ringOfSide.assign(M, -1);
    for (int32_t i = 0; i < M; ++i) {
        const int32_t ring = ringOfSlot[a[i].least];
        CHECK(ring >= 0);
        if (ring < 0) continue;
        const int32_t pos = r.ringStart[ring] + O::rank_in_ring(ringLen[ring], a[i].dist);
        CHECK(pos >= 0 && pos < M && r.sides[pos] == -1);
        if (pos < 0 || pos >= M) continue;
        r.sides[pos] = sideOf[i];
        r.ringOfSide[pos] = ring;
    }
    return r;
}

// the same rings by walking succ from every ring's lowest side
static Result walk(const Mesh& m, const std::vector<int32_t>& cls, int32_t onlyClass) {
    const int32_t n = (int32_t)m.tri.size();
    std::vector<uint8_t> seen(n, 0);
    Result r;
    for (int32_t s = 0; s < n; ++s) {
        if (seen[s] || !O::is_boundary(m.tri.data(), m.he.data(), cls.data(), onlyClass, s)) continue;
        r.ringStart.push_back((int32_t)r.sides.size());
        r.ringClass.push_back(cls[m.tri[s]]);
        int32_t len = 0;
        for (int32_t t = s; !seen[t]; t = O::succ_side(m.tri.data(), m.he.data(), cls.data(), t)) {
            seen[t] = 1;
            r.sides.push_back(t);
            r.ringOfSide.push_back((int32_t)r.ringClass.size() - 1);
            ++len;
        }
        if (len > r.longest) r.longest = len;
    }
    r.ringStart.push_back((int32_t)r.sides.size());
    return r;
}

static void run(const char* meshName, const Mesh& m, const char* field, const std::vector<int32_t>& cls, int32_t onlyClass = -1) {
    const Result got = trace(m, cls, onlyClass), want = walk(m, cls, onlyClass);
    CHECK(got.sides == want.sides && got.ringStart == want.ringStart && got.ringClass == want.ringClass && got.ringOfSide == want.ringOfSide && got.longest == want.longest);
    std::vector<float> pos(3 * got.sides.size());
    std::vector<double> ll(2 * got.sides.size());
    std::vector<float> e(m.cells(), 0.25f);
    for (size_t k = 0; k < got.sides.size(); ++k) {
        const int32_t t3 = got.sides[k] - got.sides[k] % 3;
        O::vertex_position(m.tri.data() + t3, m.xyz.data(), e.data(), 0, 1.002, pos.data() + 3 * k);
        const wo::map::LonLat v = O::vertex_lonlat(m.tri.data() + t3, m.xyz.data(), 0);
        ll[2 * k] = v.lon; ll[2 * k + 1] = v.lat;
        CHECK(pos[3 * k] == pos[3 * k] && v.lon == v.lon);
    }
    std::printf("%-12s %-14s onlyClass %2d: %5zu boundary sides, %4zu rings, longest %4d, %2d rounds\n", meshName, field, onlyClass, got.sides.size(), got.ringClass.size(),
                got.longest, got.rounds);
}

int main() {
    const Mesh meshes[2] = {octahedron(), icosphere(3)};
    const char* names[2] = {"octahedron", "icosphere 3"};
    for (int k = 0; k < 2; ++k) {
        const Mesh& m = meshes[k];
        const int32_t n = m.cells();
        CHECK((int32_t)m.tri.size() == 3 * (2 * n - 4));
        std::vector<int32_t> cls(n, 7);
        run(names[k], m, "constant", cls);
        cls.assign(n, 0); cls[n / 2] = 1;
        run(names[k], m, "one cell", cls);
        run(names[k], m, "one cell", cls, 1);
        for (int32_t r = 0; r < n; ++r) cls[r] = r;
        run(names[k], m, "all different", cls);
        for (int32_t r = 0; r < n; ++r) {
            const double lat = std::asin((double)m.xyz[3 * r + 1]), lon = std::atan2((double)m.xyz[3 * r], (double)m.xyz[3 * r + 2]);
            const double phase = lon / 6.283185307179586 + (k == 0 ? 1.0 : 4.0) * (lat + 1.5707963267948966) / 3.141592653589793;
            cls[r] = phase - std::floor(phase) < 0.5 && std::fabs(lat) < 1.3 ? 1 : 0;
        }
        run(names[k], m, "spiral", cls);
        run(names[k], m, "spiral", cls, 0);
        O::Levels L{};
        L.n = 3; L.v[0] = -0.5f; L.v[1] = 0.0f; L.v[2] = 0.5f;
        for (int32_t r = 0; r < n; ++r) cls[r] = O::class_levels(m.xyz[3 * r + 1], L);
        run(names[k], m, "levels", cls);
    }
    const float bad[3] = {0.0f, 1.0f, 1.0f};
    CHECK(O::levels_offender(bad, 3) == 2 && O::levels_offender(bad, 2) == -1);
    CHECK(O::rank_rounds(0) == 1 && O::rank_rounds(2) == 1 && O::rank_rounds(3) == 2 && O::rank_rounds(1024) == 10 && O::rank_rounds(1025) == 11 && O::rank_rounds((1 << 30) - 3) == 30);
    std::printf("%d failures\n", failures);
    return failures ? 1 : 0;
}
