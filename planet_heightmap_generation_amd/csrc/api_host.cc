// extern "C" entry points that need no GPU: status, mesh producers, noise tables.
#include <cmath>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/worogen.h"
#include "host_util.h"
#include "wo_internal.h"
#include "noise.h"
#include "pick_ops.h"

namespace wo {
static thread_local std::string g_err;
void set_error(const std::string& msg) { g_err = msg; }
}  // namespace wo

extern "C" {

int wo_abi_version(void) { return WO_ABI_VERSION; }
const char* wo_last_error(void) { return wo::g_err.c_str(); }

int wo_fib_sphere_points(int32_t N, double jitter, double seed, float* r_xyz) {
    if (N < 1 || !r_xyz) { wo::set_error("wo_fib_sphere_points: bad arguments"); return 1; }
    wo::fib_sphere_points(N, jitter, seed, r_xyz);
    return 0;
}

int wo_sphere_delaunay(int32_t numRegions, const float* r_xyz, int32_t* triangles, int32_t* halfedges) {
    if (!r_xyz || !triangles || !halfedges) { wo::set_error("wo_sphere_delaunay: null pointer"); return 1; }
    std::string err;
    int rc = wo::sphere_delaunay(numRegions, r_xyz, triangles, halfedges, err);
    if (rc) wo::set_error(err);
    return rc;
}

int wo_sphere_reference_closure(int32_t numRegions, int32_t* triangles, int32_t* halfedges) {
    if (numRegions < 4 || !triangles || !halfedges) { wo::set_error("wo_sphere_reference_closure: bad arguments"); return 1; }
    const int32_t pole = numRegions - 1, numTri = 2 * numRegions - 4;
    const int64_t allSides = 3 * (int64_t)numTri;
    try {
        // the planar part: triangles without the pole, renumbered in their order; half-edges into the fan become -1
        std::vector<int32_t> newId(numTri, -1);
        int32_t kept = 0;
        for (int32_t t = 0; t < numTri; ++t) {
            for (int k = 0; k < 3; ++k) if (triangles[3 * t + k] < 0 || triangles[3 * t + k] >= numRegions) throw std::invalid_argument("triangle vertex out of range");
            if (triangles[3 * t] != pole && triangles[3 * t + 1] != pole && triangles[3 * t + 2] != pole) newId[t] = kept++;
        }
        std::vector<int32_t> nt(allSides, 0), nh(allSides, 0);
        std::vector<int32_t> unpaired;
        for (int32_t t = 0; t < numTri; ++t) {
            if (newId[t] < 0) continue;
            for (int k = 0; k < 3; ++k) {
                const int64_t so = 3 * (int64_t)t + k, sn = 3 * (int64_t)newId[t] + k;
                const int32_t h = halfedges[so];
                if (h < 0 || h >= allSides) throw std::invalid_argument("half-edge out of range");
                nt[sn] = triangles[so];
                nh[sn] = newId[h / 3] >= 0 ? 3 * newId[h / 3] + h % 3 : -1;
                if (nh[sn] < 0) unpaired.push_back((int32_t)sn);
            }
        }
        const int32_t numSides = 3 * kept, nu = (int32_t)unpaired.size();
        if (nu < 3 || kept + nu != numTri) throw std::invalid_argument("the pole fan does not close the hull");
        // js/sphere-mesh.js:55-88: fan triangles numbered along the hull walk that starts at the last unpaired side
        std::vector<int32_t> pointToSide(numRegions, -1);
        for (int32_t s : unpaired) pointToSide[nt[s]] = s;                   // a later side replaces an earlier one
        auto next = [](int32_t s) { return s % 3 == 2 ? s - 2 : s + 1; };
        int32_t s = unpaired.back();
        for (int32_t i = 0; i < nu; ++i) {
            if (s < 0) throw std::invalid_argument("the hull is not one closed walk");
            const int32_t ns = numSides + 3 * i;
            nh[s] = ns; nh[ns] = s;
            nt[ns] = nt[next(s)]; nt[ns + 1] = nt[s]; nt[ns + 2] = pole;
            const int32_t k = numSides + (3 * i + 4) % (3 * nu);
            nh[ns + 2] = k; nh[k] = ns + 2;
            s = pointToSide[nt[next(s)]];
        }
        std::copy(nt.begin(), nt.end(), triangles);
        std::copy(nh.begin(), nh.end(), halfedges);
    } catch (const std::invalid_argument& e) { wo::set_error(std::string("wo_sphere_reference_closure: ") + e.what()); return 1; }
      catch (const std::exception& e) { wo::set_error(std::string("wo_sphere_reference_closure: ") + e.what()); return 3; }
    return 0;
}

int wo_mesh_csr(int32_t numRegions, int32_t numSides, const int32_t* triangles, const int32_t* halfedges,
                int32_t* adjOffset, int32_t* adjList, int32_t* adjTriList) {
    if (!triangles || !halfedges || !adjOffset || !adjList) { wo::set_error("wo_mesh_csr: null pointer"); return 1; }
    std::string err;
    int rc = wo::mesh_csr(numRegions, numSides, triangles, halfedges, adjOffset, adjList, adjTriList, err);
    if (rc) wo::set_error(err);
    return rc;
}

int wo_neighbor_dist(int32_t numRegions, const int32_t* adjOffset, const int32_t* adjList,
                     const float* r_xyz, float* neighborDist) {
    if (!adjOffset || !adjList || !r_xyz || !neighborDist) { wo::set_error("wo_neighbor_dist: null pointer"); return 1; }
    wo::neighbor_dist(numRegions, adjOffset, adjList, r_xyz, neighborDist);
    return 0;
}

int wo_triangle_elevations(int32_t numTriangles, const int32_t* triangles, const float* r_elevation,
                           float* t_elevation) {
    if (!triangles || !r_elevation || !t_elevation) { wo::set_error("wo_triangle_elevations: null pointer"); return 1; }
    wo::parallel_ranges(numTriangles, [&](int64_t b, int64_t e, int) {
        for (int64_t t = b; t < e; ++t) {
            // (a + b + c) / 3 in double, stored as float32 (js/planet-worker.js:33-35)
            double s = (double)r_elevation[triangles[3 * t]] + (double)r_elevation[triangles[3 * t + 1]];
            s = s + (double)r_elevation[triangles[3 * t + 2]];
            t_elevation[t] = (float)(s / 3.0);
        }
    });
    return 0;
}

int wo_triangle_centers(int32_t numTriangles, const int32_t* triangles, const float* r_xyz, float* t_xyz) {
    if (numTriangles < 0 || !triangles || !r_xyz || !t_xyz) { wo::set_error("wo_triangle_centers: bad arguments"); return 1; }
    wo::parallel_ranges(numTriangles, [&](int64_t b, int64_t e, int) {
        for (int64_t t = b; t < e; ++t) {
            const int64_t a = triangles[3 * t], c1 = triangles[3 * t + 1], c2 = triangles[3 * t + 2];
            for (int k = 0; k < 3; ++k) {
                // (r_xyz[3a+k] + r_xyz[3b+k] + r_xyz[3c+k]) / 3 in double, stored as float32 (js/sphere-mesh.js:214-216)
                double s = (double)r_xyz[3 * a + k] + (double)r_xyz[3 * c1 + k];
                s = s + (double)r_xyz[3 * c2 + k];
                t_xyz[3 * t + k] = (float)(s / 3.0);
            }
        }
    });
    return 0;
}

int wo_noise_tables(double seed, uint8_t* perm512, uint8_t* pm12_512) {
    if (!perm512 || !pm12_512) { wo::set_error("wo_noise_tables: null pointer"); return 1; }
    wo::noise_tables(seed, perm512, pm12_512);
    return 0;
}

int wo_noise_point(const uint8_t* perm512, const uint8_t* pm12_512, int32_t kind, int32_t octaves, double p0, double p1, double p2,
                   double x, double y, double z, double* out) {
    if (!perm512 || !pm12_512 || !out || kind < 0 || kind > 2) { wo::set_error("wo_noise_point: bad arguments"); return 1; }
    *out = kind == 0 ? wo::noise3d(perm512, pm12_512, x, y, z)
         : kind == 1 ? wo::fbm(perm512, pm12_512, x, y, z, octaves, p0)
                     : wo::ridged_fbm(perm512, pm12_512, x, y, z, octaves, p0, p1, p2);
    return 0;
}

int wo_smooth_reconnect_plates(int32_t numRegions, const int32_t* adjOffset, const int32_t* adjList, int32_t* r_plate,
                               const int32_t* plateSeeds, int32_t numPlateSeeds, int32_t numPasses) {
    if (numRegions < 1 || !adjOffset || !adjList || !r_plate || numPlateSeeds < 0 || (numPlateSeeds > 0 && !plateSeeds)) {
        wo::set_error("wo_smooth_reconnect_plates: bad arguments"); return 1;
    }
    try {
        wo::smooth_reconnect_plates_host(numRegions, adjOffset, adjList, r_plate, numPlateSeeds, plateSeeds, numPasses);
    } catch (const std::exception& e) { wo::set_error(std::string("wo_smooth_reconnect_plates: ") + e.what()); return 3; }
    return 0;
}

int wo_land_components(int32_t numRegions, const int32_t* adjOffset, const int32_t* adjList, const uint8_t* r_isOcean,
                       int32_t* label) {
    if (numRegions < 1 || !adjOffset || !adjList || !r_isOcean || !label) { wo::set_error("wo_land_components: bad arguments"); return 1; }
    if (adjOffset[0] != 0) { wo::set_error("wo_land_components: adjOffset[0] != 0"); return 1; }
    for (int32_t r = 0; r < numRegions; ++r) if (adjOffset[r + 1] < adjOffset[r]) { wo::set_error("wo_land_components: adjOffset is not monotone"); return 1; }
    for (int32_t i = 0; i < adjOffset[numRegions]; ++i) if (adjList[i] < 0 || adjList[i] >= numRegions) { wo::set_error("wo_land_components: adjList entry out of range"); return 1; }
    try {
        wo::mesh_components(numRegions, adjOffset, adjList, [&](int32_t r) { return r_isOcean[r] == 0; }, [](int32_t, int32_t) { return true; }, label);
        wo::parallel_ranges(numRegions, [&](int64_t b, int64_t e, int) { for (int64_t r = b; r < e; ++r) if (r_isOcean[r]) label[r] = -1; });
    } catch (const std::exception& e) { wo::set_error(std::string("wo_land_components: ") + e.what()); return 3; }
    return 0;
}

// ---- the editor's hit test, host front ends (pick_ops.h; js/edit-mode.js:43-59, :77-92): no device is touched ----
static bool pick_front_args_ok(const char* fn, int32_t numQueries, const void* in, const char* inName, const double* directionsOut, const uint8_t* validOut) {
    const std::string F = std::string(fn) + ": ";
    if (numQueries < 0 || numQueries > wo::pick::MAX_QUERIES) { wo::set_error(F + "numQueries is " + std::to_string(numQueries) + ", it must lie in [0, " + std::to_string(wo::pick::MAX_QUERIES) + "]"); return false; }
    if (!in || !directionsOut || !validOut) { wo::set_error(F + (!in ? inName : !directionsOut ? "directionsOut" : "validOut") + " is NULL"); return false; }
    return true;
}

int wo_pick_directions_globe(int32_t numQueries, const double* rays, double* directionsOut, uint8_t* validOut) {
    if (!pick_front_args_ok("wo_pick_directions_globe", numQueries, rays, "rays", directionsOut, validOut)) return 1;
    for (int32_t i = 0; i < numQueries; ++i) validOut[i] = wo::pick::direction_globe(rays + 6 * (int64_t)i, directionsOut + 3 * (int64_t)i) ? 1 : 0;
    return 0;
}

int wo_pick_directions_map(int32_t numQueries, const double* points, double centerLon, double* directionsOut, uint8_t* validOut) {
    if (!pick_front_args_ok("wo_pick_directions_map", numQueries, points, "points", directionsOut, validOut)) return 1;
    for (int32_t i = 0; i < numQueries; ++i) validOut[i] = wo::pick::direction_map(points[2 * (int64_t)i], points[2 * (int64_t)i + 1], centerLon, directionsOut + 3 * (int64_t)i) ? 1 : 0;
    return 0;
}

}  // extern "C"
