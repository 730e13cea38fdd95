/*
 * worogen.h — C ABI of libworogen, the MI355X-native implementation of World Orogen's per-cell
 * terrain pipeline (reference: raguilar011095/planet_heightmap_generation, js/terrain-post.js,
 * js/simplex-noise.js, js/rng.js, js/sphere-mesh.js; further on the climate stages and, from js/planet-mesh.js,
 * the map export and the map view's layers and centre meridian).
 *
 * This is the drop-in boundary: plain pointers and sizes, no torch / HIP types.  The N-API shim
 * (planet_heightmap_generation_amd/napi/worogen_napi.cc) and the Python ctypes loader
 * (planet_heightmap_generation_amd/capi.py) bind exactly these symbols.  Every entry point cites the
 * reference interface it replaces (paths relative to the reference repository root).
 *
 * Conventions
 *   - every function returning int returns 0 on success, non-zero on failure; the message is then
 *     available from wo_last_error() (thread-local, valid until the next failing call on the thread).
 *     The JS/Python hosts turn a non-zero status into a thrown Error/exception, which is how the
 *     reference reports failures (exceptions caught by js/planet-worker.js:336-338).
 *   - host pointers are borrowed for the duration of the call only.
 *   - "numRegions" is the reference's mesh.numRegions (requested N + 1: the pole cell is appended,
 *     js/sphere-mesh.js:179-184).  CSR arrays are mesh.adjOffset (numRegions+1) / mesh.adjList.
 *   - device entry points fail (never fall back to the CPU) when no HIP device is usable.
 *   - threading: a wo_ctx (device + stream) and the planets created on it belong to one host thread at a time, like
 *     the reference's single worker.  Different contexts may be driven from different threads concurrently (the
 *     library keeps no shared mutable state); several planets in flight on one GPU this way raise throughput ~2x
 *     (DESIGN.md section 7).
 *
 * Environment (every variable the library reads; read once per API call or flood call, never inside a pass)
 *   sizing       WO_HOST_THREADS=<n>        workers of the host-side parallel sweeps (default: the process's CPUs, <= 64)
 *                WO_FLOOD_THREADS=<n>       workers of the priority flood's per-landmass walks (default 24)
 *                WO_FLOOD_PIN=1             the walk of the largest landmass keeps its CPU and the other flood workers keep off its L3
 *                                           (the library touches no thread affinity unless asked)
 *   routes       WO_LAYOUT=index            erodeComposite on the planet's own cell order instead of the land-first Morton mirror
 *   (same bits)  WO_TILE_LDS=1              receivers / thermal passes stage their tile's neighbour window in LDS (measured no faster)
 *                WO_FLOOD=device            pass 1 of the flood as the device label-correcting fixed point (exact, ~16x slower than the host walk)
 *                WO_FLOOD_HOST=two-phase    host flood: pass 1 of all landmasses, then passes 2 / 3 (default: pipelined per landmass)
 *                WO_FLOOD_HOST=serial       host flood: the reference's single heap, one thread (WO_FLOOD_HOST is read once per process)
 *   relaxed      WO_RELAXED=full            NOT the reference's semantics: one sort per flood, affine solve, Jacobi carve
 *   (labelled)   WO_RELAXED_SORT_EVERY=<k>  NOT the reference's semantics: landCells re-sorted every k-th iteration only
 *   diagnostics  WO_FLOOD_TIMING=1          laps of the flood stage and of a new terrain's set-up -> stderr
 *                WO_STAGE_TIMING=all        wo_last_stage_timing brackets every iteration instead of every 8th
 *                WO_ELEV_TIMING=1           laps of assignElevation's host stage -> stderr
 *   tests only   WO_TEST_HOOKS=k=v,k=v      the test suite's hooks (csrc/host_util.h: forced undecided landmasses, replay cuts, a wrong basin
 *                                           layout, a carve launch that gives up, ...); never set in production
 * (The Python loader additionally honours WO_LIBWOROGEN=<path to the .so>; bench.py has WO_BENCH_* switches of its own.)
 */
#ifndef WOROGEN_H
#define WOROGEN_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define WO_ABI_VERSION 1

typedef struct wo_ctx wo_ctx;       /* one HIP device + stream + scratch pools                     */
typedef struct wo_planet wo_planet; /* device-resident mesh + fields; mirrors the worker's retained
                                       state W (js/planet-worker.js:22,277-292)                     */

/* ---------------------------------------------------------------- status ---------------------- */
int         wo_abi_version(void);
const char* wo_last_error(void);
/* number of usable HIP devices (0 when none / no driver); never fails */
int         wo_device_count(void);
/* What the library holds at this moment, over all contexts and planets of the process: bytes of device memory, bytes of
 * pinned host memory, and the number of allocations it has made so far (a call that leaves this number as it was
 * allocated nothing).  Any pointer may be NULL; returns 0. */
int         wo_memory_in_use(int64_t* deviceBytes, int64_t* pinnedBytes, int64_t* allocCalls);

/* ------------------------------------------------ host-side input producers (no GPU needed) --- */
/* generateFibonacciSphere + pole append: js/sphere-mesh.js:9-37,179-181.  r_xyz has 3*(N+1) floats;
 * `seed` is what the caller passes to makeRng (js/rng.js:3). */
int wo_fib_sphere_points(int32_t N, double jitter, double seed, float* r_xyz);
/* Spherical Delaunay of numRegions unit vectors == the reference's stereographic Delaunator run +
 * addPoleToMesh (js/sphere-mesh.js:41-90,174-186).  triangles / halfedges have 3*(2*numRegions-4)
 * entries, counter-clockwise seen from outside, same contract as Delaunator's arrays.  Status: 1 bad arguments (a NULL
 * pointer, fewer than 4 points, a zero-length point), 2 star construction failed: a star of more than 48 neighbours or a duplicate
 * point, or, with a message of its own, a point set whose hull does not hold the sphere's centre strictly inside (points inside a
 * hemisphere have no triangulation of the sphere, and are refused instead of answered with their hull), 3 triangle count != 2V-4,
 * 4 unmatched half-edges.  Nothing is written to the outputs on status 1 and 2. */
int wo_sphere_delaunay(int32_t numRegions, const float* r_xyz, int32_t* triangles, int32_t* halfedges);
/* Renumbers the closing fan of a triangulation from wo_sphere_delaunay (the pole is region numRegions - 1) the way the
 * reference's addPoleToMesh does on the planar part (js/sphere-mesh.js:55-88): the triangles without the pole first, in
 * their order, then one fan triangle per hull side along the hull walk that starts at the last unpaired side.  The
 * triangulation is the same set of triangles; only the numbering of the fan (and with it the starting neighbour of the
 * CSR rows around the pole) changes, which the order-defined host stages (generatePlates) can see.  In place. */
int wo_sphere_reference_closure(int32_t numRegions, int32_t* triangles, int32_t* halfedges);
/* SphereMesh constructor's CSR (js/sphere-mesh.js:94-146).  adjTriList may be NULL. */
int wo_mesh_csr(int32_t numRegions, int32_t numSides, const int32_t* triangles, const int32_t* halfedges,
                int32_t* adjOffset, int32_t* adjList, int32_t* adjTriList);
/* computeNeighborDist: js/sphere-mesh.js:191-203 */
int wo_neighbor_dist(int32_t numRegions, const int32_t* adjOffset, const int32_t* adjList,
                     const float* r_xyz, float* neighborDist);
/* computeTriangleElevations: js/planet-worker.js:29-37 */
int wo_triangle_elevations(int32_t numTriangles, const int32_t* triangles, const float* r_elevation,
                           float* t_elevation);
/* generateTriangleCenters: js/sphere-mesh.js:206-219.  t_xyz[3t+k] = (a + b + c) / 3 of the corners' coordinate k, summed
 * left to right in double and stored as float32.  t_xyz has 3*numTriangles floats. */
int wo_triangle_centers(int32_t numTriangles, const int32_t* triangles, const float* r_xyz, float* t_xyz);

/* ------------------------------------------------ SimplexNoise (js/simplex-noise.js:5-54) ----- */
/* constructor: perm[512] and permMod12[512] for makeRng(seed) (js/simplex-noise.js:8-14) */
int wo_noise_tables(double seed, uint8_t* perm512, uint8_t* pm12_512);
/* one point on the host, for callers that evaluate the noise a point at a time (js/wind.js:394, js/coarse-plates.js:57):
 * perm512 / pm12_512 are the instance's tables; kind / octaves / p0..p2 as for wo_noise_eval.  Same arithmetic as the
 * device passes (csrc/noise.h). */
int wo_noise_point(const uint8_t* perm512, const uint8_t* pm12_512, int32_t kind, int32_t octaves, double p0, double p1, double p2,
                   double x, double y, double z, double* out);
/* batch evaluation on the device.  kind: 0 noise3D, 1 fbm(octaves, persistence),
 * 2 ridgedFbm(octaves, lacunarity=p0, gain=p1, offset=p2).  xyz: n interleaved double triples. */
#define WO_NOISE_3D 0
#define WO_NOISE_FBM 1
#define WO_NOISE_RIDGED 2
int wo_noise_eval(wo_ctx* ctx, double seed, int32_t kind, int32_t octaves, double p0, double p1, double p2,
                  int64_t n, const double* xyz, double* out);

/* ------------------------------------------------ context / planet handle --------------------- */
wo_ctx* wo_ctx_create(int32_t device);              /* NULL on failure (see wo_last_error)        */
void    wo_ctx_destroy(wo_ctx* ctx);
/* The mesh producer on the device (csrc/mesh.hip, the bodies in csrc/mesh_ops.h): every array equals, word for word, what the host
 * sequence gives on the same points.  wo_sphere_delaunay_device is wo_sphere_delaunay.  wo_sphere_mesh_device is the whole product
 * in one call: wo_sphere_delaunay, wo_sphere_reference_closure when referenceClosure is non-zero, wo_mesh_csr and
 * wo_neighbor_dist.  triangles / halfedges have 3*(2*numRegions-4) entries, adjOffset numRegions+1; adjList, adjTriList (may be
 * NULL) and neighborDist (may be NULL) have room for 3*(2*numRegions-4) entries, of which the first adjOffset[numRegions] are
 * written.  Status and message are the host's on the same input: 1 bad arguments (a NULL context or pointer, fewer than 4 points,
 * a zero-length point; a NULL context never touches the device), 2 star construction failed (the refusal of a point set whose
 * hull does not hold the centre strictly inside included, see wo_sphere_delaunay), 3 triangle count != 2V-4,
 * 4 unmatched half-edges; 5 stands for any failure of the CSR stage, which a triangulation that passed 3 and 4 does not reach.
 * Nothing stays allocated after the call. */
int wo_sphere_delaunay_device(wo_ctx* ctx, int32_t numRegions, const float* r_xyz, int32_t* triangles, int32_t* halfedges);
int wo_sphere_mesh_device(wo_ctx* ctx, int32_t numRegions, const float* r_xyz, int32_t referenceClosure, int32_t* triangles,
                          int32_t* halfedges, int32_t* adjOffset, int32_t* adjList, int32_t* adjTriList, float* neighborDist);
/* The Fibonacci sphere's points on the device (csrc/points.hip, the bodies in csrc/points_ops.h): generateFibonacciSphere(N, jitter,
 * makeRng(seed)) plus the pole, one thread per point.  The loop's carried values are evaluated in closed form (Park-Miller jump-ahead,
 * piecewise-linear tables of the two f64 accumulations) and the trigonometry is V8's fdlibm, so the floats are the reference's.
 * wo_fib_sphere_points_device downloads them: r_xyz has 3*(N+1) floats, as for wo_fib_sphere_points.  wo_sphere_mesh_seed_device is the
 * whole mesh from the seed in one call: the points are generated into the buffer the mesh stage reads (no upload) and downloaded
 * beside the mesh arrays, whose sizes and values are wo_sphere_mesh_device's on the same points (numRegions = N + 1).  Status: 1 bad
 * arguments (a NULL context, which never touches the device; a NULL pointer, adjTriList and neighborDist excepted; N < 1; N + 1 < 4 for
 * the mesh form), 2 to 5 the mesh's own.  Nothing stays allocated after the call. */
int wo_fib_sphere_points_device(wo_ctx* ctx, int32_t N, double jitter, double seed, float* r_xyz);
int wo_sphere_mesh_seed_device(wo_ctx* ctx, int32_t N, double jitter, double seed, int32_t referenceClosure, float* r_xyz,
                               int32_t* triangles, int32_t* halfedges, int32_t* adjOffset, int32_t* adjList, int32_t* adjTriList,
                               float* neighborDist);
/* Uploads the mesh once (the worker keeps mesh / r_xyz / neighborDist in W between commands,
 * js/planet-worker.js:277-292).  neighborDist may be NULL: it is then computed on the device. */
wo_planet* wo_planet_create(wo_ctx* ctx, int32_t numRegions, const int32_t* adjOffset,
                            const int32_t* adjList, const float* r_xyz, const float* neighborDist);
void       wo_planet_destroy(wo_planet* p);

/* ------------------------------------------------ terrain-post, JS call surface --------------- */
/* mesh.numRegions the planet was created with (0 for a NULL planet) */
int32_t wo_planet_num_regions(const wo_planet* p);

/* Each mutates r_elevation (host, numRegions floats) in place and returns nothing else, exactly like
 * the five exports of js/terrain-post.js.  r_isOcean is numRegions bytes, read-only. */
/* warpTerrain(mesh, r_elevation, r_xyz, seed, strength, r_hotspot?)   js/terrain-post.js:233 */
int wo_warp_terrain(wo_planet* p, float* r_elevation, double seed, double strength, const float* r_hotspot);
/* smoothElevation(mesh, r_elevation, r_isOcean, iterations, strength) js/terrain-post.js:317 */
int wo_smooth_elevation(wo_planet* p, float* r_elevation, const uint8_t* r_isOcean, int32_t iterations, double strength);
/* erodeComposite(mesh, r_elevation, r_xyz, r_isOcean, hIters, K, m, dt, tIters, talusSlope,
 *                kThermal, gIters, glacialStrength, neighborDist)      js/terrain-post.js:369 */
int wo_erode_composite(wo_planet* p, float* r_elevation, const uint8_t* r_isOcean,
                       int32_t hIters, double K, double m, double dt,
                       int32_t tIters, double talusSlope, double kThermal,
                       int32_t gIters, double glacialStrength);
/* sharpenRidges(mesh, r_elevation, r_isOcean, iterations, strength)   js/terrain-post.js:713 */
int wo_sharpen_ridges(wo_planet* p, float* r_elevation, const uint8_t* r_isOcean, int32_t iterations, double strength);
/* applySoilCreep(mesh, r_elevation, r_isOcean, iterations, strength)  js/terrain-post.js:758 */
int wo_soil_creep(wo_planet* p, float* r_elevation, const uint8_t* r_isOcean, int32_t iterations, double strength);

/* ------------------------------------------------ assignElevation (js/elevation.js:216-1391) -- */
/* Plate tables are dense by plate id (the reference keys plateVec / plateDensity / plateIsOcean by plate id;
 * ids are coarse-mesh region indices for plates, 0..n-1 for super plates). */
typedef struct wo_plate_table {
    int32_t        numIds;   /* table length = max plate id + 1                              */
    const uint8_t* hasVec;   /* [numIds] plateVec[id] is defined                              */
    const double*  pole;     /* [3*numIds] plateVec[id].pole                                  */
    const double*  omega;    /* [numIds]   plateVec[id].omega                                 */
    const uint8_t* isOcean;  /* [numIds]   plateIsOcean.has(id)                               */
    const double*  density;  /* [numIds]   plateDensity[id]                                   */
} wo_plate_table;
/* assignElevation(mesh, r_xyz, plateIsOcean, r_plate, plateVec, plateSeeds, noise, noiseMag, seed, spread,
 *                 plateDensity, superPlateData)  ->  { r_elevation, mountain_r, coastline_r, ocean_r, r_stress,
 *                 debugLayers }                                                 js/elevation.js:216,1386-1390
 * plateSeeds is the Set in iteration order; r_superPlate / superPlates are NULL when superPlateData is null;
 * noisePerm512 / noisePm12_512 are the `noise` instance's tables; debugLayers (NULL or 12*numRegions floats,
 * layer-major) in the order base, tectonic, noise, interior, coastal, ocean, hotspot, tecActivity, margins,
 * backArc, foldRidge, orogenicPower; the three Sets come back in insertion order (arrays of numRegions ints,
 * sizes in setCounts[3]).  The resident r_elevation of the planet is set to the result as well. */
int wo_assign_elevation(wo_planet* p, const int32_t* r_plate, const wo_plate_table* plates,
                        const int32_t* plateSeeds, int32_t numPlateSeeds,
                        const int32_t* r_superPlate, const wo_plate_table* superPlates,
                        const uint8_t* noisePerm512, const uint8_t* noisePm12_512,
                        double noiseMag, double seed, double spread,
                        float* r_elevation, float* r_stress, float* debugLayers,
                        int32_t* mountain_r, int32_t* coastline_r, int32_t* ocean_r, int32_t* setCounts);

/* ------------------------------------------------ buildSuperPlates (js/super-plates.js:16-273) -- */
/* buildSuperPlates(mesh, r_plate, plateSeeds, plateVec, plateIsOcean, plateDensity) -> { r_superPlate, superPlateVec,
 *                  superPlateIsOcean, superPlateDensity, numSuperPlates }            js/super-plates.js:16,272
 * The per-cell passes run on the device, the plate-level part (at most WO_SUPER_MAX_PLATES plates) in native host code.
 * plateSeeds is the Set in iteration order throughout; a position in it is a plate's "slot". */
#define WO_SUPER_MAX_PLATES 1024
/* The device half: plate areas (js/super-plates.js:21-25) and the plate adjacency graph (:29-39) over the planet's CSR.
 * area[numPlateSeeds]: cells per plate, by slot.  firstSlot[numPlateSeeds * numPlateSeeds]: for the ordered pair (a, b),
 * the smallest adjList index at which a cell of plate a sees a cell of plate b, 0xFFFFFFFF where it never does; sorted by
 * it, a plate's neighbours are in the insertion order of the reference's plateNeighbors[a] Set.  An r_plate entry that is
 * not in plateSeeds, a repeated seed and more than WO_SUPER_MAX_PLATES seeds are errors. */
int wo_super_plate_tables(wo_planet* p, const int32_t* r_plate, const int32_t* plateSeeds, int32_t numPlateSeeds,
                          int32_t* area, uint32_t* firstSlot);
/* The host half: connected components of same-kind plates (js/super-plates.js:41-62), farthest-point seeding and the two
 * Dijkstras (:64-172), area-weighted poles, kinds and densities (:182-270), from the two tables above.  Needs no GPU.
 * `plates` is dense by plate id (a NaN density is an undefined plateDensity[id]).  plateToSuper[numPlateSeeds]: super plate
 * per slot; the four super tables have room for numPlateSeeds entries (superPole 3 * numPlateSeeds) and hold *numSuper. */
int wo_super_plates_group(int32_t numPlateSeeds, const int32_t* plateSeeds, const wo_plate_table* plates,
                          const int32_t* area, const uint32_t* firstSlot, int32_t* plateToSuper, int32_t* numSuper,
                          double* superPole, double* superOmega, uint8_t* superIsOcean, double* superDensity);
/* Both halves and the gather r_superPlate[r] = plateToSuperPlate[r_plate[r]] (js/super-plates.js:177-180) on the device.
 * r_superPlate: numRegions ints; the super tables as above.  The laps of the call are what wo_last_stage_timing reports. */
int wo_build_super_plates(wo_planet* p, const int32_t* r_plate, const wo_plate_table* plates,
                          const int32_t* plateSeeds, int32_t numPlateSeeds, int32_t* r_superPlate, int32_t* numSuper,
                          double* superPole, double* superOmega, uint8_t* superIsOcean, double* superDensity);

/* ------------------------------------------------ plate projection ----------- */
/* projectCoarsePlates(mesh, r_xyz, coarseMesh, coarse_xyz, coarse_r_plate, seed, numPlates) -> r_plate
 *                                                                       js/coarse-plates.js:51-117
 * Runs on the planet's resident r_xyz; the coarse mesh (coarseMesh.adjOffset / adjList, coarse_xyz, coarse_r_plate,
 * as generateCoarsePlates returns them, js/coarse-plates.js:19-42) is borrowed for the call.  numPlates < 0 stands
 * for `numPlates == null`.  r_plate: numRegions ints, bit-exact plate ids. */
int wo_project_coarse_plates(wo_planet* p, int32_t coarseRegions, const int32_t* coarseAdjOffset, const int32_t* coarseAdjList,
                             const float* coarse_xyz, const int32_t* coarse_r_plate, double seed, int32_t numPlates, int32_t* r_plate);
/* smoothAndReconnectPlates(mesh, r_plate, plateSeeds, numPasses)         js/plates.js:241-348
 * Host stage (order-defined in-place passes); needs no GPU.  plateSeeds in the Set's iteration order; r_plate is
 * rewritten in place. */
int wo_smooth_reconnect_plates(int32_t numRegions, const int32_t* adjOffset, const int32_t* adjList, int32_t* r_plate,
                               const int32_t* plateSeeds, int32_t numPlateSeeds, int32_t numPasses);

/* ------------------------------------------------ plate generation (host stages, no GPU) ------ */
/* Branch counters of the two calls below (optional `stats` argument: NULL or WO_PLATES_GEN_STATS int64 values, zeroed
 * by each call, which then counts its own branches). */
#define WO_PLATES_GEN_STATS 7
#define WO_PGS_GOVERNOR_HALVED 0       /* generatePlates: plate turns halved by the area governor        js/plates.js:148-150 */
#define WO_PGS_SEEDS_TRIMMED 1         /* assignOceanLand: continent seeds dropped for the land budget   js/ocean-land.js:104-112 */
#define WO_PGS_CONTINENT_AT_TARGET 2   /* assignOceanLand: continent turns skipped at their own target   :153 */
#define WO_PGS_SEA_ABSORBED 3          /* assignOceanLand: interior seas joined to their continent        :224-228 */
#define WO_PGS_SEA_REFUSED 4           /* assignOceanLand: interior seas kept by the 1.1 x cap            :224 */
#define WO_PGS_SEA_TWO_CONTINENTS 5    /* assignOceanLand: interior seas bordering two continents         :218-221 */
#define WO_PGS_ORPHANS 6               /* generatePlates: cells assigned by the orphan sweep              js/plates.js:199-214 */
/* generatePlates(mesh, r_xyz, numPlates, seed) -> { r_plate, plateSeeds, plateVec }          js/plates.js:6-232
 * Farthest-point seeds, round-robin directional growth, the orphan sweep, smoothAndReconnectPlates and the Euler poles,
 * bit for bit.  r_plate: numRegions ints.  plateSeeds / pole (3 per seed) / omega have room for min(numPlates, numRegions)
 * entries and come back in the Set's insertion order, *numPlateSeeds of them.  numPlates < 1 is refused. */
int wo_generate_plates(int32_t numRegions, const int32_t* adjOffset, const int32_t* adjList, const float* r_xyz, int32_t numPlates,
                       double seed, int32_t* r_plate, int32_t* plateSeeds, int32_t* numPlateSeeds, double* pole, double* omega,
                       int64_t* stats);
/* assignOceanLand(mesh, r_plate, plateSeeds, r_xyz, seed, numContinents, continentSizeVariety, landCoverage) -> Set
 *                                                                                          js/ocean-land.js:7-238
 * plateSeeds in the Set's insertion order; plateIsOcean: one byte per seed in that order (1: the plate id is in the
 * returned Set).  An r_plate entry that is not a seed is refused (the reference throws on it). */
int wo_assign_ocean_land(int32_t numRegions, const int32_t* adjOffset, const int32_t* adjList, const int32_t* r_plate,
                         const int32_t* plateSeeds, int32_t numPlateSeeds, const float* r_xyz, double seed, int32_t numContinents,
                         double continentSizeVariety, double landCoverage, uint8_t* plateIsOcean, int64_t* stats);
/* Test / diagnostic entry, not needed by a host: the fdlibm ports the host stages use where the reference calls V8's Math,
 * evaluated on the caller's arguments (tests/test_plates_gen.py holds them to V8's bits): fn 0 sin, 1 cos, 2 exp, over n doubles
 * (sin / cos: |x| up to about 2^20 * pi/2 = 1 647 099, NaN beyond; csrc/import_ops.h). */
int wo_v8_math(int32_t fn, int64_t n, const double* x, double* out);

/* diffuseOceanWarmth(mesh, r_oceanWarmth, r_isLand, r_plateContinentality, passes)   js/temperature.js:19-66
 * Seeds the ocean cells with their warmth, then `passes` Jacobi sweeps of (self + neighbours) / (1 + degree); cells
 * with plate continentality >= 0.95 keep their value.  r_oceanWarmth / r_plateContinentality may be NULL (the reference
 * accepts null for both).  `out` (numRegions floats) receives the Float32Array the reference returns. */
int wo_diffuse_ocean_warmth(wo_planet* planet, const float* r_oceanWarmth, const uint8_t* r_isLand, const float* r_plateContinentality,
                            int32_t passes, float* out);
/* computeWindConvergence(mesh, r_xyz, r_wind3dX, r_wind3dY, r_wind3dZ)               js/precipitation.js:18-52
 * r_xyz is the planet's resident position array. */
int wo_wind_convergence(wo_planet* planet, const float* r_wind3dX, const float* r_wind3dY, const float* r_wind3dZ, float* out);
/* advectMoisture(mesh, r_xyz, r_heightKm, r_isLand, r_windE, r_windN, r_wind3dX, r_wind3dY, r_wind3dZ, r_oceanWarmth,
 *                r_coastDistLand, maxHops, avgEdgeKm)                                js/precipitation.js:59-195
 * Start moisture per cell, then maxHops upwind-gather sweeps (ping-pong buffers); avgEdgeKm is not read by the
 * reference's body and is not part of this entry point.  r_oceanWarmth may be NULL.
 * Exactness: the depletion base 1 - pow(0.78, 1/maxHops) (js/precipitation.js:113) is evaluated with the host libm's pow,
 * which agrees with V8's Math.pow bit for bit for maxHops 1..26 — this covers the reference's own clamp of maxHops to
 * 8..20 (js/precipitation.js:210) — and differs by 1 ulp at maxHops = 27, 98, 169 (checked for 1..200).  Bit-exact results
 * are guaranteed for the reference's range only. */
int wo_advect_moisture(wo_planet* planet, const float* r_heightKm, const uint8_t* r_isLand, const float* r_windE, const float* r_windN,
                       const float* r_wind3dX, const float* r_wind3dY, const float* r_wind3dZ, const float* r_oceanWarmth,
                       const int32_t* r_coastDistLand, int32_t maxHops, float* out);

/* ------------------------------------------------ multi-GPU exchange over RCCL --- */
/* The reference is one single-threaded worker (js/planet-worker.js:944-954): it has no exchange to replace.  A multi-GPU
 * host runs one process (or worker thread) per GPU; these entry points keep the data path on the devices — RCCL over xGMI on
 * the planet's own stream.  Rank 0 obtains the 128-byte id, the HOST distributes it by whatever channel it has (a message to
 * its workers, torch.distributed, a file), every rank creates its communicator with it (collective call).
 *   wo_planet_exchange_allgather  every rank contributes the values of its send list (wo_planet_set_halo) and receives all
 *                                 the others' (its receive list = the others' contributions in rank order): the merge of the
 *                                 landmass decomposition.  counts[j] = length of rank j's send list.  ncclAllGather.
 *   wo_planet_exchange_neighbors  the first nToPrev entries of the send list go to rank-1, the rest to rank+1; the first
 *                                 nFromPrev entries of the receive list come from rank-1, the rest from rank+1: the one-ring
 *                                 halo of a band decomposition.  ncclSend / ncclRecv in one group.
 * Both return when the received values are in the resident field. */
#define WO_COMM_ID_BYTES 128
typedef struct wo_comm wo_comm;
int wo_comm_unique_id(uint8_t* id);                                                    /* WO_COMM_ID_BYTES bytes out */
int wo_comm_create(wo_ctx* ctx, const uint8_t* id, int32_t nranks, int32_t rank, wo_comm** out);
int wo_comm_destroy(wo_comm* comm);
int wo_comm_rank(const wo_comm* comm);
int wo_comm_size(const wo_comm* comm);
int wo_planet_exchange_allgather(wo_planet* planet, wo_comm* comm, const int32_t* counts);
int wo_planet_exchange_neighbors(wo_planet* planet, wo_comm* comm, int32_t nToPrev, int32_t nFromPrev);

/* The flood exchange of the landmass decomposition.  priorityFloodCarve pops ONE heap over the whole planet
 * (js/terrain-post.js:131-147); how that heap orders EQUAL keys depends on everything in it, the other ranks' landmasses at
 * their current heights included.  A rank's flood proves for each of its landmasses that no equal-key decision matters, or
 * reports it undecided (csrc/flood_host.cc).  With an exchange set, every flood call of erodeComposite then (phase 0) agrees
 * with the other ranks whether any rank is undecided and, if so, (phase 1) pools the heights of all land cells at that call;
 * ONE undecided rank (the flag is a bid: INT32_MAX - its lowest land cell id, 0 when decided; the maximum names it) floods the
 * whole planet on the true mask exactly as the unpartitioned run does and (phases 2 / 3) hands the land heights back; the
 * undecided ranks keep their own cells of them.  Never needed at 10 M cells; at 40 M cells in every call.
 * All ranks make the same sequence of calls (0; then 1 and one of 2 / 3 when the maximum is not 0).
 *   fn(user, 0, int32_t flag[1], 1)        flag := max over the ranks
 *   fn(user, 1, float field[numRegions], numRegions)   in: the rank's own land cells hold their heights; out: every land cell does
 *   fn(user, 2, float land[n], n)          this rank flooded: it SENDS land (the planet's land cells in ascending id) to every rank
 *   fn(user, 3, float land[n], n)          every other rank: land := what the one rank in phase 2 sent
 *   fn(user, -1, int32_t proto[1], 1)      handshake, once, inside wo_planet_set_flood_exchange: proto[0] arrives as
 *                                          WO_FLOOD_EXCHANGE_PROTOCOL; a callback that implements exactly these phases sets
 *                                          proto[0] = -proto[0] and returns 0 (anything else: set_flood_exchange fails)
 * fn returns 0 on success; a non-zero status fails the erodeComposite call.  fn MUST return non-zero for a phase it does
 * not implement (never guess from "phase != 0").  r_isOcean_true: the planet's real mask (the
 * resident mask is the rank's: other ranks' landmasses are ocean).  fn == NULL switches the exchange off.
 * wo_planet_set_flood_exchange_comm: the same over RCCL — counts[j] land cells of rank j, their region ids concatenated in
 * rank order in cellsByRank (ncclAllReduce of the flag, ncclAllGather of the heights, ncclBroadcast of the flooded heights).
 * The comm must outlive the exchange: switch it off (fn == NULL) or destroy the planet before wo_comm_destroy. */
#define WO_FLOOD_EXCHANGE_PROTOCOL 2
typedef int (*wo_flood_exchange_fn)(void* user, int32_t phase, void* buf, int64_t n);
int wo_planet_set_flood_exchange(wo_planet* planet, const uint8_t* r_isOcean_true, wo_flood_exchange_fn fn, void* user);
int wo_planet_set_flood_exchange_comm(wo_planet* planet, const uint8_t* r_isOcean_true, wo_comm* comm, const int32_t* counts,
                                      const int32_t* cellsByRank);

/* ------------------------------------------------ landmass decomposition --------- */
/* Connected components of the land cells (cells with r_isOcean == 0, joined along mesh edges).  label[r] = smallest
 * region id of r's landmass, -1 for ocean cells.  Every order-defined pass of erodeComposite (js/terrain-post.js:369-707:
 * flood, sort, receivers, flow, implicit solve + deposition, thermal, glacial) and applySoilCreep (:758-794) only ever
 * couples a land cell to land cells of its own landmass (rivers and talus do not cross water), so landmasses are the
 * exact domain decomposition of the stack: a rank erodes the planet with every other rank's landmasses masked as ocean
 * and the land elevations are merged once at the end (planet_heightmap_generation_amd/decomposed.py).  Host stage
 * (concurrent union-find); needs no GPU. */
int wo_land_components(int32_t numRegions, const int32_t* adjOffset, const int32_t* adjList, const uint8_t* r_isOcean,
                       int32_t* label);

/* ------------------------------------------------ heightmap import (js/planet-worker.js:682-940) */
/* handleImportHeightmap's three stages that only import uses, on the planet's resident field (csrc/heightmap.hip; the per-cell
 * bodies and their exactness contract are in csrc/import_ops.h).  All three are bit-identical to the reference.
 * sampleHeightmap(mesh, r_xyz, imageData, imgW, imgH) with sampleBilinear / grayscaleToElevation   js/planet-worker.js:682-727
 *   gray: imgW*imgH bytes, row-major, row 0 at the north pole.  Sets the resident r_elevation to the sampled field and the
 *   resident r_isOcean to r_elevation <= 0 (as wo_planet_ocean_from_elevation); r_elevation_out (numRegions floats) may be
 *   NULL (resident only).  lat = asin(clamp(y)), lon = atan2(x, z) are fdlibm ports (V8's Math.asin / Math.atan2), not libm.
 *   Fails on a NULL image, imgW or imgH <= 0, or imgW*imgH > INT32_MAX. */
int wo_sample_heightmap(wo_planet* p, const uint8_t* gray, int32_t imgW, int32_t imgH, float* r_elevation_out);
/* deriveSyntheticPlates(mesh, r_elevation) on the resident field                                   js/planet-worker.js:733-769
 *   r_plate[r] = smallest region id of r's component (cells joined along mesh edges whose endpoints share e <= 0; NaN is land);
 *   seeds = the cells with r_plate[r] == r in ascending id (the Set's insertion order), seedIsOcean[i] = (e <= 0) of seeds[i]
 *   (NULL: not wanted), *nSeeds their number.  r_plate, seeds and seedIsOcean are sized by numRegions. */
int wo_synthetic_plates(wo_planet* p, int32_t* r_plate, int32_t* seeds, uint8_t* seedIsOcean, int32_t* nSeeds);
/* The import's region classification on the resident (final) field                                 js/planet-worker.js:811-831
 *   ocean_r: e <= 0; mountain_r: e > 0.5; coastline_r: e > 0 with a neighbour e <= 0.  Each list in ascending id (the Sets'
 *   insertion order), sized by numRegions; counts[3] = their lengths (mountain, coastline, ocean). */
int wo_classify_regions(wo_planet* p, int32_t* mountain, int32_t* coastline, int32_t* ocean, int32_t* counts);

/* ------------------------------------------------ climate-util --------------- */
/* smoothField(mesh, field, passes)                                       js/climate-util.js:5-25
 * `passes` Jacobi sweeps of (self + neighbours) / (1 + degree) on a caller-owned Float32Array (numRegions floats,
 * rewritten in place); the planet's resident elevation is untouched. */
int wo_smooth_field(wo_planet* p, float* field, int32_t passes);

/* ------------------------------------------------ seasonal pressure and wind (js/wind.js) ------ */
/* computeWind(mesh, r_xyz, r_elevation, plateIsOcean, r_plate, noise, axialTilt)                   js/wind.js:394-687
 *   on the planet's resident mesh (csrc/wind.hip; the per-cell bodies and their exactness contract are in csrc/wind_ops.h).
 *   numRegions must equal the planet's (the arrays are sized by it).  r_elevation: numRegions floats, or NULL for the planet's
 *   resident field.  r_plate: numRegions ids.  oceanPlates / nOceanPlates: the ids in the reference's plateIsOcean Set (any
 *   order, duplicates allowed; NULL only with length 0).  seed: the seed of the SimplexNoise instance the reference is handed.
 *   axialTilt (degrees): converted and never read again by the reference (:397); it must be a number.
 *   The results stay on the device in a wind block the planet owns (a later call replaces them); wo_wind_download copies one
 *   field to the host by the reference's result key:
 *     numRegions floats   r_pressure_{summer,winter} r_wind_east_* r_wind_north_* r_wind_speed_*  r_lat r_lon r_sinLat
 *                         r_continentality r_plateContinentality  r_eastX r_eastY r_eastZ r_northX r_northY r_northZ
 *     numRegions int32    r_coastDistLand          numRegions bytes   r_isLand
 *     360 floats          itczLons itczLatsSummer itczLatsWinter
 *   outBytes is the size of `out`; it must be at least the field's; an unknown key fails.  bfsLevels2 (may be NULL):
 *   [0] / [1] = levels the coast / plate distance field took (for profiles).  No CPU fallback: without a device there is
 *   no planet. */
int wo_compute_wind(wo_planet* p, int32_t numRegions, const float* r_elevation, const int32_t* r_plate, const int32_t* oceanPlates,
                    int32_t nOceanPlates, double seed, double axialTilt, int32_t* bfsLevels2);
int wo_wind_download(wo_planet* p, const char* field, void* out, int64_t outBytes);
/* computeGradients(mesh, r_xyz, r_pressure, r_east*, r_north*, r_gradE, r_gradN)                   js/wind.js:306-339
 *   on caller arrays: r_pressure numRegions floats; east3 / north3 the x, y and z arrays one after another (3 * numRegions
 *   floats each); r_gradE / r_gradN numRegions floats, written. */
int wo_compute_gradients(wo_planet* p, int32_t numRegions, const float* r_pressure, const float* east3, const float* north3,
                         float* r_gradE, float* r_gradN);

/* wo_wind_upload sets one field of the planet's wind block from the host by its result key (the keys and sizes of
 *   wo_wind_download; `bytes` must be the field's size exactly); it allocates the block if there is none.  It serves a caller
 *   that brings its own windResult to a later stage.  A block filled only by uploads is no wind result: wo_wind_download of a
 *   field that was never set still fails. */
int wo_wind_upload(wo_planet* p, const char* field, const void* data, int64_t bytes);

/* ------------------------------------------------ ocean surface currents (js/ocean.js) --------- */
/* computeOceanCurrents(mesh, r_xyz, r_elevation, windResult)                                       js/ocean.js:204-382
 *   on the planet's resident mesh (csrc/ocean.hip; the per-cell bodies and their exactness contract are in csrc/ocean_ops.h).
 *   windResult is the planet's wind block: left there by wo_compute_wind, or filled by wo_wind_upload with at least r_lat r_lon
 *   r_isLand r_eastX r_eastY r_eastZ itczLons itczLatsSummer itczLatsWinter, the fields the stage reads; otherwise the call
 *   fails with "no wind result".  r_elevation is not read by the reference and is no argument here.  numRegions must equal the
 *   planet's.  All eight outputs are the reference's bit for bit.
 *   The results stay on the device in an ocean block the planet owns (a later call replaces them); wo_ocean_download copies one
 *   field (numRegions floats) to the host by the reference's result key:
 *     r_ocean_current_east_{summer,winter} r_ocean_current_north_* r_ocean_speed_* r_ocean_warmth_*
 *   outBytes is the size of `out`; it must be at least the field's; an unknown key fails.  info (may be NULL) receives what the
 *   reference logs (:243, :371) and the pass counts, for profiles and checks.  No CPU fallback. */
typedef struct wo_ocean_info {
    int32_t circumpolarNH, circumpolarSH;              /* an open ocean channel at 60 +- 5 degrees north / south */
    int32_t coastThreshold, warmthRange;               /* hops; the distance fields are built to warmthRange - 1 */
    int32_t currentSmoothPasses, warmthSmoothPasses;
    int32_t oceanCells[2];                             /* ocean cells with a speed > 0, summer / winter */
    float p95[2];                                      /* their 95th percentile, summer / winter */
} wo_ocean_info;
int wo_compute_ocean_currents(wo_planet* p, int32_t numRegions, wo_ocean_info* info);
int wo_ocean_download(wo_planet* p, const char* field, void* out, int64_t outBytes);
/* wo_ocean_upload sets one field of the planet's ocean block from the host by its result key (the eight keys of
 *   wo_ocean_download; `bytes` must be numRegions floats exactly); it allocates the block if there is none.  It serves a caller
 *   that brings its own oceanResult to a later stage.  A block filled only by uploads is no ocean result: wo_ocean_download of
 *   a field that was never set still fails. */
int wo_ocean_upload(wo_planet* p, const char* field, const void* data, int64_t bytes);

/* ------------------------------------------------ precipitation (js/precipitation.js) ---------- */
/* computePrecipitation(mesh, r_xyz, r_elevation, windResult, oceanResult, precipitationOffset, landCoverage)
 *                                                                    js/precipitation.js:196-684, js/heuristic-precip.js
 *   on the planet's resident mesh (csrc/precip.hip; the per-cell bodies and their exactness contract are in csrc/precip_ops.h).
 *   windResult is the planet's wind block (wo_compute_wind, or wo_wind_upload of at least r_lat r_lon r_isLand r_continentality
 *   r_coastDistLand, the six frame arrays, the three ITCZ arrays and per season r_wind_east_* r_wind_north_* r_pressure_*);
 *   oceanResult is the planet's ocean block (wo_compute_ocean_currents, or wo_ocean_upload of r_ocean_warmth_summer and
 *   r_ocean_warmth_winter).  Without them the call fails with "no wind result" / "no ocean result".  r_elevation: numRegions
 *   floats, NULL means the planet's resident field.  numRegions must equal the planet's.  All four outputs are the reference's
 *   bit for bit wherever the host libm's pow gives V8's three scalars (csrc/precip_ops.h lists the hop counts where it does not).
 *   The results stay on the device in a precipitation block the planet owns (a later call replaces them); wo_precip_download
 *   copies one field (numRegions floats) to the host by the reference's result key:
 *     r_precip_summer r_precip_winter r_rainshadow_summer r_rainshadow_winter
 *   info (may be NULL) receives the scalars of the call.  No CPU fallback. */
typedef struct wo_precip_info {
    int32_t maxHops, elevSmoothPasses, convSmoothPasses, shadowHops, windwardHops, rsSmoothPasses, precipSmoothPasses, wcPasses, leeCoastHops;
    int32_t listLengths[4];                            /* wind-aligned neighbours: upwind, downwind summer; upwind, downwind winter */
    int32_t reserved;
    double depletionBase, shadowDecay, windwardDecay;  /* 1 - pow(0.78, 1/maxHops), 1 - pow(0.15, 1/shadowHops), 1 - pow(0.25, 1/windwardHops) */
    float p95[2];                                      /* maxPrecip: the 95th percentile of the blended field, summer / winter */
} wo_precip_info;
int wo_compute_precipitation(wo_planet* p, int32_t numRegions, const float* r_elevation, double precipitationOffset, double landCoverage,
                             wo_precip_info* info);
int wo_precip_download(wo_planet* p, const char* field, void* out, int64_t outBytes);
/* wo_precip_upload sets one field of the planet's precipitation block from the host by its result key (the four keys of
 *   wo_precip_download; `bytes` must be numRegions floats exactly); it allocates the block if there is none.  It serves a caller
 *   that brings its own precipResult to a later stage.  A block filled only by uploads is no precipitation result: it serves
 *   the uploaded fields, and wo_precip_download of a field that was never set still fails. */
int wo_precip_upload(wo_planet* p, const char* field, const void* data, int64_t bytes);

/* ------------------------------------------------ temperature (js/temperature.js) -------------- */
/* computeTemperature(mesh, r_xyz, r_elevation, windResult, oceanResult, precipResult, temperatureOffset)
 *                                                                    js/temperature.js:69-237
 *   on the planet's resident mesh (csrc/temp.hip; the per-cell bodies and their contract are in csrc/temp_ops.h).
 *   windResult is the planet's wind block (wo_compute_wind, or wo_wind_upload of at least r_lat r_lon r_isLand r_continentality
 *   r_plateContinentality and the three ITCZ arrays), oceanResult its ocean block (wo_compute_ocean_currents, or wo_ocean_upload
 *   of r_ocean_warmth_* and r_ocean_speed_* of both seasons), precipResult its precipitation block (wo_compute_precipitation, or
 *   wo_precip_upload of r_precip_summer and r_precip_winter).  Without them the call fails with "no wind result" / "no ocean
 *   result" / "no precipitation result": the reference's branches for missing fields are not offered.  r_elevation: numRegions
 *   floats, NULL means the planet's resident field.  numRegions must equal the planet's; temperatureOffset must be a number.
 *   The per-cell code calls pow(t, 1.4) of the platform's libm, so the outputs are the reference's up to a per-cell bound
 *   (tests/test_temperature_libm.py), not bit for bit.
 *   The results stay on the device in a temperature block the planet owns (8 bytes per cell; a later call replaces them);
 *   wo_temperature_download copies one field (numRegions floats) to the host by the reference's result key:
 *     r_temperature_summer r_temperature_winter
 *   and wo_temperature_upload sets one (a block filled only by uploads serves the uploaded fields and refuses the others).
 *   info (may be NULL) receives the pass counts and the kernel launches of the call.  No CPU fallback. */
typedef struct wo_temperature_info {
    int32_t oceanWarmthPasses;                         /* max(4, round(1400 / avgEdgeKm)) */
    int32_t smoothPasses;                              /* 1 */
    int32_t launches;                                  /* kernel launches of the call */
    int32_t reserved;
} wo_temperature_info;
int wo_compute_temperature(wo_planet* p, int32_t numRegions, const float* r_elevation, double temperatureOffset, wo_temperature_info* info);
int wo_temperature_download(wo_planet* p, const char* field, void* out, int64_t outBytes);
int wo_temperature_upload(wo_planet* p, const char* field, const void* data, int64_t bytes);

/* ------------------------------------------------ Koppen classes (js/koppen.js) ---------------- */
/* classifyKoppen(mesh, r_elevation, tempResult, precipResult)                                     js/koppen.js:67-288
 *   One class id per cell (an index into the reference's KOPPEN_CLASSES: 0 Ocean, 1 Af .. 30 EF), from the elevation
 *   (r_elevation: numRegions floats, NULL means the planet's resident field), the planet's temperature block and r_precip_* of
 *   its precipitation block (computed or uploaded); otherwise the call fails with "no temperature result" / "no precipitation
 *   result".  Given the same inputs every cell has the reference's class.  The ids stay on the device in a Koppen block the
 *   planet owns (1 byte per cell); wo_koppen_download copies them (numRegions bytes) to the host. */
int wo_classify_koppen(wo_planet* p, int32_t numRegions, const float* r_elevation);
int wo_koppen_download(wo_planet* p, uint8_t* out, int64_t outBytes);

/* ------------------------------------------------ map export (js/planet-mesh.js) -------------- */
/* exportMap / exportMapBatch(types, width)                                                 js/planet-mesh.js:1752-2180
 *   The equirectangular map of the planet, width x width / 2 pixels, row 0 north, in the reference's six kinds (csrc/map.hip;
 *   the bodies and the whole contract are in csrc/map_ops.h).  The reference draws its map triangles with WebGL, whose pixels
 *   differ between GPUs; what it defines, the triangle list and the colour of every region, is reproduced bit for bit, and the
 *   coverage rule is fixed here: a pixel belongs to the lowest side index one of whose triangles contains its centre (edges
 *   included, both windings), its region is triangles[side], or -1 where nothing covers it.
 *   wo_map_raster builds the region map of the planet's resident positions for the mesh's sides (numSides = 3 * numTriangles
 *   entries of triangles and halfedges, the closing pole fan included) and keeps it on the device in a map block the planet owns
 *   (4 bytes per pixel; a raster at another width replaces it).  width must be even and from 2 to 32768; numSides a multiple
 *   of 3; every corner a region of the planet and every half-edge a side of the mesh: otherwise the call fails and the planet
 *   keeps what it had.  regionMapOut (may be NULL) receives the map, width * width / 2 int32; counts (may be NULL) the numbers
 *   of covered and uncovered pixels.
 *   wo_map_color colours the map into RGBA8 (alpha 255), through the reference's colour function per region, its quantiser and
 *   its gamma table.  r_elevation: numRegions floats, NULL means the planet's resident field.  WO_MAP_BIOME and WO_MAP_KOPPEN
 *   read the planet's Koppen block and fail with "no Koppen result" without one (the reference falls back silently to the
 *   colour map; that is not offered).  Pixels nothing covers are black in the three grey kinds and the reference's 0x1a1a2e,
 *   taken through three r160's SRGBToLinear and the gamma table, in the others.  outBytes must be width * width / 2 * 4.
 *   wo_map_download copies the resident map (outBytes: its size exactly); wo_map_free drops it, as wo_planet_destroy does. */
enum { WO_MAP_COLOR = 0, WO_MAP_HEIGHTMAP = 1, WO_MAP_LANDHEIGHTMAP = 2, WO_MAP_LANDMASK = 3, WO_MAP_BIOME = 4, WO_MAP_KOPPEN = 5 };
int wo_map_raster(wo_planet* p, int32_t numSides, const int32_t* triangles, const int32_t* halfedges, int32_t width,
                  int32_t* regionMapOut, int64_t counts[2]);
int wo_map_color(wo_planet* p, int32_t type, const float* r_elevation, uint8_t* rgbaOut, int64_t outBytes);
int wo_map_download(wo_planet* p, int32_t* out, int64_t outBytes);
int wo_map_free(wo_planet* p);
/* buildMapMesh: the map view's centre meridian and its climate and debug layers          js/planet-mesh.js:200-382, :83-172, :506-529
 *   (the bodies and the contract are in csrc/map_layer_ops.h).
 *   wo_map_raster_centered is wo_map_raster around a centre meridian: every vertex longitude goes through the reference's wrapLon
 *   (l = lon - centerLon, one turn back into [-pi, pi]) before anything else.  centerLon must be finite and within [-pi, pi]
 *   (the reference wraps once): otherwise status 1 and nothing is allocated.  centerLon == 0 gives wo_map_raster's map bit for bit.
 *   wo_map_color_layer colours the map as one of the layers of the reference's debugLayer switch, one colour per region:
 *   continentalityColor, temperatureColor, precipitationColor, rainShadowColor, oceanCurrentColor, and debugValueToColor over the
 *   range of the values (pressure, wind speed, WO_MAP_LAYER_DEBUG), which is reduced on the device.  values == NULL reads the
 *   layer's field(s) from the planet's resident wind, ocean, precipitation or temperature block ("no wind result on this planet
 *   (call wo_compute_wind first ...)" and so on without it); values != NULL are numRegions floats that take the field's place:
 *   required for WO_MAP_LAYER_DEBUG, refused for the two ocean-current layers, which read the warmth and the speed (set those with
 *   wo_ocean_upload).  r_elevation (NULL: the resident field) is read by the ocean-current layers only (ocean is elevation <= 0).
 *   Quantiser, gamma table and alpha are wo_map_color's; pixels nothing covers take the 0x1a1a2e background of the coloured kinds
 *   (our decision: the map view has no exporter of its own).  Plate colours and the stress colouring are not offered. */
enum {
    WO_MAP_LAYER_DEBUG = 0, WO_MAP_LAYER_CONTINENTALITY = 1, WO_MAP_LAYER_TEMP_SUMMER = 2, WO_MAP_LAYER_TEMP_WINTER = 3, WO_MAP_LAYER_PRECIP_SUMMER = 4,
    WO_MAP_LAYER_PRECIP_WINTER = 5, WO_MAP_LAYER_RAINSHADOW_SUMMER = 6, WO_MAP_LAYER_RAINSHADOW_WINTER = 7, WO_MAP_LAYER_OCEANCURRENT_SUMMER = 8,
    WO_MAP_LAYER_OCEANCURRENT_WINTER = 9, WO_MAP_LAYER_PRESSURE_SUMMER = 10, WO_MAP_LAYER_PRESSURE_WINTER = 11, WO_MAP_LAYER_WINDSPEED_SUMMER = 12,
    WO_MAP_LAYER_WINDSPEED_WINTER = 13, WO_MAP_LAYER_COUNT = 14
};
int wo_map_raster_centered(wo_planet* p, int32_t numSides, const int32_t* triangles, const int32_t* halfedges, int32_t width,
                           double centerLon, int32_t* regionMapOut, int64_t counts[2]);
int wo_map_color_layer(wo_planet* p, int32_t layer, const float* values, const float* r_elevation, uint8_t* rgbaOut, int64_t outBytes);
/* The cube map of the planet: six square faces by gnomonic projection (ours: the reference exports none; csrc/cube.hip, the bodies
 *   and the whole contract are in csrc/cube_ops.h).  Great-circle arcs project to straight lines, so the faces are exactly the globe
 *   mesh of wo_globe_mesh seen from its centre; there is no seam, no wrap and no pole, and on a closed mesh every pixel is covered.
 *   Faces in the OpenGL order +X, -X, +Y, -Y, +Z, -Z (px nx py ny pz nz).  For a point (x, y, z) and a face with major-axis
 *   component ma (positive in front of the face) the face coordinates are a = sc / ma, b = tc / ma, in double on the f32 inputs,
 *   stored as f32:
 *       face   ma   sc   tc          face   ma   sc   tc          face   ma   sc   tc
 *       +X     +x   -z   -y          +Y     +y   +x   +z          +Z     +z   +x   -y
 *       -X     -x   +z   -y          -Y     -y   +x   -z          -Z     -z   -x   -y
 *   North is +Y and longitude 0 is +Z, so pz is centred on the map's centre and row 0 of the four side faces is north.  The centre
 *   of pixel (i, j) of a face is a = -1 + 2 (i + 0.5) / faceSize, b = -1 + 2 (j + 0.5) / faceSize.  Vertices, coverage rule (the lowest
 *   side index whose triangle contains the centre, edges included, both windings) and region are wo_map_raster's.
 *   A side is drawn on a face only if all three of its vertices have ma > 0 there; it is neither clipped nor split.  A face's
 *   corner lies 54.74 degrees from its centre, so this loses pixels only on a mesh with a side that spans more than
 *   90 - 54.74 = 35.26 degrees; the call does not check it.
 *   wo_map_raster_cube leaves the six faces, stacked vertically in face order, in the planet's map block as ONE region map of
 *   faceSize x 6 faceSize (face f, row j, column i at (f * faceSize + j) * faceSize + i): wo_map_color, wo_map_color_layer (outBytes:
 *   6 * faceSize * faceSize * 4), wo_map_download, wo_map_free and the tints of wo_highlight_set serve it as they serve a map, and
 *   the next raster of either kind replaces it.  faceSize must be from 1 to 16384 (odd sizes are allowed); the other checks and
 *   their messages are wo_map_raster's: otherwise status 1 and the planet keeps what it had.  regionMapOut (may be NULL): 6 *
 *   faceSize * faceSize int32; counts (may be NULL): covered and uncovered pixels.
 *   wo_map_dims gives the width and height of the planet's resident region map (faceSize, 6 faceSize after wo_map_raster_cube), or
 *   0, 0 when it has none.  It does not touch the device. */
int wo_map_raster_cube(wo_planet* p, int32_t numSides, const int32_t* triangles, const int32_t* halfedges, int32_t faceSize,
                       int32_t* regionMapOut, int64_t counts[2]);
int wo_map_dims(wo_planet* p, int32_t dims[2]);
/* Relief: a smooth height per pixel, its 16-bit encoding and the normals of the displaced surface, on the equirectangular map or the
 *   cube map (ours: the reference exports neither; csrc/relief.hip, the bodies and the whole contract are in csrc/relief_ops.h).
 *   The surface is the globe mesh of wo_globe_mesh: one flat triangle per side between the centres of its two triangles (elevation:
 *   the mean of the triangle's three regions, stored f32) and its region.  The height of a pixel is the elevation of the side that
 *   covers it, interpolated at the pixel centre from the edge functions of the raster: affine in the map plane on the map,
 *   perspective-correct on a cube face (the elevation where the ray through the pixel centre meets the flat 3-D triangle).  Pixels
 *   nothing covers hold the quiet NaN 0x7FC00000; a NaN elevation propagates.
 *   wo_relief_raster is wo_map_raster_centered, and wo_relief_raster_cube is wo_map_raster_cube, with one more pass: region map,
 *   counts, checks and messages (under the relief call's name) are theirs, and the region map serves wo_map_color, wo_map_color_layer,
 *   wo_map_download, wo_map_dims and the tints as before.  The pass leaves a height map of the same shape (f32 per pixel) in the map
 *   block.  r_elevation: numRegions floats, NULL means the planet's resident field.  heightOut (may be NULL) receives the height map.
 *   Any later raster of either kind through any entry point ends the relief; wo_map_free and wo_planet_destroy drop it.  Without a
 *   relief the three calls below answer status 1, "no relief raster".
 *   wo_relief_download copies the height map (outBytes: width * height * 4).
 *   wo_relief_height16 encodes it in native-endian uint16 (outBytes: width * height * 2): q = floor(shade * 65535 + 0.5) of the
 *   reference's heightmap shade (WO_RELIEF_HEIGHT: (km + 5) / 11 clamped to [0, 1]) or land-heightmap shade (WO_RELIEF_LAND_HEIGHT:
 *   km / 6, 0 at and below sea level); NaN gives 0.  Linear: no gamma table.
 *   wo_relief_normals gives RGBA8 normals (outBytes: width * height * 4; alpha 255; byte = floor((c * 0.5 + 0.5) * 255 + 0.5)) of the
 *   surface at radius 1 + strength * (h > 0 ? 0.04 h : 0.012 h) (strength 1: the globe's displacement), by central differences
 *   between the points of the four neighbouring pixels (map: columns wrap, rows stop at the poles; cube: across the edges of the
 *   faces), less the lean that the same stencil has on a perfect sphere, so that a constant field gives exactly (128, 128, 255).
 *   WO_RELIEF_NORMAL_TANGENT: components along (image right, image up, outward): on the map (east, north, outward).
 *   WO_RELIEF_NORMAL_OBJECT: x, y, z of the planet's frame.  WO_RELIEF_FLAT_OCEAN in flags: elevations <= 0 count as 0.  strength
 *   must be finite and >= 0.  A NaN neighbour takes the pixel's own height; a NaN pixel gets the flat normal. */
enum { WO_RELIEF_HEIGHT = 0, WO_RELIEF_LAND_HEIGHT = 1 };
enum { WO_RELIEF_NORMAL_TANGENT = 0, WO_RELIEF_NORMAL_OBJECT = 1 };
enum { WO_RELIEF_FLAT_OCEAN = 1 };
int wo_relief_raster(wo_planet* p, int32_t numSides, const int32_t* triangles, const int32_t* halfedges, int32_t width, double centerLon,
                     const float* r_elevation, float* heightOut, int64_t counts[2]);
int wo_relief_raster_cube(wo_planet* p, int32_t numSides, const int32_t* triangles, const int32_t* halfedges, int32_t faceSize,
                          const float* r_elevation, float* heightOut, int64_t counts[2]);
int wo_relief_download(wo_planet* p, float* out, int64_t outBytes);
int wo_relief_height16(wo_planet* p, int32_t kind, uint16_t* out, int64_t outBytes);
int wo_relief_normals(wo_planet* p, int32_t space, double strength, int32_t flags, uint8_t* rgbaOut, int64_t outBytes);
/* The globe view: the displaced globe mesh of wo_globe_mesh seen through a camera, with a depth per pixel and a Lambert term per
 *   facet (ours: the reference draws this picture with three.js, whose rasteriser, lighting and tone pipeline are not reproduced;
 *   csrc/view.hip, the bodies and the whole contract are in csrc/view_ops.h).
 *   Camera: eye in double, finite and not the origin, looking at the origin; z = eye / |eye|, x = (0, 1, 0) x z normalised ((1, 0, 0)
 *   where that product is shorter than 1e-12: the view from a pole), y = z x x.  0 < fovY < 180 (degrees) is a perspective camera:
 *   d = v - eye, a = f (x . d) / zc, b = -f (y . d) / zc with zc = -(z . d) and f = 1 / tan(fovY / 2).  fovY == 0 is an orthographic one
 *   of half height halfHeight > 0: d = v - 10 z, a = (x . d) / halfHeight, b = -(y . d) / halfHeight.  Positions are stored as f32.  The
 *   centre of pixel (i, j) of the width x height image is a = (2 (i + 0.5) - width) / height, b = (2 (j + 0.5) - height) / height; row 0
 *   is the top.  width and height are each from 1 to 16384, odd sizes allowed.
 *   Vertices are wo_globe_mesh's f32 positions with 0.04 * exaggeration in the place of 0.04 (1: the mesh's bits, 0: the smooth
 *   sphere; finite and >= 0) from r_elevation (NULL: the planet's resident field).  A side is drawn iff all three zc > 0 (it is
 *   neither clipped nor split), it faces the camera (n = (v1 - v0) x (v2 - v0) in the mesh's winding; perspective n . (eye - v0) > 0,
 *   orthographic n . z > 0) and its projected triangle has an area.  Coverage is wo_map_raster's rule (centres, closed edges).  The
 *   depth of a covered centre is the side's zc there as f32, perspective-correct; the smallest depth wins, among equal depths the
 *   lowest side; a depth that is not > 0 is not written.  Region: triangles[side], -1 where nothing covers.  Depth: the quiet NaN
 *   0x7FC00000 where nothing covers.
 *   wo_view_raster leaves the region map in the planet's map block as a width x height map: wo_map_color, wo_map_color_rivers,
 *   wo_map_color_layer (outBytes: width * height * 4), wo_map_download, wo_map_dims, wo_map_free and the tints of wo_highlight_set
 *   serve it, and the next raster of any kind replaces it.  On this block the pixels nothing covers take backgroundRgba (R | G << 8
 *   | B << 16 | A << 24 as it stands; WO_VIEW_BACKGROUND is the reference's scene colour 0x030308, opaque; 0 is transparent), and with
 *   shade != 0 each of R, G, B of a covered pixel becomes min(255, floor(c * (ambient + diffuse * lambert) + 0.5)), lambert =
 *   max(0, nhat . lhat) of the pixel's facet as f32, light the direction towards the light in world space (finite, not zero; the
 *   reference's sun is (5, 3, 4)), ambient and diffuse finite and >= 0 (0.55 and 0.45 let a facet that faces the light keep its
 *   colour).  regionMapOut, depthOut (may be NULL): width * height int32 / float; counts (may be NULL): covered and uncovered
 *   pixels.  The other checks and their messages are wo_map_raster's: otherwise status 1 and the planet keeps what it had.
 *   wo_view_depth_download copies the depth map (outBytes: width * height * 4); without a view raster as the block's last, status 1,
 *   "no view raster".  wo_view_lambert_download copies the Lambert terms the shade pass reads (f32 per pixel, 0 where nothing covers;
 *   the same outBytes); without a raster with shade != 0 as the block's last, status 1, "no shaded view raster". */
#define WO_VIEW_BACKGROUND 0xFF080303u
typedef struct wo_view_request {
    double eye[3];
    double fovY;                 /* degrees; 0: orthographic                                        */
    double halfHeight;           /* read when fovY == 0                                             */
    double exaggeration;
    const float* r_elevation;    /* numRegions floats, NULL: the resident field                     */
    int32_t shade;
    double light[3];             /* read when shade != 0, as are ambient and diffuse                */
    double ambient, diffuse;
    uint32_t backgroundRgba;
} wo_view_request;
int wo_view_raster(wo_planet* p, int32_t numSides, const int32_t* triangles, const int32_t* halfedges, int32_t width, int32_t height,
                   const wo_view_request* request, int32_t* regionMapOut, float* depthOut, int64_t counts[2]);
int wo_view_depth_download(wo_planet* p, float* out, int64_t outBytes);
int wo_view_lambert_download(wo_planet* p, float* out, int64_t outBytes);

/* ------------------------------------------------ rivers and lakes ---------------------------- */
/* Rivers and lakes of the final terrain (ours: the reference keeps no drainage beyond the scratch of erodeComposite; csrc/rivers.hip,
 *   the bodies and the whole contract are in csrc/rivers_ops.h).  A cell is land iff e > 0.  Every land cell drains to its neighbour
 *   with the lowest key (e, index), if that key is below its own; the others are pits.  Depressions are resolved so that rivers
 *   reach the sea: the basins spill over their lowest pass towards the drained cells in the order of Prim's algorithm (the minimum
 *   spanning tree of the basin graph, built by Boruvka rounds on the device), a spilled basin's pit drains to the cell beyond the
 *   pass, and the cells of the basin below its water level carry that level as their lake level.  Basins on a landmass with no
 *   drained cell stay endorheic.  The discharge is the runoff accumulated down the final receivers in 2^-16 fixed point, uint64:
 *   exact, so every field is defined bit for bit.
 *   wo_compute_rivers leaves five fields resident in a rivers block the planet owns (24 bytes per cell; a second call replaces
 *   them; wo_planet_destroy drops the block): r_river_receiver (int32: the final receiver, -1 at roots and off land),
 *   r_river_basin (int32: the cell id of the basin's pit, -1 drained, -2 not land), r_lake_level (f32, the quiet NaN 0x7FC00000
 *   where there is no lake), r_river_discharge (uint64, units of 2^-16; ocean cells hold what reaches them) and r_river_flow
 *   (f32: discharge * 2^-16).  r_elevation: numRegions floats, NULL means the resident field.  runoffSource:
 *   WO_RIVERS_RUNOFF_PRECIP (r_precip_summer + r_precip_winter) * 0.5f of the precipitation block, computed or uploaded ("no
 *   precipitation result" without it), WO_RIVERS_RUNOFF_UNIFORM 1 per land cell, WO_RIVERS_RUNOFF_VALUES numRegions floats in
 *   runoffValues (NULL for the other two).  The runoff is clamped to [0, 16]; NaN counts 0.  info (may be NULL) receives the counts.
 *   wo_rivers_download copies one field by its key (outBytes at least its size).  Without a rivers block it, wo_river_lines and
 *   wo_map_color_rivers answer status 1, "no rivers result".
 *   wo_river_lines gives one segment of six floats per river cell, in ascending cell order: a land cell with discharge >=
 *   ceil(minFlow * 65536), a receiver among its neighbours and no lake level of its own (lakes, and the jump from a spilled pit
 *   across its pass, are not drawn).  It runs from the cell to its receiver, both ends displaced as wo_globe_lines displaces, at
 *   base 1.003, by r_elevation (NULL: the resident field).  flowsOut (may be NULL) receives r_river_flow of the segment's cell.
 *   capacity, the room of both outputs in segments, must be at least numRegions; *count receives the number written.
 *   wo_map_color_rivers is wo_map_color(p, type, ...) in every byte, except that the pixels of the resident region map (map or
 *   cube) whose region is a river cell under minFlow or has a lake level are RGBA (41, 98, 168, 255).  r_river_flow itself goes
 *   through wo_map_color_layer's WO_MAP_LAYER_DEBUG unchanged.  minFlow must be finite.
 *   A refused call returns 1, names the call and the offending value, and allocates nothing. */
enum { WO_RIVERS_RUNOFF_PRECIP = 0, WO_RIVERS_RUNOFF_UNIFORM = 1, WO_RIVERS_RUNOFF_VALUES = 2 };
typedef struct wo_rivers_info {
    int32_t landCells, pits, spilledBasins, endorheicBasins, lakeCells;
    int32_t rounds, launches;                /* contraction rounds that merged components; kernel launches of the call */
} wo_rivers_info;
int wo_compute_rivers(wo_planet* p, int32_t numRegions, const float* r_elevation, int32_t runoffSource, const float* runoffValues,
                      wo_rivers_info* info);
int wo_rivers_download(wo_planet* p, const char* field, void* out, int64_t outBytes);
int wo_river_lines(wo_planet* p, double minFlow, const float* r_elevation, float* segmentsOut, float* flowsOut, int64_t capacity,
                   int64_t* count);
int wo_map_color_rivers(wo_planet* p, int32_t type, const float* r_elevation, double minFlow, uint8_t* rgbaOut, int64_t outBytes);

/* ------------------------------------------------ globe mesh (js/planet-mesh.js) -------------- */
/* buildMesh, updateMeshColors, updateSuperPlateBorders (globe form)                  js/planet-mesh.js:620-836, :840-957, :533-576
 *   The displaced Voronoi-fan mesh three.js draws, as the reference's own Float32Arrays bit for bit (csrc/globe.hip; the bodies and
 *   the whole contract are in csrc/globe_ops.h).  Every side s of the mesh (triangles, halfedges and their checks as for
 *   wo_map_raster) gives one triangle: the centres of its inner and outer triangle and its region, each displaced by its
 *   elevation, the winding fixed; nine floats at 9 * s in positionsOut, and the region's colour three times at 9 * s in colorsOut.
 *   No quantiser and no gamma table: these are the linear f32 colours.  outFloats must be numSides * 9 exactly.  positionsOut or
 *   colorsOut may be NULL (not both): without positions the call is updateMeshColors.  bounds (may be NULL; written with positions
 *   only) receives min x, y, z, max x, y, z of the stored positions, NaN skipped, -0 < +0, all 0 where there is nothing but NaN.
 *   r_elevation: numRegions floats, NULL means the planet's resident field; t_xyz and t_elevation are built inside the call.
 *   wo_globe_mesh colours by source: WO_GLOBE_SOURCE_TYPE with id one of WO_MAP_* (not WO_MAP_LANDMASK: buildMesh has no such
 *   branch; WO_MAP_BIOME and WO_MAP_KOPPEN need the Koppen block), values must be NULL; or WO_GLOBE_SOURCE_LAYER with id one of
 *   WO_MAP_LAYER_*, values and the resident blocks under the rules and messages of wo_map_color_layer.
 *   wo_globe_mesh_plates colours by plate (:734-736): plateColors[r_plate[region]], or (0.3, 0.3, 0.3) for a plate that is not in the
 *   table.  r_plate: numRegions int32; plateSeeds: numPlates region ids; plateColors: one f32 triple per seed (of a seed listed
 *   twice the last row counts).
 *   wo_globe_lines gives line segments, six floats each, in ascending side order: WO_GLOBE_LINES_WIREFRAME one per side with
 *   s < halfedges[s] (base 1.001, superPlates must be NULL); WO_GLOBE_LINES_SUPER_PLATE_BORDERS those of them whose two regions
 *   differ in superPlates (numRegions floats, compared as floats: NaN differs from everything, -0 equals +0; base 1.002).
 *   capacity is the room of segmentsOut in segments and must be at least numSides / 2; *count receives the number written, and
 *   nothing is written behind them.
 *   A refused call returns 1, names the offending value and allocates nothing. */
enum { WO_GLOBE_SOURCE_TYPE = 0, WO_GLOBE_SOURCE_LAYER = 1 };
enum { WO_GLOBE_LINES_WIREFRAME = 0, WO_GLOBE_LINES_SUPER_PLATE_BORDERS = 1 };
int wo_globe_mesh(wo_planet* p, int32_t numSides, const int32_t* triangles, const int32_t* halfedges, int32_t source, int32_t id,
                  const float* values, const float* r_elevation, float* positionsOut, float* colorsOut, int64_t outFloats,
                  float bounds[6]);
int wo_globe_mesh_plates(wo_planet* p, int32_t numSides, const int32_t* triangles, const int32_t* halfedges, const int32_t* r_plate,
                         int32_t numPlates, const int32_t* plateSeeds, const float* plateColors, const float* r_elevation,
                         float* positionsOut, float* colorsOut, int64_t outFloats, float bounds[6]);
int wo_globe_lines(wo_planet* p, int32_t numSides, const int32_t* triangles, const int32_t* halfedges, int32_t kind,
                   const float* r_elevation, const float* superPlates, float* segmentsOut, int64_t capacity, int64_t* count);

/* ------------------------------------------------ region outlines (ours) ---------------------- */
/* Region outlines as ordered closed rings (ours: the reference draws no outline but the loose border segments above;
 *   csrc/outline.hip, the bodies and the whole contract are in csrc/outline_ops.h).  The line where one class of cells ends and
 *   another begins: a coastline, a lake shore, a plate, a Koppen zone, an elevation band.  The mesh must be a closed triangulation:
 *   the checks and messages of wo_globe_lines (numSides a multiple of 3, every corner a region, every half-edge a side), and in
 *   addition halfedges[halfedges[s]] == s.  Every Voronoi vertex then has exactly three cells around it, and the directed boundary
 *   sides form a permutation whose cycles are the rings: there are no ambiguous junctions.
 *   Classes, one int32 per cell, by source: WO_OUTLINE_COAST e > 0 ? 1 : 0 (a NaN is ocean; r_elevation NULL means the resident
 *   field); WO_OUTLINE_LAKES 1 where the rivers block's r_lake_level is no NaN ("no rivers result" without that block);
 *   WO_OUTLINE_KOPPEN the resident Koppen class ("no Koppen result" without it); WO_OUTLINE_LEVELS the number of levels[k] <= e for
 *   numLevels (1 to 32) finite, strictly ascending floats, a NaN elevation class 0; WO_OUTLINE_VALUES the caller's numRegions int32
 *   in values.  An argument that does not belong to the source (values with COAST, levels without LEVELS, r_elevation with any but
 *   COAST and LEVELS) is refused.
 *   Side s, with h = halfedges[s], is a boundary side iff class[triangles[s]] != class[triangles[h]] and, with onlyClass >= 0,
 *   class[triangles[s]] == onlyClass.  onlyClass -1 traces every class: every undirected boundary edge then appears twice, once per
 *   class, in opposite directions.  A ring keeps its class on the side of triangles[s] throughout; the successor of a side is an
 *   O(1) expression in triangles, halfedges and the classes (csrc/outline_ops.h).  The boundary sides in ascending order take the
 *   slots 0 .. M - 1; a ring's leader is its lowest slot; rings are numbered by ascending leader and run from their leader on.
 *   wo_outline_build leaves four fields resident in an outline block the planet owns (a second call replaces them; wo_outline_free
 *   and wo_planet_destroy drop them): sides (int32[M], ring after ring), ring_start (int32[R + 1], the last entry is M),
 *   ring_class (int32[R]) and ring_of_side (int32[M]).  Everything is integer arithmetic: every word is defined.  The ordering is
 *   list ranking by pointer doubling in rounds = ceil(log2(max(M, 2))) launches.  info (may be NULL) receives M, R, the longest ring,
 *   the rounds and the kernel launches of the call.  M == 0 is a valid result: ring_start == {0}.
 *   wo_outline_download copies one field by its key (outBytes at least its size).
 *   The vertex of entry k is the centre of triangle sides[k] / 3; a ring is closed implicitly, its first vertex is not repeated.
 *   wo_outline_positions gives 3 M floats, t_xyz * (base + displacement of t_elevation) exactly as wo_globe_lines displaces its
 *   centres (base 1.002 over super plates gives the very floats of its border segments); base 0 means t_xyz itself.  r_elevation
 *   NULL means the resident field; base must be finite.  wo_outline_lonlat gives 2 M doubles, longitude and latitude in radians, of
 *   the same centres as wo_map_raster places them: outlines lie exactly on the vertices of the exported map.
 *   Without an outline block the download, positions and lonlat calls answer status 1, "no outline result".
 *   A refused call returns 1, names the call and the offending value, allocates nothing and leaves the planet what it had. */
enum { WO_OUTLINE_COAST = 0, WO_OUTLINE_LAKES = 1, WO_OUTLINE_KOPPEN = 2, WO_OUTLINE_LEVELS = 3, WO_OUTLINE_VALUES = 4 };
typedef struct wo_outline_info { int32_t boundarySides, rings, longestRing, rounds, launches; } wo_outline_info;
int wo_outline_build(wo_planet* p, int32_t numSides, const int32_t* triangles, const int32_t* halfedges, int32_t source,
                     const float* r_elevation, const int32_t* values, const float* levels, int32_t numLevels, int32_t onlyClass,
                     wo_outline_info* info);
int wo_outline_download(wo_planet* p, const char* field, void* out, int64_t outBytes);
int wo_outline_positions(wo_planet* p, double base, const float* r_elevation, float* xyzOut, int64_t outFloats);
int wo_outline_lonlat(wo_planet* p, double* lonLatOut, int64_t outDoubles);
int wo_outline_free(wo_planet* p);

/* ------------------------------------------------ arrow overlays (js/planet-mesh.js) ---------- */
/* buildWindArrows, buildOceanCurrentArrows                                        js/planet-mesh.js:1289-1465, :1545-1720
 *   The arrows the reference draws over its wind and ocean-current views, as its own Float32Arrays bit for bit (csrc/overlay.hip;
 *   the bodies and the whole contract are in csrc/overlay_ops.h).  The regions are binned into 60 x 120 cells of 3 x 3 degrees; per
 *   cell the region closest to its centre is kept, as the reference's loop over its f32 `gridDist2` leaves it.
 *   wo_overlay_bins gives those regions, WO_OVERLAY_BINS int32 in gridRegionsOut, -1 for an empty cell, from the planet's resident
 *   positions.  skipLand 1 is the ocean form: regions with r_elevation > 0 take part in no cell (a NaN does); r_elevation is
 *   numRegions floats, NULL means the resident field, and it is not read with skipLand 0.
 *   wo_overlay_arrows gives the arrows of kind WO_OVERLAY_WIND (the season's r_wind_east_* and r_wind_north_* of the wind block;
 *   cells whose speed sqrt(e * e + n * n) is below 0.001 are dropped) or WO_OVERLAY_OCEAN (the season's r_ocean_current_east_*,
 *   r_ocean_current_north_*, r_ocean_speed_* and r_ocean_warmth_* of the ocean block, skipLand binning with r_elevation; cells
 *   with a speed below 0.01 are dropped), season 0 summer or 1 winter, in ascending cell order: per arrow 18 floats (the shaft and
 *   the two wings of its head, two vertices each) in globePos and globeCol, and the map form around the centre meridian centerLon
 *   (NaN counts as 0) in mapPos and mapCol.  The fields are computed or uploaded (wo_wind_upload, wo_ocean_upload): without them
 *   the call fails with "no wind result" / "no ocean result".  Any of the four outputs may be NULL; with one given,
 *   capacityArrows, the room of each in arrows, must be at least WO_OVERLAY_BINS: the count is not known before the call has run,
 *   and a refusal comes before anything is allocated.  *count receives the number of arrows, and nothing is written behind them.
 *   A refused call returns 1, names the offending value and allocates nothing. */
enum { WO_OVERLAY_WIND = 0, WO_OVERLAY_OCEAN = 1 };
enum { WO_OVERLAY_BINS = 7200 };
int wo_overlay_bins(wo_planet* p, int32_t skipLand, const float* r_elevation, int32_t* gridRegionsOut);
int wo_overlay_arrows(wo_planet* p, int32_t kind, int32_t season, double centerLon, const float* r_elevation, float* globePos,
                      float* globeCol, float* mapPos, float* mapCol, int64_t capacityArrows, int64_t* count);

/* ------------------------------------------------ the editor: hit test and highlights --------- */
/* findNearestRegion, getHitInfoGlobe, getHitInfoMap                                              js/edit-mode.js:18-28, :32-60, :63-93
 * updatePendingHighlight, updateHoverHighlight, updateKoppenHoverHighlight                        js/planet-mesh.js:1143-1244, :960-1139
 *   The bodies and the whole contract are in csrc/pick_ops.h; every result is the reference's bit for bit.
 *   wo_pick_regions answers numQueries directions (three doubles each) from the planet's resident f32 positions (csrc/pick.hip): per
 *   region dot = nx * (double)x + ny * (double)y + nz * (double)z, left to right in double, uncontracted; the region is the lowest
 *   index among those whose dot equals the maximum of the dots above -2, compared by value (-0 equals +0, a NaN dot never wins), or
 *   -1 when no dot is above -2 (a NaN query, a query such as (-3, 0, 0)).  dotsOut (may be NULL) receives the winning dot, or -2.
 *   numQueries 0 succeeds and touches nothing; numQueries below 0 or above WO_PICK_MAX_QUERIES, a NULL planet, directions or
 *   regionsOut return 1.  Two calls give identical words.
 *   wo_pick_directions_globe and wo_pick_directions_map are the two front ends, on the host (no device is touched): the direction
 *   that reaches findNearestRegion, three doubles per query in directionsOut, and 1 in validOut; or 0 and a NaN direction where the
 *   reference returns null, which wo_pick_regions answers with -1.  Globe form: rays holds six doubles per query, the origin and the
 *   NORMALISED direction of the ray in the planet's local space (three's camera and matrices are the caller's business); the sphere
 *   has radius 1.08; no hit when the discriminant or the nearer root is negative.  Map form: points holds wx, wy per query on the
 *   map plane (x in [-2, 2], y in [-1, 1]: lon = wx * PI / 2 + centerLon, wrapped once, lat = wy * PI / 2, invalid outside
 *   [-PI/2, PI/2]); a centerLon of NaN counts as 0.  Math.sin and Math.cos are V8's fdlibm (|lon| below about 1.6e6).  As in the
 *   reference a NaN input passes both tests: valid 1, a NaN direction.
 *   wo_highlight_set sets the editor state of the planet: one class byte per region, kept on the device and counted by
 *   wo_memory_in_use, built from r_plate (numRegions int32, uploaded for the call): with pid = r_plate[r], bit 1 pid is one of the
 *   numPending pendingPlates and pendingIsOcean of that plate is not 0 (ocean now, to become land), bit 2 pid is pending and the
 *   plate is land now, bit 4 pid == hoveredPlate >= 0, bit 8 koppen[r] == hoveredKoppen >= 0.  counts (may be NULL) receives the
 *   number of regions per bit.  Pending ids and a non-negative hoveredPlate must lie in [0, numRegions); a plate listed twice is
 *   refused; hoveredKoppen >= 0 without a Koppen block is refused with "no Koppen result" (the reference skips silently: not
 *   offered); r_plate entries outside [0, numRegions) match nothing.  The byte is evaluated at set time: a later wo_classify_koppen
 *   does not change it.  A second call replaces the state; wo_highlight_clear and wo_planet_destroy drop it.  A refusal returns 1,
 *   names the value and leaves the planet's state as it was.
 *   While the state is set, wo_globe_mesh, wo_globe_mesh_plates, wo_map_color and wo_map_color_layer tint each region's f32 colour
 *   before the vertex write or the quantiser, in the reference's order, every step stored as f32, arithmetic in double, min as
 *   Math.min: pending and ocean now r * 0.7, min(1, g + 0.25), b * 0.7; pending and land now r * 0.7, g * 0.7, min(1, b + 0.25);
 *   plate hover, then Koppen hover, each channel min(1, c + 0.22).  A region whose byte is 0, and every region without a state, has
 *   exactly the words it had.  That the raster shows the tints is our decision (the reference tints its map mesh the same way); the
 *   pixels nothing covers are never tinted. */
enum { WO_PICK_MAX_QUERIES = 65536 };
int wo_pick_regions(wo_planet* p, int32_t numQueries, const double* directions, int32_t* regionsOut, double* dotsOut);
int wo_pick_directions_globe(int32_t numQueries, const double* rays, double* directionsOut, uint8_t* validOut);
int wo_pick_directions_map(int32_t numQueries, const double* points, double centerLon, double* directionsOut, uint8_t* validOut);
int wo_highlight_set(wo_planet* p, const int32_t* r_plate, int32_t numPending, const int32_t* pendingPlates,
                     const uint8_t* pendingIsOcean, int32_t hoveredPlate, int32_t hoveredKoppen, int64_t counts[4]);
int wo_highlight_clear(wo_planet* p);

/* ------------------------------------------------ device-resident variants -------------------- */
/* The "reapply" pattern (js/planet-worker.js:341-440): fields stay in HBM, only scalars arrive.
 * wo_planet_upload sets the resident r_elevation (and r_isOcean when not NULL); the *_resident
 * functions are the same passes as above without the H2D/D2H copies; all are asynchronous on the
 * planet's stream until wo_planet_sync / wo_planet_download. */
int wo_planet_upload(wo_planet* p, const float* r_elevation, const uint8_t* r_isOcean);
int wo_planet_download(wo_planet* p, float* r_elevation);
/* Band-decomposed Jacobi passes (smoothElevation / applySoilCreep on one index band per GPU, banded.py): the planet is a
 * band plus its one-ring halo.  set_halo stores the local indices whose values go to / come from the neighbouring
 * bands; after each *_resident iteration pack gathers the resident r_elevation at the send indices (into hostOut, or
 * into the device buffer deviceOut that is handed to RCCL) and unpack scatters the received values to the receive
 * indices.  Exactly one of the host / device pointers is non-NULL. */
int wo_planet_set_halo(wo_planet* p, const int32_t* sendIdx, int32_t nSend, const int32_t* recvIdx, int32_t nRecv);
int wo_planet_pack_halo(wo_planet* p, float* hostOut, void* deviceOut);
int wo_planet_unpack_halo(wo_planet* p, const float* hostIn, const void* deviceIn);
/* r_isOcean[r] = r_elevation[r] <= 0 on the resident field (js/planet-worker.js:51-54) */
int wo_planet_ocean_from_elevation(wo_planet* p);
int wo_planet_download_ocean(wo_planet* p, uint8_t* r_isOcean);
int wo_planet_sync(wo_planet* p);
/* Keep / bring back a device-side copy of (r_elevation, r_isOcean): the worker's W.prePostElev that every
 * "reapply" starts from (js/planet-worker.js:353); D2D copies on the planet's stream. */
int wo_planet_save_state(wo_planet* p);
int wo_planet_restore_state(wo_planet* p);
int wo_warp_terrain_resident(wo_planet* p, double seed, double strength, int32_t useHotspot);
int wo_planet_upload_hotspot(wo_planet* p, const float* r_hotspot);
int wo_smooth_elevation_resident(wo_planet* p, int32_t iterations, double strength);
int wo_erode_composite_resident(wo_planet* p, int32_t hIters, double K, double m, double dt,
                                int32_t tIters, double talusSlope, double kThermal,
                                int32_t gIters, double glacialStrength);
int wo_sharpen_ridges_resident(wo_planet* p, int32_t iterations, double strength);
int wo_soil_creep_resident(wo_planet* p, int32_t iterations, double strength);
/* Synthetic bench terrain: e = 0.9*fbm(1.5p,5) - 0.12 + 0.25*ridged(3p,4)*max(0,fbm(1.5p,5))
 * with SimplexNoise(seed), written to the resident elevation; isOcean = e <= 0. */
int wo_planet_synthetic_terrain(wo_planet* p, double seed);

/* ------------------------------------------------ measurement ------------------------------- */
/* HIP-event stopwatch on the planet's stream (the stream every kernel of the path is launched on). */
int wo_timer_start(wo_planet* p);
int wo_timer_stop_ms(wo_planet* p, double* ms);   /* records, synchronises the stop event, returns elapsed */
/* Per-kernel-family HIP-event profiling: when enabled every launch is bracketed by events on the
 * planet's stream (slower; used by bench.py's roofline pass only). */
int wo_profile_enable(wo_planet* p, int32_t on);
int wo_profile_reset(wo_planet* p);
/* Fills up to cap entries; returns the number of families through *count. names[i] points to static
 * storage.  total_ms / launches are per family since the last reset. */
int wo_profile_report(wo_planet* p, int32_t cap, const char** names, double* total_ms, int64_t* launches,
                      int32_t* count);
/* Stage timings of the last erodeComposite call, same {stage, ms} shape the reference ships in
 * _postTiming (js/planet-worker.js:42-93).  Stages inside the iteration loop are bracketed by events on every
 * 8th iteration only and scaled to all of them (the brackets themselves cost stream time); setup and the
 * floods are timed exactly.  WO_STAGE_TIMING=all brackets every iteration. */
int wo_last_stage_timing(wo_planet* p, int32_t cap, const char** stages, double* ms, int32_t* count);
/* Counters of the last erodeComposite call (land cells, dependency rounds, ...), for DESIGN/bench. */
int wo_last_erode_stats(wo_planet* p, int32_t cap, const char** names, double* values, int32_t* count);

#ifdef __cplusplus
}
#endif
#endif /* WOROGEN_H */
