// Drop-in for the reference's js/coarse-plates.js.
//
//   generateCoarsePlates(seed, numPlates, numContinents, continentSizeVariety = 0, landCoverage = 0.3)
//       -> { coarseMesh, coarse_xyz, coarse_r_plate, coarsePlateSeeds, coarsePlateVec, coarsePlateIsOcean }
//       (js/coarse-plates.js:19-38) — generatePlates and assignOceanLand (native host stages) on the fixed coarse mesh
//       buildSphere(20000, 0.75, seed + 137), its pole fan numbered as the reference numbers it.
//   projectCoarsePlates(mesh, r_xyz, coarseMesh, coarse_xyz, coarse_r_plate, seed, numPlates) -> Int32Array
//       (js/coarse-plates.js:51-117) — HIP kernel, one thread per hi-res cell; plate ids bit-exact.
//
import addon, { planetFor } from './native.js';
import { buildSphere } from './sphere-mesh.js';
import { generatePlates } from './plates.js';
import { assignOceanLand } from './ocean-land.js';

const N_COARSE = 20000;
const COARSE_JITTER = 0.75;        // fixed: the coarse mesh does not depend on the caller's jitter

export function generateCoarsePlates(seed, numPlates, numContinents, continentSizeVariety = 0, landCoverage = 0.3) {
    const { mesh: coarseMesh, r_xyz: coarse_xyz } = buildSphere(N_COARSE, COARSE_JITTER, seed + 137, true);
    const { r_plate: coarse_r_plate, plateSeeds: coarsePlateSeeds, plateVec: coarsePlateVec } = generatePlates(coarseMesh, coarse_xyz, numPlates, seed);
    const coarsePlateIsOcean = assignOceanLand(coarseMesh, coarse_r_plate, coarsePlateSeeds, coarse_xyz, seed, numContinents, continentSizeVariety, landCoverage);
    return { coarseMesh, coarse_xyz, coarse_r_plate, coarsePlateSeeds, coarsePlateVec, coarsePlateIsOcean };
}

export function projectCoarsePlates(mesh, r_xyz, coarseMesh, coarse_xyz, coarse_r_plate, seed, numPlates) {
    const planet = planetFor(mesh, r_xyz, null);
    return addon.projectCoarsePlates(planet, coarseMesh.adjOffset, coarseMesh.adjList, coarse_xyz, coarse_r_plate, seed,
                                     numPlates == null ? null : numPlates);
}
