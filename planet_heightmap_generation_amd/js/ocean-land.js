// Drop-in for the reference's js/ocean-land.js (:7-238): continent seeds by farthest plate centroid, round-robin growth over
// the plate graph to the land budget, absorption of trapped interior seas.  Native host stage (RNG-ordered serial logic on the
// plate table, no device part); the reference's Set bit for bit on the same mesh: the oceanic plate ids in plateSeeds order.
import addon from './native.js';

export function assignOceanLand(mesh, r_plate, plateSeeds, r_xyz, seed, numContinents, continentSizeVariety = 0, landCoverage = 0.3) {
    if (!(r_plate instanceof Int32Array)) throw new TypeError('r_plate must be an Int32Array');
    const seeds = Int32Array.from(plateSeeds);          // Set or Array, in iteration order
    const res = addon.assignOceanLand(mesh.adjOffset, mesh.adjList, r_plate, seeds, r_xyz, seed, numContinents, continentSizeVariety, landCoverage);
    const plateIsOcean = new Set();
    seeds.forEach((id, i) => { if (res.isOcean[i]) plateIsOcean.add(id); });
    return plateIsOcean;
}
