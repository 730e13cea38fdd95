// Drop-in for the reference's js/plates.js, both exports native host stages (order-defined serial logic, no device part):
//
//   generatePlates(mesh, r_xyz, numPlates, seed) -> { r_plate: Int32Array, plateSeeds: Set, plateVec: { id: { pole: [x, y, z], omega } } }
//       (:6-232) farthest-point seeds, round-robin directional growth, orphan sweep, smoothing and the Euler poles; the
//       reference's results bit for bit on the same mesh.
//   smoothAndReconnectPlates(mesh, r_plate, plateSeeds, numPasses)
//       (:241-348) majority-vote smoothing of plate boundaries, then re-attachment of fragments cut off from their plate's
//       largest component; r_plate is mutated like in the reference, nothing is returned.
import addon from './native.js';

export function generatePlates(mesh, r_xyz, numPlates, seed) {
    const res = addon.generatePlates(mesh.adjOffset, mesh.adjList, r_xyz, numPlates, seed);
    const plateSeeds = new Set(res.plateSeeds);
    const plateVec = {};
    res.plateSeeds.forEach((id, i) => { plateVec[id] = { pole: [res.pole[3 * i], res.pole[3 * i + 1], res.pole[3 * i + 2]], omega: res.omega[i] }; });
    return { r_plate: res.r_plate, plateSeeds, plateVec };
}

export function smoothAndReconnectPlates(mesh, r_plate, plateSeeds, numPasses) {
    if (!(r_plate instanceof Int32Array)) throw new TypeError('r_plate must be an Int32Array');
    const seeds = Int32Array.from(plateSeeds);          // Set or Array, in iteration order
    addon.smoothAndReconnectPlates(mesh.numRegions, mesh.adjOffset, mesh.adjList, r_plate, seeds, numPasses);
}
