// Drop-in for the reference's js/super-plates.js `buildSuperPlates` (js/super-plates.js:16-273): same argument list and the
// same result object { r_superPlate:Int32Array, superPlateVec:{ id: { pole:[x,y,z], omega } }, superPlateIsOcean:Set,
// superPlateDensity:{ id: density }, numSuperPlates }.  The per-cell passes over the CSR run in HIP kernels, the plate-level
// part in native host code; this module only converts the reference's keyed objects / Sets into dense tables and back.
// The planet needs positions only when it is first created for this mesh: pass r_xyz as a trailing argument then.
import addon, { planetFor } from './native.js';
import { denseTable } from './plate-table.js';

export function buildSuperPlates(mesh, r_plate, plateSeeds, plateVec, plateIsOcean, plateDensity, r_xyz) {
    const p = planetFor(mesh, r_xyz);
    const seeds = Int32Array.from(plateSeeds);
    const res = addon.buildSuperPlates(p, r_plate, denseTable(plateIsOcean, plateVec, plateDensity, seeds), seeds);
    const superPlateVec = {}, superPlateDensity = {}, superPlateIsOcean = new Set();
    for (let sp = 0; sp < res.numSuperPlates; sp++) {
        superPlateVec[sp] = { pole: [res.pole[3 * sp], res.pole[3 * sp + 1], res.pole[3 * sp + 2]], omega: res.omega[sp] };
        if (res.isOcean[sp]) superPlateIsOcean.add(sp);
        superPlateDensity[sp] = res.density[sp];
    }
    return { r_superPlate: res.r_superPlate, superPlateVec, superPlateIsOcean, superPlateDensity, numSuperPlates: res.numSuperPlates };
}
