// Counterpart of the reference's heightmap import stages (js/planet-worker.js:682-831) on the device: same names, argument
// order and result shapes.  sampleHeightmap / deriveSyntheticPlates / classifyRegions run in HIP kernels (csrc/heightmap.hip)
// on the planet bound to `mesh` (native.js: planetFor) and are bit-identical to the reference (csrc/import_ops.h).
import addon, { planetFor } from './native.js';

// sampleHeightmap(mesh, r_xyz, imageData, imgW, imgH) -> Float32Array; the sampled field also stays resident
export function sampleHeightmap(mesh, r_xyz, imageData, imgW, imgH) {
    if (!(imageData instanceof Uint8Array) && !(imageData instanceof Uint8ClampedArray)) throw new TypeError('sampleHeightmap: imageData must be a Uint8Array or Uint8ClampedArray');
    if (!(imgW >= 1 && imgH >= 1) || imageData.length !== imgW * imgH) throw new RangeError('sampleHeightmap: imageData length must be imgW*imgH');
    return addon.sampleHeightmap(planetFor(mesh, r_xyz), imageData, imgW, imgH, true);
}

// the Set-shaped results of the device lists (ascending ids: the reference's insertion order)
export function platesFromDevice(res) {
    const plateSeeds = new Set(res.seeds), plateIsOcean = new Set(), plateVec = {};
    for (let i = 0; i < res.seeds.length; i++) {
        plateVec[res.seeds[i]] = [0, 0, 0];
        if (res.seedIsOcean[i]) plateIsOcean.add(res.seeds[i]);
    }
    return { r_plate: res.r_plate, plateSeeds, plateIsOcean, plateVec };
}

// deriveSyntheticPlates(mesh, r_elevation) -> { r_plate, plateSeeds, plateIsOcean, plateVec }
export function deriveSyntheticPlates(mesh, r_elevation) {
    const p = planetFor(mesh);
    addon.planetUpload(p, r_elevation, null);
    return platesFromDevice(addon.syntheticPlates(p));
}

// the import's region classification (:811-831) -> { mountain_r, coastline_r, ocean_r } as Sets
export function classifyRegions(mesh, r_elevation) {
    const p = planetFor(mesh);
    addon.planetUpload(p, r_elevation, null);
    const c = addon.classifyRegions(p);
    return { mountain_r: new Set(c.mountain_r), coastline_r: new Set(c.coastline_r), ocean_r: new Set(c.ocean_r) };
}
