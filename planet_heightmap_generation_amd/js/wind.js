// Counterpart of the reference's js/wind.js on the device: the same exported names, argument order and result object
// (the same keys with the same typed-array types, without _windTiming).  computeWind and computeGradients run in HIP
// kernels (csrc/wind.hip) on the planet bound to `mesh` (native.js: planetFor); the exactness contract is in
// csrc/wind_ops.h.  There is no JavaScript fallback: without the addon or a device the calls throw.
import addon, { planetFor } from './native.js';

// js/wind.js:75-79 (plain arithmetic, kept in JavaScript)
export function smoothstep(edge0, edge1, x) {
    if (edge0 === edge1) return x >= edge1 ? 1 : 0;
    const t = Math.max(0, Math.min(1, (x - edge0) / (edge1 - edge0)));
    return t * t * (3 - 2 * t);
}

// computeGradients(mesh, r_xyz, r_pressure, r_east*, r_north*, r_gradE, r_gradN): r_gradE / r_gradN are written
export function computeGradients(mesh, r_xyz, r_pressure, r_eastX, r_eastY, r_eastZ, r_northX, r_northY, r_northZ, r_gradE, r_gradN) {
    addon.computeGradients(planetFor(mesh, r_xyz), r_pressure, r_eastX, r_eastY, r_eastZ, r_northX, r_northY, r_northZ, r_gradE, r_gradN);
}

// computeWind(mesh, r_xyz, r_elevation, plateIsOcean: Set, r_plate, noise: SimplexNoise, axialTilt = 23.5)
export function computeWind(mesh, r_xyz, r_elevation, plateIsOcean, r_plate, noise, axialTilt = 23.5) {
    if (!(plateIsOcean instanceof Set)) throw new TypeError('computeWind: plateIsOcean must be a Set of plate ids');
    if (!noise || typeof noise.seed !== 'number') throw new TypeError('computeWind: noise must be a SimplexNoise instance (js/simplex-noise.js)');
    if (!(r_elevation instanceof Float32Array) || r_elevation.length !== mesh.numRegions) throw new RangeError('computeWind: r_elevation must be a Float32Array of numRegions entries');
    if (!(r_plate instanceof Int32Array) || r_plate.length !== mesh.numRegions) throw new RangeError('computeWind: r_plate must be an Int32Array of numRegions entries');
    return addon.computeWind(planetFor(mesh, r_xyz), r_elevation, r_plate, Int32Array.from(plateIsOcean), noise.seed, axialTilt);
}
