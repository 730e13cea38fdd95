// Counterpart of the reference's js/ocean.js on the device: the same exported name, argument order and result object (the
// same keys, all Float32Array, without _oceanTiming).  computeOceanCurrents runs in HIP kernels (csrc/ocean.hip) on the
// planet bound to `mesh` (native.js: planetFor); the exactness contract is in csrc/ocean_ops.h.  There is no JavaScript
// fallback: without the addon or a device the call throws.
import addon, { planetFor } from './native.js';

const RESULT_KEYS = ['summer', 'winter'].flatMap((s) => ['current_east', 'current_north', 'speed', 'warmth'].map((k) => `r_ocean_${k}_${s}`));
// the keys of windResult the stage reads
const WIND_INPUTS = ['r_lat', 'r_lon', 'r_isLand', 'r_eastX', 'r_eastY', 'r_eastZ', 'itczLons', 'itczLatsSummer', 'itczLatsWinter'];

// computeOceanCurrents(mesh, r_xyz, r_elevation, windResult): windResult is the object computeWind returned (its arrays are
// uploaded to the planet's wind block), or null / undefined for the wind block the planet's last computeWind left on the
// device.  r_elevation is accepted and unused, as in the reference.
export function computeOceanCurrents(mesh, r_xyz, r_elevation, windResult) {
    const given = windResult !== null && windResult !== undefined;
    if (given) {
        for (const k of WIND_INPUTS) {
            const a = windResult[k], n = k.startsWith('itcz') ? 360 : mesh.numRegions;
            const ok = k === 'r_isLand' ? a instanceof Uint8Array : a instanceof Float32Array;
            if (!ok || a.length !== n) throw new RangeError(`computeOceanCurrents: windResult.${k} must be a ${k === 'r_isLand' ? 'Uint8Array' : 'Float32Array'} of ${n} entries`);
        }
    }
    const planet = planetFor(mesh, r_xyz);
    if (given) for (const k of WIND_INPUTS) addon.windUpload(planet, k, windResult[k]);
    addon.computeOceanCurrents(planet);
    const result = {};
    for (const k of RESULT_KEYS) result[k] = addon.oceanDownload(planet, k);
    return result;
}
