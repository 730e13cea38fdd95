// Counterpart of the reference's js/ocean.js on the device: the same exported name, argument order and result object (the
// same keys, all Float32Array, without _oceanTiming).  computeOceanCurrents runs in HIP kernels (csrc/ocean.hip) on the
// planet bound to `mesh` (native.js: planetFor); the exactness contract is in csrc/ocean_ops.h.  There is no JavaScript
// fallback: without the addon or a device the call throws.
import addon, { planetFor } from './native.js';
import { OCEAN_KEYS, given, checkInputs, uploadInputs, downloadAll } from './climate-blocks.js';

// the keys of windResult the stage reads
const WIND_INPUTS = ['r_lat', 'r_lon', 'r_isLand', 'r_eastX', 'r_eastY', 'r_eastZ', 'itczLons', 'itczLatsSummer', 'itczLatsWinter'];

// computeOceanCurrents(mesh, r_xyz, r_elevation, windResult): windResult is the object computeWind returned (its arrays are
// uploaded to the planet's wind block), or null / undefined for the wind block the planet's last computeWind left on the
// device.  r_elevation is accepted and unused, as in the reference.
export function computeOceanCurrents(mesh, r_xyz, r_elevation, windResult) {
    if (given(windResult)) checkInputs('computeOceanCurrents', 'windResult', windResult, WIND_INPUTS, mesh.numRegions);
    const planet = planetFor(mesh, r_xyz);
    if (given(windResult)) uploadInputs(planet, addon.windUpload, WIND_INPUTS, windResult);
    addon.computeOceanCurrents(planet);
    return downloadAll(planet, addon.oceanDownload, OCEAN_KEYS);
}
