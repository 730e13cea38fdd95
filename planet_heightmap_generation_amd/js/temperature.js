// Counterpart of the reference's js/temperature.js on the device: the same exported name, argument order and result object
// (the same keys in the same order, both Float32Array, without _tempTiming).  computeTemperature runs in HIP kernels
// (csrc/temp.hip) on the planet bound to `mesh` (native.js: planetFor); the contract is in csrc/temp_ops.h.  The reference's
// branches for missing inputs are not offered.  There is no JavaScript fallback: without the addon or a device the call throws.
import addon, { planetFor } from './native.js';
import { TEMP_KEYS, given, checkInputs, uploadInputs, downloadAll } from './climate-blocks.js';

// the keys of windResult, oceanResult and precipResult the stage reads
const WIND_INPUTS = ['r_lat', 'r_lon', 'r_isLand', 'r_continentality', 'r_plateContinentality', 'itczLons', 'itczLatsSummer', 'itczLatsWinter'];
const OCEAN_INPUTS = ['r_ocean_warmth_summer', 'r_ocean_speed_summer', 'r_ocean_warmth_winter', 'r_ocean_speed_winter'];
const PRECIP_INPUTS = ['r_precip_summer', 'r_precip_winter'];

// computeTemperature(mesh, r_xyz, r_elevation, windResult, oceanResult, precipResult, temperatureOffset = 0): the three results are
// the objects the earlier stages returned (their arrays are uploaded to the planet's blocks), or null / undefined for the blocks
// the planet's last computeWind / computeOceanCurrents / computePrecipitation left on the device.
export function computeTemperature(mesh, r_xyz, r_elevation, windResult, oceanResult, precipResult, temperatureOffset = 0) {
    if (!(r_elevation instanceof Float32Array) || r_elevation.length !== mesh.numRegions) {
        throw new RangeError(`computeTemperature: r_elevation must be a Float32Array of ${mesh.numRegions} entries`);
    }
    if (given(windResult)) checkInputs('computeTemperature', 'windResult', windResult, WIND_INPUTS, mesh.numRegions);
    if (given(oceanResult)) checkInputs('computeTemperature', 'oceanResult', oceanResult, OCEAN_INPUTS, mesh.numRegions);
    if (given(precipResult)) checkInputs('computeTemperature', 'precipResult', precipResult, PRECIP_INPUTS, mesh.numRegions);
    if (Number.isNaN(Number(temperatureOffset))) throw new RangeError('computeTemperature: temperatureOffset must be a number');
    const planet = planetFor(mesh, r_xyz);
    if (given(windResult)) uploadInputs(planet, addon.windUpload, WIND_INPUTS, windResult);
    if (given(oceanResult)) uploadInputs(planet, addon.oceanUpload, OCEAN_INPUTS, oceanResult);
    if (given(precipResult)) uploadInputs(planet, addon.precipUpload, PRECIP_INPUTS, precipResult);
    addon.computeTemperature(planet, r_elevation, Number(temperatureOffset));
    return downloadAll(planet, addon.temperatureDownload, TEMP_KEYS);
}
