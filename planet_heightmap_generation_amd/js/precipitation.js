// Counterpart of the reference's js/precipitation.js on the device: the same exported name, argument order and result object
// (the same keys in the same order, all Float32Array, without _precipTiming).  computePrecipitation runs in HIP kernels
// (csrc/precip.hip) on the planet bound to `mesh` (native.js: planetFor); the exactness contract is in csrc/precip_ops.h.  There
// is no JavaScript fallback: without the addon or a device the call throws.
import addon, { planetFor } from './native.js';
import { PRECIP_KEYS, given, checkInputs, uploadInputs, downloadAll } from './climate-blocks.js';

// the keys of windResult and of oceanResult the stage reads
const WIND_INPUTS = ['r_lat', 'r_lon', 'r_isLand', 'r_continentality', 'r_coastDistLand', 'r_eastX', 'r_eastY', 'r_eastZ', 'r_northX', 'r_northY', 'r_northZ',
    'itczLons', 'itczLatsSummer', 'itczLatsWinter', 'r_wind_east_summer', 'r_wind_north_summer', 'r_pressure_summer',
    'r_wind_east_winter', 'r_wind_north_winter', 'r_pressure_winter'];
const OCEAN_INPUTS = ['r_ocean_warmth_summer', 'r_ocean_warmth_winter'];

// computePrecipitation(mesh, r_xyz, r_elevation, windResult, oceanResult, precipitationOffset = 0, landCoverage = 0.3): windResult
// and oceanResult are the objects computeWind and computeOceanCurrents returned (their arrays are uploaded to the planet's wind
// and ocean blocks), or null / undefined for the blocks the planet's last computeWind / computeOceanCurrents left on the device.
export function computePrecipitation(mesh, r_xyz, r_elevation, windResult, oceanResult, precipitationOffset = 0, landCoverage = 0.3) {
    if (!(r_elevation instanceof Float32Array) || r_elevation.length !== mesh.numRegions) {
        throw new RangeError(`computePrecipitation: r_elevation must be a Float32Array of ${mesh.numRegions} entries`);
    }
    if (given(windResult)) checkInputs('computePrecipitation', 'windResult', windResult, WIND_INPUTS, mesh.numRegions);
    if (given(oceanResult)) checkInputs('computePrecipitation', 'oceanResult', oceanResult, OCEAN_INPUTS, mesh.numRegions);
    if (Number.isNaN(Number(precipitationOffset)) || Number.isNaN(Number(landCoverage))) throw new RangeError('computePrecipitation: precipitationOffset and landCoverage must be numbers');
    const planet = planetFor(mesh, r_xyz);
    if (given(windResult)) uploadInputs(planet, addon.windUpload, WIND_INPUTS, windResult);
    if (given(oceanResult)) uploadInputs(planet, addon.oceanUpload, OCEAN_INPUTS, oceanResult);
    addon.computePrecipitation(planet, r_elevation, Number(precipitationOffset), Number(landCoverage));
    return downloadAll(planet, addon.precipDownload, PRECIP_KEYS);
}
