// What the climate stages share on the JavaScript side: the result keys of the four blocks a planet keeps on the device (each in
// the order the reference's stage sets them) with their typed-array types, the check of a caller's result object, and the loops
// that upload its arrays to a block and download a block's fields.  The C side of the same path is csrc/stage_block.h.
export const WIND_KEYS = ['r_pressure_summer', 'r_wind_east_summer', 'r_wind_north_summer', 'r_wind_speed_summer',
    'r_pressure_winter', 'r_wind_east_winter', 'r_wind_north_winter', 'r_wind_speed_winter',
    'itczLons', 'itczLatsSummer', 'itczLatsWinter', 'r_lat', 'r_lon', 'r_sinLat', 'r_isLand',
    'r_continentality', 'r_coastDistLand', 'r_plateContinentality', 'r_eastX', 'r_eastY', 'r_eastZ', 'r_northX', 'r_northY', 'r_northZ'];
export const OCEAN_KEYS = ['r_ocean_current_east_summer', 'r_ocean_current_north_summer', 'r_ocean_speed_summer', 'r_ocean_warmth_summer',
    'r_ocean_current_east_winter', 'r_ocean_current_north_winter', 'r_ocean_speed_winter', 'r_ocean_warmth_winter'];
// summer's pair, then winter's
export const PRECIP_KEYS = ['r_precip_summer', 'r_rainshadow_summer', 'r_precip_winter', 'r_rainshadow_winter'];
export const TEMP_KEYS = ['r_temperature_summer', 'r_temperature_winter'];

// the typed array of a result key, and its length on a mesh of numRegions cells (the ITCZ arrays are per longitude sample)
export const typeOf = (k) => (k === 'r_isLand' ? Uint8Array : k === 'r_coastDistLand' ? Int32Array : Float32Array);
export const lengthOf = (k, numRegions) => (k.startsWith('itcz') ? 360 : numRegions);

export const given = (x) => x !== null && x !== undefined;

// every key of `keys` in the caller's result object `what` must hold the typed array of its block, at full length
export function checkInputs(fn, what, result, keys, numRegions) {
    for (const k of keys) {
        const a = result[k], n = lengthOf(k, numRegions), T = typeOf(k);
        if (!(a instanceof T) || a.length !== n) throw new RangeError(`${fn}: ${what}.${k} must be a ${T.name} of ${n} entries`);
    }
}

// uploadFn: addon.windUpload, .oceanUpload, .precipUpload or .temperatureUpload
export function uploadInputs(planet, uploadFn, keys, result) {
    for (const k of keys) uploadFn(planet, k, result[k]);
}

// downloadFn: addon.oceanDownload, .precipDownload or .temperatureDownload; the object has the keys in the order of `keys`
export function downloadAll(planet, downloadFn, keys) {
    const result = {};
    for (const k of keys) result[k] = downloadFn(planet, k);
    return result;
}
