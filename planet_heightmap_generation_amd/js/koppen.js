// Counterpart of the reference's js/koppen.js on the device: the same exported names, argument order and result (a Uint8Array of
// class ids, indices into KOPPEN_CLASSES).  classifyKoppen runs in one HIP kernel (csrc/temp.hip; the body is csrc/temp_ops.h's
// koppen_cell) on the planet bound to `mesh` (native.js: planetFor).  Given the same inputs every cell has the reference's class.
// There is no JavaScript fallback: without the addon or a device the call throws.
import addon, { planetFor } from './native.js';
import { TEMP_KEYS as TEMP_INPUTS, given, checkInputs, uploadInputs } from './climate-blocks.js';

// class id -> { code, name, color [r, g, b] 0-1 } (the reference's table, js/koppen.js:19-51)
export const KOPPEN_CLASSES = [
    { code: 'Ocean', name: 'Ocean', color: [0.29, 0.44, 0.65] },
    { code: 'Af', name: 'Tropical rainforest', color: [0.00, 0.00, 1.00] },
    { code: 'Am', name: 'Tropical monsoon', color: [0.00, 0.47, 1.00] },
    { code: 'Aw', name: 'Tropical savanna', color: [0.27, 0.67, 0.98] },
    { code: 'BWh', name: 'Hot desert', color: [1.00, 0.00, 0.00] },
    { code: 'BWk', name: 'Cold desert', color: [1.00, 0.59, 0.59] },
    { code: 'BSh', name: 'Hot steppe', color: [0.96, 0.65, 0.00] },
    { code: 'BSk', name: 'Cold steppe', color: [1.00, 0.86, 0.39] },
    { code: 'Cfa', name: 'Humid subtropical', color: [0.78, 1.00, 0.31] },
    { code: 'Cfb', name: 'Oceanic', color: [0.39, 1.00, 0.31] },
    { code: 'Cfc', name: 'Subpolar oceanic', color: [0.20, 0.78, 0.00] },
    { code: 'Csa', name: 'Hot-summer Mediterranean', color: [1.00, 1.00, 0.00] },
    { code: 'Csb', name: 'Warm-summer Mediterranean', color: [0.78, 0.78, 0.00] },
    { code: 'Csc', name: 'Cold-summer Mediterranean', color: [0.59, 0.59, 0.00] },
    { code: 'Cwa', name: 'Humid subtropical (monsoon)', color: [0.59, 1.00, 0.59] },
    { code: 'Cwb', name: 'Subtropical highland', color: [0.39, 0.78, 0.39] },
    { code: 'Cwc', name: 'Cold subtropical highland', color: [0.20, 0.59, 0.20] },
    { code: 'Dfa', name: 'Hot-summer continental', color: [0.00, 1.00, 1.00] },
    { code: 'Dfb', name: 'Warm-summer continental', color: [0.22, 0.78, 1.00] },
    { code: 'Dfc', name: 'Subarctic', color: [0.00, 0.49, 0.49] },
    { code: 'Dfd', name: 'Extremely cold subarctic', color: [0.00, 0.27, 0.37] },
    { code: 'Dsa', name: 'Hot-summer continental (dry summer)', color: [0.90, 0.50, 1.00] },
    { code: 'Dsb', name: 'Warm-summer continental (dry summer)', color: [0.70, 0.35, 0.85] },
    { code: 'Dsc', name: 'Subarctic (dry summer)', color: [0.50, 0.20, 0.65] },
    { code: 'Dsd', name: 'Extremely cold subarctic (dry summer)', color: [0.35, 0.10, 0.45] },
    { code: 'Dwa', name: 'Hot-summer continental (monsoon)', color: [0.67, 0.69, 1.00] },
    { code: 'Dwb', name: 'Warm-summer continental (monsoon)', color: [0.43, 0.47, 0.78] },
    { code: 'Dwc', name: 'Subarctic (monsoon)', color: [0.29, 0.31, 0.78] },
    { code: 'Dwd', name: 'Extremely cold subarctic (monsoon)', color: [0.20, 0.00, 0.53] },
    { code: 'ET', name: 'Tundra', color: [0.70, 0.70, 0.70] },
    { code: 'EF', name: 'Ice cap', color: [0.41, 0.41, 0.41] },
];
const PRECIP_INPUTS = ['r_precip_summer', 'r_precip_winter'];

// classifyKoppen(mesh, r_elevation, tempResult, precipResult): the two results are the objects computeTemperature and
// computePrecipitation returned (uploaded to the planet's blocks), or null / undefined for the blocks they left on the device.
export function classifyKoppen(mesh, r_elevation, tempResult, precipResult) {
    if (!(r_elevation instanceof Float32Array) || r_elevation.length !== mesh.numRegions) {
        throw new RangeError(`classifyKoppen: r_elevation must be a Float32Array of ${mesh.numRegions} entries`);
    }
    if (given(tempResult)) checkInputs('classifyKoppen', 'tempResult', tempResult, TEMP_INPUTS, mesh.numRegions);
    if (given(precipResult)) checkInputs('classifyKoppen', 'precipResult', precipResult, PRECIP_INPUTS, mesh.numRegions);
    const planet = planetFor(mesh);
    if (given(tempResult)) uploadInputs(planet, addon.temperatureUpload, TEMP_INPUTS, tempResult);
    if (given(precipResult)) uploadInputs(planet, addon.precipUpload, PRECIP_INPUTS, precipResult);
    return addon.classifyKoppen(planet, r_elevation);
}
