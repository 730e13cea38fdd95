// Rivers and lakes for hosts of the worker (ours: the reference keeps no drainage beyond the scratch of erodeComposite): the drainage of
// the final terrain with its depressions resolved so that rivers reach the sea, lake levels, the runoff accumulated down the
// receivers in exact fixed point, and the segments of the cells whose flow reaches a threshold.  Everything runs in HIP kernels
// (csrc/rivers.hip; the contract is in csrc/rivers_ops.h) on the planet bound to `mesh` (native.js: planetFor); there is no JavaScript
// fallback.  The five fields stay on the planet, where mapColorRivers and exportGlobe's `rivers` read them.
import addon, { planetFor } from './native.js';

// the runoff sources in the order of WO_RIVERS_RUNOFF_PRECIP, _UNIFORM, _VALUES (include/worogen.h)
export const RIVER_RUNOFF = ['precip', 'uniform', 'values'];
// the fields of the rivers block: Int32Array, Int32Array, Float32Array, BigUint64Array (units of 2^-16), Float32Array
export const RIVER_KEYS = ['r_river_receiver', 'r_river_basin', 'r_lake_level', 'r_river_discharge', 'r_river_flow'];
export const RIVER_TINT = [41, 98, 168, 255];

// a command's or a caller's { minFlow } -> the number
export function checkedMinFlow(fn, rivers) {
    const minFlow = rivers && typeof rivers === 'object' ? rivers.minFlow : rivers;
    if (typeof minFlow !== 'number' || !Number.isFinite(minFlow)) throw new RangeError(`${fn}: rivers takes { minFlow }, a finite number`);
    return minFlow;
}

// on a planet handle (what the worker holds); r_elevation null: the planet's resident field.  runoff: 'precip' (the planet's resident
// precipitation fields), 'uniform', or a Float32Array of numRegions values.  -> the counts of wo_rivers_info, and with `download` the
// five fields under RIVER_KEYS
export function computeRiversOnPlanet(planet, r_elevation, runoff, download) {
    const src = runoff === undefined || runoff === null ? 'precip' : runoff;
    let source = 2, values = null;
    if (src instanceof Float32Array) values = src;
    else {
        source = RIVER_RUNOFF.indexOf(src);
        if (source < 0 || source > 1) throw new RangeError(`computeRivers: unknown runoff '${src}' (one of precip, uniform, or a Float32Array of values)`);
    }
    const res = addon.computeRivers(planet, r_elevation || null, source, values);
    if (download) for (const k of RIVER_KEYS) res[k] = addon.riversDownload(planet, k);
    return res;
}
// -> { segments: Float32Array(count * 6), flows: Float32Array(count), count }, in ascending cell order
export function riverLinesOnPlanet(planet, minFlow, r_elevation) {
    return addon.riverLines(planet, checkedMinFlow('riverLines', minFlow), r_elevation || null);
}

// computeRivers(mesh, r_xyz, r_elevation, { runoff, download = true })
export function computeRivers(mesh, r_xyz, r_elevation, opts) {
    const o = opts || {};
    return computeRiversOnPlanet(planetFor(mesh, r_xyz), r_elevation, o.runoff, o.download !== false);
}
// riverLines(mesh, r_xyz, minFlow, r_elevation): after computeRivers on the same mesh
export function riverLines(mesh, r_xyz, minFlow, r_elevation) {
    return riverLinesOnPlanet(planetFor(mesh, r_xyz), minFlow, r_elevation);
}
