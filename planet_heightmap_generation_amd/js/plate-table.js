// The dense-by-id plate table the addon takes (include/worogen.h: wo_plate_table) from the reference's keyed objects and Sets, and
// the names of assignElevation's twelve debug layers in the addon's order: shared by elevation.js, super-plates.js and the worker.
export const LAYERS = ['base', 'tectonic', 'noise', 'interior', 'coastal', 'ocean', 'hotspot', 'tecActivity', 'margins', 'backArc', 'foldRidge', 'orogenicPower'];

// ids (optional): further plate ids the table must have room for (a plate with no vector, no density and no ocean flag has no key)
export function denseTable(isOceanSet, vec, density, ids) {
    let maxId = -1;
    if (ids) for (const k of ids) maxId = Math.max(maxId, +k);
    for (const k of Object.keys(vec)) maxId = Math.max(maxId, +k);
    for (const k of Object.keys(density)) maxId = Math.max(maxId, +k);
    for (const k of isOceanSet) maxId = Math.max(maxId, +k);
    const n = maxId + 1;
    const t = { numIds: n, hasVec: new Uint8Array(n), pole: new Float64Array(3 * n), omega: new Float64Array(n),
                isOcean: new Uint8Array(n), density: new Float64Array(n).fill(NaN) };
    for (const k of Object.keys(vec)) { const id = +k, v = vec[k]; t.hasVec[id] = 1; t.pole.set(v.pole, 3 * id); t.omega[id] = v.omega; }
    for (const k of isOceanSet) t.isOcean[+k] = 1;
    for (const k of Object.keys(density)) t.density[+k] = density[k];
    return t;
}
