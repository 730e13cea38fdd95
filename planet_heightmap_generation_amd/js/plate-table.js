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

// The three density tables of handleGenerate (js/planet-worker.js:193-201): per plate a Park-Miller stream seeded with id + 777
// (js/rng.js:3-6), first draw oceanic (3.0 .. 3.5), second continental (2.4 .. 2.9); plateDensity takes the one of the plate's kind.
export function plateDensities(plateSeeds, plateIsOcean) {
    const isOcean = plateIsOcean instanceof Set ? plateIsOcean : new Set(plateIsOcean);
    const plateDensity = {}, plateDensityLand = {}, plateDensityOcean = {};
    for (const r of plateSeeds) {
        let s = (Math.abs(Math.floor((r + 777) * 9301 + 49297)) % 2147483646) + 1;
        const draw = () => { s = (s * 16807) % 2147483647; return (s - 1) / 2147483646; };
        plateDensityOcean[r] = 3.0 + draw() * 0.5;
        plateDensityLand[r] = 2.4 + draw() * 0.5;
        plateDensity[r] = isOcean.has(r) ? plateDensityOcean[r] : plateDensityLand[r];
    }
    return { plateDensity, plateDensityLand, plateDensityOcean };
}
