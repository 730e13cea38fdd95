// Runs the REFERENCE's buildSuperPlates (js/super-plates.js) on the cases of a job file and dumps its outputs.  The function is
// imported at run time from a scratch copy of the reference's file (argument 1, beside a {"type":"module"} package.json); none of
// it is part of this repository.  Node 12 or later.  Test infrastructure.
//
//   node run_super_plates.mjs <dir with super-plates.js> <job.json>
import fs from 'fs';
import path from 'path';
import { pathToFileURL } from 'url';

const refDir = process.argv[2];
const job = JSON.parse(fs.readFileSync(process.argv[3], 'utf8'));

function readArr(file, Type) {
    const buf = fs.readFileSync(file);
    return new Type(buf.buffer.slice(buf.byteOffset, buf.byteOffset + buf.byteLength));
}
function writeArr(file, arr) { fs.writeFileSync(file, Buffer.from(arr.buffer, arr.byteOffset, arr.byteLength)); }

async function main() {
    const { buildSuperPlates } = await import(pathToFileURL(path.join(refDir, 'super-plates.js')).href);
    const adjOffset = readArr(job.adjOffset, Int32Array), adjList = readArr(job.adjList, Int32Array);
    const mesh = { numRegions: adjOffset.length - 1, adjOffset, adjList };
    const timing = {};
    for (const c of job.cases) {
        const r_plate = readArr(c.r_plate, Int32Array);
        const seeds = Array.from(readArr(c.plateSeeds, Int32Array));
        const vec4 = readArr(c.plateVec, Float64Array), hasVec = readArr(c.hasVec, Uint8Array);
        const isOcean = readArr(c.plateIsOcean, Uint8Array), dens = readArr(c.plateDensity, Float64Array);
        const plateVec = {}, plateDensity = {}, plateIsOcean = new Set();
        seeds.forEach((pid, i) => {
            if (hasVec[i]) plateVec[pid] = { pole: [vec4[4 * i], vec4[4 * i + 1], vec4[4 * i + 2]], omega: vec4[4 * i + 3] };
            if (!Number.isNaN(dens[i])) plateDensity[pid] = dens[i];
            if (isOcean[i]) plateIsOcean.add(pid);
        });
        let res = null;
        const reps = c.reps || 1, ms = [];
        for (let k = 0; k < reps; k++) {
            const t0 = process.hrtime.bigint();
            res = buildSuperPlates(mesh, r_plate, new Set(seeds), plateVec, plateIsOcean, plateDensity);
            ms.push(Number(process.hrtime.bigint() - t0) / 1e6);
        }
        timing[c.name] = ms;
        const n = res.numSuperPlates;
        const v = new Float64Array(4 * n), d = new Float64Array(n), o = new Uint8Array(n);
        for (let s = 0; s < n; s++) {
            v.set(res.superPlateVec[s].pole, 4 * s); v[4 * s + 3] = res.superPlateVec[s].omega;
            d[s] = res.superPlateDensity[s]; o[s] = res.superPlateIsOcean.has(s) ? 1 : 0;
        }
        if (c.out) {
            writeArr(c.out + 'r_superPlate.bin', res.r_superPlate); writeArr(c.out + 'superPlateVec.bin', v);
            writeArr(c.out + 'superPlateDensity.bin', d); writeArr(c.out + 'superPlateIsOcean.bin', o);
        }
    }
    if (job.timing) fs.writeFileSync(job.timing, JSON.stringify(timing));
}
main().catch((e) => { console.error(e.stack || e); process.exit(1); });
