// Golden generation only: runs the REFERENCE's generateFibonacciSphere(N, jitter, makeRng(seed)) and Node's own Math.sin / Math.cos.
// usage: node run_points.mjs <scratch copy of the reference's js/> <job.json>
import fs from 'fs';
import path from 'path';
import { pathToFileURL } from 'url';

const [refJs, jobPath] = process.argv.slice(2);
const job = JSON.parse(fs.readFileSync(jobPath, 'utf8'));
async function main() {
    const { generateFibonacciSphere } = await import(pathToFileURL(path.join(refJs, 'sphere-mesh.js')).href);
    const { makeRng } = await import(pathToFileURL(path.join(refJs, 'rng.js')).href);

    const crcTable = new Uint32Array(256);
    for (let n = 0; n < 256; n++) { let c = n; for (let k = 0; k < 8; k++) c = (c & 1) ? (0xEDB88320 ^ (c >>> 1)) : (c >>> 1); crcTable[n] = c >>> 0; }
    function crc32(bytes) {
        let c = 0xFFFFFFFF;
        for (let i = 0; i < bytes.length; i++) c = crcTable[(c ^ bytes[i]) & 0xFF] ^ (c >>> 8);
        return (c ^ 0xFFFFFFFF) >>> 0;
    }
    const write = (file, typed) => fs.writeFileSync(file, Buffer.from(typed.buffer, typed.byteOffset, typed.byteLength));

    const crcs = {};
    for (const c of job.cases) {
        const xyz = generateFibonacciSphere(c.N, c.jitter, makeRng(c.seed));
        crcs[c.name] = crc32(new Uint8Array(xyz.buffer, xyz.byteOffset, xyz.byteLength));
        write(c.out, xyz);
    }
    fs.writeFileSync(job.crcOut, JSON.stringify(crcs));

    for (const m of job.math) {
        const b = fs.readFileSync(m.x);
        const x = new Float64Array(b.buffer, b.byteOffset, b.byteLength / 8);
        const s = new Float64Array(x.length), c = new Float64Array(x.length);
        for (let i = 0; i < x.length; i++) { s[i] = Math.sin(x[i]); c[i] = Math.cos(x[i]); }
        write(m.sin, s); write(m.cos, c);
    }
}
main().catch((e) => { console.error(e); process.exit(1); });
