#!/usr/bin/env python3
"""Generate the fixtures of plate generation and of the worker's `generate` by running the REFERENCE under Node 12 in this
container: tests/golden/coarse_plates_cases.npz, math_v8_trig.npz, generate_N10000_s1.npz and generate_N5000_s3_P6.npz.

The reference sources are copied to a scratch directory (oracle/ref_harness/make_golden.py: prepare_reference); they never enter
this repository.  In the scratch copy only, planet-worker.js gets its CDN Delaunator import replaced by a local stub module that
returns the build's planar triangulation for the point set (the same stub as make_golden_import.py; keyed by point count and a
checksum of the points, because every case of the table has a coarse mesh of the same size).  run_generate.mjs then calls the
reference's generateCoarsePlates / generatePlates / assignOceanLand on the case table, V8's Math.sin / cos / exp on the math
arguments, and the worker's own self.onmessage with the two `generate` commands, whose `done` messages are recorded.

Running this again reproduces every array exactly.  The host time of the reference's generateCoarsePlates is printed.

Usage:  python tools/ref_harness/make_golden_generate.py [--ref /root/reference]
"""
from __future__ import annotations

import argparse
import json
import subprocess
import sys
import tempfile
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(REPO))
from oracle.ref_harness.make_golden import prepare_reference  # noqa: E402
from oracle.ref_harness.make_golden_elevation import planar_triangulation  # noqa: E402
from planet_heightmap_generation_amd import sphere_mesh as SM  # noqa: E402

GOLD = REPO / "tests" / "golden"
HARNESS = Path(__file__).resolve().parent / "run_generate.mjs"
# the generator page's default sliders (index.html)
UI = dict(terrainWarp=0.75, smoothing=0.10, glacialErosion=0.50, hydraulicErosion=0.50, thermalErosion=0.10, ridgeSharpening=0.50)
STUB = """// stub Delaunay provider (golden generation only): the build's planar triangulation for the point set
export default class Delaunator {
    constructor(flat) {
        let h = 0;
        for (let i = 0; i < flat.length; i += 97) h = (h * 31 + Math.floor(flat[i] * 1e6)) | 0;
        const t = globalThis.__woTriangulations[flat.length / 2 + ':' + h];
        if (!t) throw new Error('no triangulation for n=' + flat.length / 2 + ' crc ' + h);
        this.triangles = new Uint32Array(t.triangles); this.halfedges = t.halfedges;
    }
}
"""

# (seed, P, numContinents, continentSizeVariety, landCoverage); every P of {1, 2, 7, 8, 20, 21, 50, 79, 80, 120} (both ends and the
# interior of lowPlateT, odd and even counts, 1 / 2 / 3 smoothing passes), numContinents 1, 4 and more than P, variety 0 / 0.5 / 1,
# coverage 0.1 / 0.3 / 0.6, many continents on little land (the seed trim)
CASES = [
    (1, 1, 4, 0, 0.3), (2, 2, 1, 0, 0.3), (3, 2, 4, 0.5, 0.6), (4, 7, 4, 0, 0.3), (5, 7, 12, 1, 0.1), (6, 8, 4, 0.5, 0.3),
    (7, 8, 1, 0, 0.6), (8, 20, 4, 0, 0.3), (9, 20, 30, 0.5, 0.1), (10, 21, 4, 1, 0.3), (11, 21, 1, 0.5, 0.6), (12, 50, 4, 0, 0.3),
    (13, 50, 12, 1, 0.1), (14, 50, 8, 0.5, 0.6), (15, 79, 4, 0, 0.3), (16, 79, 6, 1, 0.6), (17, 80, 4, 0.5, 0.3), (18, 80, 1, 0, 0.1),
    (19, 120, 4, 0, 0.3), (20, 120, 40, 1, 0.1), (21, 120, 10, 0.5, 0.6), (22, 30, 10, 0, 0.6), (23, 40, 6, 0.5, 0.45), (24, 12, 3, 1, 0.6),
    (28, 20, 30, 0, 0.6), (29, 50, 60, 0.5, 0.6),        # every plate a continent seed, trimmed to the budget: seas between two continents
]
MESH_CASES = [("mesh_N2000_s1", 31, 9, 3, 0.5, 0.3), ("mesh_N2000_s1", 32, 40, 4, 0, 0.3)]     # (mesh golden, seed, P, ...)
GENERATE = {
    "generate_N10000_s1": dict(N=10000, P=80, jitter=0.75, nMag=0.4, numContinents=4, seed=1, skipClimate=True, **UI),
    "generate_N5000_s3_P6": dict(N=5000, P=6, jitter=0.75, nMag=0.4, numContinents=2, continentSizeVariety=0.7, landCoverage=0.45,
                                 toggledIndices=[0, 3], seed=3, skipClimate=True, **UI),
}


def stub_key(n: int, jitter: float, seed: float) -> int:
    """The stub's checksum of the stereographic points the reference hands its Delaunay provider (js/sphere-mesh.js:160-172)."""
    xyz = SM.fibonacci_sphere(n, jitter, seed).astype(np.float64).reshape(-1, 3)[:n]
    flat = np.empty(2 * n)
    flat[0::2] = xyz[:, 0] / (1 - xyz[:, 2])
    flat[1::2] = xyz[:, 1] / (1 - xyz[:, 2])
    h = 0
    for v in flat[::97]:
        h = (h * 31 + int(np.floor(v * 1e6))) & 0xFFFFFFFF
        h = h - (1 << 32) if h >= (1 << 31) else h
    return h


def trig_args():
    """[0, 2pi): (the harness prepends every theta the case table's generatePlates calls hand Math.cos) the neighbourhoods of the multiples of pi/4 (+- 4 ulps), 0, the largest double below
    2pi, the kernels' thresholds, and a uniform sample; exp on [-1.25, 1.25] with its branch boundaries."""
    rng = np.random.default_rng(2718)
    two_pi = 2 * np.pi
    near = []
    for k in range(0, 9):
        for base in (k * np.pi / 4, np.float64(np.float32(k * np.pi / 4))):
            v = base
            near.append(v)
            up = dn = v
            for _ in range(4):
                up = np.nextafter(up, np.inf); dn = np.nextafter(dn, -np.inf)
                near += [up, dn]
    for b in (2.0 ** -27, 2.0 ** -26, 0.3, 0.78125, 0.2999999523162842, 2.356194490192345):
        near += [b, np.nextafter(b, 0), np.nextafter(b, 7)]
    near = np.array(near)
    near = near[(near >= 0) & (near < two_pi)]
    x = np.concatenate([near, [0.0, np.nextafter(two_pi, 0)], rng.uniform(0, two_pi, 3000), rng.uniform(0, 1e-6, 50)])
    ex = [0.0, -0.0, 1.0, -1.0, 1.25, -1.25, 2.0 ** -28, 2.0 ** -29, -2.0 ** -28]
    for b in (0.5 * np.log(2), 1.5 * np.log(2)):
        v = b
        for _ in range(4):
            ex += [v, -v]
            v = np.nextafter(v, np.inf)
        v = b
        for _ in range(4):
            v = np.nextafter(v, 0)
            ex += [v, -v]
    e = np.concatenate([np.array(ex), rng.uniform(-1.25, 1.25, 3000)])
    return x.astype(np.float64), e.astype(np.float64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    args = ap.parse_args()
    with tempfile.TemporaryDirectory(prefix="wo_golden_gen_") as td:
        work = Path(td)
        ref_js = prepare_reference(Path(args.ref), work)
        pw = ref_js / "planet-worker.js"
        src = pw.read_text()
        line = next(ln for ln in src.splitlines() if ln.startswith("import Delaunator from 'https://"))
        (ref_js / "wo-stub-delaunator.js").write_text(STUB)
        pw.write_text(src.replace(line, "import Delaunator from './wo-stub-delaunator.js';"))
        put = lambda name, a: (np.ascontiguousarray(a).tofile(work / name), str(work / name))[1]  # noqa: E731

        meshes = {(20000, 0.75, float(c[0] + 137)) for c in CASES} | {(20000, 0.75, 1.0 + 137), (20000, 0.75, 3.0 + 137)}
        meshes |= {(m["N"], m["jitter"], float(m["seed"])) for m in GENERATE.values()}
        meshes |= {(20000, 0.75, 137.0 + s) for s in (101, 102)}
        trs = []
        for n, jit, sd in sorted(meshes):
            t, h = planar_triangulation(n, jit, sd)
            trs.append(dict(n=n, crc=stub_key(n, jit, sd), triangles=put(f"tri_{n}_{sd}.bin", t), halfedges=put(f"he_{n}_{sd}.bin", h)))
        job = dict(triangulations=trs, cases=[], generate=[])
        for i, (seed, P, nc, var, cov) in enumerate(CASES):
            job["cases"].append(dict(seed=seed, P=P, numContinents=nc, variety=var, coverage=cov, out=str(work / f"c{i}_")))
        for j, (mname, seed, P, nc, var, cov) in enumerate(MESH_CASES):
            g = np.load(GOLD / f"{mname}.npz")
            nr = int(g["numRegions"])
            E = int(g["ref_adjOffset"][-1])
            mesh = dict(numRegions=nr, adjOffset=put(f"m{j}_off.bin", g["ref_adjOffset"]), adjList=put(f"m{j}_adj.bin", g["ref_adjList"][:E]),
                        xyz=put(f"m{j}_xyz.bin", g["xyz"]))
            job["cases"].append(dict(seed=seed, P=P, numContinents=nc, variety=var, coverage=cov, mesh=mesh, out=str(work / f"m{j}_")))
        tx, ex = trig_args()
        job["math"] = dict(trig_x=put("trig_x.bin", tx), exp_x=put("exp_x.bin", ex), trig_x_out=str(work / "trig_x_all.bin"), sin_out=str(work / "sin.bin"), cos_out=str(work / "cos.bin"),
                           exp_out=str(work / "exp.bin"))
        job["timing"] = dict(runs=9, cases=[dict(seed=101, P=20), dict(seed=102, P=80)], out=str(work / "timing.json"))
        for name, msg in GENERATE.items():
            job["generate"].append(dict(message=msg, out=str(work / f"{name}_")))
        (work / "job.json").write_text(json.dumps(job))
        subprocess.run(["node", "--harmony-optional-chaining", "--harmony-nullish", "--max-old-space-size=6000", str(HARNESS), str(ref_js),
                        str(work / "job.json")], check=True)

        # ---- coarse_plates_cases.npz ----
        table = [dict(seed=s, P=P, numContinents=nc, variety=v, coverage=c, mesh=None) for s, P, nc, v, c in CASES]
        table += [dict(seed=s, P=P, numContinents=nc, variety=v, coverage=c, mesh=m) for m, s, P, nc, v, c in MESH_CASES]
        data = {"meta_json": np.frombuffer(json.dumps(dict(cases=table)).encode(), np.uint8)}
        prefixes = [f"c{i}_" for i in range(len(CASES))] + [f"m{j}_" for j in range(len(MESH_CASES))]
        for i, pre in enumerate(prefixes):
            rp = np.fromfile(work / f"{pre}r_plate.bin", np.int32)
            data[f"c{i}_r_plate"] = rp.astype(np.uint16) if rp.max() < 65536 and rp.min() >= 0 else rp
            data[f"c{i}_seeds"] = np.fromfile(work / f"{pre}seeds.bin", np.int32)
            data[f"c{i}_vec"] = np.fromfile(work / f"{pre}vec.bin", np.float64)
            data[f"c{i}_ocean"] = np.fromfile(work / f"{pre}ocean.bin", np.uint8)
        np.savez_compressed(GOLD / "coarse_plates_cases.npz", **data)
        # ---- math_v8_trig.npz ----
        tx = np.fromfile(work / "trig_x_all.bin", np.float64)
        assert tx.size >= sum(min(c[1], 20001) for c in CASES) and (tx >= 0).all() and (tx < 2 * np.pi).all()
        np.savez_compressed(GOLD / "math_v8_trig.npz", trig_x=tx, sin_v8=np.fromfile(work / "sin.bin", np.float64),
                            cos_v8=np.fromfile(work / "cos.bin", np.float64), exp_x=ex, exp_v8=np.fromfile(work / "exp.bin", np.float64))
        # ---- the two done messages ----
        f32 = ("r_xyz", "t_xyz", "prePostElev", "r_elevation", "t_elevation", "r_stress")
        i32 = ("triangles", "halfedges", "r_plate", "plateSeeds", "plateIsOcean", "originalPlateIsOcean", "mountain_r", "coastline_r", "ocean_r")
        f64 = ("plateVec", "plateDensity", "plateDensityLand", "plateDensityOcean")
        for name in GENERATE:
            meta = json.loads((work / f"{name}_meta.json").read_text())
            d = {"meta_json": np.frombuffer(json.dumps(meta).encode(), np.uint8)}
            for k in f32:
                d[k] = np.fromfile(work / f"{name}_{k}.bin", np.float32)
            for k in i32:
                d[k] = np.fromfile(work / f"{name}_{k}.bin", np.int32)
            for k in f64:
                d[k] = np.fromfile(work / f"{name}_{k}.bin", np.float64)
            for k in meta["debugLayers"]:
                d[f"dl_{k}"] = np.fromfile(work / f"{name}_dl_{k}.bin", np.float32)
            np.savez_compressed(GOLD / f"{name}.npz", **d)
        for f in ["coarse_plates_cases", "math_v8_trig"] + list(GENERATE):
            print(f"wrote tests/golden/{f}.npz ({(GOLD / (f + '.npz')).stat().st_size / 1024:.0f} KiB)")
        print("reference generateCoarsePlates, host time (ms):", (work / "timing.json").read_text())


if __name__ == "__main__":
    main()
