#!/usr/bin/env python3
"""Generate tests/golden/wind_*.npz by running the REFERENCE's unmodified computeWind (js/wind.js:394-687) under Node 12.

The reference sources are copied to a scratch directory (oracle/ref_harness/make_golden.py: prepare_reference); they never
enter this repository and no reference file is patched: run_wind.mjs sets globalThis.performance before its dynamic import.

Cases (inputs that another fixture already holds are not stored twice):
  wind_config1_N10000_s1   mesh, r_plate, plates and ref_final_elevation of elev_config1_N10000_s1.npz, noise seed 1
  wind_import_N10000_s1    done_r_elevation / done_r_plate / done_plateIsOcean of import_N10000_s1.npz on mesh_N10000_s1
  wind_N2000_ocean_s1      mesh_N2000_s1, every cell at -0.5, four plates, all oceanic
  wind_N2000_land_s1       mesh_N2000_s1, every cell at 0.25, four plates, none oceanic
  wind_N250000_s4          the planet of elev_N250000_s4_large.npz (mesh rebuilt, checksums checked); r_coastDistLand and the
                           ITCZ arrays in full, every other output as its CRC32 plus every 16th cell
  wind_N2000_edges_s1      mesh_N2000_s1 with twelve cells moved (by less than a cell spacing) onto the poles, the date line and
                           lon = +-pi/2 (EDGE_TARGETS), the terrain and plates of rule_terrain / band_plates; positions stored
  wind_N{63,255,256,4096}_shape_s1   reference_mesh(N, 0.75, 1): 64, 256, 257 and 4 097 cells (one wave, one block, one block and a
                           cell, one radix tile and a pair), the same terrain and plate rule; the mesh is not stored, its CRC32s are

Usage:  python tools/ref_harness/make_golden_wind.py [--ref /root/reference] [--only NAME] [--time-cells N]
  --time-cells N   no fixture is written: the reference's wall time of computeWind on the N-cell planet of
                   tests/wind_common.py: synthetic_case (the planet profiles/wind_probe.py runs on the device) is printed
"""
from __future__ import annotations

import argparse
import json
import subprocess
import sys
import tempfile
import zlib
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(REPO))
sys.path.insert(0, str(REPO / "tests"))
from oracle.ref_harness.make_golden import prepare_reference  # noqa: E402

GOLD = REPO / "tests" / "golden"
HARNESS = Path(__file__).resolve().parent / "run_wind.mjs"
STRIDE = 16
TYPES = dict(Float32Array=np.float32, Int32Array=np.int32, Uint8Array=np.uint8)


def crc(a) -> int:
    return zlib.crc32(np.ascontiguousarray(a).tobytes()) & 0xFFFFFFFF


def _f32(v) -> float:
    return float(np.float32(v))


def edge_targets():
    """Positions (f64 values of exact f32 numbers) that no Fibonacci planet has: both poles (the south one through the tangent
    frame's fallback with non-zero x and z), one just outside the fallback, one at the largest |y| below 1, lon = +-pi/2 with
    z = +-0, and six cells on the date line whose x alternates between -0 and +0."""
    t = [(0.0, 1.0, 0.0), (1e-11, -1.0, -5e-11), (1.0, 0.0, 0.0), (-1.0, 0.0, -0.0)]
    for i, deg in enumerate((-60, -30, 0, 30, 60, 80)):
        y = _f32(np.sin(np.radians(deg)))
        t.append((-0.0 if i % 2 == 0 else 0.0, y, -_f32(np.sqrt(1 - y * y))))
    y = float(np.nextafter(np.float32(1), np.float32(0)))
    t.append((_f32(np.sqrt(1 - y * y)), y, 0.0))                    # |y| one f32 step under 1, z = +0 in the northern cap
    t.append((1e-10, 1.0, 1e-10))                                    # |(x, z)| = 1.41e-10: the first frame past the fallback
    return np.array(t, np.float64).astype(np.float32)


def snap_to_targets(xyz, targets):
    """For each target in turn, the nearest cell not used yet and not the closing cell (0, 0, 1) is moved onto it."""
    P = np.array(xyz, np.float32).reshape(-1, 3)
    closing = np.flatnonzero((P == np.array([0, 0, 1], np.float32)).all(axis=1))
    used, moved = set(closing.tolist()), []
    for t in targets:
        d = np.linalg.norm(P.astype(np.float64) - t.astype(np.float64), axis=1)
        d[list(used)] = np.inf
        r = int(np.argmin(d))
        moved.append((r, float(d[r])))
        used.add(r)
        P[r] = t
    return P.reshape(-1), moved


def rule_terrain(xyz):
    """Land (+0.25) where sin(3 lon + 1) cos(2 lat) > 0.25 or lat < -70 degrees, ocean (-0.5) elsewhere."""
    P = np.asarray(xyz, np.float32).reshape(-1, 3).astype(np.float64)
    lat, lon = np.arcsin(np.clip(P[:, 1], -1, 1)), np.arctan2(P[:, 0], P[:, 2])
    land = (np.sin(3 * lon + 1) * np.cos(2 * lat) > 0.25) | (lat < np.radians(-70))
    return np.where(land, 0.25, -0.5).astype(np.float32)


def band_plates(n):
    """Plate ids 0, 7, 14, 21 in four bands of cells; 0 and 14 are oceanic."""
    return (np.arange(n, dtype=np.int32) * 4 // n).astype(np.int32) * 7, np.array([0, 14], np.int32)


SHAPE_SIZES = (63, 255, 256, 4096)


def cases(only=None):
    out = []
    want = lambda name: only in (None, name)  # noqa: E731
    if want("wind_N2000_edges_s1"):
        m = np.load(GOLD / "mesh_N2000_s1.npz")
        xyz, moved = snap_to_targets(m["xyz"], edge_targets())
        print("wind_N2000_edges_s1: cells moved (cell, distance): " + ", ".join(f"{r} {d:.3f}" for r, d in moved))
        assert max(d for _, d in moved) < 0.07
        plate, ocean = band_plates(xyz.size // 3)
        out.append(dict(name="wind_N2000_edges_s1", off=m["ref_adjOffset"], adj=m["ref_adjList"], xyz=xyz, e=rule_terrain(xyz), plate=plate, ocean=ocean, seed=1,
                        store=("xyz", "e", "plate", "ocean"), sparse=False, extra=dict(mesh="mesh_N2000_s1", moved=[r for r, _ in moved])))
    for n in SHAPE_SIZES:
        if want(f"wind_N{n}_shape_s1"):
            from plates_common import reference_mesh
            mesh, xyz = reference_mesh(n, 0.75, 1)
            plate, ocean = band_plates(mesh.numRegions)
            out.append(dict(name=f"wind_N{n}_shape_s1", off=mesh.adjOffset, adj=mesh.adjList, xyz=xyz, e=rule_terrain(xyz), plate=plate, ocean=ocean, seed=1,
                            store=("e", "plate", "ocean"), sparse=False,
                            extra=dict(mesh_N=n, crc_xyz=crc(np.asarray(xyz, np.float32)), crc_adjOffset=crc(mesh.adjOffset), crc_adjList=crc(mesh.adjList))))
    if only is not None and out:
        return out
    g = np.load(GOLD / "elev_config1_N10000_s1.npz")
    out.append(dict(name="wind_config1_N10000_s1", off=g["adjOffset"], adj=g["adjList"], xyz=g["xyz"], e=g["ref_final_elevation"], plate=g["r_plate"],
                    ocean=g["plateSeeds"][g["plateIsOcean"] == 1], seed=1, store=(), sparse=False))
    m = np.load(GOLD / "mesh_N10000_s1.npz")
    i = np.load(GOLD / "import_N10000_s1.npz")
    out.append(dict(name="wind_import_N10000_s1", off=m["ref_adjOffset"], adj=m["ref_adjList"], xyz=m["xyz"], e=i["done_r_elevation"], plate=i["done_r_plate"],
                    ocean=i["done_plateIsOcean"], seed=1, store=(), sparse=False))
    m = np.load(GOLD / "mesh_N2000_s1.npz")
    n = int(m["numRegions"])
    plate = (np.arange(n, dtype=np.int32) * 4 // n).astype(np.int32) * 7          # plate ids 0, 7, 14, 21 in four bands of cells
    for tag, v, oc in (("ocean", -0.5, [0, 7, 14, 21]), ("land", 0.25, [])):
        out.append(dict(name=f"wind_N2000_{tag}_s1", off=m["ref_adjOffset"], adj=m["ref_adjList"], xyz=m["xyz"], e=np.full(n, v, np.float32), plate=plate,
                        ocean=np.array(oc, np.int32), seed=1, store=("e", "plate", "ocean"), sparse=False))
    g = np.load(GOLD / "elev_N250000_s4_large.npz")
    meta = json.loads(bytes(g["meta_json"]).decode())
    from plates_common import reference_mesh
    mesh, xyz = reference_mesh(meta["N"], 0.75, meta["seed"])
    assert crc(xyz) == meta["crc_xyz"] and crc(mesh.adjOffset) == meta["crc_adjOffset"] and crc(mesh.adjList) == meta["crc_adjList"], "not the mesh of elev_N250000_s4_large"
    out.append(dict(name="wind_N250000_s4", off=mesh.adjOffset, adj=mesh.adjList, xyz=xyz, e=g["ref_elevation"], plate=g["r_plate"],
                    ocean=g["plateSeeds"][g["plateIsOcean"] == 1], seed=4, store=("ocean",), sparse=True))
    return out


def timing_case(n_cells: int):
    import wind_common as WC
    c = WC.synthetic_case(n_cells)
    return dict(name=c["name"], off=c["off"], adj=c["adj"], xyz=c["xyz"], e=c["e"], plate=c["plate"], ocean=c["ocean"], seed=c["seed"], store=(), sparse=False)


def run(ref: Path, cs, write: bool):
    with tempfile.TemporaryDirectory(prefix="wo_golden_wind_") as td:
        work = Path(td)
        ref_js = prepare_reference(ref, work)
        put = lambda name, a, ty: (np.ascontiguousarray(a, ty).tofile(work / name), str(work / name))[1]  # noqa: E731
        job = dict(cases=[], meta=str(work / "meta.json"))
        for c in cs:
            k = c["name"]
            job["cases"].append(dict(name=k, numRegions=int(len(c["off"]) - 1), adjOffset=put(f"{k}_off.bin", c["off"], np.int32),
                                     adjList=put(f"{k}_adj.bin", c["adj"], np.int32), xyz=put(f"{k}_xyz.bin", c["xyz"], np.float32),
                                     elevation=put(f"{k}_e.bin", c["e"], np.float32), r_plate=put(f"{k}_plate.bin", c["plate"], np.int32),
                                     plateIsOcean=put(f"{k}_ocean.bin", c["ocean"], np.int32), seed=c["seed"], axialTilt=23.5, out=str(work / f"{k}_o_")))
        (work / "job.json").write_text(json.dumps(job))
        subprocess.run(["node", "--harmony-optional-chaining", "--harmony-nullish", "--max-old-space-size=6000", str(HARNESS), str(ref_js),
                        str(work / "job.json")], check=True)
        meta = json.loads((work / "meta.json").read_text())
        for c in cs:
            k = c["name"]
            cm = meta["cases"][k]
            print(f"{k}: reference computeWind {cm['ms']:.1f} ms; " + ", ".join(f"{s}: {ms:.1f}" for s, ms in cm["stages"]))
            if not write:
                continue
            data = {}
            info = dict(exports=meta["exports"], keys=cm["keys"], arrays=cm["arrays"], seed=c["seed"], axialTilt=23.5, numRegions=int(len(c["off"]) - 1),
                        ref_ms=cm["ms"], stride=STRIDE if c["sparse"] else 1, crc={}, **c.get("extra", {}))
            for name, ty in cm["arrays"].items():
                a = np.fromfile(work / f"{k}_o_{name}.bin", TYPES[ty])
                info["crc"][name] = crc(a)
                full = not c["sparse"] or name == "r_coastDistLand" or name.startswith("itcz")
                data[f"ref_{name}"] = a if full else a[::STRIDE].copy()
            for s in c["store"]:
                data[f"in_{s}"] = np.ascontiguousarray(c[s])
            data["meta_json"] = np.frombuffer(json.dumps(info).encode(), np.uint8)
            f = GOLD / f"{k}.npz"
            np.savez_compressed(f, **data)
            print(f"wrote {f.relative_to(REPO)} ({f.stat().st_size / 1024:.0f} KiB)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    ap.add_argument("--only", default=None)
    ap.add_argument("--time-cells", type=int, default=0)
    args = ap.parse_args()
    if args.time_cells:
        run(Path(args.ref), [timing_case(args.time_cells)], write=False)
        return
    cs = [c for c in cases(args.only) if args.only in (None, c["name"])]
    run(Path(args.ref), cs, write=True)


if __name__ == "__main__":
    main()
