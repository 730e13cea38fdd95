#!/usr/bin/env python3
"""Generate tests/golden/ocean_*.npz by running the REFERENCE's unmodified computeWind (js/wind.js) and then its unmodified
computeOceanCurrents (js/ocean.js:204-382) under Node 12.

The reference sources are copied to a scratch directory (oracle/ref_harness/make_golden.py: prepare_reference); they never
enter this repository and no reference file is patched.  A fixture holds arrays and logged numbers only: the eight outputs
(ref_*), the nine wind outputs the stage reads (win_*: r_lat r_lon r_isLand r_eastX r_eastY r_eastZ itczLons itczLatsSummer
itczLatsWinter, so that the stage can be checked without a wind of our own), and in meta_json the two lines the reference logs
during the call (the circumpolar flags; coastThreshold, warmthRange, p95 and oceanCells of each season).

Cases (the planet of a wind fixture is not stored twice; `planet` in the metadata names it):
  ocean_config1_N10000_s1   planet of wind_config1_N10000_s1
  ocean_import_N10000_s1    planet of wind_import_N10000_s1
  ocean_N2000_ocean_s1      planet of wind_N2000_ocean_s1: no coast at all
  ocean_N2000_land_s1       planet of wind_N2000_land_s1: no ocean cell, the percentile's empty-array branch
  ocean_N10000_wedge_s1     mesh_N10000_s1, every cell at -0.5 except a land wedge at +0.25 where -72 deg < lat < -48 deg and
                            0 deg < lon < 25 deg (74 cells); one plate, oceanic.  The circumpolar flags differ per hemisphere.
  ocean_N2000_edges_s1      planet of wind_N2000_edges_s1: cells at both poles, on the date line and at lon = +-pi/2
  ocean_N{63,255,256,4096}_shape_s1   planets of wind_N{...}_shape_s1: 64, 256, 257 and 4 097 cells
  ocean_N250000_s4          planet of wind_N250000_s4, the only one with coastThreshold 18; stored sparse as that fixture is:
                            every 16th cell plus the CRC32 of each whole array (the ITCZ arrays in full; the per-cell wind
                            inputs as CRC32 only: wind_N250000_s4 holds their samples)

Usage:  python tools/ref_harness/make_golden_ocean.py [--ref /root/reference] [--only NAME] [--time-cells N]
  --time-cells N   no fixture is written: the reference's wall time of computeOceanCurrents on the N-cell planet of
                   tests/wind_common.py: synthetic_case is printed
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
sys.path.insert(0, str(REPO / "tests"))
sys.path.insert(0, str(Path(__file__).resolve().parent))
from oracle.ref_harness.make_golden import prepare_reference  # noqa: E402
import make_golden_wind as MW  # noqa: E402

GOLD = REPO / "tests" / "golden"
HARNESS = Path(__file__).resolve().parent / "run_ocean.mjs"
STRIDE = MW.STRIDE
TYPES = MW.TYPES
crc = MW.crc


def wedge_case():
    m = np.load(GOLD / "mesh_N10000_s1.npz")
    xyz = np.asarray(m["xyz"], np.float32).reshape(-1, 3).astype(np.float64)
    lat = np.degrees(np.arcsin(np.clip(xyz[:, 1], -1, 1)))
    lon = np.degrees(np.arctan2(xyz[:, 0], xyz[:, 2]))
    land = (lat > -72) & (lat < -48) & (lon > 0) & (lon < 25)
    assert int(land.sum()) == 74, int(land.sum())
    n = land.size
    return dict(name="ocean_N10000_wedge_s1", planet=None, off=m["ref_adjOffset"], adj=m["ref_adjList"], xyz=m["xyz"],
                e=np.where(land, 0.25, -0.5).astype(np.float32), plate=np.zeros(n, np.int32), ocean=np.array([0], np.int32), seed=1,
                store=("e", "plate", "ocean"), sparse=False)


def cases(only=None):
    out = []
    want = lambda name: only in (None, name)  # noqa: E731
    wind = {c["name"]: c for c in MW.cases(None if only is None else "wind_" + only[len("ocean_"):])} if only != "ocean_N10000_wedge_s1" else {}
    for k, c in wind.items():
        name = "ocean_" + k[len("wind_"):]
        if want(name):
            out.append(dict(c, name=name, planet=k, store=()))
    if want("ocean_N10000_wedge_s1"):
        out.append(wedge_case())
    order = ["ocean_config1_N10000_s1", "ocean_import_N10000_s1", "ocean_N2000_ocean_s1", "ocean_N2000_land_s1", "ocean_N10000_wedge_s1", "ocean_N250000_s4",
             "ocean_N2000_edges_s1"] + [f"ocean_N{n}_shape_s1" for n in MW.SHAPE_SIZES]
    return sorted(out, key=lambda c: order.index(c["name"]))


def timing_case(n_cells: int):
    return dict(MW.timing_case(n_cells), planet=None)


def run(ref: Path, cs, write: bool):
    with tempfile.TemporaryDirectory(prefix="wo_golden_ocean_") as td:
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
                        str(work / "job.json")], check=True, stdout=subprocess.DEVNULL)      # the reference logs on module load
        meta = json.loads((work / "meta.json").read_text())
        for c in cs:
            k = c["name"]
            cm = meta["cases"][k]
            print(f"{k}: reference computeOceanCurrents {cm['ms']:.1f} ms; " + ", ".join(f"{s}: {ms:.1f}" for s, ms in cm["stages"]))
            for line in cm["log"]:
                print(f"    {line}")
            if not write:
                continue
            data = {}
            info = dict(exports=meta["exports"], keys=cm["keys"], arrays=cm["arrays"], inputs=cm["inputs"], planet=c["planet"], seed=c["seed"],
                        numRegions=int(len(c["off"]) - 1), ref_ms=cm["ms"], log=cm["log"], stride=STRIDE if c["sparse"] else 1, crc={}, crc_inputs={})
            for name, ty in cm["arrays"].items():
                a = np.fromfile(work / f"{k}_o_{name}.bin", TYPES[ty])
                info["crc"][name] = crc(a)
                data[f"ref_{name}"] = a[::STRIDE].copy() if c["sparse"] else a
            for name, ty in cm["inputs"].items():
                a = np.fromfile(work / f"{k}_o_in_{name}.bin", TYPES[ty])
                info["crc_inputs"][name] = crc(a)
                if not c["sparse"] or name.startswith("itcz"):
                    data[f"win_{name}"] = a
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
    run(Path(args.ref), cases(args.only), write=True)


if __name__ == "__main__":
    main()
