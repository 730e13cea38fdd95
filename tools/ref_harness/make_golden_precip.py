#!/usr/bin/env python3
"""Generate tests/golden/precip_*.npz by running the REFERENCE's unmodified computeWind, computeOceanCurrents and then
computePrecipitation (js/precipitation.js:196-684) under Node 12.

The reference sources are copied to a scratch directory (oracle/ref_harness/make_golden.py: prepare_reference); they never
enter this repository and no reference file is patched.  A fixture holds arrays and logged numbers only: the four outputs
(ref_*), in meta_json the reference's _precipTiming, the module's export names, the result keys, the scalars of the call by the
reference's formulas under V8 (sc_f64: depletionBase, shadowDecay, windwardDecay), and the CRC32 of every wind and ocean input
the stage read.  The inputs themselves are not stored twice: wind_<planet>.npz holds the wind result and ocean_<planet>.npz the
two warmths of the same planet; tests/precip_common.py takes them from there and checks the CRCs.

Cases (planet = the wind / ocean fixture pair of the same suffix):
  precip_config1_N10000_s1, precip_import_N10000_s1     defaults (offset 0, coverage 0.3)
  precip_config1_N10000_s1_wet    the planet of config1 with precipitationOffset 0.6, landCoverage 0.7 (the > 0.4 branch)
  precip_N2000_ocean_s1           no land: empty neighbour lists, ocean base only
  precip_N2000_land_s1            no ocean: coast distance -1 everywhere, all-zero advection seeds
  precip_N2000_edges_s1, precip_N{63,255,256,4096}_shape_s1
  precip_N250000_s4               sparse like its wind and ocean siblings: every 16th cell plus whole-array CRCs
and precip_pow_v8.npz: V8's Math.pow(0.15, 1/h), Math.pow(0.25, 1/h) for h = 1 .. 1024 and Math.pow(0.78, 1/h) for h = 1 .. 200.

Usage:  python tools/ref_harness/make_golden_precip.py [--ref /root/reference] [--only NAME] [--time-cells N]
  --time-cells N   no fixture is written: the reference's wall time of computePrecipitation on the N-cell planet of
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
HARNESS = Path(__file__).resolve().parent / "run_precip.mjs"
STRIDE = MW.STRIDE
TYPES = MW.TYPES
crc = MW.crc
POW_TABLES = ((0.15, 1024), (0.25, 1024), (0.78, 200))
ORDER = ["precip_config1_N10000_s1", "precip_import_N10000_s1", "precip_config1_N10000_s1_wet", "precip_N2000_ocean_s1", "precip_N2000_land_s1",
         "precip_N2000_edges_s1"] + [f"precip_N{n}_shape_s1" for n in MW.SHAPE_SIZES] + ["precip_N250000_s4"]


def cases(only=None):
    out = []
    for c in MW.cases(None):
        planet = c["name"][len("wind_"):]
        out.append(dict(c, name="precip_" + planet, planet=planet, args=None))
        if planet == "config1_N10000_s1":
            out.append(dict(c, name="precip_config1_N10000_s1_wet", planet=planet, args=(0.6, 0.7)))
    out = [c for c in out if only in (None, c["name"])]
    return sorted(out, key=lambda c: ORDER.index(c["name"]))


def timing_case(n_cells: int):
    return dict(MW.timing_case(n_cells), planet=None, args=None)


def run(ref: Path, cs, write: bool, pow_tables: bool):
    with tempfile.TemporaryDirectory(prefix="wo_golden_precip_") as td:
        work = Path(td)
        ref_js = prepare_reference(ref, work)
        put = lambda name, a, ty: (np.ascontiguousarray(a, ty).tofile(work / name), str(work / name))[1]  # noqa: E731
        job = dict(cases=[], meta=str(work / "meta.json"))
        if pow_tables:
            job["pow"] = [[b, n, str(work / f"pow_{i}.bin")] for i, (b, n) in enumerate(POW_TABLES)]
        for c in cs:
            k = c["name"]
            j = dict(name=k, numRegions=int(len(c["off"]) - 1), adjOffset=put(f"{k}_off.bin", c["off"], np.int32),
                     adjList=put(f"{k}_adj.bin", c["adj"], np.int32), xyz=put(f"{k}_xyz.bin", c["xyz"], np.float32),
                     elevation=put(f"{k}_e.bin", c["e"], np.float32), r_plate=put(f"{k}_plate.bin", c["plate"], np.int32),
                     plateIsOcean=put(f"{k}_ocean.bin", c["ocean"], np.int32), seed=c["seed"], axialTilt=23.5, out=str(work / f"{k}_o_"))
            if c["args"] is not None:
                j["precipitationOffset"], j["landCoverage"] = c["args"]
            job["cases"].append(j)
        (work / "job.json").write_text(json.dumps(job))
        subprocess.run(["node", "--harmony-optional-chaining", "--harmony-nullish", "--max-old-space-size=6000", str(HARNESS), str(ref_js),
                        str(work / "job.json")], check=True, stdout=subprocess.DEVNULL)      # the reference logs on module load
        meta = json.loads((work / "meta.json").read_text())
        if pow_tables:
            data = {f"pow_{str(b).replace('.', '_')}": np.fromfile(work / f"pow_{i}.bin", np.float64) for i, (b, n) in enumerate(POW_TABLES)}
            np.savez_compressed(GOLD / "precip_pow_v8.npz", **data)
            print(f"wrote tests/golden/precip_pow_v8.npz ({(GOLD / 'precip_pow_v8.npz').stat().st_size / 1024:.0f} KiB)")
        for c in cs:
            k = c["name"]
            cm = meta["cases"][k]
            print(f"{k}: reference computePrecipitation {cm['ms']:.1f} ms; " + ", ".join(f"{s}: {ms:.1f}" for s, ms in cm["stages"]))
            print(f"    scalars {cm['scalars']}")
            if not write:
                continue
            sparse = c["sparse"]
            data = {}
            info = dict(exports=meta["exports"], keys=cm["keys"], arrays=cm["arrays"], inputs=cm["inputs"], planet=c["planet"], seed=c["seed"],
                        numRegions=int(len(c["off"]) - 1), ref_ms=cm["ms"], log=cm["log"], timing=cm["stages"], scalars=cm["scalars"],
                        precipitationOffset=0 if c["args"] is None else c["args"][0], landCoverage=0.3 if c["args"] is None else c["args"][1],
                        stride=STRIDE if sparse else 1, crc={}, crc_inputs={})
            for name, ty in cm["arrays"].items():
                a = np.fromfile(work / f"{k}_o_{name}.bin", TYPES[ty])
                info["crc"][name] = crc(a)
                data[f"ref_{name}"] = a[::STRIDE].copy() if sparse else a
            for name, ty in cm["inputs"].items():
                info["crc_inputs"][name] = crc(np.fromfile(work / f"{k}_o_in_{name}.bin", TYPES[ty]))
            data["sc_f64"] = np.fromfile(work / f"{k}_o_scalars_f64.bin", np.float64)
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
        run(Path(args.ref), [timing_case(args.time_cells)], write=False, pow_tables=False)
        return
    run(Path(args.ref), cases(args.only), write=True, pow_tables=args.only is None)


if __name__ == "__main__":
    main()
