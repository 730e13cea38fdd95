#!/usr/bin/env python3
"""Wall time of the REFERENCE's buildSuperPlates (js/super-plates.js under Node, run by run_super_plates.mjs from a scratch copy of
that one file) on tests/elev_inputs.py: realistic_case(N) — the 80 plates of plates_N10000_s1_P80 projected onto an N-cell mesh and
smoothed, the planet `profiles/super_plates_probe.py` times the device on.  Prints every repetition and the median.  The figure is
the figure of the CPU it runs on; DESIGN section 8.7 quotes it as such.

Usage: python tests/golden_gen/time_reference_super_plates.py --ref <reference checkout> [N ...] [--reps K]     (default: 1000000 10000000, 5)
"""
from __future__ import annotations

import argparse
import json
import shutil
import subprocess
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(REPO))
sys.path.insert(0, str(REPO / "tests"))
HARNESS = Path(__file__).resolve().parent / "run_super_plates.mjs"


def main():
    import elev_inputs as EI
    import super_plates_common as SP
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("sizes", nargs="*", type=int, default=[1_000_000, 10_000_000])
    args = ap.parse_args()
    with tempfile.TemporaryDirectory(prefix="wo_super_time_") as td:
        work = Path(td)
        (work / "ref").mkdir()
        shutil.copy(Path(args.ref) / "js" / "super-plates.js", work / "ref" / "super-plates.js")
        (work / "ref" / "package.json").write_text('{"type":"module"}')
        for N in args.sizes:
            t = time.time()
            c = SP.from_elev_case(EI.realistic_case(N))
            print(f"N={N}: case built in {time.time() - t:.1f} s", flush=True)
            pre = str(work / f"N{N}_")
            files = dict(r_plate=c.r_plate, plateSeeds=c.seeds, plateVec=c.vec4, hasVec=c.hasVec, plateIsOcean=c.isoc, plateDensity=c.dens)
            c.off.tofile(pre + "off.bin"); c.adj.tofile(pre + "adj.bin")
            for k, a in files.items():
                np.ascontiguousarray(a).tofile(pre + k + ".bin")
            job = dict(adjOffset=pre + "off.bin", adjList=pre + "adj.bin", timing=pre + "timing.json",
                       cases=[dict(name=f"N{N}", reps=args.reps, **{k: pre + k + ".bin" for k in files})])
            Path(pre + "job.json").write_text(json.dumps(job))
            subprocess.run(["node", "--max-old-space-size=12000", str(HARNESS), str(work / "ref"), pre + "job.json"], check=True)
            ms = json.loads(Path(pre + "timing.json").read_text())[f"N{N}"]
            print(f"N={N}: reference buildSuperPlates, ms per call {[round(x, 1) for x in ms]}, median {float(np.median(ms)):.1f}", flush=True)


if __name__ == "__main__":
    main()
