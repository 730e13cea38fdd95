"""computeOceanCurrents on the device at N cells, for DESIGN section 8.3: wall time of the call (best of the calls after the first on
one planet), what the stage found, and the same with the masked smoothing done field by field (WO_TEST_HOOKS=ocean_split_smooth,
the A/B of the interleaved smoothing kernel).  Run it under `rocprofv3 --kernel-trace --stats -- python profiles/ocean_probe.py N`
for the per-kernel times.  The planet is tests/wind_common.py: synthetic_case(N), the one
`tools/ref_harness/make_golden_ocean.py --time-cells N` times the reference on; at 10 M cells and above its terrain is made on the
device (the same field bit for bit).

Usage:  python profiles/ocean_probe.py N [--check] [--split | --no-ab] [--calls K]
  --check   also compare with the host emulator, bit for bit
  --split   every call with the field-by-field smoothing (for a trace of its own)
  --no-ab   the default route only (for a trace of its own); without either flag the A/B is K more calls
"""
import json
import os
import sys
import time
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))
sys.path.insert(0, str(REPO / "tests"))


def main():
    import wind_common as WC
    from planet_heightmap_generation_amd import ocean as OD, sphere_mesh as S, terrain_post as TP, wind as WD
    N = int(sys.argv[1])
    calls = int(sys.argv[sys.argv.index("--calls") + 1]) if "--calls" in sys.argv else 3
    e = None
    if N >= 10_000_000:
        mesh, xyz, nd = S.build_sphere(N, 0.75, 1)
        pl = TP.Planet(mesh, xyz, nd)
        pl.synthetic_terrain(3)
        e = pl.download()
        pl.close()
    case = WC.synthetic_case(N, 3, e=e)
    pl = TP.Planet(WC.Mesh(case["off"], case["adj"]), case["xyz"])
    wind = WD.compute_wind(pl, None, case["e"], case["ocean"], case["plate"], case["seed"], fields=OD.WIND_INPUTS if "--check" in sys.argv else ())

    def timed(k):
        ms = []
        for _ in range(k):
            t0 = time.perf_counter()
            OD.compute_ocean_currents(pl, None, None, fields=())
            ms.append((time.perf_counter() - t0) * 1e3)
        return ms

    if "--split" in sys.argv:
        os.environ["WO_TEST_HOOKS"] = "ocean_split_smooth"
    ms = timed(calls)
    info = OD.info(pl)
    levels = info["warmthRange"] - 1
    out = dict(cells=pl.numRegions, ocean_fraction=float((case["e"] <= 0).mean()), split_smooth="--split" in sys.argv, wall_ms_first=ms[0], wall_ms=min(ms[1:]) if len(ms) > 1 else ms[0],
               info=info, bfs_levels=levels, kernel_launches=2 + levels + 1 + info["currentSmoothPasses"] + 1 + 6 + 1 + info["warmthSmoothPasses"] + 1)
    got = {k: OD.download(pl, k) for k, _ in OD.RESULT_FIELDS}
    if "--split" not in sys.argv and "--no-ab" not in sys.argv:
        os.environ["WO_TEST_HOOKS"] = "ocean_split_smooth"
        ms = timed(calls)
        out["wall_ms_split_smooth"] = min(ms[1:]) if len(ms) > 1 else ms[0]
        out["split_smooth_same_bits"] = all(np.array_equal(OD.download(pl, k).view(np.uint32), got[k].view(np.uint32)) for k, _ in OD.RESULT_FIELDS)
        os.environ.pop("WO_TEST_HOOKS")
    pl.close()
    if "--check" in sys.argv:
        import ocean_common as OC
        OC.assert_equal(f"device vs emulator, {N} cells", got, OC.emulate(case, wind))
        out["checked_against_emulator"] = True
    print(json.dumps(out))


if __name__ == "__main__":
    main()
