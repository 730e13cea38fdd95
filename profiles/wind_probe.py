"""computeWind on the device at N cells, for DESIGN section 8.2: wall time of the call (second of two calls on one planet), the BFS
level counts and the kernel launch count of the stage.  Run it under `rocprofv3 --kernel-trace --stats -- python
profiles/wind_probe.py N` for the per-kernel times.  The planet is tests/wind_common.py: synthetic_case(N), the one
`tools/ref_harness/make_golden_wind.py --time-cells N` times the reference on.

Usage:  python profiles/wind_probe.py N [--check]      (--check: also compare with the host emulator on the bar of the tests)
"""
import json
import sys
import time
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))
sys.path.insert(0, str(REPO / "tests"))


def main():
    import wind_common as WC
    from planet_heightmap_generation_amd import capi, terrain_post as TP, wind as WD
    N = int(sys.argv[1])
    case = WC.synthetic_case(N)
    pl = TP.Planet(WC.Mesh(case["off"], case["adj"]), case["xyz"])
    e, plate, ids = case["e"], case["plate"], case["ocean"]
    L = capi.lib()
    ms, levels = [], np.zeros(2, np.int32)
    for _ in range(3):
        t0 = time.perf_counter()
        capi.check(L.wo_compute_wind(pl.handle, pl.numRegions, capi.ptr(e), capi.ptr(plate), capi.ptr(ids), int(ids.size), float(case["seed"]), 23.5, capi.ptr(levels)), "computeWind")
        ms.append((time.perf_counter() - t0) * 1e3)
    out = dict(cells=pl.numRegions, land_fraction=float((e > 0).mean()), wall_ms_first=ms[0], wall_ms=min(ms[1:]), bfs_levels=[int(levels[0]), int(levels[1])])
    t0 = time.perf_counter()
    got = {k: WD.download(pl, k) for k, _ in WD.RESULT_FIELDS}
    out["download_all_fields_ms"] = (time.perf_counter() - t0) * 1e3
    pl.close()
    if "--check" in sys.argv:
        WC.compare(f"device vs emulator, {N} cells", got, WC.emulate(case), case["N"])
        out["checked_against_emulator"] = True
    print(json.dumps(out))


if __name__ == "__main__":
    main()
