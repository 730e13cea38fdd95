#!/usr/bin/env python3
"""Generate tests/golden/points_large.npz, math_v8_trig_large.npz and math_v8_trig_large_cos.npz by running the REFERENCE's
generateFibonacciSphere(N, jitter, makeRng(seed)) (js/sphere-mesh.js:9-37) and Node's Math.sin / Math.cos under Node in this container.

The reference sources are copied to a scratch directory (oracle/ref_harness/make_golden.py: prepare_reference); they never enter
this repository.  run_points.mjs imports the scratch copy's sphere-mesh.js and rng.js unchanged.

points_large.npz, per case: the CRC32 of the whole Float32Array (3 N floats, no pole), the first 2 000 points, the last 2 000 and
every 997th point.

The sine / cosine arguments are three sets: "lonr", the lonR of every 400th point of a jittered 40 M-cell sphere, which the host
emulator of csrc/points_ops.h (tests/emu_points) forms and the test forms again (the fixture keeps their CRC32, not the 100 000
doubles); "rand", seeded random doubles up to 2^27 in both signs; "edge", the doubles just below and just above the high word
0x413921fb where the large-argument reduction takes over.  Node's results are stored in full; the cosines of the lonr set live in a
file of their own so that no file passes the repository's size limit.

Usage:  python tools/ref_harness/make_golden_points.py --ref <root of the reference project>
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import subprocess
import sys
import tempfile
import zlib
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(REPO))
from oracle.ref_harness.make_golden import prepare_reference  # noqa: E402

GOLD = REPO / "tests" / "golden"
HARNESS = Path(__file__).resolve().parent / "run_points.mjs"
EMU_DIR = REPO / "tests" / "emu_points"
CASES = (("N700000_j75_s1", 700000, 0.75, 1), ("N1000000_j75_s1", 1000000, 0.75, 1), ("N1000000_j0_s3", 1000000, 0.0, 3))
LONR = dict(N=40000000, jitter=0.75, seed=1, stride=400)
HEAD, TAIL, EVERY = 2000, 2000, 997


def lonr_args() -> np.ndarray:
    subprocess.run(["make", "-s", "-C", str(EMU_DIR)], check=True)
    emu = C.CDLL(str(EMU_DIR / "_build" / "libemu_points.so"))
    emu.emu_lonr_samples.restype = C.c_int64
    out = np.empty((LONR["N"] + LONR["stride"] - 1) // LONR["stride"], np.float64)
    n = emu.emu_lonr_samples(C.c_int32(LONR["N"]), C.c_double(LONR["jitter"]), C.c_double(LONR["seed"]), C.c_int32(LONR["stride"]),
                             out.ctypes.data_as(C.c_void_p))
    assert n == out.size
    return out


def rand_args() -> np.ndarray:
    rng = np.random.default_rng(41413)
    mag = np.concatenate([rng.uniform(0, 2.0 ** 27, 5000), 2.0 ** rng.uniform(20, 27, 3000)])
    return mag * np.where(rng.random(mag.size) < 0.5, -1.0, 1.0)


def edge_args() -> np.ndarray:
    """300 doubles on either side of the boundary, in both signs: high word <= 0x413921fb is the medium path, above it the large one"""
    first_large = np.array([0x413921fc << 32], np.uint64).view(np.float64)[0]
    below, above = [], [first_large]
    v = first_large
    for _ in range(300):
        v = np.nextafter(v, 0.0)
        below.append(v)
    for _ in range(299):
        above.append(np.nextafter(above[-1], np.inf))
    a = np.array(below + above, np.float64)
    return np.concatenate([a, -a])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="root of the reference project (its js/ is copied to a scratch directory)")
    args = ap.parse_args()
    sets = dict(lonr=lonr_args(), rand=rand_args(), edge=edge_args())
    with tempfile.TemporaryDirectory(prefix="wo_golden_pts_") as td:
        work = Path(td)
        ref_js = prepare_reference(Path(args.ref), work)
        job = dict(cases=[dict(name=n, N=N, jitter=j, seed=s, out=str(work / f"{n}.bin")) for n, N, j, s in CASES], crcOut=str(work / "crc.json"), math=[])
        for k, x in sets.items():
            np.ascontiguousarray(x).tofile(work / f"x_{k}.bin")
            job["math"].append(dict(x=str(work / f"x_{k}.bin"), sin=str(work / f"sin_{k}.bin"), cos=str(work / f"cos_{k}.bin")))
        (work / "job.json").write_text(json.dumps(job))
        subprocess.run(["node", "--max-old-space-size=6000", str(HARNESS), str(ref_js), str(work / "job.json")], check=True)
        crcs = json.loads((work / "crc.json").read_text())
        pts = {}
        for n, N, j, s in CASES:
            xyz = np.fromfile(work / f"{n}.bin", np.float32)
            assert xyz.size == 3 * N and zlib.crc32(xyz.tobytes()) == crcs[n]
            p = xyz.reshape(-1, 3)
            pts[f"{n}_crc"] = np.array([crcs[n]], np.uint32)
            pts[f"{n}_head"], pts[f"{n}_tail"], pts[f"{n}_every"] = p[:HEAD].copy(), p[-TAIL:].copy(), p[::EVERY].copy()
        pts["meta_json"] = np.frombuffer(json.dumps(dict(cases=[dict(name=n, N=N, jitter=j, seed=s) for n, N, j, s in CASES], head=HEAD, tail=TAIL,
                                                         every=EVERY)).encode(), np.uint8)
        res = {k: (np.fromfile(work / f"sin_{k}.bin", np.float64), np.fromfile(work / f"cos_{k}.bin", np.float64)) for k in sets}
    math = dict(rand_x=sets["rand"], rand_sin=res["rand"][0], rand_cos=res["rand"][1], edge_x=sets["edge"], edge_sin=res["edge"][0],
                edge_cos=res["edge"][1], lonr_sin=res["lonr"][0], lonr_x_crc=np.array([zlib.crc32(sets["lonr"].tobytes())], np.uint32),
                meta_json=np.frombuffer(json.dumps(dict(lonr=LONR)).encode(), np.uint8))
    np.savez_compressed(GOLD / "points_large.npz", **pts)
    np.savez_compressed(GOLD / "math_v8_trig_large.npz", **math)
    np.savez_compressed(GOLD / "math_v8_trig_large_cos.npz", lonr_cos=res["lonr"][1])
    for f in ("points_large.npz", "math_v8_trig_large.npz", "math_v8_trig_large_cos.npz"):
        print(f"wrote tests/golden/{f} ({(GOLD / f).stat().st_size / 1024:.0f} KiB)")


if __name__ == "__main__":
    main()
