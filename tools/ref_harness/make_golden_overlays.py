#!/usr/bin/env python3
"""Generate tests/golden/overlays_N2000_s1.npz and tests/golden/overlays_crafted.npz by running the REFERENCE's own buildWindArrows,
buildOceanCurrentArrows (with the ITCZ line they draw on the pressure views) and rebuildGrids (js/planet-mesh.js:1289-1749,
:385-503) under Node 12.

As in make_golden_globe.py the reference's sources are copied to a scratch directory and never enter this repository; in the scratch
copy only, stubs of our own stand in for three and scene.js, and the line `const globePositions = [];` of the two builders gains
`globalThis.__gridRegions = gridRegions;` in front of it, so that the winners of the bins can be read out.  Nothing is drawn: the
goldens hold the arrays the builders hand to the renderer.

overlays_N2000_s1.npz, on tests/golden/mesh_N2000_s1.npz with map_N2000_s1.npz's elevation:
  * smooth synthetic wind and current fields; at winners of the bins: speeds just below, at and just above each threshold (0.001,
    0.01), a NaN speed, a zero vector (with a non-zero `speed` in the ocean form, which reaches `rawSpeed || 1`), warmth at +-0.1 as
    f32, just inside them and NaN, a wind fast enough for the ramp's upper half and its clamp;
  * wind_*: buildWindArrows('summer') at mapCenterLon 0 with its gridRegions, its four arrays and the ITCZ line in both forms;
    wind_c_map_position: the map positions of the same call at mapCenterLon 2.5;
  * ocean_*: buildOceanCurrentArrows('winter') at mapCenterLon 2.5 with its gridRegions and its four arrays;
  * grid30_*, grid22_*: rebuildGrids at 30 degrees (centre 0) and at 22.5 degrees (centre 2.5).
overlays_crafted.npz: one position per region of that mesh (2001) and the gridRegions the loop leaves for them.  The bulk lies in three bins; in the first the
  closest position is one whose d2 rounds up when it is stored, in the second one whose d2 rounds down, in the third one of either
  kind, each of them present several times at scattered indices, among further groups of identical positions of both kinds.  Then the
  poles (0, +-1, 0) and (-0, +-1, +-0), (+-0, 0, -1) on the antimeridian, a NaN y, a NaN x and y = 1.0000001f, which land in bins of
  their own.  The generator asserts that both rounding kinds decide a bin and prints how many groups of each kind there are.
Running this again reproduces every array exactly.

Usage:  python tools/ref_harness/make_golden_overlays.py --ref <checkout of the reference>
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
sys.path.insert(0, str(Path(__file__).resolve().parent))
from oracle.ref_harness.make_golden import prepare_reference  # noqa: E402
from make_golden_globe import THREE_GLOBE  # noqa: E402
from make_golden_map_layers import SCENE_STUB  # noqa: E402

GOLD = REPO / "tests" / "golden"
HARNESS = Path(__file__).resolve().parent / "run_overlays.mjs"
N, SEED = 2000, 1
BINS = 7200
f32 = np.float32
MARK = "const globePositions = [];"


class Reference:
    """the scratch copy and a way to run a job in it"""

    def __init__(self, ref: Path, work: Path):
        self.work = work
        self.js = prepare_reference(ref, work)
        three = self.js.parent / "node_modules" / "three"
        three.mkdir(parents=True)
        (three / "package.json").write_text('{"name":"three","type":"module","main":"three.js","exports":"./three.js"}')
        (three / "three.js").write_text(THREE_GLOBE)
        (self.js / "scene.js").write_text(SCENE_STUB)
        pm = self.js / "planet-mesh.js"
        text = pm.read_text()
        assert text.count(MARK) == 2, "the two arrow builders no longer start their output with this line"
        pm.write_text(text.replace(MARK, "globalThis.__gridRegions = gridRegions; " + MARK))
        self.runs = 0

    def run(self, arrays: dict, fields: dict, **job) -> "Result":
        self.runs += 1
        d = self.work / f"run{self.runs}"
        d.mkdir()
        put = lambda name, a: (np.ascontiguousarray(a).tofile(d / name), str(d / name))[1]  # noqa: E731
        job = dict(job, out=str(d / "o_"), fields={k: put(k + ".bin", np.ascontiguousarray(v, f32)) for k, v in fields.items()},
                   **{k: put(k + ".bin", np.ascontiguousarray(v, f32)) for k, v in arrays.items()})
        (d / "job.json").write_text(json.dumps(job))
        subprocess.run(["node", "--harmony-optional-chaining", "--harmony-nullish", str(HARNESS), str(self.js), str(d / "job.json")], check=True)
        return Result(d)


class Result:
    def __init__(self, d: Path):
        self.d = d
        self.meta = json.loads((d / "o_meta.json").read_text())

    def __call__(self, name, ty=np.float32):
        return np.fromfile(self.d / f"o_{name}.bin", ty)


# ---- case 1: the golden mesh with synthetic fields -----------------------------------------------------------------------------------
def smooth_fields(xyz: np.ndarray) -> dict:
    p = np.asarray(xyz, np.float64).reshape(-1, 3)
    lat, lon = np.arcsin(np.clip(p[:, 1], -1, 1)), np.arctan2(p[:, 0], p[:, 2])
    F = {}
    for s, ph in (("summer", 0.0), ("winter", 0.7)):
        F[f"r_wind_east_{s}"] = 0.12 * np.cos(3 * lat + ph) + 0.03 * np.sin(2 * lon)
        F[f"r_wind_north_{s}"] = 0.05 * np.sin(2 * lat) * np.cos(lon + ph)
        F[f"r_ocean_current_east_{s}"] = 0.4 * np.sin(2 * lat + ph) * np.cos(lon)
        F[f"r_ocean_current_north_{s}"] = 0.3 * np.cos(lat) * np.sin(2 * lon + ph)
        F[f"r_ocean_speed_{s}"] = np.abs(0.5 * np.cos(2 * lat) * np.sin(lon + ph))
        F[f"r_ocean_warmth_{s}"] = 0.4 * np.sin(lat * 2) * np.cos(lon - ph)
    return {k: v.astype(f32) for k, v in F.items()}


def around(v: float) -> list:
    x = f32(v)
    return [np.nextafter(x, f32(-np.inf)), x, np.nextafter(x, f32(np.inf))]


def plant_specials(F: dict, wind_winners: np.ndarray, ocean_winners: np.ndarray) -> dict:
    """edge values at regions that win a bin (so that they reach the arrow loop); -> what was planted where"""
    w = [int(r) for r in wind_winners[wind_winners >= 0][5::37][:12]]
    E, Nn = F["r_wind_east_summer"], F["r_wind_north_summer"]
    speeds = around(0.001) + [f32(0.00099), f32(0.00101)]
    for r, v in zip(w[:5], speeds):
        E[r], Nn[r] = v, 0.0
    E[w[5]], Nn[w[5]] = np.nan, 0.01                          # a NaN speed is kept
    E[w[6]], Nn[w[6]] = 0.0, -0.0                             # speed 0: dropped
    E[w[7]], Nn[w[7]] = 0.3, 0.4                              # t clamps to 1
    E[w[8]], Nn[w[8]] = 0.2, 0.0                              # the ramp's upper half
    E[w[9]], Nn[w[9]] = 0.0, 1 / 6                            # t at 0.5 or beside it
    E[w[10]], Nn[w[10]] = np.inf, 0.0
    o = [int(r) for r in ocean_winners[ocean_winners >= 0][3::29][:16]]
    S, Wm = F["r_ocean_speed_winter"], F["r_ocean_warmth_winter"]
    CE, CN = F["r_ocean_current_east_winter"], F["r_ocean_current_north_winter"]
    for r, v in zip(o[:5], around(0.01) + [f32(0.0099), f32(0.0101)]):
        S[r] = v
    S[o[5]] = np.nan                                          # a NaN speed is kept
    S[o[6]], CE[o[6]], CN[o[6]] = 0.5, 0.0, -0.0              # a zero vector with a speed: rawSpeed || 1
    S[o[7]], CE[o[7]], CN[o[7]] = 0.5, np.nan, 0.1
    for r, v in zip(o[8:14], around(0.1) + around(-0.1)):
        S[r], Wm[r] = 0.3, v
    S[o[14]], Wm[o[14]] = 0.3, np.nan
    S[o[15]] = 0.0
    return dict(wind=w, ocean=o)


def case_mesh(R: Reference) -> dict:
    gm = np.load(GOLD / f"mesh_N{N}_s{SEED}.npz")
    e = np.ascontiguousarray(np.load(GOLD / f"map_N{N}_s{SEED}.npz")["r_elevation"], f32)
    xyz = np.ascontiguousarray(gm["xyz"], f32)
    F = smooth_fields(xyz)
    lons = np.linspace(-np.pi, np.pi, 360, endpoint=False).astype(f32)
    F["itczLons"] = lons
    F["itczLatsSummer"] = (0.15 + 0.1 * np.sin(3 * lons.astype(np.float64)) + 0.04 * np.cos(7 * lons.astype(np.float64))).astype(f32)
    F["itczLatsWinter"] = (-0.12 + 0.08 * np.cos(2 * lons.astype(np.float64))).astype(f32)
    calls = [dict(fn="wind", season="summer", centerLon=0, prefix="wind", itcz=True), dict(fn="wind", season="summer", centerLon=2.5, prefix="wind_c", itcz=False),
             dict(fn="ocean", season="winter", centerLon=2.5, prefix="ocean", itcz=False)]
    first = R.run(dict(xyz=xyz, elevation=e), F, calls=calls)
    planted = plant_specials(F, first("wind_gridRegions", np.int32), first("ocean_gridRegions", np.int32))
    res = R.run(dict(xyz=xyz, elevation=e), F, calls=calls, grids=[dict(spacing=30, centerLon=0, prefix="grid30"), dict(spacing=22.5, centerLon=2.5, prefix="grid22")])
    data = dict(r_elevation=e, **{"field_" + k: v for k, v in F.items()})
    for k in ("gridRegions",):
        data["wind_" + k], data["ocean_" + k] = res("wind_" + k, np.int32), res("ocean_" + k, np.int32)
    assert np.array_equal(data["wind_gridRegions"], first("wind_gridRegions", np.int32)) and np.array_equal(res("wind_c_gridRegions", np.int32), data["wind_gridRegions"])
    for pre in ("wind", "ocean"):
        for k in ("globe_position", "globe_color", "map_position", "map_color"):
            data[f"{pre}_{k}"] = res(f"{pre}_{k}")
        assert data[f"{pre}_globe_position"].size == 18 * res.meta["calls"][pre]["count"] > 0
    data["wind_c_map_position"] = res("wind_c_map_position")
    assert res("wind_c_globe_position").tobytes() == data["wind_globe_position"].tobytes() and not np.array_equal(data["wind_c_map_position"], data["wind_map_position"])
    data["itcz_globe"], data["itcz_map"] = res("wind_itcz_globe"), res("wind_itcz_map")
    assert data["itcz_globe"].size == 360 * 6 and data["itcz_map"].size == 359 * 6
    for g in ("grid30", "grid22"):
        data[g + "_globe"], data[g + "_map"] = res(g + "_globe"), res(g + "_map")
    meta = dict(res.meta, planted=planted, windSeason="summer", oceanSeason="winter", windCenterLon=0, oceanCenterLon=2.5, windCCenterLon=2.5,
                grids=dict(grid30=dict(spacing=30, centerLon=0), grid22=dict(spacing=22.5, centerLon=2.5)))
    data["meta_json"] = np.frombuffer(json.dumps(meta).encode(), np.uint8)
    # the planted cells did what they were planted for
    wn, on = res.meta["calls"]["wind"]["count"], res.meta["calls"]["ocean"]["count"]
    kept_w = int((data["wind_gridRegions"] >= 0).sum()), int((data["ocean_gridRegions"] >= 0).sum())
    assert wn < kept_w[0] and on < kept_w[1], "no bin was dropped for its speed"
    assert np.isnan(data["wind_globe_position"]).any() and np.isnan(data["ocean_map_position"]).any(), "the NaN speeds left no trace"
    print(f"mesh case: wind {wn} arrows of {kept_w[0]} winners, ocean {on} of {kept_w[1]}")
    return data


# ---- case 2: crafted positions -------------------------------------------------------------------------------------------------------
def unit(lat_deg, lon_deg) -> np.ndarray:
    lat, lon = np.radians(lat_deg), np.radians(lon_deg)
    return np.stack([np.sin(lon) * np.cos(lat), np.sin(lat), np.cos(lon) * np.cos(lat)], axis=-1).astype(f32)


SPECIAL = np.array([[0, 1, 0], [0, -1, 0], [-0.0, 1, 0.0], [-0.0, 1, -0.0], [-0.0, -1, 0.0], [-0.0, -1, -0.0], [0.0, 0, -1], [-0.0, 0, -1],
                    [0.3, np.nan, 0.2], [np.nan, 0.3, 0.2], [0.0, np.nextafter(f32(1), f32(2)), 0.0]], f32)


def case_crafted(R: Reference) -> dict:
    n = int(np.load(GOLD / f"mesh_N{N}_s{SEED}.npz")["numRegions"])     # the planet under test is that mesh with its positions replaced
    rng = np.random.default_rng(20261019)
    cells = [(30, 60), (30, 61), (45, 10)]                    # (lat band, lon band) of the three bins
    # a pool of positions per bin, probed for their d2 and its rounding
    pool = np.concatenate([unit(-90 + 3 * li + rng.uniform(0.05, 2.95, 1500), -180 + 3 * lo + rng.uniform(0.05, 2.95, 1500)) for li, lo in cells])
    pr = R.run(dict(xyz=pool), {}, calls=[], probe=True)
    idx, d2, up = pr("probe_idx", np.int32), pr("probe_d2", np.float64), pr("probe_up", np.uint8)
    bulk = n - len(SPECIAL)
    per = [bulk // 3, bulk // 3, bulk - 2 * (bulk // 3)]
    chosen, groups = [], []
    for b, (li, lo) in enumerate(cells):
        mine = np.flatnonzero(idx == li * 120 + lo)
        assert mine.size >= 1400
        order = mine[np.argsort(d2[mine])]
        want_up = [1, 0, None][b]                             # the kind of the position that decides the bin
        k0 = next(k for k, r in enumerate(order) if want_up is None or up[r] == want_up)
        rest = order[k0 + 1:]
        # the decider five times, twelve further groups of three (both kinds among them), singles for the rest
        dup = list(rest[:60:5])
        singles = [r for r in rest if r not in set(dup)][: per[b] - 5 - 3 * len(dup)]
        members = [order[k0]] * 5 + [r for r in dup for _ in range(3)] + singles
        assert len(members) == per[b]
        chosen += members
        groups += [(int(order[k0]), 5)] + [(int(r), 3) for r in dup]
    chosen = np.array(chosen)
    xyz = np.concatenate([pool[rng.permutation(chosen)], SPECIAL])      # identical positions land at scattered indices
    assert xyz.shape == (n, 3)
    ups, downs = sum(1 for r, _ in groups if up[r]), sum(1 for r, _ in groups if not up[r])
    print(f"crafted case: {len(groups)} groups of identical positions, {ups} whose d2 rounds up, {downs} whose d2 rounds down or is exact")
    assert ups > 0 and downs > 0
    F = {"r_wind_east_summer": np.full(n, 0.1, f32), "r_wind_north_summer": np.zeros(n, f32), "r_wind_east_winter": np.zeros(n, f32), "r_wind_north_winter": np.zeros(n, f32)}
    res = R.run(dict(xyz=xyz), F, calls=[dict(fn="wind", season="summer", centerLon=0, prefix="wind", itcz=False)], probe=True)
    win = res("wind_gridRegions", np.int32)
    pidx, pup = res("probe_idx", np.int32), res("probe_up", np.uint8)
    # the deciders: in the first bin the LAST copy wins (its d2 rounds up), in the second the FIRST
    same = lambda r: np.flatnonzero((xyz.view(np.uint32) == xyz[r].view(np.uint32)).all(axis=1))  # noqa: E731
    for b, (li, lo) in enumerate(cells):
        r = win[li * 120 + lo]
        copies = same(r)
        assert copies.size == 5, copies
        if b == 0:
            assert pup[r] == 1 and r == copies[-1], "a d2 that rounds up: the last copy wins"
        if b == 1:
            assert pup[r] == 0 and r == copies[0], "a d2 that rounds down or is exact: the first copy wins"
    occupied = np.flatnonzero(win >= 0)
    print(f"crafted case: bins {occupied.tolist()} are occupied; regions in no bin: {int((pidx < 0).sum())}")
    assert (pidx < 0).sum() == 2
    # PI / (3 * DEG) is 59.99999999999999 in double, so longitude 0 falls into band 59 and latitude 0 into band 29
    edge = {59 * 120 + 59, 59 * 120 + 0, 0 * 120 + 59, 0 * 120 + 0, 29 * 120 + 119, 29 * 120 + 0}
    assert set(occupied) == edge | {li * 120 + lo for li, lo in cells}, "the poles and the antimeridian fall into the outermost bands"
    return dict(xyz=xyz, gridRegions=win, cells=np.array(cells, np.int32))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="the reference's checkout (the directory that holds its js/)")
    args = ap.parse_args()
    with tempfile.TemporaryDirectory(prefix="wo_golden_overlays_") as td:
        R = Reference(Path(args.ref), Path(td))
        outs = {f"overlays_N{N}_s{SEED}.npz": case_mesh(R), "overlays_crafted.npz": case_crafted(R)}
    for name, data in outs.items():
        out = GOLD / name
        np.savez_compressed(out, **data)
        print(f"wrote {out.relative_to(REPO)} ({out.stat().st_size / 1024:.0f} KiB)")
        assert out.stat().st_size < (1 << 20)


if __name__ == "__main__":
    main()
