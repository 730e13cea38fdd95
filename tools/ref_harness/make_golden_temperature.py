#!/usr/bin/env python3
"""Generate tests/golden/temp_*.npz, koppen_lattice.npz, koppen_classes.json and climate_import_N10000_s1.npz by running the
REFERENCE's unmodified climate chain (computeWind, computeOceanCurrents, computePrecipitation, then computeTemperature of
js/temperature.js:69-237 and classifyKoppen of js/koppen.js:67-288) under Node 12.

The reference sources are copied to a scratch directory (oracle/ref_harness/make_golden.py: prepare_reference); they never
enter this repository.  For the worker fixture alone the scratch copy of planet-worker.js gets its CDN Delaunator import
replaced by the stub of make_golden_import.py; no other reference file is touched.  A fixture holds arrays and logged numbers
only: r_temperature_summer, r_temperature_winter and koppen (ref_*), in meta_json the reference's _tempTiming, the modules'
export names, the result keys, oceanWarmthPasses by the reference's formula under V8 and the CRC32 of every wind, ocean and
precipitation input the stage read.  The inputs themselves are not stored twice: the wind_, ocean_ and precip_ fixtures of the
same planet hold them; tests/temperature_common.py takes them from there and checks the CRCs.

Cases (planet = the wind / ocean / precip fixtures of the same suffix):
  temp_config1_N10000_s1, temp_import_N10000_s1        defaults
  temp_config1_N10000_s1_wet      precip_config1_N10000_s1_wet's precipitation (offset 0.6, coverage 0.7)
  temp_config1_N10000_s1_cold / _warm   temperatureOffset -15 / +15: the polar and the tropical bands
  temp_N2000_ocean_s1, temp_N2000_land_s1, temp_N2000_edges_s1, temp_N{63,255,256,4096}_shape_s1
  temp_N250000_s4                 sparse like its siblings: every 16th cell plus whole-array CRCs
koppen_lattice.npz: classifyKoppen on a synthetic lattice of (elevation, Ts, Tw, Ps, Pw), see lattice() below.
koppen_classes.json: the reference's KOPPEN_CLASSES table (codes, names, colours) as data.
climate_import_N10000_s1.npz: the reference worker's `climateDone` after its importHeightmap of import_N10000_s1's image.

Usage:  python tools/ref_harness/make_golden_temperature.py [--ref /root/reference] [--only NAME] [--time-cells N]
  --only NAME      one planet case, or `lattice` (with the class table), or `climate`
  --time-cells N   no fixture is written: the reference's wall time of computeTemperature + classifyKoppen on the N-cell planet of
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
HARNESS = Path(__file__).resolve().parent / "run_temperature.mjs"
STRIDE = MW.STRIDE
TYPES = MW.TYPES
crc = MW.crc
# name suffix -> (precipitationOffset, landCoverage) or None, temperatureOffset or None, the precip fixture that holds r_precip_*
VARIANTS = {"": (None, None, ""), "_wet": ((0.6, 0.7), None, "_wet"), "_cold": (None, -15, ""), "_warm": (None, 15, "")}
ORDER = ["temp_config1_N10000_s1", "temp_import_N10000_s1", "temp_config1_N10000_s1_wet", "temp_config1_N10000_s1_cold", "temp_config1_N10000_s1_warm",
         "temp_N2000_ocean_s1", "temp_N2000_land_s1", "temp_N2000_edges_s1"] + [f"temp_N{n}_shape_s1" for n in MW.SHAPE_SIZES] + ["temp_N250000_s4"]


def cases(only=None):
    out = []
    for c in MW.cases(None):
        planet = c["name"][len("wind_"):]
        for suffix, (pargs, toff, psuffix) in VARIANTS.items():
            if suffix and planet != "config1_N10000_s1":
                continue
            out.append(dict(c, name="temp_" + planet + suffix, planet=planet, precip="precip_" + planet + psuffix, pargs=pargs, toff=toff))
    out = [c for c in out if only in (None, c["name"])]
    return sorted(out, key=lambda c: ORDER.index(c["name"]))


def timing_case(n_cells: int):
    return dict(MW.timing_case(n_cells), planet=None, precip=None, pargs=None, toff=None)


def _triple(v):
    """The f32 nearest to v and its two f32 neighbours"""
    c = np.float32(v)
    return [np.nextafter(c, np.float32(-np.inf)), c, np.nextafter(c, np.float32(np.inf))]


def _t(deg):
    """normalised temperature of deg C"""
    return (deg + 45.0) / 90.0


def lattice():
    """(elevation, tSummer, tWinter, pSummer, pWinter) f32 arrays, a few thousand cells:
      A  a coarse grid: every pair of 13 temperatures with 8 of the 64 pairs of 8 precipitations (rotating)
      B  every threshold of the classifier, the f32 value at it and its two f32 neighbours, both season orders:
         elevation <= 0; Thot < 0, < 10, >= 22; Tcold >= 18, >= 0, >= -38; Tann >= 18; Tshoulder >= 10; Ts >= Tw;
         summerFrac >= 0.7, <= 0.3 (where the arm decides B or not B); Pann < Pthresh; Pann < Pthresh * 0.5; PsummerLocal <
         PwinterLocal; PsMonthLocal < 50; PsMonthLocal < PwMonthLocal / 2; PwMonthLocal < PsMonthLocal / 10; Pdry >= 60;
         Pann >= 25 * (100 - Pdry)
      C  1 200 random cells, values beyond [0, 1] included (the clamps of the conversion)
      D  30 cells with exactly one input NaN, +inf or -inf (Math.max / Math.min on a NaN; the clamps on an infinity): each of the
         five inputs in turn, the other four those of an ordinary land cell of class C and of an ordinary ocean cell
    Rows are only ever appended: run() holds a regenerated lattice to the committed one on the rows both have."""
    rows = []
    add = lambda e, ts, tw, ps, pw: rows.append((e, ts, tw, ps, pw))  # noqa: E731
    TC = [-44, -40, -30, -10, -2, 3, 8, 12, 16, 19, 21, 25, 35]
    PC = [0, 0.02, 0.1, 0.25, 0.3, 0.36, 0.6, 1.0]
    i = 0
    for a in TC:
        for b in TC:
            for j in range(8):
                k = (i * 7 + j * 11) % 64
                add(0.2, _t(a), _t(b), PC[k // 8], PC[k % 8])
            i += 1
    wet, dry, summer_dry, winter_dry = (0.6, 0.6), (0.03, 0.03), (0.05, 0.6), (0.7, 0.02)
    both = lambda hot, cold, hp, cp: (add(0.2, hot, cold, hp, cp), add(0.2, cold, hot, cp, hp))  # noqa: E731  (local summer = sim summer, then the flip)
    # elevation <= 0
    for e in (np.float32(-0.0), np.float32(0.0), np.nextafter(np.float32(0), np.float32(1)), np.nextafter(np.float32(0), np.float32(-1)), np.float32(-0.3)):
        add(e, _t(20), _t(5), 0.5, 0.5)
    # Thot thresholds, with colder winters of several depths
    for X in (0, 10, 22):
        for hot in _triple(_t(X)):
            for depth in (0.5, 5, 15, 30, 60):
                for P in (wet, dry, summer_dry, winter_dry):
                    both(hot, _t(max(X - depth, -45)), P[0], P[1])
    # Tcold thresholds, with hotter summers
    for X in (18, 0, -38):
        for cold in _triple(_t(X)):
            for rise in (0.5, 4, 12, 25, 50):
                for P in (wet, dry, summer_dry, winter_dry):
                    both(_t(min(X + rise, 45)), cold, P[0], P[1])
    # Tann >= 18 (decides h / k): (Ts + Tw) / 2 = 18
    for hot, coldX in ((30, 6), (20, 16), (40, -4)):
        for cold in _triple(_t(coldX)):
            for P in (dry, (0.12, 0.12), (0.2, 0.05)):
                both(np.float32(_t(hot)), cold, P[0], P[1])
    # Tshoulder >= 10: Thot - (Thot - Tcold) / 3 = 10
    for hot in (11, 12, 15, 18, 20, 21.5):
        for cold in _triple(_t(10 - (hot - 10) * 2)):
            for P in (wet, summer_dry, winter_dry):
                both(np.float32(_t(hot)), cold, P[0], P[1])
    # Ts >= Tw: equal temperatures and their neighbours decide which season is local summer
    for X in (-5, 12, 20, 30):
        for ts in _triple(_t(X)):
            for P in (summer_dry, winter_dry, (0.5, 0.2), (0.2, 0.5)):
                add(0.2, ts, np.float32(_t(X)), P[0], P[1])
                add(0.2, np.float32(_t(X)), ts, P[0], P[1])
    # summerFrac: Pann = 500 mm with thresholds 20 T + {0, 140, 280}: T = 14 puts 0.7 between 560 and 420, T = 20 puts 0.3 between 400 and 540
    for T in (14, 20, 23.5):
        for frac in (0.7, 0.3):
            for ps in _triple(0.5 * frac):
                both(_t(T + 1), _t(T - 1), ps, np.float32(0.5) - np.float32(0.5 * frac))
    # Pann < Pthresh and Pann < Pthresh * 0.5 (the middle arm: Pthresh = 20 Tann + 140), and with Pthresh = 0 (Tann = -7)
    for T in (10, 19, 2, -7):
        th = max(0.0, 20 * T + 140) / 1000
        for part in (1.0, 0.5):
            half = np.float32(th * part / 2)
            for pw in _triple(th * part - float(half)):
                both(_t(T + 6), _t(T - 6), half, pw)
    # the precipitation pattern: PsummerLocal < PwinterLocal, PsMonthLocal < 50, < PwMonthLocal / 2, PwMonthLocal < PsMonthLocal / 10
    for hot, cold in ((25, 5), (15, 3), (24, -10), (16, -20), (13, -40)):
        for p in _triple(0.5):
            both(_t(hot), _t(cold), p, np.float32(0.5))
        for p in _triple(0.3):
            both(_t(hot), _t(cold), p, np.float32(0.9))
        for p in _triple(0.25):
            both(_t(hot), _t(cold), p, np.float32(0.5))
        for p in _triple(0.08):
            both(_t(hot), _t(cold), np.float32(0.8), p)
        for p in _triple(0.1):
            both(_t(hot), _t(cold), np.float32(1.0), p)
    # tropical: Pdry >= 60 (0.36 of a half year) and Pann >= 25 * (100 - Pdry): Pw = 0.3 -> Ps = 2.5 - 0.3 - 1.25 = 0.95
    for hot, cold in ((30, 20), (26, 18.5), (40, 25)):
        for p in _triple(0.36):
            both(_t(hot), _t(cold), np.float32(0.8), p)
            both(_t(hot), _t(cold), p, np.float32(0.36))
        for p in _triple(0.95):
            both(_t(hot), _t(cold), p, np.float32(0.3))
        for p in _triple(0.3):
            both(_t(hot), _t(cold), np.float32(0.95), p)
    rng = np.random.default_rng(31031)
    for _ in range(1200):
        add(rng.choice([0.2, 0.2, 0.2, -0.1]), rng.uniform(-0.1, 1.1), rng.uniform(-0.1, 1.1), rng.uniform(-0.05, 1.2) ** 2, rng.uniform(-0.05, 1.2) ** 2)
    for base in ((0.2, _t(20), _t(5), 0.5, 0.5), (-0.3, _t(20), _t(5), 0.5, 0.5)):
        for i in range(5):
            for v in (np.nan, np.inf, -np.inf):
                add(*[v if j == i else x for j, x in enumerate(base)])
    a = np.array(rows, np.float64).astype(np.float32)
    return {k: np.ascontiguousarray(a[:, i]) for i, k in enumerate(("elevation", "tSummer", "tWinter", "pSummer", "pWinter"))}


def climate_job(work: Path, ref_js: Path, put):
    """The worker fixture: make_golden_import.py's import command, then computeClimate"""
    import make_golden_import as MI
    from oracle.ref_harness.make_golden_elevation import planar_triangulation
    pw = ref_js / "planet-worker.js"
    src = pw.read_text()
    line = next(ln for ln in src.splitlines() if ln.startswith("import Delaunator from 'https://"))
    (ref_js / "wo-stub-delaunator.js").write_text(MI.STUB)
    pw.write_text(src.replace(line, "import Delaunator from './wo-stub-delaunator.js';"))
    t, h = planar_triangulation(MI.N, MI.JITTER, MI.SEED)
    im = np.load(GOLD / f"import_N{MI.N}_s{MI.SEED}.npz")["img_512x256"]
    return dict(N=MI.N, jitter=MI.JITTER, seed=MI.SEED, params=MI.PARAMS, image=put("img_import.bin", im, np.uint8), W=int(im.shape[1]), H=int(im.shape[0]),
                triangulations=[dict(n=MI.N, triangles=put("tri.bin", t, t.dtype), halfedges=put("he.bin", h, h.dtype))], out=str(work / "climate_"))


def run(ref: Path, cs, write: bool, with_lattice: bool, with_climate: bool):
    with tempfile.TemporaryDirectory(prefix="wo_golden_temp_") as td:
        work = Path(td)
        ref_js = prepare_reference(ref, work)
        put = lambda name, a, ty: (np.ascontiguousarray(a, ty).tofile(work / name), str(work / name))[1]  # noqa: E731
        job = dict(cases=[], meta=str(work / "meta.json"))
        lat = None
        if with_lattice:
            lat = lattice()
            job["lattice"] = dict({k: put(f"lat_{k}.bin", v, np.float32) for k, v in lat.items()}, numRegions=int(lat["elevation"].size), out=str(work / "lat_out.bin"))
            job["classes"] = str(work / "classes.json")
        if with_climate:
            job["climate"] = climate_job(work, ref_js, put)
        for c in cs:
            k = c["name"]
            j = dict(name=k, numRegions=int(len(c["off"]) - 1), adjOffset=put(f"{k}_off.bin", c["off"], np.int32),
                     adjList=put(f"{k}_adj.bin", c["adj"], np.int32), xyz=put(f"{k}_xyz.bin", c["xyz"], np.float32),
                     elevation=put(f"{k}_e.bin", c["e"], np.float32), r_plate=put(f"{k}_plate.bin", c["plate"], np.int32),
                     plateIsOcean=put(f"{k}_ocean.bin", c["ocean"], np.int32), seed=c["seed"], axialTilt=23.5, out=str(work / f"{k}_o_"))
            if c["pargs"] is not None:
                j["precipitationOffset"], j["landCoverage"] = c["pargs"]
            if c["toff"] is not None:
                j["temperatureOffset"] = c["toff"]
            job["cases"].append(j)
        (work / "job.json").write_text(json.dumps(job))
        subprocess.run(["node", "--harmony-optional-chaining", "--harmony-nullish", "--max-old-space-size=6000", str(HARNESS), str(ref_js),
                        str(work / "job.json")], check=True, stdout=subprocess.DEVNULL)      # the reference logs on module load
        meta = json.loads((work / "meta.json").read_text())
        if with_lattice:
            out = np.fromfile(work / "lat_out.bin", np.uint8)
            classes = json.loads((work / "classes.json").read_text())
            reached = np.bincount(out, minlength=len(classes))
            print(f"koppen lattice: {out.size} cells, cells per class {reached.tolist()}")
            assert len(classes) == 31 and (reached > 0).all(), "the lattice does not reach every class"
            table = json.dumps(dict(classes=classes, exports=meta["koppenExports"]), indent=1) + "\n"
            if (GOLD / "koppen_lattice.npz").exists():          # the committed rows stay what they are, bytes and classes; so does the table
                old = np.load(GOLD / "koppen_lattice.npz")
                n = old["ref_koppen"].size
                assert n <= out.size and old["ref_koppen"].tobytes() == out[:n].tobytes(), "the classes of the committed rows changed"
                for k, v in lat.items():
                    assert old[f"in_{k}"].tobytes() == v[:n].tobytes(), f"the committed rows of {k} changed"
                assert (GOLD / "koppen_classes.json").read_text() == table, "koppen_classes.json changed"
                print(f"koppen lattice: the {n} committed rows and koppen_classes.json are unchanged byte for byte; {out.size - n} rows appended, "
                      f"classes {out[n:].tolist()}")
            np.savez_compressed(GOLD / "koppen_lattice.npz", ref_koppen=out, **{f"in_{k}": v for k, v in lat.items()})
            (GOLD / "koppen_classes.json").write_text(table)
            print("wrote tests/golden/koppen_lattice.npz, tests/golden/koppen_classes.json")
        if with_climate:
            cm = meta["climate"]
            data = {f"done_{k}": np.fromfile(work / f"climate_{k}.bin", TYPES[ty]) for k, ty in cm["arrays"].items()}
            data.update({f"layer_{k}": np.fromfile(work / f"climate_layer_{k}.bin", TYPES[ty]) for k, ty in cm["layers"].items()})
            # the debug layers are views of result arrays: stored once, the key mapping goes into the meta
            same = {}
            for k in list(data):
                if k.startswith("layer_"):
                    twin = next((d for d in data if not d.startswith("layer_") and data[d].dtype == data[k].dtype and np.array_equal(data[d], data[k])), None)
                    if twin:
                        same[k[len("layer_"):]] = twin[len("done_"):]
                        del data[k]
            cm["layerSameAs"] = same
            data["meta_json"] = np.frombuffer(json.dumps(cm).encode(), np.uint8)
            f = GOLD / "climate_import_N10000_s1.npz"
            np.savez_compressed(f, **data)
            print(f"wrote {f.relative_to(REPO)} ({f.stat().st_size / 1024:.0f} KiB); progress {cm['progress']}; second call's wind time {cm['secondWind']}")
        for c in cs:
            k = c["name"]
            cm = meta["cases"][k]
            print(f"{k}: reference computeTemperature {cm['ms']:.1f} ms, classifyKoppen {cm['msKoppen']:.1f} ms, together {cm['ms'] + cm['msKoppen']:.1f} ms; scalars {cm['scalars']}")
            if not write:
                continue
            sparse = c["sparse"]
            data = {}
            info = dict(exports=meta["exports"], koppenExports=meta["koppenExports"], keys=cm["keys"], arrays=cm["arrays"], inputs=cm["inputs"], planet=c["planet"],
                        precip=c["precip"], seed=c["seed"], numRegions=int(len(c["off"]) - 1), ref_ms=cm["ms"], ref_ms_koppen=cm["msKoppen"], log=cm["log"],
                        timing=cm["stages"], scalars=cm["scalars"], temperatureOffset=0 if c["toff"] is None else c["toff"], stride=STRIDE if sparse else 1, crc={},
                        crc_inputs={})
            for name, ty in cm["arrays"].items():
                a = np.fromfile(work / f"{k}_o_{name}.bin", TYPES[ty])
                info["crc"][name] = crc(a)
                data[f"ref_{name}"] = a[::STRIDE].copy() if sparse else a
            for name, ty in cm["inputs"].items():
                info["crc_inputs"][name] = crc(np.fromfile(work / f"{k}_o_in_{name}.bin", TYPES[ty]))
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
        run(Path(args.ref), [timing_case(args.time_cells)], write=False, with_lattice=False, with_climate=False)
        return
    special = args.only in ("lattice", "climate")
    run(Path(args.ref), [] if special else cases(args.only), write=True, with_lattice=args.only in (None, "lattice"), with_climate=args.only in (None, "climate"))


if __name__ == "__main__":
    main()
