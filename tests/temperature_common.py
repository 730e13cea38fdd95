"""Shared pieces of the temperature and Koppen tests: the golden cases with their inputs, the host emulator of csrc/temp_ops.h
(tests/emu_temperature, built on first use; a second build routes pow through the libm hook of tests/emu) and the comparisons.

Temperature takes a per-cell bound, as assignElevation and computeWind do (its per-cell code calls pow): every cell within
TEMP_ULP_BOUND * 2^-23 * max(1, |ref|) and at most max(8, N / 10^4) cells different at all.  TEMP_ULP_BOUND is derived in
tests/test_temperature_libm.py.  Koppen classes are compared for equality in every cell."""
from __future__ import annotations

import ctypes as C
import json
import subprocess
from functools import lru_cache

import numpy as np

import ocean_common as OC
import precip_common as PC
import wind_common as WC
from conftest import GOLDEN, REPO

EMU_DIR = REPO / "tests" / "emu_temperature"
FULL_CASES = ("temp_config1_N10000_s1", "temp_import_N10000_s1", "temp_config1_N10000_s1_wet", "temp_config1_N10000_s1_cold", "temp_config1_N10000_s1_warm",
              "temp_N2000_ocean_s1", "temp_N2000_land_s1", "temp_N2000_edges_s1", "temp_N63_shape_s1", "temp_N255_shape_s1", "temp_N256_shape_s1",
              "temp_N4096_shape_s1")
SPARSE_CASE = "temp_N250000_s4"
GOLDEN_CASES = FULL_CASES + (SPARSE_CASE,)
WIND_INPUTS = ("r_lat", "r_lon", "r_isLand", "r_continentality", "r_plateContinentality", "itczLons", "itczLatsSummer", "itczLatsWinter")
OCEAN_INPUTS = ("r_ocean_warmth_summer", "r_ocean_speed_summer", "r_ocean_warmth_winter", "r_ocean_speed_winter")
PRECIP_INPUTS = ("r_precip_summer", "r_precip_winter")
RESULT_KEYS = ("r_temperature_summer", "r_temperature_winter")
# the branches of temp_ops.h's enum Branch, in its order: computeTemperature's, then classifyKoppen's
TEMP_BRANCHES = ("ocean", "coast_warm", "coast_none", "inland", "p_high", "p_low", "p_mid", "lapse", "no_lapse", "local_summer", "local_winter")
KOPPEN_BRANCHES = ("frac_high", "frac_low", "frac_mid", "desert", "steppe", "pattern_s", "pattern_w", "pattern_f", "letter_a", "letter_b", "letter_c", "letter_d")
BRANCHES = TEMP_BRANCHES + KOPPEN_BRANCHES
TEMP_ULP_BOUND = 2                  # x 2^-23 per cell, relative to max(1, |ref|): see test_temperature_libm.py for the measurement behind it
HOOK_K = 4                          # double ulps: twice the 2-ulp bound taken for ocml's double pow
_emu = {}
ptr, crc, same_bits, Mesh, diff_cap = WC.ptr, WC.crc, WC.same_bits, WC.Mesh, WC.diff_cap


def emu(libm_hook=False):
    if not _emu:
        subprocess.run(["make", "-s", "-C", str(EMU_DIR)], check=True)
        for hook, lib in ((False, "libemu_temperature.so"), (True, "libemu_temperature_libm.so")):
            L = C.CDLL(str(EMU_DIR / "_build" / lib))
            assert L.emu_temperature_branch_count() == len(BRANCHES)
            _emu[hook] = L
    return _emu[bool(libm_hook)]


def passes(N) -> int:
    return int(emu().emu_temperature_passes(C.c_int32(N)))


def libm_calls(lib):
    out = np.zeros(7, np.uint64)
    lib.emu_libm_calls(ptr(out))
    return int(out[5])                      # pow


@lru_cache(maxsize=None)
def _sparse_inputs(planet):
    """The sparse planet's per-cell inputs, rebuilt by the wind, ocean and precipitation emulators"""
    base = WC.golden_case("wind_" + planet)
    own = WC.emulate(base)
    oc = OC.golden_case("ocean_" + planet)
    own_ocean = OC.emulate(oc, {k: own[k] for k in OC.WIND_INPUTS})
    pc = PC.golden_case("precip_" + planet)
    own_precip = PC.emulate(pc, pc["wind"], pc["warm"], pc["offset"], pc["coverage"])
    return own, own_ocean, own_precip


@lru_cache(maxsize=None)
def golden_case(name):
    """A wind_common case (mesh, positions, terrain, plates, seed) with ref (r_temperature_* and koppen: every meta['stride']-th
    cell in the sparse fixture), meta, and the inputs the stage reads: wind, sea (the four fields of oceanResult; `ocean` stays the
    planet's oceanic plate ids), precip, taken from the wind_ / ocean_ /
    precip_ fixtures of the same planet.  inputs_exact: do their CRCs equal the ones recorded when the fixture was made?  The
    sparse planet's per-cell inputs are rebuilt by the emulators of the earlier stages; its season winds carry the platform's
    libm, so inputs_exact may be False there and inputs_differ names the fields."""
    g = np.load(GOLDEN / f"{name}.npz")
    meta = json.loads(bytes(g["meta_json"]).decode())
    base = WC.golden_case("wind_" + meta["planet"])
    if meta["stride"] == 1:
        oc = OC.golden_case("ocean_" + meta["planet"])
        pc = PC.golden_case(meta["precip"])
        wind = {k: base["ref"][k] for k in WIND_INPUTS}
        ocean = {k: oc["ref"][k] for k in OCEAN_INPUTS}
        precip = {k: pc["ref"][k] for k in PRECIP_INPUTS}
    else:
        own, own_ocean, own_precip = _sparse_inputs(meta["planet"])
        wind = {k: own[k] for k in WIND_INPUTS}
        ocean = {k: own_ocean[k] for k in OCEAN_INPUTS}
        precip = {k: own_precip[k] for k in PRECIP_INPUTS}
    every = dict(wind, **ocean, **precip)
    differs = [k for k in WIND_INPUTS + OCEAN_INPUTS + PRECIP_INPUTS if crc(every[k]) != meta["crc_inputs"][k]]
    ref = {k[4:]: g[k] for k in g.files if k.startswith("ref_")}
    return dict(base, name=name, ref=ref, meta=meta, wind=wind, sea=ocean, precip=precip, inputs_exact=not differs, inputs_differ=differs,
                offset=float(meta["temperatureOffset"]))


def emulate(case, wind=None, ocean=None, precip=None, offset=0.0, pair=False, census=None, lib=None, e=None):
    """computeTemperature on the host.  Returns the two arrays plus _passes.  census: a uint64 array of len(BRANCHES) counters that
    is added to."""
    wind = case["wind"] if wind is None else wind
    ocean = case["sea"] if ocean is None else ocean
    precip = case["precip"] if precip is None else precip
    N = case["N"]
    f32 = lambda a: np.ascontiguousarray(a, np.float32)  # noqa: E731
    w = {k: f32(wind[k]) for k in WIND_INPUTS if k != "r_isLand"}
    land = np.ascontiguousarray(wind["r_isLand"], np.uint8)
    arr = lambda xs: (C.c_void_p * len(xs))(*[ptr(a) for a in xs])  # noqa: E731
    season = lambda src, k: [f32(src[f"{k}_summer"]), f32(src[f"{k}_winter"])]  # noqa: E731
    p, wm, sp = season(precip, "r_precip"), season(ocean, "r_ocean_warmth"), season(ocean, "r_ocean_speed")
    elev = f32(case["e"] if e is None else e)
    out = {k: np.zeros(N, np.float32) for k in RESULT_KEYS}
    L = emu() if lib is None else lib
    n = L.emu_temperature(C.c_int32(N), ptr(case["off"]), ptr(case["adj"]), ptr(elev), ptr(w["r_lat"]), ptr(w["r_lon"]), ptr(land), ptr(w["r_continentality"]),
                          ptr(w["r_plateContinentality"]), arr([w["itczLatsSummer"], w["itczLatsWinter"]]), arr(p), arr(wm), arr(sp), C.c_double(offset),
                          C.c_int32(1 if pair else 0), arr(list(out.values())), None if census is None else ptr(census))
    out["_passes"] = int(n)
    return out


def emulate_koppen(elevation, temp, precip, census=None):
    """classifyKoppen on the host: a uint8 array"""
    f32 = lambda a: np.ascontiguousarray(a, np.float32)  # noqa: E731
    a = [f32(elevation), f32(temp["r_temperature_summer"]), f32(temp["r_temperature_winter"]), f32(precip["r_precip_summer"]), f32(precip["r_precip_winter"])]
    assert len({x.size for x in a}) == 1
    out = np.zeros(a[0].size, np.uint8)
    emu().emu_koppen(C.c_int32(a[0].size), *[ptr(x) for x in a], ptr(out), None if census is None else ptr(census))
    return out


def deviation(got, ref):
    """(cells that differ, largest |difference|, cells past the per-cell bound, largest difference relative to max(1, |ref|))"""
    a, b = np.asarray(got, np.float32).astype(np.float64), np.asarray(ref, np.float32).astype(np.float64)
    differ = np.ascontiguousarray(got, np.float32).view(np.uint32) != np.ascontiguousarray(ref, np.float32).view(np.uint32)
    d = np.abs(a - b)
    scale = np.maximum(1.0, np.abs(b))
    over = ~(d <= TEMP_ULP_BOUND * 2.0 ** -23 * scale)          # NaN on either side counts as past the bound
    rel = d / scale
    return int(differ.sum()), float(d.max()) if d.size else 0.0, int(over.sum()), float(rel.max()) if d.size else 0.0


def check(label, got, ref, N, stride=1):
    """Both outputs under the bound and the cap.  Prints every figure before asserting; returns {key: cells that differ}."""
    figs = {}
    for k in RESULT_KEYS:
        g = got[k] if ref[k].size == got[k].size else got[k][::stride]
        assert g.shape == ref[k].shape, (label, k, g.shape, ref[k].shape)
        figs[k] = deviation(g, ref[k])
    cap = diff_cap(N)
    print(f"{label}: " + "; ".join(f"{k}: {n} cells differ (cap {cap}), largest {m:.3g}, {o} past {TEMP_ULP_BOUND} x 2^-23 x max(1, |ref|)" for k, (n, m, o, _) in figs.items()))
    for k, (n, m, o, _) in figs.items():
        assert o == 0, f"{label}: {k}: {o} cells past the per-cell bound (largest difference {m:.3g})"
        assert n <= cap, f"{label}: {k}: {n} cells differ, the cap is {cap}"
    return {k: v[0] for k, v in figs.items()}


def check_golden(label, got, case):
    return check(label, got, case["ref"], case["N"], case["meta"]["stride"])


def koppen_differing(got, ref, stride=1):
    g = got if ref.size == got.size else got[::stride]
    assert g.shape == ref.shape, (g.shape, ref.shape)
    return int((g != ref).sum())


LATTICE_FINITE = 3841               # the lattice's rows before its 30 non-finite ones: 15 x 256 + 1


def lattice():
    """(elevation, temp, precip, the reference's recorded classes) of tests/golden/koppen_lattice.npz"""
    g = np.load(GOLDEN / "koppen_lattice.npz")
    temp = dict(r_temperature_summer=g["in_tSummer"], r_temperature_winter=g["in_tWinter"])
    precip = dict(r_precip_summer=g["in_pSummer"], r_precip_winter=g["in_pWinter"])
    return g["in_elevation"], temp, precip, g["ref_koppen"]
