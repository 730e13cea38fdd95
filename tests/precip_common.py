"""Shared pieces of the precipitation tests: the golden cases with their inputs, the host emulator of csrc/precip_ops.h
(tests/emu_precip, built on first use) and the comparison.  The bar is bit equality on all four outputs, with no tolerance: no
per-cell code of the stage calls libm, and its three pow scalars are held to V8's by tests/test_precip.py at every size used."""
from __future__ import annotations

import ctypes as C
import json
import subprocess
from functools import lru_cache

import numpy as np

import ocean_common as OC
import wind_common as WC
from conftest import GOLDEN, REPO

EMU_DIR = REPO / "tests" / "emu_precip"
FULL_CASES = ("precip_config1_N10000_s1", "precip_import_N10000_s1", "precip_config1_N10000_s1_wet", "precip_N2000_ocean_s1", "precip_N2000_land_s1",
              "precip_N2000_edges_s1", "precip_N63_shape_s1", "precip_N255_shape_s1", "precip_N256_shape_s1", "precip_N4096_shape_s1")
SPARSE_CASE = "precip_N250000_s4"
GOLDEN_CASES = FULL_CASES + (SPARSE_CASE,)
SEASON_INPUTS = ("r_wind_east", "r_wind_north", "r_pressure")
FRAME = ("r_eastX", "r_eastY", "r_eastZ", "r_northX", "r_northY", "r_northZ")
WIND_INPUTS = ("r_lat", "r_lon", "r_isLand", "r_continentality", "r_coastDistLand") + FRAME + ("itczLons", "itczLatsSummer", "itczLatsWinter") \
    + tuple(f"{k}_{s}" for s in ("summer", "winter") for k in SEASON_INPUTS)
OCEAN_INPUTS = ("r_ocean_warmth_summer", "r_ocean_warmth_winter")
RESULT_KEYS = ("r_precip_summer", "r_precip_winter", "r_rainshadow_summer", "r_rainshadow_winter")
COUNT_FIELDS = ("maxHops", "elevSmoothPasses", "convSmoothPasses", "shadowHops", "windwardHops", "rsSmoothPasses", "precipSmoothPasses", "wcPasses", "leeCoastHops")
LIST_FIELDS = ("upCountSummer", "downCountSummer", "upCountWinter", "downCountWinter")
F64_FIELDS = ("depletionBase", "shadowDecay", "windwardDecay", "p95Summer", "p95Winter")
# the branches of precip_ops.h's enum Branch, in its order
BRANCHES = ("itcz_in", "itcz_out", "itcz_core", "conv_pos", "conv_not", "oro_windward", "oro_leeward", "oro_none", "local_summer", "local_winter",
            "monsoon_relief", "monsoon_none", "monsoon_no_coast", "latband_in", "latband_out", "press_high", "press_low", "suppress_pos", "suppress_not",
            "polar_in", "polar_out", "polar_no_coast", "cont_dry", "cont_not", "lee_high", "lee_cyclo", "lee_not", "ocean_cell", "cut_near", "cut_far", "cut_none",
            "seed_windward", "seed_shadow", "seed_low", "seed_zero",
            "zonal0", "zonal1", "zonal2", "zonal3", "zonal4", "zonal5", "hwind0", "hwind1", "hwind2", "hwind3",
            "med_in", "med_out", "heur_windward", "heur_leeward", "heur_cut_far", "cap_in", "cap_binds", "cap_out", "apply_shadow", "apply_windward", "apply_none")
# a land cell above 0.8 km whose wind . gradient is exactly 0 leaves its seed at 0: not one of the branches the census must reach
OPTIONAL_BRANCHES = ("seed_zero",)
_emu = []
ptr, crc, same_bits, Mesh = WC.ptr, WC.crc, WC.same_bits, WC.Mesh


def emu():
    if not _emu:
        subprocess.run(["make", "-s", "-C", str(EMU_DIR)], check=True)
        L = C.CDLL(str(EMU_DIR / "_build" / "libemu_precip.so"))
        assert L.emu_precip_branch_count() == len(BRANCHES)
        _emu.append(L)
    return _emu[0]


def pow_differs(N) -> bool:
    """Does precip_ops.h list one of this size's three hop counts as one where the host pow is not V8's?"""
    return bool(emu().emu_precip_pow_differs(C.c_int32(N)))


def pow_diff_list(which):
    out = np.zeros(64, np.int32)
    n = emu().emu_precip_pow_diff_list(C.c_int32(which), ptr(out))
    return [int(v) for v in out[:n]]


def params(N):
    out = np.zeros(9, np.int32)
    emu().emu_precip_params(C.c_int32(N), ptr(out))
    return dict(zip(COUNT_FIELDS, (int(v) for v in out)))


def host_pow(base, count):
    out = np.zeros(count, np.float64)
    emu().emu_precip_pow(C.c_double(base), C.c_int32(1), C.c_int32(count), ptr(out))
    return out


@lru_cache(maxsize=None)
def golden_case(name):
    """A wind_common case (mesh, positions, terrain, plates, seed) with ref (the four outputs: every meta['stride']-th cell in the
    sparse fixture), meta, sc_f64, wind (the twenty wind outputs the stage reads) and warm (the two warmths of oceanResult), taken from the
    wind_ / ocean_ fixtures of the same planet.  inputs_exact: do their CRCs equal the ones recorded when the fixture was made?
    The sparse planet's per-cell inputs are rebuilt by the wind and ocean emulators; their season arrays carry the platform's
    libm, so inputs_exact may be False there and names the first field that differs."""
    g = np.load(GOLDEN / f"{name}.npz")
    meta = json.loads(bytes(g["meta_json"]).decode())
    base = WC.golden_case("wind_" + meta["planet"])
    oc = OC.golden_case("ocean_" + meta["planet"])
    if meta["stride"] == 1:
        wind = {k: base["ref"][k] for k in WIND_INPUTS}
        ocean = {k: oc["ref"][k] for k in OCEAN_INPUTS}
    else:
        own = WC.emulate(base)
        wind = {k: own[k] for k in WIND_INPUTS}
        own_ocean = OC.emulate(oc, {k: own[k] for k in OC.WIND_INPUTS})
        ocean = {k: own_ocean[k] for k in OCEAN_INPUTS}
    differs = [k for k in WIND_INPUTS + OCEAN_INPUTS if crc((wind if k in wind else ocean)[k]) != meta["crc_inputs"][k]]
    ref = {k[4:]: g[k] for k in g.files if k.startswith("ref_")}
    return dict(base, name=name, ref=ref, meta=meta, sc_f64=g["sc_f64"], wind=wind, warm=ocean, inputs_exact=not differs, inputs_differ=differs,
                offset=float(meta["precipitationOffset"]), coverage=float(meta["landCoverage"]))


def emulate(case, wind=None, ocean=None, offset=0.0, coverage=0.3, compact=False, census=None):
    """The whole stage on the host.  Returns the four arrays plus _info (as precipitation.info) and _up_cells.  census: a uint64 array of
    len(BRANCHES) counters that is added to."""
    wind = case["wind"] if wind is None else wind
    ocean = case["warm"] if ocean is None else ocean
    N = case["N"]
    f32 = lambda a: np.ascontiguousarray(a, np.float32)  # noqa: E731
    w = {k: f32(wind[k]) for k in WIND_INPUTS if k not in ("r_isLand", "r_coastDistLand")}
    land, cd = np.ascontiguousarray(wind["r_isLand"], np.uint8), np.ascontiguousarray(wind["r_coastDistLand"], np.int32)
    warm = [f32(ocean[k]) for k in OCEAN_INPUTS]
    e = f32(case["e"])
    arr = lambda xs: (C.c_void_p * len(xs))(*[ptr(a) for a in xs])  # noqa: E731
    out = {k: np.zeros(N, np.float32) for k in RESULT_KEYS}
    ints, dbls = np.zeros(15, np.int32), np.zeros(5, np.float64)
    season = lambda k: arr([w[f"{k}_summer"], w[f"{k}_winter"]])  # noqa: E731
    emu().emu_precip(C.c_int32(N), ptr(case["off"]), ptr(case["adj"]), ptr(case["xyz"]), ptr(e), ptr(w["r_lat"]), ptr(w["r_lon"]), ptr(land),
                     ptr(w["r_continentality"]), ptr(cd), arr([w[k] for k in FRAME]), arr([w["itczLatsSummer"], w["itczLatsWinter"]]),
                     season("r_wind_east"), season("r_wind_north"), season("r_pressure"), arr(warm), C.c_double(offset), C.c_double(coverage),
                     C.c_int32(1 if compact else 0), arr(list(out.values())), ptr(ints), ptr(dbls), None if census is None else ptr(census))
    out["_info"] = dict(zip(COUNT_FIELDS + LIST_FIELDS, (int(v) for v in ints[:13])), **dict(zip(F64_FIELDS, (float(v) for v in dbls))))
    out["_up_cells"] = (int(ints[13]), int(ints[14]))          # land cells with a non-empty upwind list, summer / winter
    return out


def differing(got, ref, stride=1, crcs=None):
    """{key: cells that differ} over the four outputs (or 'crc' where only the checksum of the whole array differs)"""
    bad = {}
    for k in RESULT_KEYS:
        g = got[k] if ref[k].size == got[k].size else got[k][::stride]
        if g.shape != ref[k].shape:
            bad[k] = "shape"
        elif not same_bits(g, ref[k]):
            bad[k] = int((np.ascontiguousarray(g).view(np.uint32) != np.ascontiguousarray(ref[k]).view(np.uint32)).sum())
        elif crcs is not None and crc(got[k]) != crcs[k]:
            bad[k] = "crc"
    return bad


def assert_equal(label, got, ref, stride=1, crcs=None):
    bad = differing(got, ref, stride, crcs)
    print(f"{label}: " + ("all four outputs equal bit for bit" if not bad else f"cells that differ: {bad}"))
    assert not bad, f"{label}: {bad}"


def assert_golden(label, got, case):
    m = case["meta"]
    assert_equal(label, got, case["ref"], m["stride"], m["crc"] if m["stride"] > 1 else None)


def reference_info(case):
    """The scalars of the call as the harness recorded them under V8 (counts, then depletionBase, shadowDecay, windwardDecay)"""
    return dict(case["meta"]["scalars"], **dict(zip(F64_FIELDS[:3], (float(v) for v in case["sc_f64"]))))
