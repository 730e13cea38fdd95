"""computePrecipitation (js/precipitation.js:196-684, js/heuristic-precip.js) without a GPU: the host emulator of csrc/precip_ops.h
(tests/emu_precip drives the very bodies the kernels of csrc/precip.hip run) against the reference's goldens, bit for bit; the
scalars of a call against V8's; the host pow against V8's Math.pow; which branches the goldens reach; the compacted-list form of
the propagations against the row-shaped form the kernels use; the Python argument checks.

The device itself is held to the same goldens in test_gpu_precip.py.  Every comparison prints its figures before it asserts.

Mutation notes (each made on a scratch copy of the tree with the emulator standing in for the device, then
`pytest tests/test_precip.py`; none is in the tree):
  * upWt / dnWt kept in double (aligned_weights hands out the doubles, the emulator's compacted-list route carries them and is
    made the default route): test_emulator_matches_reference fails for the four cases with relief above 0.8 km (config1, its wet
    twin, import, the 250 k planet); the others seed no rain shadow.
  * dnDot formed as a sum of negated terms: all 38 tests still pass.  Negation is exact and rounding to nearest is symmetric, so
    the two forms give the same double; no test can tell them apart, and the form is held by reading (precip_ops.h says so).
  * the fold after the last pass left out (shadow_merge_cell merges the seed alone): test_emulator_matches_reference fails for
    the same four cases.
  * itczLookup(lon) * 0.3 without the 0.3 in the heuristic wind field: test_emulator_matches_reference fails for all 11 cases.
  * percentile rank ceil instead of floor: test_emulator_matches_reference fails for all 11 cases (N * 0.95 is whole at no size
    used).
"""
import json

import numpy as np
import pytest

import precip_common as PC
from conftest import GOLDEN

# every planet size a test of the precipitation stage uses (CPU and GPU); test_pow_agrees_at_every_size_used holds each to V8's
# three scalars
SIZES_USED = (64, 256, 257, 2001, 4096, 4097, 10000, 131072, 131073, 200000, 250001, 1000001)


@pytest.mark.parametrize("name", PC.GOLDEN_CASES)
def test_emulator_matches_reference(name):
    """All four outputs bit for bit; the sparse case on the stored cells and on the checksums of the whole arrays, where it counts
    only when the emulated wind and ocean inputs have the recorded checksums (printed either way)."""
    case = PC.golden_case(name)
    from planet_heightmap_generation_amd import precipitation as PD
    assert set(case["ref"]) == {k for k, _ in PD.RESULT_FIELDS} == set(case["meta"]["keys"]) - {"_precipTiming"}
    assert case["meta"]["exports"] == ["computePrecipitation"]
    out = PC.emulate(case, offset=case["offset"], coverage=case["coverage"])
    m = case["meta"]
    bad = PC.differing(out, case["ref"], m["stride"], m["crc"] if m["stride"] > 1 else None)
    print(f"{name}: N {case['N']}, inputs have the reference's checksums: {case['inputs_exact']}"
          + ("" if case["inputs_exact"] else f" (first field that differs: {case['inputs_differ'][0]}, {len(case['inputs_differ'])} in all)")
          + f"; cells that differ from the golden: {bad or 'none'}; {out['_info']}")
    if name != PC.SPARSE_CASE:
        assert case["inputs_exact"], case["inputs_differ"]
    if case["inputs_exact"]:
        assert not bad, bad
    for k in PC.RESULT_KEYS:
        assert np.isfinite(out[k]).all() and out[k].min() >= (0 if "precip" in k else -1) and out[k].max() <= 1


@pytest.mark.parametrize("name", PC.GOLDEN_CASES)
def test_scalars_match_v8(name):
    """The nine counts and the three pow scalars of params_for(N) against the reference's formulas evaluated under V8.  maxPrecip
    is not observable in the unmodified reference (it is a local of computePrecipitation and is not logged); it is held through
    the two precipitation outputs, every cell of which is divided by it."""
    case = PC.golden_case(name)
    want = PC.reference_info(case)
    got = PC.params(case["N"])
    host = {"depletionBase": 1 - PC.host_pow(0.78, 200)[want["maxHops"] - 1], "shadowDecay": 1 - PC.host_pow(0.15, 1024)[want["shadowHops"] - 1],
            "windwardDecay": 1 - PC.host_pow(0.25, 1024)[want["windwardHops"] - 1]}
    print(f"{name}: {got}, {host}; V8: {want}")
    assert got == {k: want[k] for k in PC.COUNT_FIELDS}
    assert all(np.float64(host[k]).tobytes() == np.float64(want[k]).tobytes() for k in host)
    assert not PC.pow_differs(case["N"])
    if name == PC.SPARSE_CASE:
        assert [got[k] for k in ("shadowHops", "windwardHops", "convSmoothPasses", "elevSmoothPasses", "rsSmoothPasses", "precipSmoothPasses", "wcPasses", "maxHops")] \
            == [62, 37, 10, 5, 4, 2, 7, 20]


def test_pow_fixture():
    """The host's pow(b, 1 / h) against V8's Math.pow for b = 0.15, 0.25 (h = 1 .. 1024) and 0.78 (h = 1 .. 200): the hop counts
    at which they differ are the lists of csrc/precip_ops.h, by one ulp each."""
    g = np.load(GOLDEN / "precip_pow_v8.npz")
    for which, (key, base) in enumerate((("pow_0_15", 0.15), ("pow_0_25", 0.25), ("pow_0_78", 0.78))):
        v8 = g[key]
        assert v8.size == (200 if base == 0.78 else 1024)
        host = PC.host_pow(base, v8.size)
        d = np.flatnonzero(v8.view(np.uint64) != host.view(np.uint64))
        ulps = np.abs(v8.view(np.int64)[d] - host.view(np.int64)[d])
        print(f"pow({base}, 1/h): the host differs from V8 at h = {(d + 1).tolist()} by {ulps.tolist()} ulp; the header lists {PC.pow_diff_list(which)}")
        assert (d + 1).tolist() == PC.pow_diff_list(which)
        assert (ulps <= 1).all()
    assert all(h > 20 for h in PC.pow_diff_list(2)), "depletionBase is V8's at every reachable maxHops (8 .. 20)"


def test_pow_agrees_at_every_size_used():
    """At every planet size a precipitation test uses, all three hop counts are ones where the host pow is V8's."""
    g = np.load(GOLDEN / "precip_pow_v8.npz")
    sizes = sorted(set(SIZES_USED) | {PC.golden_case(n)["N"] for n in PC.FULL_CASES} | {json.loads(bytes(np.load(GOLDEN / f"{PC.SPARSE_CASE}.npz")["meta_json"]).decode())["numRegions"]})
    for N in sizes:
        q = PC.params(N)
        ok = [g[k][q[h] - 1].tobytes() == PC.host_pow(b, q[h])[-1].tobytes() for k, b, h in (("pow_0_15", 0.15, "shadowHops"), ("pow_0_25", 0.25, "windwardHops"), ("pow_0_78", 0.78, "maxHops"))]
        print(f"N {N}: shadowHops {q['shadowHops']}, windwardHops {q['windwardHops']}, maxHops {q['maxHops']}: host pow equals V8's: {ok}")
        assert all(ok) and not PC.pow_differs(N)


def test_branch_census():
    """How many (cell, season) pairs of the full-size goldens take each branch of the bodies; every branch is taken by at least one
    cell of at least one case."""
    total = np.zeros(len(PC.BRANCHES), np.uint64)
    rows = {}
    for name in PC.FULL_CASES:
        case = PC.golden_case(name)
        c = np.zeros(len(PC.BRANCHES), np.uint64)
        PC.emulate(case, offset=case["offset"], coverage=case["coverage"], census=c)
        rows[name] = c
        total += c
    width = max(len(b) for b in PC.BRANCHES)
    print(f"{'branch':<{width}} " + " ".join(f"{n[len('precip_'):]:>20}" for n in PC.FULL_CASES) + f" {'total':>10}")
    for i, b in enumerate(PC.BRANCHES):
        print(f"{b:<{width}} " + " ".join(f"{int(rows[n][i]):>20}" for n in PC.FULL_CASES) + f" {int(total[i]):>10}")
    missing = [b for i, b in enumerate(PC.BRANCHES) if total[i] == 0 and b not in PC.OPTIONAL_BRANCHES]
    assert not missing, f"no cell of any golden takes: {missing}"


@pytest.mark.parametrize("name", PC.FULL_CASES)
def test_compacted_lists_give_the_same_bits(name):
    """The propagations over compacted neighbour lists, written as the reference writes them, against the row-shaped weights with
    0 for non-members that the kernels use: the same four arrays and the same list lengths."""
    case = PC.golden_case(name)
    rows = PC.emulate(case, offset=case["offset"], coverage=case["coverage"])
    lists = PC.emulate(case, offset=case["offset"], coverage=case["coverage"], compact=True)
    PC.assert_equal(f"{name}: compacted lists against row-shaped weights", lists, rows)
    assert lists["_info"] == rows["_info"]


def test_goldens_need_every_step():
    """What the cases are there for: the ocean planet has empty lists and no rain shadow, the land planet has coast distance -1
    everywhere, the wet case differs from the default one, shadow and windward zones both occur."""
    sea = PC.emulate(PC.golden_case("precip_N2000_ocean_s1"))
    assert [sea["_info"][k] for k in PC.LIST_FIELDS] == [0, 0, 0, 0] and not sea["r_rainshadow_summer"].any()
    land = PC.golden_case("precip_N2000_land_s1")
    assert (land["wind"]["r_coastDistLand"] == -1).all() and (land["wind"]["r_isLand"] == 1).all()
    a, wet = PC.golden_case("precip_config1_N10000_s1"), PC.golden_case("precip_config1_N10000_s1_wet")
    assert wet["coverage"] > 0.4 and not PC.same_bits(a["ref"]["r_precip_summer"], wet["ref"]["r_precip_summer"])
    assert PC.same_bits(a["ref"]["r_rainshadow_summer"], wet["ref"]["r_rainshadow_summer"])
    rs = a["ref"]["r_rainshadow_summer"]
    assert rs.min() < -0.01 and rs.max() > 0.01
    info = PC.emulate(a)["_info"]
    assert info["upCountSummer"] > 0.01 * int((a["wind"]["r_isLand"] != 0).sum()) and info["p95Summer"] != 1


class _NoDevicePlanet:
    """Stands where a Planet would: any use of its handle is a use of the device."""
    numRegions = 100

    @property
    def handle(self):
        raise AssertionError("device work was started")


def test_python_argument_checks_refuse_before_device_work():
    from planet_heightmap_generation_amd import ocean as OD, precipitation as PD
    p, n = _NoDevicePlanet(), 100
    xyz, e = np.zeros(3 * n, np.float32), np.zeros(n, np.float32)
    ty = dict(r_isLand=np.uint8, r_coastDistLand=np.int32)
    wind = {k: np.zeros(360 if k.startswith("itcz") else n, ty.get(k, np.float32)) for k in PD.WIND_INPUTS}
    ocean = {k: np.zeros(n, np.float32) for k in PD.OCEAN_INPUTS}
    with pytest.raises(ValueError, match="r_xyz"):
        PD.compute_precipitation(p, xyz[:-3], e)
    with pytest.raises(ValueError, match="r_elevation"):
        PD.compute_precipitation(p, xyz, e[:-1])
    with pytest.raises(ValueError, match="r_pressure_winter"):
        PD.compute_precipitation(p, xyz, e, {k: v for k, v in wind.items() if k != "r_pressure_winter"}, ocean)
    with pytest.raises(ValueError, match="r_northZ has 99 values"):
        PD.compute_precipitation(p, xyz, e, dict(wind, r_northZ=np.zeros(n - 1, np.float32)), ocean)
    with pytest.raises(ValueError, match="r_ocean_warmth_winter"):
        PD.compute_precipitation(p, xyz, e, wind, {"r_ocean_warmth_summer": ocean["r_ocean_warmth_summer"]})
    with pytest.raises(ValueError, match="r_ocean_warmth_summer has 99 values"):
        PD.compute_precipitation(p, xyz, e, wind, dict(ocean, r_ocean_warmth_summer=np.zeros(n - 1, np.float32)))
    with pytest.raises(ValueError, match="numbers"):
        PD.compute_precipitation(p, xyz, e, wind, ocean, precipitation_offset=float("nan"))
    with pytest.raises(KeyError):
        PD.compute_precipitation(p, xyz, e, wind, ocean, fields=("_precipTiming",))
    with pytest.raises(KeyError):
        PD.download(p, "_precipTiming")
    with pytest.raises(KeyError):
        OD.upload(p, "r_ocean_depth", e)
    assert PD.WIND_INPUTS == tuple(PC.golden_case("precip_config1_N10000_s1")["meta"]["inputs"])[:len(PD.WIND_INPUTS)]
    assert set(PD.WIND_INPUTS) == set(PC.WIND_INPUTS) and PD.OCEAN_INPUTS == PC.OCEAN_INPUTS
    assert [k for k, _ in PD.RESULT_FIELDS] == sorted(k for k in PC.golden_case("precip_config1_N10000_s1")["meta"]["keys"] if k != "_precipTiming")


def test_c_abi_refuses_null_planet():
    """Status 1 and a message that names the entry point, never a dereference."""
    from planet_heightmap_generation_amd import capi
    L = capi.lib()
    a = np.zeros(8, np.float32)
    assert L.wo_compute_precipitation(None, 8, None, 0.0, 0.3, None) != 0 and "wo_compute_precipitation" in capi.last_error()
    assert L.wo_precip_download(None, b"r_precip_summer", capi.ptr(a), 32) != 0 and "wo_precip_download" in capi.last_error()
    assert L.wo_ocean_upload(None, b"r_ocean_warmth_summer", capi.ptr(a), 32) != 0 and "wo_ocean_upload" in capi.last_error()
