"""computeOceanCurrents on gfx950 (csrc/ocean.hip) through ctypes: against the reference's goldens by two routes (the device's own
wind block; the golden's stored wind inputs uploaded to a fresh planet, which separates an ocean fault from a wind fault), and
against the host emulator of the same bodies (tests/emu_ocean, itself held to the goldens by test_ocean.py) where there are no
goldens: the 200 k hub mesh (rows of degree 24), the relabelled row-shuffled mesh and a planet of 1 M cells (threshold 35, 70
levels, 6 and 45 passes).  The reference is never the device code.

The bar is bit equality on all eight outputs.  Every comparison prints its figures before it asserts."""
from functools import lru_cache

import numpy as np
import pytest

import ocean_common as OC
import wind_common as WC

pytestmark = pytest.mark.gpu


def _planet(case):
    from planet_heightmap_generation_amd import terrain_post as TP
    return TP.Planet(WC.Mesh(case["off"], case["adj"]), case["xyz"])


def _wind(pl, case, fields=()):
    from planet_heightmap_generation_amd import wind as WD
    return WD.compute_wind(pl, case["xyz"], case["e"], set(case["ocean"].tolist()), case["plate"], case["seed"], fields=fields)


def _ocean(pl, case, wind_result=None):
    from planet_heightmap_generation_amd import ocean as OD
    got = OD.compute_ocean_currents(pl, case["xyz"], case["e"], wind_result)
    return got, OD.info(pl)


@pytest.mark.parametrize("name", OC.GOLDEN_CASES)
def test_matches_reference_after_device_wind(name):
    """computeWind on the device, then the stage on the resident wind block."""
    case = OC.golden_case(name)
    pl = _planet(case)
    try:
        _wind(pl, case)
        got, info = _ocean(pl, case)
    finally:
        pl.close()
    print(f"{name}: {info}")
    OC.assert_golden(f"{name} (device wind)", got, case)
    assert not OC.info_matches_log(info, case["meta"])


@pytest.mark.parametrize("name", OC.GOLDEN_CASES)
def test_matches_reference_from_uploaded_wind(name):
    """The reference's own wind outputs uploaded to a planet that never ran computeWind."""
    from planet_heightmap_generation_amd import capi
    case = OC.golden_case(name)
    pl = _planet(case)
    try:
        got, info = _ocean(pl, case, case["wind"])
        # a block filled by uploads is no wind result: a field that was never set is not served
        assert capi.lib().wo_wind_download(pl.handle, b"r_sinLat", capi.ptr(np.zeros(case["N"], np.float32)), 4 * case["N"]) != 0 and "no wind result" in capi.last_error()
        from planet_heightmap_generation_amd import wind as WD
        assert WC.same_bits(WD.download(pl, "r_lon"), np.ascontiguousarray(case["wind"]["r_lon"], np.float32))
    finally:
        pl.close()
    OC.assert_golden(f"{name} (uploaded wind)", got, case)
    assert not OC.info_matches_log(info, case["meta"])


@lru_cache(maxsize=None)
def _scale_case(which):
    import elev_inputs as EI
    if which == "synthetic_N1000000":
        return WC.synthetic_case(1_000_000)
    ec = {"hub_N200000_deg24": lambda: EI.hub_case(200_000), "relabelled_N200000": lambda: EI.relabelled_case(200_000)}[which]()
    return WC.case_from_elev(ec, WC.plate_mask_elevation(ec, seed=11))


@pytest.mark.parametrize("which", ["hub_N200000_deg24", "relabelled_N200000", "synthetic_N1000000"])
def test_matches_emulator(which):
    """The device against the emulator fed the device's own wind result."""
    case = _scale_case(which)
    pl = _planet(case)
    try:
        wind = _wind(pl, case, fields=OC.WIND_INPUTS)
        got, info = _ocean(pl, case)
    finally:
        pl.close()
    ref = OC.emulate(case, wind)
    ocean = wind["r_isLand"] == 0
    print(f"{which}: ocean {ocean.mean():.3f}, largest degree {int(np.diff(case['off']).max())}, device {info}, reached by the west / east field "
          f"{int((ref['_dist'][0] >= 0).sum())} / {int((ref['_dist'][1] >= 0).sum())} cells")
    assert info == ref["_info"]
    assert (ref["_dist"][0] >= 0).sum() > 1000 and (ref["_dist"][1] >= 0).sum() > 1000 and np.abs(ref["r_ocean_warmth_summer"]).max() > 0.05
    if which == "synthetic_N1000000":
        assert (info["coastThreshold"], info["warmthRange"], info["currentSmoothPasses"], info["warmthSmoothPasses"]) == (35, 70, 6, 45)
    if which == "hub_N200000_deg24":
        assert int(np.diff(case["off"]).max()) >= 24
    OC.assert_equal(which, got, ref)


@pytest.mark.parametrize("cells", WC.BOUNDARY_CELLS)
def test_matches_emulator_at_sort_boundaries(cells):
    """The planets of test_gpu_wind.py's test of this name (4 096, 131 072 and 131 073 cells): the device against the emulator fed
    the device's own wind result."""
    case = WC.boundary_case(cells)
    pl = _planet(case)
    try:
        wind = _wind(pl, case, fields=OC.WIND_INPUTS)
        got, info = _ocean(pl, case)
    finally:
        pl.close()
    ref = OC.emulate(case, wind)
    print(f"{cells} cells: device {info}, reached by the west / east field {int((ref['_dist'][0] >= 0).sum())} / {int((ref['_dist'][1] >= 0).sum())} cells")
    assert info == ref["_info"]
    assert (ref["_dist"][0] >= 0).sum() > cells // 100 and (ref["_dist"][1] >= 0).sum() > cells // 100 and np.abs(ref["r_ocean_warmth_summer"]).max() > 0.05
    OC.assert_equal(f"{cells} cells", got, ref)


def test_second_call_equals_fresh_planet():
    """Another terrain through computeWind on the same planet, then the stage again: what a fresh planet gives.  A repeat of the
    first pair of calls gives the first result."""
    a = OC.golden_case("ocean_config1_N10000_s1")
    imp = OC.golden_case("ocean_import_N10000_s1")         # the same cells (positions), rows in another order: its terrain and plates on a's mesh
    assert np.array_equal(a["xyz"], imp["xyz"])
    other = dict(a, name="import terrain on config 1's mesh", e=imp["e"], plate=imp["plate"], ocean=imp["ocean"])
    pl = _planet(a)
    try:
        _wind(pl, a)
        first, info1 = _ocean(pl, a)
        repeat, _ = _ocean(pl, a)
        _wind(pl, other)
        second, info2 = _ocean(pl, other)
        _wind(pl, a)
        again, _ = _ocean(pl, a)
    finally:
        pl.close()
    fresh = _planet(other)
    try:
        wind = _wind(fresh, other, fields=OC.WIND_INPUTS)
        want, info3 = _ocean(fresh, other)
    finally:
        fresh.close()
    OC.assert_golden("first call", first, a)
    OC.assert_equal("repeat of the first call", repeat, first)
    OC.assert_equal("second call against a fresh planet", second, want)
    OC.assert_equal("first terrain again", again, first)
    assert info2 == info3 and info2 != info1
    assert not WC.same_bits(second["r_ocean_warmth_summer"], first["r_ocean_warmth_summer"])
    OC.assert_equal("second call against the emulator", second, OC.emulate(other, wind))


def test_refusals_leave_the_planet_usable():
    """No wind block, a partially uploaded block, a wrong numRegions, an unknown download key, a short out, a NULL planet: each
    fails with a message, and the planet still gives the golden afterwards."""
    from planet_heightmap_generation_amd import capi, ocean as OD, wind as WD
    case = OC.golden_case("ocean_N10000_wedge_s1")
    N = case["N"]
    buf = np.zeros(N, np.float32)
    pl = _planet(case)
    try:
        L = capi.lib()
        assert L.wo_compute_ocean_currents(pl.handle, N, None) != 0 and "no wind result" in capi.last_error()
        assert L.wo_ocean_download(pl.handle, b"r_ocean_speed_summer", capi.ptr(buf), buf.nbytes) != 0 and "no ocean result" in capi.last_error()
        for k in OC.WIND_INPUTS[:-1]:                       # everything but itczLatsWinter
            WD.upload(pl, k, case["wind"][k])
        assert L.wo_compute_ocean_currents(pl.handle, N, None) != 0 and "no wind result" in capi.last_error()
        assert L.wo_wind_upload(pl.handle, b"nope", capi.ptr(buf), buf.nbytes) != 0 and "unknown field" in capi.last_error()
        assert L.wo_wind_upload(pl.handle, b"r_lat", capi.ptr(buf), buf.nbytes - 4) != 0 and "bytes" in capi.last_error()
        assert L.wo_wind_upload(pl.handle, b"r_lat", None, buf.nbytes) != 0 and "null pointer" in capi.last_error()
        WD.upload(pl, "itczLatsWinter", case["wind"]["itczLatsWinter"])
        assert L.wo_compute_ocean_currents(pl.handle, N - 1, None) != 0 and "numRegions" in capi.last_error()
        assert L.wo_compute_ocean_currents(None, N, None) != 0 and "wo_compute_ocean_currents" in capi.last_error()
        got, info = _ocean(pl, case)
        assert L.wo_ocean_download(pl.handle, b"nope", capi.ptr(buf), buf.nbytes) != 0 and "unknown field" in capi.last_error()
        assert L.wo_ocean_download(pl.handle, b"r_ocean_speed_summer", capi.ptr(buf), buf.nbytes - 4) != 0 and "bytes" in capi.last_error()
        assert L.wo_ocean_download(None, b"r_ocean_speed_summer", capi.ptr(buf), buf.nbytes) != 0 and "wo_ocean_download" in capi.last_error()
        after = {k: OD.download(pl, k) for k, _ in OC.result_fields()}
    finally:
        pl.close()
    OC.assert_golden("after refused calls", got, case)
    OC.assert_equal("downloads after refused downloads", after, got)
    assert not OC.info_matches_log(info, case["meta"])


REFERENCE_MS_1M = 2693.4            # the reference's computeOceanCurrents under Node 12 on wind_common.synthetic_case(1 000 000)


def test_faster_than_the_reference_at_1m():
    """The one pass / fail condition on speed: the device stage at 1 M cells takes less wall time than the reference under Node on
    the same planet (the second call on a planet: the first also allocates the ocean block)."""
    import time
    from planet_heightmap_generation_amd import ocean as OD
    case = _scale_case("synthetic_N1000000")
    pl = _planet(case)
    try:
        _wind(pl, case)
        ms = []
        for _ in range(2):
            t0 = time.perf_counter()
            OD.compute_ocean_currents(pl, None, None, fields=())
            ms.append((time.perf_counter() - t0) * 1e3)
        info = OD.info(pl)
    finally:
        pl.close()
    print(f"computeOceanCurrents at 1 M cells: {ms[0]:.1f} ms (first call), {ms[1]:.1f} ms; {info}; the reference under Node: {REFERENCE_MS_1M:.0f} ms")
    assert ms[1] < REFERENCE_MS_1M


def test_field_by_field_smoothing_gives_the_same_bits(monkeypatch):
    """The A/B route of DESIGN section 8.3 (the masked smoothing as single-field sweeps, the hook ocean_split_smooth) against the
    interleaved kernels: the same eight arrays, on the 250 k planet (3 and 22 passes, the odd count leaves a result in the other
    buffer)."""
    case = OC.golden_case("ocean_N250000_s4")
    pl = _planet(case)
    try:
        base, _ = _ocean(pl, case, case["wind"])
        monkeypatch.setenv("WO_TEST_HOOKS", "ocean_split_smooth")
        split, _ = _ocean(pl, case)
    finally:
        pl.close()
    OC.assert_golden("interleaved smoothing", base, case)
    OC.assert_equal("field-by-field smoothing against the interleaved one", split, base)
