"""computeWind on gfx950 (csrc/wind.hip) through ctypes: against the reference's goldens, and against the host emulator of the same
bodies (tests/emu_wind, itself held to the goldens by test_wind.py) where there are none: 1 M cells of realistic plates, the 200 k
hub mesh, the relabelled row-shuffled mesh and a planet of 10 M cells.  The reference is never the device code.

The bar is wind_common's: integer, flag, latitude / longitude, frame, continentality and ITCZ outputs bit for bit; the season
arrays within 4 * 2^-23 * max(1, |ref|) per cell (1013 for the pressures) and at most max(8, N / 10^4) cells different at all.
Every comparison prints its figures before it asserts."""
from functools import lru_cache

import numpy as np
import pytest

import wind_common as WC

pytestmark = pytest.mark.gpu


def _planet(case):
    from planet_heightmap_generation_amd import terrain_post as TP
    return TP.Planet(WC.Mesh(case["off"], case["adj"]), case["xyz"])


def _device(pl, case, e="host"):
    from planet_heightmap_generation_amd import wind as WD
    return WD.compute_wind(pl, case["xyz"], case["e"] if e == "host" else None, set(case["ocean"].tolist()), case["plate"], case["seed"])


@pytest.mark.parametrize("name", WC.GOLDEN_CASES)
def test_matches_reference(name):
    from planet_heightmap_generation_amd import wind as WD
    case = WC.golden_case(name)
    pl = _planet(case)
    try:
        got = _device(pl, case)
        levels = WD.bfs_levels(pl)
    finally:
        pl.close()
    print(f"{name}: BFS levels (coast, plates) {levels}")
    WC.compare_golden(name, got, case)


def _elev_on_device(ec):
    """The terrain of an elev_inputs case: assignElevation on the device (an input here, checked by its own tests)."""
    import elev_inputs as EI
    from planet_heightmap_generation_amd import terrain_post as TP
    pl = TP.Planet(ec.mesh, ec.xyz, ec.nd)
    try:
        return np.ascontiguousarray(EI.on_device(ec, pl, debug=False)["r_elevation"], np.float32)
    finally:
        pl.close()


@lru_cache(maxsize=None)
def _scale_case(which):
    import elev_inputs as EI
    ec = {"realistic_N1000000": lambda: EI.realistic_case(1_000_000), "hub_N200000_deg24": lambda: EI.hub_case(200_000),
          "relabelled_N200000": lambda: EI.relabelled_case(200_000)}[which]()
    return WC.case_from_elev(ec, _elev_on_device(ec))


@pytest.mark.parametrize("which", ["realistic_N1000000", "hub_N200000_deg24", "relabelled_N200000"])
def test_matches_emulator(which):
    from planet_heightmap_generation_amd import wind as WD
    case = _scale_case(which)
    ref = WC.emulate(case)
    pl = _planet(case)
    try:
        got = _device(pl, case)
        levels = WD.bfs_levels(pl)
    finally:
        pl.close()
    land = case["e"] > 0
    print(f"{which}: land {land.mean():.3f}, BFS levels device {levels} emulator {ref['_levels']}, largest coast distance {int(ref['r_coastDistLand'].max())}")
    assert levels == ref["_levels"]
    WC.compare(which, got, ref, case["N"])


@pytest.mark.parametrize("cells", WC.BOUNDARY_CELLS)
def test_matches_emulator_at_sort_boundaries(cells):
    """Planets whose cell count, the launch shape of every kernel and the pair count of the geo index's radix sort, is exactly one
    tile (4 096), exactly one group of 32 tiles (131 072), and one pair more."""
    from planet_heightmap_generation_amd import wind as WD
    case = WC.boundary_case(cells)
    ref = WC.emulate(case)
    pl = _planet(case)
    try:
        got = _device(pl, case)
        levels = WD.bfs_levels(pl)
    finally:
        pl.close()
    print(f"{cells} cells: land {(case['e'] > 0).mean():.3f}, BFS levels device {levels} emulator {ref['_levels']}")
    assert levels == ref["_levels"]
    WC.compare(f"{cells} cells", got, ref, case["N"])


def test_edge_planet_values_need_no_reference():
    """The check of test_wind.py's test of this name on the device's own outputs (all downloaded through wind_download): the poles,
    the date line, lon = +-pi/2, the fallback frame, finite fields, the coast distance of a plain host BFS; then the ocean stage on
    the resident block: every output finite."""
    from planet_heightmap_generation_amd import ocean as OD, wind as WD
    case = WC.golden_case("wind_N2000_edges_s1")
    pl = _planet(case)
    try:
        _device(pl, case, e="host")
        got = {k: WD.download(pl, k) for k, _ in WC.result_fields()}
        sea = OD.compute_ocean_currents(pl, case["xyz"], case["e"])
    finally:
        pl.close()
    WC.check_edge_values("device", got, case)
    for k, v in sea.items():
        assert np.isfinite(v).all(), k
    assert np.abs(sea["r_ocean_current_east_summer"]).max() > 0.5


def test_libm_sensitivity_1m():
    """The perturbed emulator at 1 M cells (K = 4 double ulps; all up, all down, two hashed draws): cells of any output that change,
    against a tenth of the cap.  DESIGN section 3 records the counts."""
    case = _scale_case("realistic_N1000000")
    base = WC.emulate(case, libm_hook=True)
    worst = {}
    for seed in (1, 2, 77, 4242):
        got = WC.emulate(case, perturb=(seed, WC.HOOK_K))
        for k, _ in WC.result_fields():
            n = int((got[k].view(np.uint8) != base[k].view(np.uint8)).reshape(base[k].size, -1).any(axis=1).sum())
            worst[k] = max(worst.get(k, 0), n)
    print(f"1 M cells: cells changed by +-{WC.HOOK_K} ulps of libm, worst of 4 draws: { {k: v for k, v in worst.items() if v} or 'none' }; "
          f"a tenth of the cap is {WC.diff_cap(case['N']) // 10}")
    assert max(worst.values()) * 10 <= WC.diff_cap(case["N"]), worst


def test_resident_elevation_equals_host_pointer():
    """Elevation left on the device by erode_composite_resident, then computeWind with a NULL elevation pointer: bit for bit what the
    host-pointer form gives on the downloaded field."""
    case = WC.golden_case("wind_config1_N10000_s1")
    pl = _planet(case)
    try:
        pl.upload(case["e"], (case["e"] <= 0).astype(np.uint8))
        pl.erode_composite_resident(4, 3e-4, 0.5, 1.0, 2, 1.16, 0.015, 0, 0.0)
        res = _device(pl, case, e="resident")
        e = pl.download()
        assert not np.array_equal(e, case["e"]), "the erosion changed nothing"
        host = _device(pl, dict(case, e=np.ascontiguousarray(e, np.float32)))
    finally:
        pl.close()
    for k, _ in WC.result_fields():
        assert WC.same_bits(res[k], host[k]), k
    assert (res["r_isLand"] == (e > 0)).all()


def test_second_call_equals_fresh_planet():
    """Another elevation (and other ocean plates) on the same planet: what a fresh planet gives.  No table keyed to the first
    call's land mask, plates or percentile survives."""
    a = WC.golden_case("wind_config1_N10000_s1")
    imp = WC.golden_case("wind_import_N10000_s1")          # the same cells (positions), rows in another order: its terrain and plates on a's mesh
    assert np.array_equal(a["xyz"], imp["xyz"])
    other = dict(a, name="import terrain on config 1's mesh", e=imp["e"], plate=imp["plate"], ocean=imp["ocean"])
    pl = _planet(a)
    try:
        first = _device(pl, a)
        second = _device(pl, other)
        again = _device(pl, a)
    finally:
        pl.close()
    fresh = _planet(other)
    try:
        want = _device(fresh, other)
    finally:
        fresh.close()
    for k, _ in WC.result_fields():
        assert WC.same_bits(second[k], want[k]), k
        assert WC.same_bits(again[k], first[k]), k
    assert not WC.same_bits(second["r_isLand"], first["r_isLand"])
    WC.compare("second call", second, WC.emulate(other), other["N"])


def test_compute_gradients_and_argument_checks():
    """wo_compute_gradients on caller arrays reproduces the stage's own gradient (through pressureToWind's inverse it cannot be read
    back, so: the emulator's bodies on the golden pressure); mis-sized arguments fail with a message and leave the planet usable."""
    from planet_heightmap_generation_amd import capi, wind as WD
    case = WC.golden_case("wind_config1_N10000_s1")
    ref = case["ref"]
    pl = _planet(case)
    try:
        L = capi.lib()
        assert L.wo_wind_download(pl.handle, b"r_lat", capi.ptr(np.zeros(4, np.float32)), 16) != 0 and "no wind result" in capi.last_error()
        assert L.wo_compute_wind(pl.handle, case["N"] - 1, None, capi.ptr(case["plate"]), None, 0, 1.0, 23.5, None) != 0 and "numRegions" in capi.last_error()
        assert L.wo_compute_wind(pl.handle, case["N"], None, None, None, 0, 1.0, 23.5, None) != 0 and "r_plate" in capi.last_error()
        assert L.wo_compute_wind(pl.handle, case["N"], None, capi.ptr(case["plate"]), None, 3, 1.0, 23.5, None) != 0
        got = _device(pl, case)
        assert L.wo_wind_download(pl.handle, b"r_lat", capi.ptr(np.zeros(4, np.float32)), 16) != 0 and "bytes" in capi.last_error()
        assert L.wo_wind_download(pl.handle, b"nope", capi.ptr(np.zeros(4, np.float32)), 16) != 0 and "unknown field" in capi.last_error()
        p = (ref["r_pressure_summer"].astype(np.float64) + 1013).astype(np.float32)
        ge, gn = WD.compute_gradients(pl, p, *(ref[k] for k in ("r_eastX", "r_eastY", "r_eastZ", "r_northX", "r_northY", "r_northZ")))
    finally:
        pl.close()
    WC.compare_golden("after refused calls", got, case)
    # numpy restatement of js/wind.js:306-339 in f64
    off, adj, xyz = case["off"], case["adj"], case["xyz"].reshape(-1, 3).astype(np.float64)
    row = np.repeat(np.arange(case["N"]), np.diff(off))
    d = xyz[adj] - xyz[row]
    E = np.stack([ref["r_eastX"], ref["r_eastY"], ref["r_eastZ"]], 1).astype(np.float64)
    Nn = np.stack([ref["r_northX"], ref["r_northY"], ref["r_northZ"]], 1).astype(np.float64)
    de, dn, dp = (d * E[row]).sum(1), (d * Nn[row]).sum(1), p[adj].astype(np.float64) - p[row].astype(np.float64)
    sEP, sEE, sNP, sNN = (np.bincount(row, w, case["N"]) for w in (de * dp, de * de, dn * dp, dn * dn))
    assert np.allclose(ge, np.where(sEE > 1e-12, sEP / sEE, 0), rtol=1e-5, atol=1e-6) and np.allclose(gn, np.where(sNN > 1e-12, sNP / sNN, 0), rtol=1e-5, atol=1e-6)
    assert np.abs(ge).max() > 0.1


REFERENCE_MS_1M = 4693.8            # the reference's computeWind under Node 12 on wind_common.synthetic_case(1 000 000)


def test_faster_than_the_reference_at_1m():
    """The one pass / fail condition on speed: the device stage at 1 M cells takes less wall time than the reference under Node on
    the same planet (the second call on a planet: the first also allocates the wind block)."""
    import time
    from planet_heightmap_generation_amd import wind as WD
    case = WC.synthetic_case(1_000_000)
    pl = _planet(case)
    try:
        ms = []
        for _ in range(2):
            t0 = time.perf_counter()
            WD.compute_wind(pl, None, case["e"], case["ocean"], case["plate"], case["seed"], fields=())
            ms.append((time.perf_counter() - t0) * 1e3)
        levels = WD.bfs_levels(pl)
    finally:
        pl.close()
    print(f"computeWind at 1 M cells: {ms[0]:.1f} ms (first call), {ms[1]:.1f} ms; BFS levels {levels}; the reference under Node: {REFERENCE_MS_1M:.0f} ms")
    assert ms[1] < REFERENCE_MS_1M


def _ten_million_case():
    """10 M cells: wind_common.synthetic_case with the terrain made on the device."""
    from planet_heightmap_generation_amd import sphere_mesh as S, terrain_post as TP
    mesh, xyz, nd = S.build_sphere(10_000_000, 0.75, 1)
    pl = TP.Planet(mesh, xyz, nd)
    try:
        pl.synthetic_terrain(3)
        e = pl.download()
    finally:
        pl.close()
    return WC.synthetic_case(10_000_000, 3, e=e)


@pytest.mark.isolated
@pytest.mark.timeout(900)
def test_ten_million_cells():
    """Finite fields, r_coastDistLand equal to a host BFS, and the device against the emulator on the bar, at 10 M cells."""
    from planet_heightmap_generation_amd import wind as WD
    case = _ten_million_case()
    pl = _planet(case)
    try:
        got = _device(pl, case)
        levels = WD.bfs_levels(pl)
    finally:
        pl.close()
    for k, _ in WC.result_fields():
        assert np.isfinite(got[k]).all(), k
    _, _, coast, _ = WC.emulate_graph(case)
    print(f"10 M cells: land {float((case['e'] > 0).mean()):.3f}, BFS levels (coast, plates) {levels}, largest coast distance {int(coast.max())}")
    assert np.array_equal(got["r_coastDistLand"], coast)
    assert levels[0] == int(coast.max()) + 1
    ref = WC.emulate(case)
    WC.compare("10 M cells", got, ref, case["N"])
