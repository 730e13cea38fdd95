"""computeWind (js/wind.js:394-687) without a GPU: the host emulator of csrc/wind_ops.h (tests/emu_wind drives the very bodies the
kernels of csrc/wind.hip run) against the reference's goldens, the order-free parts under several thread orders, the percentile
select, the sensitivity of the outputs to the platform's exp / sin / cos, and the Python argument checks.

The device itself is held to the same goldens in test_gpu_wind.py."""
import numpy as np
import pytest

import wind_common as WC


@pytest.mark.parametrize("name", WC.GOLDEN_CASES)
def test_emulator_matches_reference(name):
    """Every output of the reference, on the bar of wind_common (the exact fields bit for bit)."""
    case = WC.golden_case(name)
    ref = case["ref"]
    assert set(ref) == {k for k, _ in WC.result_fields()} == set(case["meta"]["keys"]) - {"_windTiming"}
    if "ocean" not in name and "land" not in name:
        far = 8 if case["N"] >= 10_000 else 0               # a planet of 64 cells has no land eight hops from the sea: there, a coast at all
        assert np.ptp(ref["r_pressure_summer"]) > 10 and ref["r_wind_speed_winter"].max() == 1.0 and ref["r_coastDistLand"].max() >= far
    out = WC.emulate(case)
    print(f"{name}: BFS levels (coast, plates) {out['_levels']}")
    WC.compare_golden(name, out, case)


def test_edge_planet_values_need_no_reference():
    """Cells exactly at the poles, on the date line and at lon = +-pi/2 (no Fibonacci planet has one): latitude, longitude and the
    fallback frame from f64 numpy, every output finite, the coast distance from a plain host BFS.  The same check runs on the
    device in test_gpu_wind.py."""
    case = WC.golden_case("wind_N2000_edges_s1")
    WC.check_edge_values("emulator", WC.emulate(case), case)
    # the fixture reaches what it is there for: the bins before their clamp (js/wind.js:95-100) are 36 and 72 at the north pole and at
    # lon = +pi, and -1 at the south pole and at lon = -pi (fl32(pi) lies above pi)
    lat, lon = case["ref"]["r_lat"].astype(np.float64), case["ref"]["r_lon"].astype(np.float64)
    assert np.floor((lat + np.pi / 2) / np.pi * 36).max() == 36 and np.floor((lon + np.pi) / (2 * np.pi) * 72).max() == 72
    assert np.floor((lat + np.pi / 2) / np.pi * 36).min() == -1 and np.floor((lon + np.pi) / (2 * np.pi) * 72).min() == -1
    land = case["e"] > 0
    c = WC.edge_cells(case)
    moved = np.unique(np.concatenate(list(c.values())))
    assert land[moved].any() and not land[moved].all() and abs(land.mean() - 0.315) < 0.002, "the moved cells lie on both sides of the coast"


def test_shape_planets_sit_on_the_launch_boundaries():
    """64, 256, 257 and 4 097 cells: one wave, one 256-thread block, one block and a cell, one 4 096-pair radix tile and a pair."""
    assert [WC.golden_case(f"wind_N{n}_shape_s1")["N"] for n in (63, 255, 256, 4096)] == [64, 256, 257, 4097]


def test_degenerate_planets():
    """All ocean: no land, no coast, both continentalities zero.  All land: no ocean cell, so no main ocean (label -1) and both
    distance fields stay -1."""
    for name, land in (("wind_N2000_ocean_s1", 0), ("wind_N2000_land_s1", 1)):
        case = WC.golden_case(name)
        label, main, coast, plate = WC.emulate_graph(case)
        assert (coast == -1).all() and (plate == -1).all()
        assert main == (-1 if land else 0) and ((label == -1).all() if land else (label == 0).all())
        assert (case["ref"]["r_isLand"] == land).all() and (case["ref"]["r_coastDistLand"] == -1).all()
        assert not case["ref"]["r_continentality"].any() and not case["ref"]["r_plateContinentality"].any()


def _irregular_cases():
    import elev_inputs as EI
    return {"hub": lambda: EI.hub_case(20_000), "row_shuffled": lambda: EI.relabelled_case(20_000)}


@pytest.mark.parametrize("which", ["wind_config1_N10000_s1", "wind_import_N10000_s1", "hub", "row_shuffled"])
def test_labeller_and_bfs_are_order_independent(which):
    """Hooks, flattening and the claims inside a BFS level in four different orders (the interleavings of the device's threads):
    the same labels, the same main ocean and the same two distance fields; on the goldens the coast distance is the reference's."""
    if which.startswith("wind_"):
        case = WC.golden_case(which)
    else:
        ec = _irregular_cases()[which]()
        case = WC.case_from_elev(ec, WC.plate_mask_elevation(ec, seed=11))
    base = WC.emulate_graph(case, 0)
    ocean = case["e"] <= 0
    assert (base[0][ocean] >= 0).all() and (base[0][~ocean] == -1).all()
    if not which.startswith("wind_"):
        sizes = np.bincount(base[0][ocean])
        assert np.count_nonzero(sizes) > 10 and base[1] == int(np.argmax(sizes)), "the stand-in terrain should have lakes beside its main ocean"
    for seed in (1, 2, 3):
        got = WC.emulate_graph(case, seed)
        assert np.array_equal(got[0], base[0]) and got[1] == base[1], f"labels differ under order {seed}"
        assert np.array_equal(got[2], base[2]) and np.array_equal(got[3], base[3]), f"distances differ under order {seed}"
    if which.startswith("wind_"):
        assert np.array_equal(base[2], case["ref"]["r_coastDistLand"])
    if which == "wind_import_N10000_s1":
        sizes = np.bincount(base[0][ocean])
        assert np.count_nonzero(sizes) > 3 and ((base[2] == -1) & ~ocean).any(), "this planet has lakes, and land the main ocean does not reach"


def test_main_ocean_tie_goes_to_the_smallest_first_cell():
    """Two oceans of equal size on a ring: the reference's `size > mainOceanSize` keeps the one found first."""
    n = 40
    i = np.arange(n)
    adj = np.stack([(i - 1) % n, (i + 1) % n], 1).reshape(-1).astype(np.int32)
    off = np.arange(0, 2 * n + 1, 2, dtype=np.int32)
    e = np.full(n, 0.5, np.float32)
    e[5:12] = -1
    e[25:32] = -1
    case = WC.make_case("ring", WC.Mesh(off, adj), np.zeros(3 * n, np.float32), e, np.zeros(n, np.int32), np.zeros(0, np.int32))
    for seed in range(4):
        label, main, coast, _ = WC.emulate_graph(case, seed)
        assert main == 5 and set(label[e <= 0]) == {5, 25}
        assert coast[4] == 0 and coast[12] == 0 and coast[18] == 6 and coast[24] == 12 and coast[32] == 12 and coast[0] == 4


@pytest.mark.parametrize("kind", ["ties", "zeros", "random", "two_values", "with_inf"])
def test_percentile_select(kind):
    """percentile(speed, 0.95) (js/climate-util.js:103-110): the value at index floor(0.95 n) of the ascending order, `|| 1`."""
    rng = np.random.default_rng(5)
    for n in (1, 2, 19, 20, 21, 1000, 65537):
        if kind == "ties":
            v = rng.integers(0, 4, n).astype(np.float32) * np.float32(0.25)
        elif kind == "zeros":
            v = np.zeros(n, np.float32)
        elif kind == "random":
            v = (rng.random(n) ** 4).astype(np.float32)
        elif kind == "two_values":
            v = np.where(rng.random(n) < 0.95, np.float32(1e-30), np.float32(3e38)).astype(np.float32)
        else:
            v = rng.random(n).astype(np.float32)
            v[rng.random(n) < 0.1] = np.inf
        want = float(np.sort(v)[int(np.floor(0.95 * n))]) or 1.0
        assert WC.emu_percentile(v) == want, (kind, n)
    assert WC.emu_percentile(np.zeros(777, np.float32)) == 1.0


@pytest.mark.parametrize("name", WC.GOLDEN_CASES)
def test_libm_sensitivity(name):
    """Every exp / sin / cos of the bodies moved by K = 4 double ulps (all up, all down, two hashed draws): the number of cells of
    any output that change must stay under a tenth of the cap of the bar, so that ocml's own (2-ulp) differences cannot use the
    cap up.  The figures are recorded in DESIGN section 3."""
    case = WC.golden_case(name)
    base = WC.emulate(case, libm_hook=True)
    WC.compare_golden(f"{name} (hook build, K = 0)", base, case)
    worst = {}
    for seed in (1, 2, 77, 4242):
        got = WC.emulate(case, perturb=(seed, WC.HOOK_K))
        calls = got["_libm_calls"]
        assert calls[1] > 0 and calls[2] > 0 and calls[3] > 0, "the hook was not reached"
        for k, _ in WC.result_fields():
            n = int((got[k].view(np.uint8) != base[k].view(np.uint8)).reshape(base[k].size, -1).any(axis=1).sum())
            worst[k] = max(worst.get(k, 0), n)
    print(f"{name}: cells changed by +-{WC.HOOK_K} ulps of libm, worst of 4 draws: { {k: v for k, v in worst.items() if v} or 'none' }")
    assert max(worst.values()) * 10 <= WC.diff_cap(case["N"]), worst


class _NoDevicePlanet:
    """Stands where a Planet would: any use of its handle is a use of the device."""
    numRegions = 100

    @property
    def handle(self):
        raise AssertionError("device work was started")


def test_python_argument_checks_refuse_before_device_work():
    from planet_heightmap_generation_amd import wind as WD
    p, n = _NoDevicePlanet(), 100
    xyz, e, plate = np.zeros(3 * n, np.float32), np.zeros(n, np.float32), np.zeros(n, np.int32)
    with pytest.raises(ValueError, match="r_xyz"):
        WD.compute_wind(p, xyz[:-3], e, {1}, plate, 1)
    with pytest.raises(ValueError, match="r_elevation"):
        WD.compute_wind(p, xyz, e[:-1], {1}, plate, 1)
    with pytest.raises(ValueError, match="r_plate"):
        WD.compute_wind(p, xyz, e, {1}, plate[:-1], 1)
    with pytest.raises(ValueError, match="r_plate"):
        WD.compute_wind(p, xyz, e, {1}, None, 1)
    with pytest.raises(TypeError, match="r_plate"):
        WD.compute_wind(p, xyz, e, {1}, plate.astype(np.float32), 1)
    with pytest.raises(TypeError, match="plate_is_ocean"):
        WD.compute_wind(p, xyz, e, {1.5}, plate, 1)
    with pytest.raises(ValueError, match="numbers"):
        WD.compute_wind(p, xyz, e, {1}, plate, float("nan"))
    with pytest.raises(ValueError, match="numbers"):
        WD.compute_wind(p, xyz, e, {1}, plate, 1, axial_tilt=float("nan"))
    with pytest.raises(ValueError, match="expected 100"):
        WD.compute_gradients(p, e[:-1], e, e, e, e, e, e)
    with pytest.raises(KeyError):
        WD.download(p, "_windTiming")
    assert [k for k, _ in WD.RESULT_FIELDS] == [k for k in WC.golden_case("wind_config1_N10000_s1")["meta"]["keys"] if k != "_windTiming"]
    assert WD.smoothstep(0, 2000, 1000) == 0.5 and WD.smoothstep(1, 1, 1) == 1 and WD.smoothstep(1, 1, 0.5) == 0 and WD.smoothstep(90, 60, 75) == 0.5


def test_c_abi_refuses_null_planet():
    """Status 1 and a message that names the entry point, never a dereference."""
    from planet_heightmap_generation_amd import capi
    L = capi.lib()
    a = np.zeros(8, np.int32)
    assert L.wo_compute_wind(None, 8, None, capi.ptr(a), None, 0, 1.0, 23.5, None) != 0 and "wo_compute_wind" in capi.last_error()
    assert L.wo_wind_download(None, b"r_lat", capi.ptr(a), 32) != 0 and "wo_wind_download" in capi.last_error()
    assert L.wo_compute_gradients(None, 8, None, None, None, None, None) != 0 and "wo_compute_gradients" in capi.last_error()
