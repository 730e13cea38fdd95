"""The arrow overlays on the device (csrc/overlay.hip: wo_overlay_bins, wo_overlay_arrows) against the host emulator of the same bodies
(tests/emu_overlay) in every word, every call twice: the winners of the bins on planets of less than one workgroup and of several,
under contention, with identical positions across wave and workgroup boundaries, with land skipped, and by the test-hook form of
the kernel; the compaction of the arrows with none, all and exactly one bin kept; absent outputs; the error answers of the C ABI;
and both kinds and seasons after the device's own climate chain."""
import ctypes as C
import itertools

import numpy as np
import pytest

import globe_common as GC
import map_common as MC
import overlay_common as OC

pytestmark = pytest.mark.gpu
BLOCK = 256                                                   # regions per workgroup of the bin kernel (csrc/device.h: WO_BLOCK)
SENTINEL = np.float32(-12345.5)


def _planet(mesh, xyz):
    from planet_heightmap_generation_amd import terrain_post as TP
    return TP.Planet(mesh, xyz)


def _in_use():
    from planet_heightmap_generation_amd import capi
    d, h, n = C.c_int64(0), C.c_int64(0), C.c_int64(0)
    assert capi.lib().wo_memory_in_use(C.byref(d), C.byref(h), C.byref(n)) == 0
    return d.value, h.value


def same(a, b):
    return MC.same_bits(np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32))


def _upload(pl, kind, season, fields):
    from planet_heightmap_generation_amd import climate_blocks as CB, ocean, wind
    block, keys = (ocean.BLOCK, OC.OCEAN_KEYS) if kind == OC.OCEAN else (wind.BLOCK, OC.WIND_KEYS)
    for k, a in zip(keys, fields):
        CB.upload(pl, block, k.format(s=season), a)


def _raw_arrows(pl, kind, season, center, e, mask=(True, True, True, True), capacity=OC.BINS):
    """wo_overlay_arrows itself, with buffers that hold a sentinel: -> (status, count, the four buffers or None)"""
    from planet_heightmap_generation_amd import capi
    bufs = [np.full(OC.BINS * 18, SENTINEL, np.float32) if m else None for m in mask]
    count = C.c_int64(-1)
    e = None if e is None else np.ascontiguousarray(e, np.float32)
    rc = capi.lib().wo_overlay_arrows(pl.handle, kind, season, C.c_double(center), capi.ptr(e), *[capi.ptr(b) for b in bufs], capacity, C.byref(count))
    return rc, count.value, bufs


def _check_call(pl, kind, season, xyz, e, fields, center=0.0, what=""):
    """the device's four arrays equal the emulator's, twice, and nothing is written behind them; -> (count, winners)"""
    winners, n, want = OC.emu_call(kind, xyz, e, fields, center)
    for turn in range(2):
        rc, got_n, bufs = _raw_arrows(pl, kind, season, center, e if kind == OC.OCEAN else None)
        assert rc == 0 and got_n == n, (what, rc, got_n, n)
        for b, w in zip(bufs, want):
            assert same(b[: n * 18], w), (what, turn)
            assert (b[n * 18:].view(np.uint32) == SENTINEL.view(np.uint32)).all(), (what, "written behind count")
    return n, winners


def three_bins(n, seed=3):
    """n positions, all of them in the bins (30, 60), (30, 61) and (45, 10): region r lies in bin r % 3"""
    rng = np.random.default_rng(seed)
    cells = np.array([(30, 60), (30, 61), (45, 10)])[np.arange(n) % 3]
    lat = np.radians(-90 + 3 * cells[:, 0] + rng.uniform(0.05, 2.95, n))
    lon = np.radians(-180 + 3 * cells[:, 1] + rng.uniform(0.05, 2.95, n))
    return np.stack([np.sin(lon) * np.cos(lat), np.sin(lat), np.cos(lon) * np.cos(lat)], axis=1).astype(np.float32)


def plant_pairs(xyz, rounds_up):
    """Three pairs of identical positions, each the closest of its bin and of the rounding kind asked for, at indices that a
    workgroup boundary (255 / 256), the two ends of the planet (0 / N - 1) and a wave boundary (63 / 64) separate.
    -> (xyz, the index the reference's loop leaves per pair)"""
    xyz = xyz.copy()
    n = xyz.shape[0]
    idx, d2 = OC.emu_candidates(xyz)
    up = OC.round_kinds(d2)
    pairs = [(255, 256), (0, n - 1), (63, 64)]
    taken = set(i for p in pairs for i in p)
    expect = []
    for (lo, hi), b in zip(pairs, np.unique(idx)):
        mine = np.array([r for r in np.flatnonzero(idx == b) if r not in taken])
        order = mine[np.argsort(d2[mine])]
        k = next(k for k, r in enumerate(order) if up[r] == rounds_up)
        far, point = xyz[order[-1]].copy(), xyz[order[k]].copy()
        xyz[order[: k + 1]] = far                             # nothing of the other kind lies closer, and the pair has no third copy
        xyz[lo] = xyz[hi] = point
        expect.append((b, hi if rounds_up else lo))
    return xyz, expect


# ---- 1. the winners ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["257", "10k", "10k three bins"])
def test_winners_equal_the_emulator(shape, monkeypatch):
    from planet_heightmap_generation_amd import overlay_export as OE
    mesh, xyz = GC.small_sphere(257) if shape == "257" else MC.golden_mesh("mesh_N10000_s1")
    n = mesh.numRegions
    xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    if shape == "10k three bins":
        xyz = three_bins(n)
    assert (n < BLOCK + 2) if shape == "257" else (n > 30 * BLOCK and n % BLOCK != 0)      # less than two workgroups; several and a partial one
    e = GC.rough_elevation(xyz, 5)
    want = OC.emu_winners(xyz)
    assert np.array_equal(want, OC.emu_winners(xyz, form="loop"))
    occupied = int((want >= 0).sum())
    print(f"{shape}: {n} regions, {occupied} bins occupied")
    assert occupied == 3 if shape == "10k three bins" else occupied > n // 2
    pl = _planet(mesh, xyz)
    try:
        own = _in_use()
        for turn in range(2):
            assert np.array_equal(OE.grid_regions(pl), want), turn
        # the ocean form: land is skipped, a NaN elevation is not; from the caller's field and from the resident one
        want_ocean = OC.emu_winners(xyz, e, True)
        assert np.isnan(e).any() and not np.array_equal(want_ocean, want)
        assert np.array_equal(OE.grid_regions(pl, True, e), want_ocean)
        pl.upload(e)
        assert np.array_equal(OE.grid_regions(pl, True), want_ocean) and np.array_equal(OE.grid_regions(pl, False), want)
        assert np.array_equal(OE.grid_regions(pl, True, np.ones(n, np.float32)), np.full(OC.BINS, -1, np.int32))           # all land
        assert np.array_equal(OE.grid_regions(pl, True, np.full(n, -0.5, np.float32)), want)                               # all ocean
        nan = np.ones(n, np.float32)
        nan[want[want >= 0][0]] = np.nan                                                                                 # one region that is no land
        got = OE.grid_regions(pl, True, nan)
        assert np.array_equal(got, OC.emu_winners(xyz, nan, True)) and int((got >= 0).sum()) == 1
        # the other form of the kernel: a candidate reads the bin's key before it sends its atomic
        monkeypatch.setenv("WO_TEST_HOOKS", "overlay_precheck=1")
        assert np.array_equal(OE.grid_regions(pl), want) and np.array_equal(OE.grid_regions(pl, True, e), want_ocean)
        monkeypatch.delenv("WO_TEST_HOOKS")
        assert _in_use() == own
    finally:
        pl.close()


@pytest.mark.parametrize("rounds_up", [True, False])
def test_identical_positions_across_wave_and_workgroup_boundaries(rounds_up, monkeypatch):
    from planet_heightmap_generation_amd import overlay_export as OE
    mesh, _ = MC.golden_mesh("mesh_N10000_s1")
    n = mesh.numRegions
    xyz, expect = plant_pairs(three_bins(n), rounds_up)
    want = OC.emu_winners(xyz, form="loop")
    for b, r in expect:
        assert want[b] == r, (b, r, want[b])                  # the last copy where d2 rounds up, the first where it does not
    assert np.array_equal(OC.emu_winners(xyz), want)
    pl = _planet(mesh, xyz)
    try:
        for hook in (None, "overlay_precheck=1"):
            if hook:
                monkeypatch.setenv("WO_TEST_HOOKS", hook)
            for turn in range(2):
                assert np.array_equal(OE.grid_regions(pl), want), (hook, turn)
    finally:
        pl.close()


def test_crafted_positions_on_the_device():
    from planet_heightmap_generation_amd import overlay_export as OE
    mesh, _ = MC.golden_mesh("mesh_N2000_s1")
    c = OC.crafted()
    pl = _planet(mesh, c["xyz"])
    try:
        assert np.array_equal(OE.grid_regions(pl), c["gridRegions"]) and np.array_equal(OE.grid_regions(pl), c["gridRegions"])
    finally:
        pl.close()


# ---- 2. the arrows -------------------------------------------------------------------------------------------------------------------
def test_golden_arrows_on_the_device():
    """the reference's own arrays from the device: both kinds, the centre meridians of the golden"""
    from planet_heightmap_generation_amd import overlay_export as OE
    g = OC.golden()
    mesh, xyz = MC.golden_mesh("mesh_N2000_s1")
    meta = g["meta"]
    pl = _planet(mesh, xyz)
    try:
        pl.upload(g["r_elevation"])
        _upload(pl, OC.WIND, meta["windSeason"], OC.golden_fields(OC.WIND, meta["windSeason"]))
        _upload(pl, OC.OCEAN, meta["oceanSeason"], OC.golden_fields(OC.OCEAN, meta["oceanSeason"]))
        wind = OE.wind_arrows(pl, meta["windSeason"], meta["windCenterLon"])
        ocean = OE.ocean_current_arrows(pl, meta["oceanSeason"], meta["oceanCenterLon"])
        for pre, got in (("wind", wind), ("ocean", ocean)):
            assert got["count"] == meta["calls"][pre]["count"]
            for form, k in itertools.product(("globe", "map"), ("position", "color")):
                assert same(got[form][k], g[f"{pre}_{form}_{k}"]), (pre, form, k)
        assert same(OE.wind_arrows(pl, meta["windSeason"], meta["windCCenterLon"])["map"]["position"], g["wind_c_map_position"])
        assert np.array_equal(OE.grid_regions(pl), g["wind_gridRegions"]) and np.array_equal(OE.grid_regions(pl, True), g["ocean_gridRegions"])
    finally:
        pl.close()


def test_arrows_and_the_compaction():
    mesh, xyz = MC.golden_mesh("mesh_N10000_s1")
    xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    n = mesh.numRegions
    winners = OC.emu_winners(xyz)
    occupied = np.flatnonzero(winners >= 0)
    assert occupied.size > 5000 and occupied[0] < BLOCK and occupied[-1] >= OC.BINS - 64           # the first and the last chunk of the arrow pass
    smooth_e, smooth_n = (0.3 * MC.fbm_like(xyz, 21)).astype(np.float32), (0.3 * MC.fbm_like(xyz, 22)).astype(np.float32)
    cases = {"no bin kept": (np.zeros(n, np.float32), np.zeros(n, np.float32), 0), "every occupied bin kept": (np.full(n, 0.1, np.float32), np.zeros(n, np.float32), occupied.size)}
    for what, b in (("only the first occupied bin kept", occupied[0]), ("only the last occupied bin kept", occupied[-1])):
        f = np.zeros(n, np.float32)
        f[winners[b]] = -0.2
        cases[what] = (np.zeros(n, np.float32), f, 1)
    special = smooth_e.copy()
    special[winners[occupied[5]]], special[winners[occupied[70]]] = np.nan, np.inf            # a NaN speed is kept
    cases["smooth fields with a NaN and an infinite speed"] = (special, smooth_n, None)
    pl = _planet(mesh, xyz)
    try:
        _upload(pl, OC.WIND, "summer", [smooth_e, smooth_n])      # the two blocks are the planet's, not temporaries of a call
        _upload(pl, OC.OCEAN, "winter", [smooth_e])
        own = _in_use()
        for what, (fe, fn, count) in cases.items():
            for season in (0, 1):
                _upload(pl, OC.WIND, OC.SEASONS[season], [fe, fn])
                got, _ = _check_call(pl, OC.WIND, season, xyz, None, [fe, fn], center=0.0 if season == 0 else -2.5, what=what)
                print(f"{what} ({OC.SEASONS[season]}): {got} arrows")
                assert count is None or got == count, (what, got, count)
        # the ocean form on the same planet: its own bins (land skipped), its own thresholds and colours
        e = GC.rough_elevation(xyz, 5)
        fields = [smooth_e, smooth_n, np.abs(smooth_e) * 0.2, MC.fbm_like(xyz, 23).astype(np.float32)]
        _upload(pl, OC.OCEAN, "winter", fields)
        got, ocean_winners = _check_call(pl, OC.OCEAN, 1, xyz, e, fields, center=2.5, what="ocean")
        assert 0 < got < int((ocean_winners >= 0).sum()) < occupied.size
        rc, all_land, _ = _raw_arrows(pl, OC.OCEAN, 1, 0.0, np.ones(n, np.float32))
        assert rc == 0 and all_land == 0
        pl.upload(e)                                          # the resident elevation gives the same arrows
        rc, resident, bufs = _raw_arrows(pl, OC.OCEAN, 1, 2.5, None)
        assert rc == 0 and resident == got and same(bufs[0][: got * 18], OC.emu_call(OC.OCEAN, xyz, e, fields, 2.5)[2][0])
        assert _in_use() == own
    finally:
        pl.close()


def test_absent_outputs():
    """every combination of NULL output pointers gives the count and the arrays that were asked for"""
    mesh, xyz = GC.small_sphere(257)
    xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    fe, fn = (0.3 * MC.fbm_like(xyz, 21)).astype(np.float32), (0.3 * MC.fbm_like(xyz, 22)).astype(np.float32)
    _, n, want = OC.emu_call(OC.WIND, xyz, None, [fe, fn], 1.0)
    assert n > 100
    pl = _planet(mesh, xyz)
    try:
        _upload(pl, OC.WIND, "summer", [fe, fn])
        own = _in_use()
        for mask in itertools.product((True, False), repeat=4):
            rc, got, bufs = _raw_arrows(pl, OC.WIND, 0, 1.0, None, mask, capacity=OC.BINS if any(mask) else 0)
            assert rc == 0 and got == n, (mask, rc, got)
            for b, w in zip(bufs, want):
                assert b is None or (same(b[: n * 18], w) and (b[n * 18:].view(np.uint32) == SENTINEL.view(np.uint32)).all()), mask
        assert _in_use() == own
    finally:
        pl.close()


# ---- 3. the error answers ------------------------------------------------------------------------------------------------------------
def test_refusals_allocate_nothing_and_leave_the_planet_usable():
    from planet_heightmap_generation_amd import capi, overlay_export as OE
    L = capi.lib()
    mesh, xyz = GC.small_sphere(257)
    xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    n = mesh.numRegions
    out = np.empty(OC.BINS, np.int32)
    fe = np.full(n, 0.1, np.float32)

    def refused(rc, *want):
        msg = capi.last_error()
        print(f"    status {rc}: {msg}")
        assert rc == 1 and all(w in msg for w in want), (rc, msg, want)

    pl = _planet(mesh, xyz)
    try:
        own = _in_use()
        refused(L.wo_overlay_bins(None, 0, None, capi.ptr(out)), "wo_overlay_bins", "null planet")
        refused(L.wo_overlay_bins(pl.handle, 0, None, None), "wo_overlay_bins", "null pointer")
        refused(L.wo_overlay_bins(pl.handle, 2, None, capi.ptr(out)), "wo_overlay_bins", "skipLand is 2")
        for kind in (-1, 2):
            refused(_raw_arrows(pl, kind, 0, 0.0, None)[0], "wo_overlay_arrows", f"unknown arrow kind {kind}")
        for season in (-1, 2):
            refused(_raw_arrows(pl, OC.WIND, season, 0.0, None)[0], "wo_overlay_arrows", f"unknown season {season}")
        for season in (0, 1):
            refused(_raw_arrows(pl, OC.WIND, season, 0.0, None)[0], "wo_overlay_arrows", "no wind result", "wo_compute_wind first", f"r_wind_east_{OC.SEASONS[season]}")
            refused(_raw_arrows(pl, OC.OCEAN, season, 0.0, None)[0], "wo_overlay_arrows", "no ocean result", "wo_compute_ocean_currents first", f"r_ocean_speed_{OC.SEASONS[season]}")
        with pytest.raises(capi.WorogenError, match="no wind result"):
            OE.wind_arrows(pl, "summer")
        with pytest.raises(ValueError, match="unknown season"):
            OE.wind_arrows(pl, "spring")
        assert _in_use() == own                               # nothing was allocated by a refused call
        # one field of two is no wind result for the arrows; the other season stays refused
        _upload(pl, OC.WIND, "summer", [fe])
        with_block = _in_use()
        refused(_raw_arrows(pl, OC.WIND, 0, 0.0, None)[0], "wo_overlay_arrows", "no wind result")
        _upload(pl, OC.WIND, "summer", [fe, fe])
        refused(_raw_arrows(pl, OC.WIND, 1, 0.0, None)[0], "wo_overlay_arrows", "no wind result")
        refused(_raw_arrows(pl, OC.WIND, 0, 0.0, None, capacity=OC.BINS - 1)[0], "wo_overlay_arrows", f"can give {OC.BINS} arrows", f"capacityArrows is {OC.BINS - 1}")
        refused(L.wo_overlay_arrows(pl.handle, 0, 0, C.c_double(0.0), None, None, None, None, None, 0, None), "wo_overlay_arrows", "null pointer")
        assert _in_use() == with_block
        # after all of it the planet gives what the emulator gives, and every temporary is gone again
        _check_call(pl, OC.WIND, 0, xyz, None, [fe, fe], what="after the refusals")
        rc, count, bufs = _raw_arrows(pl, OC.WIND, 0, float("nan"), None)                      # a NaN centre meridian counts as 0
        assert rc == 0 and same(bufs[2][: count * 18], OC.emu_call(OC.WIND, xyz, None, [fe, fe], 0.0)[2][2])
        assert np.array_equal(OE.grid_regions(pl), OC.emu_winners(xyz))
        assert _in_use() == with_block
    finally:
        pl.close()


# ---- 4. after the device's own climate chain -----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def imported():
    """importHeightmap's fixture left resident, then the climate chain on the device"""
    import import_common as IC
    from planet_heightmap_generation_amd import heightmap_import as HI
    g = IC.golden()
    imp = IC.meta(g)["import"]
    img = g["img_512x256"]
    keep = []
    d = HI.import_heightmap(imp["N"], imp["jitter"], img, img.shape[1], img.shape[0], imp["params"], seed=imp["seed"], planet_out=keep)
    pl = keep[0]
    MC.climate_chain(pl, d["r_plate"], d["plateIsOcean"], d["seed"])
    yield dict(planet=pl, xyz=np.ascontiguousarray(d["r_xyz"], np.float32).reshape(-1, 3), e=pl.download())
    pl.close()


def test_arrows_after_the_climate_chain(imported):
    """both kinds and both seasons from the resident blocks equal the emulator on the downloaded fields, word for word"""
    from planet_heightmap_generation_amd import ocean, overlay_export as OE, wind
    pl, xyz, e = imported["planet"], imported["xyz"], imported["e"]
    seen = set()
    for kind, mod, keys in ((OC.WIND, wind, OC.WIND_KEYS), (OC.OCEAN, ocean, OC.OCEAN_KEYS)):
        for season in OC.SEASONS:
            fields = [mod.download(pl, k.format(s=season)) for k in keys]
            _, n, want = OC.emu_call(kind, xyz, e, fields, 0.5)
            got = OE.wind_arrows(pl, season, 0.5) if kind == OC.WIND else OE.ocean_current_arrows(pl, season, 0.5)
            print(f"{'ocean' if kind else 'wind'} {season}: {n} arrows")
            assert got["count"] == n > 500
            for a, w in zip((got["globe"]["position"], got["globe"]["color"], got["map"]["position"], got["map"]["color"]), want):
                assert same(a, w), (kind, season)
            seen.add(got["globe"]["position"].tobytes())
    assert len(seen) == 4
    line = OE.itcz(pl, "summer")
    assert line["globe"].size == 360 * 6 and np.isfinite(line["globe"]).all() and same(line["globe"], OE.itcz_line(wind.download(pl, "itczLons"), wind.download(pl, "itczLatsSummer"))["globe"])
