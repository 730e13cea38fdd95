"""Who owns device and pinned memory (csrc/device_mem.h: DeviceArena), checked through wo_memory_in_use: a planet that has
used every lazily built piece gives all of it back on close(), a repeated call allocates nothing, a regrown buffer replaces
the old one, the temporaries of a call are gone when it returns, and a refused call leaves nothing behind.

Every test works with DIFFERENCES from a reading taken at its start (other tests of the process may hold planets).  The
planet is elev_inputs.realistic_case(5000): a mesh-builder sphere with the realistic plates, land and ocean mixed
(wind_common.plate_mask_elevation: continents, lakes, islands).  Only the flood-state regrow needs more cells (see there).
Every test prints its figures before it asserts."""
import gc
from functools import lru_cache

import numpy as np
import pytest

import elev_inputs as EI
import wind_common as WC

pytestmark = pytest.mark.gpu

# hydraulic, K, m, dt, thermal, talus, kThermal, glacial, strength (1.0: ice from 50 degrees of latitude on, 71 land cells of the case)
ERODE = (3, 3e-4, 0.5, 1.0, 3, 1.16, 0.015, 2, 1.0)


def in_use():
    """(device bytes, pinned bytes, allocation calls so far) of the whole process"""
    import ctypes as C
    from planet_heightmap_generation_amd import capi
    d, h, n = C.c_int64(0), C.c_int64(0), C.c_int64(0)
    assert capi.lib().wo_memory_in_use(C.byref(d), C.byref(h), C.byref(n)) == 0
    return np.array([d.value, h.value, n.value], np.int64)


def baseline():
    gc.collect()                      # a planet that an earlier test dropped without close() goes now, not in the middle of this test
    return in_use()


@lru_cache(maxsize=None)
def _case():
    ec = EI.realistic_case(5000)
    e = WC.plate_mask_elevation(ec, 1)
    ocean = np.ascontiguousarray(e <= 0, np.uint8)
    assert 0.15 < 1 - ocean.mean() < 0.85, "land and ocean are not mixed"
    return ec, WC.case_from_elev(ec, e), ocean


def _planet(ec):
    from planet_heightmap_generation_amd import terrain_post as TP
    return TP.Planet(ec.mesh, ec.xyz, ec.nd)


def _image(W, H):
    y, x = np.mgrid[0:H, 0:W]
    return np.ascontiguousarray((128 + 100 * np.sin(x * 6.283 / W * 3) * np.cos(y * 3.1416 / H * 2)).astype(np.uint8))


def _wind(pl, wc, ocean_ids=None):
    from planet_heightmap_generation_amd import wind as WD
    ids = wc["ocean"] if ocean_ids is None else ocean_ids
    return WD.compute_wind(pl, wc["xyz"], wc["e"], set(int(i) for i in ids), wc["plate"], wc["seed"], fields=("r_pressure_summer",))


def _resident_round(pl, wc, ocean, monkeypatch):
    """The calls that work on the planet's resident state, each lazily built piece reached: erode scratch, carve buffers, basin
    layout, mirror (and its hotspot copy), radix scratch, flow tiles, the device flood's state, saved state, wind block, ocean
    block, import scratch.  Returns the erode stats of the three erosion calls."""
    from planet_heightmap_generation_amd import heightmap_import as HI, ocean as OD
    stats = []
    for env in ({}, {"WO_LAYOUT": "index"}, {"WO_FLOOD": "device"}):
        with monkeypatch.context() as m:
            for k, v in env.items():
                m.setenv(k, v)
            pl.upload(wc["e"], ocean)
            pl.erode_composite_resident(*ERODE)
            stats.append(pl.last_erode_stats())
    pl.smooth_elevation_resident(2, 0.25)
    pl.sharpen_ridges_resident(2, 0.04)
    pl.apply_soil_creep_resident(3, 0.1125)
    pl.upload_hotspot(np.abs(wc["e"]))
    pl.warp_terrain_resident(1, 0.75, True)
    pl.save_state()
    pl.restore_state()
    _wind(pl, wc)
    OD.compute_ocean_currents(pl, wc["xyz"], wc["e"], fields=("r_ocean_speed_summer",))
    HI.sample_heightmap(pl, _image(64, 32), 64, 32)
    HI.derive_synthetic_plates(pl)
    HI.classify_regions(pl)
    return stats


def _per_call(pl, ec, wc):
    """The calls whose device memory is a temporary of the call; yields (name, live bytes before, live bytes after)"""
    from planet_heightmap_generation_amd import climate_util as CU, terrain_post as TP, wind as WD
    f = np.ascontiguousarray(wc["e"].copy())
    frames = [np.ascontiguousarray(np.roll(wc["xyz"].reshape(-1, 3), k, axis=1)[:, j]) for k in (1, 2) for j in range(3)]
    calls = (("wo_assign_elevation", lambda: EI.on_device(ec, pl, debug=True)),
             ("wo_smooth_field", lambda: CU.smooth_field(ec.mesh, f, 2, planet=pl)),
             ("wo_compute_gradients", lambda: WD.compute_gradients(pl, wc["e"], *frames)),
             ("wo_noise_eval", lambda: TP.noise_eval(1, 1, wc["xyz"].astype(np.float64), ctx=pl.ctx)))
    for name, call in calls:
        before = in_use()
        call()
        yield name, before, in_use()


def test_round_trip_returns_everything(monkeypatch):
    ec, wc, ocean = _case()
    base = baseline()
    pl = _planet(ec)
    try:
        created = in_use() - base
        stats = _resident_round(pl, wc, ocean, monkeypatch)
        for name, before, after in _per_call(pl, ec, wc):
            print(f"{name}: live (device, pinned) {before[:2] - base[:2]} -> {after[:2] - base[:2]}, allocations {after[2] - before[2]}")
        full = in_use() - base
    finally:
        pl.close()
    left = in_use() - base
    print(f"created (device, pinned, allocations) {created}; after the round {full}; after close() {left}")
    for s, what in zip(stats, ("default", "WO_LAYOUT=index", "WO_FLOOD=device")):
        print(f"erode [{what}]: mirror {s['mirror_layout']}, two-level flow {s['flow_two_level']}, carve tasks {s['carve_active_total']}, "
              f"device flood ms {s['flood_device_pass1_ms']}, basin passes {s['solve_basin_passes']}")
    # the round did reach the pieces it is there for
    assert stats[0]["mirror_layout"] == 1 and stats[1]["mirror_layout"] == 0 and stats[0]["flow_two_level"] == 1
    assert stats[0]["carve_active_total"] > 0 and stats[0]["solve_basin_passes"] > 0 and stats[2]["flood_device_rounds"] > 0
    assert full[0] > created[0] > 0 and full[1] > created[1] > 0
    assert left[0] == 0 and left[1] == 0, left


def test_second_round_allocates_nothing(monkeypatch):
    ec, wc, ocean = _case()
    base = baseline()
    pl = _planet(ec)
    try:
        _resident_round(pl, wc, ocean, monkeypatch)
        first = in_use() - base
        _resident_round(pl, wc, ocean, monkeypatch)
        second = in_use() - base
    finally:
        pl.close()
    left = in_use() - base
    print(f"after round 1 (device, pinned, allocations) {first}; after round 2 {second}; after close() {left}")
    assert np.array_equal(first, second), (first, second)          # live bytes AND the allocation count (no entry point of the round is excepted)
    assert left[0] == 0 and left[1] == 0, left


def test_per_call_memory_is_gone_when_the_call_returns():
    ec, wc, ocean = _case()
    base = baseline()
    pl = _planet(ec)
    try:
        pl.upload(wc["e"], ocean)
        seen = list(_per_call(pl, ec, wc))
    finally:
        pl.close()
    left = in_use() - base
    for name, before, after in seen:
        print(f"{name}: live (device, pinned) {before[:2] - base[:2]} -> {after[:2] - base[:2]}, allocations made {after[2] - before[2]}")
    for name, before, after in seen:
        assert after[2] > before[2], f"{name} allocated nothing: not a call this test is about"
        assert np.array_equal(before[:2], after[:2]), (name, before, after)
    assert left[0] == 0 and left[1] == 0, left


def test_regrown_buffers_replace_the_old_ones():
    """The image of the import and the ocean plate ids of the wind block are allocated at exactly the size asked for, so a
    regrow changes the live bytes by new size - old size, to the byte."""
    from planet_heightmap_generation_amd import heightmap_import as HI
    ec, wc, ocean = _case()
    base = baseline()
    pl = _planet(ec)
    try:
        HI.sample_heightmap(pl, _image(64, 32), 64, 32)
        a = in_use()
        HI.sample_heightmap(pl, _image(128, 64), 128, 64)
        b = in_use()
        HI.sample_heightmap(pl, _image(64, 32), 64, 32)              # fits: nothing happens
        c = in_use()
        print(f"import image 64x32 -> 128x64: device bytes {a[0] - base[0]} -> {b[0] - base[0]}, allocations {b[2] - a[2]}; back to 64x32: allocations {c[2] - b[2]}")
        assert b[0] - a[0] == 128 * 64 - 64 * 32 and b[2] - a[2] == 1 and b[1] == a[1]
        assert np.array_equal(b, c)
        ids = np.unique(wc["ocean"])
        assert ids.size >= 5
        _wind(pl, wc, ids[:2])
        a = in_use()
        _wind(pl, wc, ids[:5])
        b = in_use()
        _wind(pl, wc, ids[:3])                                       # fits
        c = in_use()
        print(f"wind, 2 -> 5 ocean plate ids: device bytes {a[0] - base[0]} -> {b[0] - base[0]}, allocations {b[2] - a[2]}; then 3 ids: allocations {c[2] - b[2]}")
        assert b[0] - a[0] == 4 * (5 - 2) and b[2] - a[2] == 1 and b[1] == a[1]
        assert np.array_equal(b, c)
    finally:
        pl.close()
    left = in_use() - base
    assert left[0] == 0 and left[1] == 0, left


@lru_cache(maxsize=None)
def _cap_planet():
    """40 000 cells, land where z is above a threshold: the device flood's state holds L + L / 16 + 1024 cells, so 20 % more land
    outgrows it only from about 7 500 land cells on (0.2 L > L / 16 + 1024)."""
    from planet_heightmap_generation_amd import sphere_mesh as S
    mesh, xyz, nd = S.build_sphere(40000, 0.75, 1)
    z = np.asarray(xyz, np.float32).reshape(-1, 3)[:, 2]
    rough = np.random.default_rng(5).uniform(0, 0.02, z.size).astype(np.float32)      # no two heights equal: the device flood's result is taken
    return mesh, xyz, nd, z, rough


def test_device_flood_state_regrows_in_place(monkeypatch):
    """Every buffer of the device flood's state is proportional to its capacity C = L + L / 16 + 1024 (or to the land's
    adjacency, which grows with the land).  With 20 % more land the new state is 1.2 x the old one: if the old one was released
    the call adds about 0.2 of the first call's growth, if it was kept at least 1.0.  The bound between them: one half."""
    from planet_heightmap_generation_amd import terrain_post as TP
    mesh, xyz, nd, z, rough = _cap_planet()
    order = np.sort(z)[::-1]
    L1, L2 = 12000, 14400
    assert L2 > L1 + L1 // 16 + 1024
    base = baseline()
    pl = TP.Planet(mesh, xyz, nd)
    grown = []
    try:
        for L in (L1, L2):
            t = 0.5 * (order[L - 1] + order[L])
            e = np.ascontiguousarray((z - t) * 0.5 + np.where(z > t, rough, -rough), np.float32)
            oc = np.ascontiguousarray(e <= 0, np.uint8)
            assert int((oc == 0).sum()) == L
            pl.upload(e, oc)
            pl.erode_composite_resident(2, 3e-4, 0.5, 1.0, 0, 1.16, 0.015, 0, 0.0)          # host flood: everything else the call builds
            a = in_use()
            monkeypatch.setenv("WO_FLOOD", "device")
            pl.upload(e, oc)
            pl.erode_composite_resident(2, 3e-4, 0.5, 1.0, 0, 1.16, 0.015, 0, 0.0)
            monkeypatch.delenv("WO_FLOOD")
            s = pl.last_erode_stats()
            b = in_use()
            grown.append(b - a)
            print(f"device flood, {L} land cells: grew by (device, pinned, allocations) {b - a}; rounds {s['flood_device_rounds']}, on host after all {s['flood_pass1_on_host']}")
            assert s["flood_device_rounds"] > 0
    finally:
        pl.close()
    left = in_use() - base
    g1, g2 = grown
    assert g1[0] > 0 and g1[1] > 0 and g2[2] > 1, "the state was not built / did not regrow"
    assert 0 < g2[0] < g1[0] / 2 and 0 < g2[1] < g1[1] / 2, (g1, g2)
    assert left[0] == 0 and left[1] == 0, left


def test_refused_call_leaves_nothing_behind():
    """wo_wind_upload of a known field with the wrong byte count: the wind block is built, then the call returns 1."""
    from planet_heightmap_generation_amd import capi
    ec, wc, ocean = _case()
    base = baseline()
    pl = _planet(ec)
    try:
        created = in_use() - base
        data = np.zeros(ec.N - 1, np.float32)
        rc = capi.lib().wo_wind_upload(pl.handle, b"r_lat", capi.ptr(data), data.nbytes)
        held = in_use() - base
        print(f"wo_wind_upload with {data.nbytes} bytes for r_lat: status {rc} ({capi.last_error()}); live (device, pinned) {created[:2]} -> {held[:2]}")
        assert rc == 1 and "bytes" in capi.last_error()
        assert held[0] > created[0] and held[1] > created[1]          # the block is there (and stays usable)
    finally:
        pl.close()
    left = in_use() - base
    assert left[0] == 0 and left[1] == 0, left
