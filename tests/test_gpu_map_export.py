"""Map export on the device (csrc/map.hip) against the host emulator of the same bodies (tests/emu_map): the region map and its
counts in every pixel, the RGBA of all six kinds, the map block's memory, and the error answers of the C ABI; on the sweep planet
(every Koppen class with every elevation of the golden's colour sweep) also against the pixels the reference's recorded colours
give; and the climate chain with the map export on planets in flight against the same jobs one after the other."""
import ctypes as C

import numpy as np
import pytest

import map_common as MC

pytestmark = pytest.mark.gpu


def _planet(mesh, xyz):
    from planet_heightmap_generation_amd import terrain_post as TP
    return TP.Planet(mesh, xyz)


def _in_use():
    from planet_heightmap_generation_amd import capi
    d, h, n = C.c_int64(0), C.c_int64(0), C.c_int64(0)
    assert capi.lib().wo_memory_in_use(C.byref(d), C.byref(h), C.byref(n)) == 0
    return d.value, h.value


def _small_planet():
    from planet_heightmap_generation_amd import sphere_mesh as S
    mesh, xyz, _ = S.build_sphere(256, 0.75, 1)
    return mesh, xyz


def _big_planet():
    from planet_heightmap_generation_amd import sphere_mesh as S
    mesh, xyz, _ = S.build_sphere(200000, 0.75, 3)
    return mesh, xyz


# ---- 5. region map and counts ------------------------------------------------------------------------------------------------
# the box split, the seam and the pole fan occur in every one; at 8192 x 4096 every triangle of the 256-cell planet takes the
# large-box route; 200 000 cells at 4096 x 2048 is the grid and the 64-bit indexing at size.  250 is 250 x 125: the height is width / 2.
CASES = [("N10000", 256), ("N10000", 250), ("N10000", 1024), ("N256", 64), ("N256", 8192), ("N200000", 4096)]


@pytest.mark.parametrize("which,W", CASES)
def test_region_map_equals_emulator(which, W):
    from planet_heightmap_generation_amd import map_export as ME
    mesh, xyz = MC.golden_mesh("mesh_N10000_s1") if which == "N10000" else _small_planet() if which == "N256" else _big_planet()
    want, covered, uncovered = MC.emu_raster(xyz, mesh.triangles, mesh.halfedges, W)
    pl = _planet(mesh, xyz)
    try:
        first = ME.raster(pl, mesh, W, download=True)
        again = ME.raster(pl, mesh, W, download=False)
        resident = ME.download(pl, W)
    finally:
        pl.close()
    print(f"{which} at {W} x {W // 2}: covered {first['covered']}, uncovered {first['uncovered']}")
    assert (first["width"], first["height"]) == (W, W // 2) and first["regionMap"].shape == (W // 2, W)
    bad = int((first["regionMap"] != want).sum())
    assert bad == 0, f"{bad} pixels differ from the emulator"
    assert (first["covered"], first["uncovered"]) == (covered, uncovered) == (again["covered"], again["uncovered"])
    assert np.array_equal(resident, first["regionMap"])                              # the second run's bits


# ---- 6. RGBA of all six types ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def imported():
    """importHeightmap's fixture left resident, then the climate chain on the device"""
    import import_common as IC
    from planet_heightmap_generation_amd import heightmap_import as HI, sphere_mesh as SM
    g = IC.golden()
    imp = IC.meta(g)["import"]
    img = g["img_512x256"]
    keep = []
    d = HI.import_heightmap(imp["N"], imp["jitter"], img, img.shape[1], img.shape[0], imp["params"], seed=imp["seed"], planet_out=keep)
    pl = keep[0]
    mesh = SM.sphere_mesh_from_triangles(d["triangles"], d["halfedges"], d["numRegions"])
    koppen = MC.climate_chain(pl, d["r_plate"], d["plateIsOcean"], d["seed"])
    yield dict(planet=pl, mesh=mesh, xyz=d["r_xyz"], e=pl.download(), koppen=koppen)
    pl.close()


def test_rgba_equals_emulator(imported):
    from planet_heightmap_generation_amd import map_export as ME
    I, W = imported, 1024
    pl, mesh = I["planet"], I["mesh"]
    assert np.array_equal(I["e"], pl.download()) and (I["e"] > 0).any() and (I["e"] <= 0).any() and np.unique(I["koppen"]).size > 5
    rm = ME.raster(pl, mesh, W, download=True)["regionMap"]
    want_rm, _, _ = MC.emu_raster(I["xyz"], mesh.triangles, mesh.halfedges, W)
    assert np.array_equal(rm, want_rm)
    for type in MC.TYPES:
        got = ME.color(pl, type)
        want = MC.emu_rgba(type, I["e"], I["koppen"], mesh.adjOffset, mesh.adjList, want_rm)
        bad = int((got != want).any(axis=-1).sum())
        print(f"{type}: {bad} pixels differ from the emulator; {np.unique(got.reshape(-1, 4), axis=0).shape[0]} distinct colours")
        assert got.shape == (W // 2, W, 4) and bad == 0, type
        assert np.array_equal(ME.color(pl, type, I["e"]), got), type                   # the passed elevation: the same bytes
    res = ME.export_map(pl, mesh, ["heightmap", "koppen"], 64)
    assert list(res["maps"]) == ["heightmap", "koppen"] and res["maps"]["koppen"].shape == (32, 64, 4)


# ---- 6b. the colour sweep: every class with every boundary elevation, against the reference's recorded colours -------------------
@pytest.fixture(scope="module")
def sweep():
    """The sweep planet classified and rastered on the device.  Conditions, asserted from the emulator's raster
    (map_common.sweep_raster): every one of the 10 001 regions owns a pixel at 2048 x 1024, and the device's region map is the
    emulator's in every pixel.  The device takes no class ids, so it classifies lattice rows; the ids 31 and 255 of the golden's
    sweep_k stay with the emulator (tests/test_map_export.py)."""
    from planet_heightmap_generation_amd import koppen as KD, map_export as ME
    S = MC.sweep_planet()
    want_rm, covered, uncovered = MC.sweep_raster()
    pl = _planet(S["mesh"], S["xyz"])
    try:
        classes = KD.classify_koppen(pl, S["e_koppen"], temp_result=S["temp"], precip_result=S["precip"])
        bad = int((classes != S["k"]).sum())
        print(f"sweep planet: {bad} of {classes.size} regions have another class than k = r % 31")
        assert bad == 0 and np.unique(classes).size == 31
        res = ME.raster(pl, S["mesh"], MC.SWEEP_WIDTH, download=True)
        bad = int((res["regionMap"] != want_rm).sum())
        print(f"sweep planet at {MC.SWEEP_WIDTH} x {MC.SWEEP_WIDTH // 2}: {bad} pixels of the region map differ from the emulator; covered {res['covered']}, uncovered {res['uncovered']}")
        assert bad == 0 and (res["covered"], res["uncovered"]) == (covered, uncovered)
        yield dict(S, planet=pl, rm=want_rm)
    finally:
        pl.close()


@pytest.mark.parametrize("type", MC.TYPES)
def test_sweep_rgba_equals_emulator_and_recorded_colours(sweep, type):
    """Bytes in every pixel: against emu_rgba, against the expectation built in numpy from the golden's recorded sweep colours,
    its table and its background alone (for biome with the smoothing restated in numpy), and the resident elevation against the
    passed one."""
    from planet_heightmap_generation_amd import map_export as ME
    pl, rm, W = sweep["planet"], sweep["rm"], MC.SWEEP_WIDTH
    got = ME.color(pl, type, sweep["e_sweep"])
    emu = MC.emu_rgba(type, sweep["e_sweep"], sweep["k"], sweep["mesh"].adjOffset, sweep["mesh"].adjList, rm)
    want = MC.sweep_expected(type, rm)
    assert got.shape == emu.shape == want.shape == (W // 2, W, 4)
    bad_emu, bad_ref = int((got != emu).any(axis=-1).sum()), int((got != want).any(axis=-1).sum())
    print(f"{type}: {bad_emu} pixels differ from the emulator, {bad_ref} from the reference-built expectation; {np.unique(got.reshape(-1, 4), axis=0).shape[0]} distinct colours")
    for r in np.unique(rm[(got != want).any(axis=-1) & (rm >= 0)])[:6]:
        y, x = np.argwhere(rm == r)[0]
        print(f"    region {int(r)}: class {int(sweep['k'][r])}, elevation {float(sweep['e_sweep'][r])!r}: device {got[y, x].tolist()}, expected {want[y, x].tolist()}")
    assert bad_emu == 0 and bad_ref == 0
    pl.upload(sweep["e_sweep"])
    assert np.array_equal(ME.color(pl, type), got)                                      # the resident elevation: the same bytes


# ---- 6c. planets in flight ---------------------------------------------------------------------------------------------------
def test_climate_and_map_in_flight_match_sequential():
    """Six terrains on one mesh through the five climate stages, the raster and the six colourings, four at a time (own context,
    stream and host thread each; a worker's planet is reused, so every block is also replaced) and one after the other: every
    array of every job is the same, f32 as bits.  The climate blocks and the map block share no mutable state between planets."""
    import wind_common as WC
    from planet_heightmap_generation_amd import koppen as KD, map_export as ME, precipitation as PD, sphere_mesh as SM, temperature as TD
    from planet_heightmap_generation_amd.ensemble import EnsembleRunner
    mesh, xyz, _ = SM.build_sphere(20000, 0.75, 1)
    cases = [WC.synthetic_case(20000, seed=s) for s in (1, 2, 3, 4, 5, 6)]                # the same mesh six times, six terrains
    assert all(np.array_equal(c["xyz"], np.asarray(xyz, np.float32).reshape(-1)) and np.array_equal(c["off"], mesh.adjOffset) for c in cases)

    def job(pl, case):
        pl.upload(case["e"])
        out = dict(koppen=MC.climate_chain(pl, case["plate"], case["ocean"], case["seed"]))
        for k in KD.TEMP_INPUTS:
            out[k] = TD.download(pl, k)
        for k in KD.PRECIP_INPUTS:
            out[k] = PD.download(pl, k)
        assert np.array_equal(out["koppen"], KD.download(pl))
        out["regionMap"] = ME.raster(pl, mesh, 512, download=True)["regionMap"]
        for type in MC.TYPES:
            out["rgba_" + type] = ME.color(pl, type)
        return out

    seq = EnsembleRunner(mesh, xyz, in_flight=1).map(job, cases)
    par = EnsembleRunner(mesh, xyz, in_flight=4).map(job, cases)
    for i, (a, b) in enumerate(zip(seq, par)):
        assert list(a) == list(b) and len(a) == 12
        for k in a:
            assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, (i, k)
            same = np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)) if a[k].dtype == np.float32 else np.array_equal(a[k], b[k])
            assert same, f"terrain {i}: {k} differs between one and four planets in flight"
    for k in seq[0]:
        if k != "regionMap":                                                            # the mesh is shared, so the region map is too
            assert not np.array_equal(seq[0][k], seq[1][k]), k
    assert np.array_equal(seq[0]["regionMap"], seq[1]["regionMap"]) and np.unique(seq[0]["koppen"]).size > 5


# ---- 7. the map block's memory ----------------------------------------------------------------------------------------------
def test_map_block_memory():
    from planet_heightmap_generation_amd import map_export as ME
    start = _in_use()
    mesh, xyz = _small_planet()
    pl = _planet(mesh, xyz)
    try:
        own = _in_use()
        ME.raster(pl, mesh, 256)
        assert _in_use() == (own[0] + 256 * 128 * 4, own[1])
        ME.raster(pl, mesh, 512)                                                       # replaces the map
        assert _in_use() == (own[0] + 512 * 256 * 4, own[1])
        ME.color(pl, "color")
        assert _in_use() == (own[0] + 512 * 256 * 4, own[1])
        ME.free(pl)
        assert _in_use() == own
        ME.raster(pl, mesh, 64)
    finally:
        pl.close()
    assert _in_use() == start


# ---- 8. the error answers ----------------------------------------------------------------------------------------------------
def test_errors_leave_the_planet_usable():
    from planet_heightmap_generation_amd import capi, map_export as ME
    L = capi.lib()
    mesh, xyz = _small_planet()
    tri, he = np.ascontiguousarray(mesh.triangles, np.int32), np.ascontiguousarray(mesh.halfedges, np.int32)
    ns = tri.size
    pl = _planet(mesh, xyz)
    counts = np.zeros(2, np.int64)
    out = np.empty(64 * 32 * 4, np.uint8)

    def refused(rc, *want):
        msg = capi.last_error()
        print(f"    status {rc}: {msg}")
        assert rc == 1 and all(w in msg for w in want), (rc, msg, want)

    try:
        own = _in_use()
        refused(L.wo_map_color(pl.handle, 0, None, capi.ptr(out), out.nbytes), "wo_map_color", "no region map", "wo_map_raster first")
        refused(L.wo_map_download(pl.handle, capi.ptr(out), out.nbytes), "wo_map_download", "no region map")
        for w in (255, 0, 1, -2, 32770):
            refused(L.wo_map_raster(pl.handle, ns, capi.ptr(tri), capi.ptr(he), w, None, capi.ptr(counts)), "wo_map_raster", f"width is {w}", "even and from 2 to 32768")
        refused(L.wo_map_raster(pl.handle, ns - 1, capi.ptr(tri), capi.ptr(he), 64, None, capi.ptr(counts)), "wo_map_raster", f"numSides is {ns - 1}", "multiple of 3")
        bad_he = he.copy()
        bad_he[5] = ns
        refused(L.wo_map_raster(pl.handle, ns, capi.ptr(tri), capi.ptr(bad_he), 64, None, capi.ptr(counts)), "wo_map_raster", "half-edge out of range", "halfedges[5]")
        bad_he[5] = -1
        refused(L.wo_map_raster(pl.handle, ns, capi.ptr(tri), capi.ptr(bad_he), 64, None, capi.ptr(counts)), "wo_map_raster", "half-edge out of range")
        bad_tri = tri.copy()
        bad_tri[7] = mesh.numRegions
        refused(L.wo_map_raster(pl.handle, ns, capi.ptr(bad_tri), capi.ptr(he), 64, None, capi.ptr(counts)), "wo_map_raster", "corner out of range", "triangles[7]")
        assert _in_use() == own                                                         # nothing was allocated by a refused call
        assert L.wo_map_raster(pl.handle, ns, capi.ptr(tri), capi.ptr(he), 64, None, capi.ptr(counts)) == 0
        refused(L.wo_map_color(pl.handle, 0, None, capi.ptr(out), out.nbytes - 4), "wo_map_color", "64 x 32", f"{out.nbytes} bytes", f"rgbaOut has {out.nbytes - 4}")
        refused(L.wo_map_download(pl.handle, capi.ptr(out), out.nbytes + 4), "wo_map_download", f"{out.nbytes} bytes")
        for t in (4, 5):
            refused(L.wo_map_color(pl.handle, t, None, capi.ptr(out), out.nbytes), "wo_map_color", "no Koppen result")
        for t in (-1, 6):
            refused(L.wo_map_color(pl.handle, t, None, capi.ptr(out), out.nbytes), "wo_map_color", f"unknown map type {t}")
        refused(L.wo_map_raster(None, ns, capi.ptr(tri), capi.ptr(he), 64, None, None), "wo_map_raster")
        with pytest.raises(capi.WorogenError, match="no Koppen result"):
            ME.color(pl, "biome", width=64)
        with pytest.raises(ValueError, match="unknown map type"):
            ME.color(pl, "plates", width=64)
        # after all of it the planet rasters and colours as the emulator does
        e = MC.fbm_like(xyz, 9)
        pl.upload(e)
        rm = ME.raster(pl, mesh, 64, download=True)["regionMap"]
        want_rm, _, _ = MC.emu_raster(xyz, tri, he, 64)
        assert np.array_equal(rm, want_rm)
        for type in ("color", "heightmap", "landheightmap", "landmask"):
            assert np.array_equal(ME.color(pl, type), MC.emu_rgba(type, e, np.zeros(e.size, np.uint8), mesh.adjOffset, mesh.adjList, want_rm)), type
    finally:
        pl.close()
