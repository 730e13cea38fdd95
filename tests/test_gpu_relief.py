"""Relief export on the device (csrc/relief.hip) against the host emulator of the same bodies (tests/emu_relief), in every bit: the f32
height map with its NaN positions, both 16-bit kinds, and both normal spaces with and without FLAT_OCEAN, on the map and on the cube,
on the small-box and the large-box routes of the rasters; the region map and counts against the plain rasters; the rules of the map
block; the error answers of the C ABI; and the resident elevation against the same field passed by pointer."""
import numpy as np
import pytest

import map_common as MC
import relief_common as RC

pytestmark = pytest.mark.gpu


def _planet(mesh, xyz):
    from planet_heightmap_generation_amd import terrain_post as TP
    return TP.Planet(mesh, xyz)


def _small_planet():
    from planet_heightmap_generation_amd import sphere_mesh as S
    mesh, xyz, _ = S.build_sphere(256, 0.75, 1)
    return mesh, xyz


def _mesh(which):
    return MC.golden_mesh("mesh_N10000_s1") if which == "N10000" else MC.golden_mesh("mesh_N2000_s1") if which == "N2000" else _small_planet()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else a.dtype)


def _products(RE, pl):
    """everything the device makes of the resident relief"""
    out = dict(heights=RE.heights(pl), height16=RE.height16(pl, "height16"), landHeight16=RE.height16(pl, "landHeight16"))
    for space in RE.NORMAL_KINDS:
        for flat in (False, True):
            out[(space, flat)] = RE.normals(pl, space, 1.0, flat)
    return out


def _expected(h, center_lon):
    out = dict(heights=h, height16=RC.emu_height16(0, h), landHeight16=RC.emu_height16(1, h))
    for k, space in enumerate(("normal", "normalObject")):
        for flat in (False, True):
            out[(space, flat)] = RC.emu_normals(h, k, 1.0, int(flat), center_lon)
    return out


def _compare(tag, got, want, uncovered):
    for key, w in want.items():
        g = got[key]
        assert g.shape == w.shape and g.dtype == w.dtype, (tag, key, g.shape, w.shape)
        if key == "heights":
            assert np.array_equal(np.isnan(g), np.isnan(w)), (tag, "NaN positions")
            bad = int(((_bits(g) != _bits(w)) & ~np.isnan(w)).sum())
            assert (_bits(g)[uncovered] == 0x7FC00000).all(), (tag, "the NaN of an uncovered pixel")
        else:
            bad = int((g != w).sum())
        print(f"{tag} {key}: {bad} of {w.size} values differ from the emulator")
        assert bad == 0, (tag, key, bad)


# 256 and 250 (odd boxes, a height that is no power of two) and a centre meridian are the small route with the seam and the pole fan
# in every one; at 2048 x 1024 every triangle of the 256-cell planet takes the large-box route and has thousands of pixels, plain
# and around a centre meridian
MAP_CASES = [("N10000", 256, 0.0), ("N10000", 250, 0.0), ("N10000", 256, 1.0), ("N256", 2048, 0.0), ("N256", 2048, 1.0)]
# 64 and 50 are the small route; S = 1 is six pixels whose four neighbours all lie on other faces; 2 000 cells at 1024 is the list
CUBE_CASES = [("N10000", 64), ("N10000", 50), ("N10000", 1), ("N2000", 1024)]


@pytest.mark.parametrize("which,W,center_lon", MAP_CASES)
def test_map_relief_equals_emulator(which, W, center_lon):
    from planet_heightmap_generation_amd import map_export as ME, relief_export as RE
    mesh, xyz = _mesh(which)
    e = RC.field(xyz, 11, nans=min(7, mesh.numRegions // 40))
    side, region, h = RC.emu_map(xyz, mesh.triangles, mesh.halfedges, W, center_lon, e)
    want = _expected(h, center_lon)
    pl = _planet(mesh, xyz)
    try:
        plain = ME.raster(pl, mesh, W, download=True, center_lon=center_lon)
        first = RE.raster(pl, mesh, W, e, center_lon, download=True)
        assert ME.map_dims(pl) == (W, W // 2) and first["heights"].shape == (W // 2, W)
        assert np.array_equal(ME.download(pl), plain["regionMap"]) and np.array_equal(plain["regionMap"], region)
        assert (first["covered"], first["uncovered"]) == (plain["covered"], plain["uncovered"]) == (int((side != RC.NO_SIDE).sum()), int((side == RC.NO_SIDE).sum()))
        got = _products(RE, pl)
        assert np.array_equal(_bits(first["heights"]), _bits(got["heights"]))
        _compare(f"{which} {W} x {W // 2} around {center_lon}", got, want, side == RC.NO_SIDE)
        again = RE.raster(pl, mesh, W, e, center_lon)                 # the second run's bits
        assert again["heights"] is None and (again["covered"], again["uncovered"]) == (first["covered"], first["uncovered"])
        second = _products(RE, pl)
        assert all(np.array_equal(_bits(second[k]), _bits(got[k])) for k in got)
    finally:
        pl.close()
    assert np.isnan(e).any() and np.isnan(h[side != RC.NO_SIDE]).any() and (h > 0).any() and (h < 0).any()


@pytest.mark.parametrize("which,S", CUBE_CASES)
def test_cube_relief_equals_emulator(which, S):
    from planet_heightmap_generation_amd import map_export as ME, relief_export as RE
    mesh, xyz = _mesh(which)
    e = RC.field(xyz, 12, nans=7)
    side, region, h = RC.emu_cube(xyz, mesh.triangles, mesh.halfedges, S, e)
    want = _expected(h, 0.0)
    pl = _planet(mesh, xyz)
    try:
        plain = ME.raster_cube(pl, mesh, S, download=True)
        first = RE.raster_cube(pl, mesh, S, e, download=True)
        assert ME.map_dims(pl) == (S, 6 * S) and first["heights"].shape == (6, S, S)
        assert np.array_equal(ME.download(pl), plain["regionMap"]) and np.array_equal(plain["regionMap"], region)
        assert (first["covered"], first["uncovered"]) == (plain["covered"], plain["uncovered"]) == (6 * S * S, 0)
        got = _products(RE, pl)
        assert np.array_equal(_bits(first["heights"]), _bits(got["heights"]))
        _compare(f"{which} 6 x {S} x {S}", got, want, side == RC.NO_SIDE)
        RE.raster_cube(pl, mesh, S, e)                                # the second run's bits
        second = _products(RE, pl)
        assert all(np.array_equal(_bits(second[k]), _bits(got[k])) for k in got)
    finally:
        pl.close()
    assert S == 1 or np.isnan(h).any()


# ---- the resident elevation ---------------------------------------------------------------------------------------------------------
def test_resident_elevation_gives_the_pointers_bits():
    from planet_heightmap_generation_amd import relief_export as RE
    mesh, xyz = MC.golden_mesh("mesh_N2000_s1")
    e = RC.field(xyz, 5, nans=3)
    pl = _planet(mesh, xyz)
    try:
        pl.upload(e)
        for raster in (lambda **k: RE.raster(pl, mesh, 128, center_lon=0.5, download=True, **k), lambda **k: RE.raster_cube(pl, mesh, 24, download=True, **k)):
            by_pointer = raster(r_elevation=e)["heights"]
            p16, pn = RE.height16(pl), RE.normals(pl)
            resident = raster()["heights"]
            assert np.array_equal(_bits(by_pointer), _bits(resident)) and np.isnan(resident).any()
            assert np.array_equal(p16, RE.height16(pl)) and np.array_equal(pn, RE.normals(pl))
            other = raster(r_elevation=e + np.float32(0.125))["heights"]
            assert not np.array_equal(_bits(other), _bits(resident))
    finally:
        pl.close()


# ---- the map block -------------------------------------------------------------------------------------------------------------------
def _no_relief(pl):
    from planet_heightmap_generation_amd import capi, relief_export as RE
    for call in (lambda: RE.heights(pl), lambda: RE.height16(pl), lambda: RE.normals(pl)):
        with pytest.raises(capi.WorogenError, match="no relief raster"):
            call()


def test_block_rules():
    from planet_heightmap_generation_amd import map_export as ME, relief_export as RE
    mesh, xyz = MC.golden_mesh("mesh_N2000_s1")
    e = RC.field(xyz, 3)
    pl = _planet(mesh, xyz)
    try:
        pl.upload(e)
        _no_relief(pl)                                         # a planet without a map
        ME.raster(pl, mesh, 64)
        want_colour = ME.color(pl, "color")
        _no_relief(pl)                                         # a map without a relief
        RE.raster(pl, mesh, 64)
        h64 = RE.heights(pl)
        assert h64.shape == (32, 64) and RE.height16(pl).shape == (32, 64) and RE.normals(pl).shape == (32, 64, 4)
        assert np.array_equal(ME.color(pl, "color"), want_colour)          # the region map serves the colours as before
        for plain in (lambda: ME.raster(pl, mesh, 64), lambda: ME.raster(pl, mesh, 64, center_lon=0.3), lambda: ME.raster_cube(pl, mesh, 16)):
            RE.raster(pl, mesh, 64)
            RE.heights(pl)
            plain()                                            # any plain raster ends the relief, at the same size too
            _no_relief(pl)
            ME.color(pl, "color")                              # while colouring still works
        ME.raster(pl, mesh, 64)
        assert np.array_equal(ME.color(pl, "color"), want_colour)
        RE.raster(pl, mesh, 128)                               # another size replaces both maps
        assert ME.map_dims(pl) == (128, 64) and RE.heights(pl).shape == (64, 128) and ME.download(pl).shape == (64, 128)
        RE.raster_cube(pl, mesh, 16)                           # and the other projection
        assert ME.map_dims(pl) == (16, 96) and RE.heights(pl).shape == (6, 16, 16) and RE.normals(pl, "normalObject").shape == (6, 16, 16, 4)
        RE.raster(pl, mesh, 64)
        assert np.array_equal(_bits(RE.heights(pl)), _bits(h64))
        ME.free(pl)                                            # drops both
        assert ME.map_dims(pl) == (0, 0)
        _no_relief(pl)
        with pytest.raises(Exception, match="no region map"):
            ME.color(pl, "color")
    finally:
        pl.close()


def test_export_relief_and_file_names():
    from planet_heightmap_generation_amd import relief_export as RE
    mesh, xyz = MC.golden_mesh("mesh_N2000_s1")
    e = RC.field(xyz, 3)
    pl = _planet(mesh, xyz)
    try:
        res = RE.export_relief(pl, mesh, RE.KINDS, width=64, r_elevation=e, center_lon=0.25, strength=2.0, flat_ocean=True)
        _, _, h = RC.emu_map(xyz, mesh.triangles, mesh.halfedges, 64, 0.25, e)
        assert list(res["maps"]) == list(RE.KINDS) and res["width"] == 64 and "heights" not in res
        assert np.array_equal(res["maps"]["landHeight16"], RC.emu_height16(1, h)) and np.array_equal(res["maps"]["normal"], RC.emu_normals(h, 0, 2.0, 1, 0.25))
        res = RE.export_relief(pl, mesh, "normalObject", face_size=8, projection="cube", r_elevation=e)
        _, _, h = RC.emu_cube(xyz, mesh.triangles, mesh.halfedges, 8, e)
        assert res["faceSize"] == 8 and np.array_equal(res["maps"]["normalObject"], RC.emu_normals(h, 1))
        with pytest.raises(ValueError):
            RE.export_relief(pl, mesh, "heightmap", width=64)
        with pytest.raises(ValueError):
            RE.export_relief(pl, mesh, "normal", width=64, projection="cylinder")
    finally:
        pl.close()
    assert RE.relief_filename("height16", 42) == "orogen-height16-42.png" and RE.relief_filename("normalObject", 7, "nz") == "orogen-cube-normal-object-nz-7.png"


# ---- the error answers ----------------------------------------------------------------------------------------------------------------
def test_bad_arguments_change_nothing():
    from planet_heightmap_generation_amd import capi, map_export as ME, relief_export as RE
    L = capi.lib()
    mesh, xyz = MC.golden_mesh("mesh_N2000_s1")
    tri, he = np.ascontiguousarray(mesh.triangles, np.int32), np.ascontiguousarray(mesh.halfedges, np.int32)
    ns = tri.size
    counts = np.zeros(2, np.int64)
    pl = _planet(mesh, xyz)

    def refused(rc, *want):
        msg = capi.last_error()
        print(f"    status {rc}: {msg}")
        assert rc == 1 and all(w in msg for w in want), (rc, msg, want)

    try:
        pl.upload(RC.field(xyz, 4))
        RE.raster(pl, mesh, 32)
        before = dict(colour=ME.color(pl, "heightmap"), h=RE.heights(pl), h16=RE.height16(pl), n=RE.normals(pl))
        refused(L.wo_relief_raster(pl.handle, ns, capi.ptr(tri), capi.ptr(he), 33, 0.0, None, None, capi.ptr(counts)), "wo_relief_raster", "width is 33", "even")
        refused(L.wo_relief_raster(pl.handle, ns, capi.ptr(tri), capi.ptr(he), 32, 4.0, None, None, capi.ptr(counts)), "wo_relief_raster", "centerLon")
        refused(L.wo_relief_raster(pl.handle, ns - 1, capi.ptr(tri), capi.ptr(he), 32, 0.0, None, None, capi.ptr(counts)), "wo_relief_raster", "multiple of 3")
        for size in (0, 16385):
            refused(L.wo_relief_raster_cube(pl.handle, ns, capi.ptr(tri), capi.ptr(he), size, None, None, capi.ptr(counts)), "wo_relief_raster_cube", f"faceSize is {size}", "from 1 to 16384")
        refused(L.wo_relief_raster_cube(pl.handle, ns, None, capi.ptr(he), 8, None, None, capi.ptr(counts)), "wo_relief_raster_cube", "null pointer")
        rgba, h16, h = np.empty((16, 32, 4), np.uint8), np.empty((16, 32), np.uint16), np.empty((16, 32), np.float32)
        for strength in (-1.0, float("nan"), float("inf")):
            refused(L.wo_relief_normals(pl.handle, 0, strength, 0, capi.ptr(rgba), rgba.nbytes), "wo_relief_normals", "strength", "finite and not negative")
        refused(L.wo_relief_normals(pl.handle, 2, 1.0, 0, capi.ptr(rgba), rgba.nbytes), "wo_relief_normals", "unknown space 2")
        refused(L.wo_relief_normals(pl.handle, 0, 1.0, 2, capi.ptr(rgba), rgba.nbytes), "wo_relief_normals", "unknown flags 2")
        refused(L.wo_relief_normals(pl.handle, 0, 1.0, 0, capi.ptr(rgba), rgba.nbytes - 4), "wo_relief_normals", "32 x 16", f"out has {rgba.nbytes - 4}")
        refused(L.wo_relief_normals(pl.handle, 0, 1.0, 0, None, rgba.nbytes), "wo_relief_normals", "null pointer")
        refused(L.wo_relief_height16(pl.handle, 2, capi.ptr(h16), h16.nbytes), "wo_relief_height16", "unknown kind 2")
        refused(L.wo_relief_height16(pl.handle, -1, capi.ptr(h16), h16.nbytes), "wo_relief_height16", "unknown kind -1")
        refused(L.wo_relief_height16(pl.handle, 0, capi.ptr(h16), h16.nbytes * 2), "wo_relief_height16", f"out has {h16.nbytes * 2}")
        refused(L.wo_relief_download(pl.handle, capi.ptr(h), h.nbytes + 4), "wo_relief_download", f"out has {h.nbytes + 4}")
        assert L.wo_relief_download(None, capi.ptr(h), h.nbytes) != 0
        assert ME.map_dims(pl) == (32, 16)                     # the planet kept what it had, and is paintable
        after = dict(colour=ME.color(pl, "heightmap"), h=RE.heights(pl), h16=RE.height16(pl), n=RE.normals(pl))
        assert all(np.array_equal(_bits(before[k]), _bits(after[k])) for k in before)
    finally:
        pl.close()
