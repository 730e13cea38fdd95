"""The globe view's contract (csrc/view_ops.h) on the CPU: the host emulator of the shared bodies (tests/emu_view) against the contract
restated in numpy and against a ray cast in 3-D that knows neither the projection nor the culling; the vertices against the globe
mesh's; the per-side rules with the eye close to the surface and with a NaN and an infinite elevation; the shade formula; and the
host module's pieces that need no device."""
import ctypes as C
import math

import numpy as np
import pytest

import globe_common as GC
import view_common as VC


def _same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


# ---- 1. the four shapes --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", VC.CPU_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}-fov{s[3]:g}")
def test_emulator_equals_numpy_and_ray_cast(shape):
    W, H, eye, fov, hh = shape
    mesh, xyz, e = VC.golden_case()
    got = VC.cpu_case(shape)
    want = VC.numpy_raster(xyz, e, mesh.triangles, mesh.halfedges, W, H, eye, fov, hh, 1.0, VC.SUN)
    bad = int((got["regionMap"] != want["regionMap"]).sum())
    print(f"{W} x {H}: covered {got['covered']}, uncovered {got['uncovered']}; {bad} pixels differ from the numpy statement")
    assert bad == 0
    assert _same_bits(got["depth"], want["depth"]) and _same_bits(got["lambert"], want["lambert"])
    assert got["covered"] == int((want["regionMap"] >= 0).sum()) and got["covered"] + got["uncovered"] == W * H
    assert np.array_equal(np.isnan(got["depth"]), got["regionMap"] < 0)                  # NaN exactly where nothing covers
    assert (got["depth"].view(np.uint32)[got["regionMap"] < 0] == VC.NAN_BITS).all()
    rays = VC.ray_cast(xyz, e, mesh.triangles, mesh.halfedges, W, H, eye, fov, hh)
    clear = ~want["ambiguous"]
    bad = int((got["regionMap"] != rays)[clear].sum())
    share = float(want["ambiguous"].mean())
    print(f"{W} x {H}: {bad} unambiguous pixels differ from the ray cast; {share:.3%} of the pixels are ambiguous")
    assert bad == 0
    assert share <= 0.005
    if (W, H) == (33, 64):
        assert got["uncovered"] == 0                          # the planet fills this image


def test_camera_basis():
    for _, _, eye, fov, hh in VC.CPU_SHAPES + [VC.NEAR_EYE, VC.SURFACE_EYE]:
        got, want = VC.emu_camera(eye, fov, hh), VC.numpy_camera(eye, fov, hh)
        for k in ("origin", "x", "y", "z"):
            assert np.array_equal(got[k], want[k]), k
        assert got["f"] == want["f"] and got["ortho"] == want["ortho"]
    pole = VC.emu_camera((0.0, 3.0, 0.0), 0.0, 1.1)
    assert np.array_equal(pole["x"], [1.0, 0.0, 0.0]) and np.array_equal(pole["y"], [0.0, 0.0, -1.0]) and np.array_equal(pole["origin"], [0.0, 10.0, 0.0])
    front = VC.emu_camera((0.0, 0.0, 2.0), 90.0, 1.1)
    assert np.array_equal(front["x"], [1.0, 0.0, 0.0]) and np.array_equal(front["y"], [0.0, 1.0, 0.0]) and abs(front["f"] - 1.0) < 1e-15
    for eye, fov, hh in (((0.0, 0.0, 0.0), 50.0, 1.1), ((math.nan, 0.0, 1.0), 50.0, 1.1), ((math.inf, 0.0, 1.0), 50.0, 1.1), ((0.0, 0.0, 2.0), 180.0, 1.1), ((0.0, 0.0, 2.0), -1.0, 1.1),
                         ((0.0, 0.0, 2.0), math.nan, 1.1), ((0.0, 0.0, 2.0), 0.0, 0.0), ((0.0, 0.0, 2.0), 0.0, math.inf)):
        assert VC.emu_camera(eye, fov, hh) is None, (eye, fov, hh)


# ---- 2. the vertices are the globe mesh's ----------------------------------------------------------------------------------------------
def test_positions_are_the_globe_mesh():
    mesh, xyz, e = VC.golden_case()
    W, H, eye, fov, hh = VC.CPU_SHAPES[0]
    g1 = VC.emu_geometry(xyz, e, mesh.triangles, mesh.halfedges, W, H, eye, fov, hh, 1.0)
    want, _ = GC.emu_positions(xyz, e, mesh.triangles, mesh.halfedges)
    assert _same_bits(g1["positions"].reshape(-1), want)
    assert _same_bits(g1["positions"].reshape(-1, 3, 3), VC.numpy_positions(xyz, e, mesh.triangles, mesh.halfedges, 1.0))
    g0 = VC.emu_geometry(xyz, e, mesh.triangles, mesh.halfedges, W, H, eye, fov, hh, 0.0)
    p0, r = g0["positions"].reshape(-1, 3, 3), np.asarray(xyz, np.float32).reshape(-1, 3)[np.asarray(mesh.triangles)]
    region_vertex = np.where((p0[:, 1] == r).all(axis=1)[:, None], p0[:, 1], p0[:, 2])   # the winding may have moved it to the middle
    assert _same_bits(region_vertex, r)
    g3 = VC.emu_geometry(xyz, e, mesh.triangles, mesh.halfedges, W, H, eye, fov, hh, 3.0)
    assert _same_bits(g3["positions"].reshape(-1, 3, 3), VC.numpy_positions(xyz, e, mesh.triangles, mesh.halfedges, 3.0))
    assert not np.array_equal(g3["positions"], g1["positions"])


def test_per_side_rules_against_numpy():
    mesh, xyz, e = VC.golden_case()
    for W, H, eye, fov, hh in VC.CPU_SHAPES + [VC.NEAR_EYE, VC.SURFACE_EYE]:
        g = VC.emu_geometry(xyz, e, mesh.triangles, mesh.halfedges, W, H, eye, fov, hh)
        S = VC.numpy_sides(VC.numpy_positions(xyz, e, mesh.triangles, mesh.halfedges), VC.numpy_camera(eye, fov, hh))
        assert np.array_equal(g["zc"], S["zc"]) and _same_bits(g["screen"][:, :, 0], S["a"]) and _same_bits(g["screen"][:, :, 1], S["b"])
        assert np.array_equal(g["front"], S["front"]) and np.array_equal(g["facing"], S["facing"])
        assert not (g["drawn"] & ~S["drawn"]).any()           # a box only where the three rules hold
        share = float(g["drawn"].mean())
        print(f"{W} x {H} from {eye}: {share:.1%} of the sides are drawn, {float(g['front'].mean()):.1%} lie in front, {float(g['facing'].mean()):.1%} face the camera")
        assert 0.0 < share <= 0.51                           # at most the half that faces a camera at infinity, the odd side more


# ---- 3. rule cases -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["near", "surface"])
def test_eye_close_to_the_surface(which):
    """Distance 1.2 and a field of view of 100 degrees: the camera looks at the centre, so every vertex still lies in front of it.
    At 1.15 under an eightfold relief the land around the eye rises behind the camera plane: those sides are not drawn."""
    W, H, eye, fov, hh = VC.NEAR_EYE if which == "near" else VC.SURFACE_EYE
    ex = 1.0 if which == "near" else VC.SURFACE_EXAGGERATION
    mesh, xyz, e = VC.golden_case()
    g = VC.emu_geometry(xyz, e, mesh.triangles, mesh.halfedges, W, H, eye, fov, hh, ex)
    behind = int((~g["front"]).sum())
    print(f"{which}: {behind} sides have a vertex behind the camera plane")
    assert (behind == 0) if which == "near" else (behind > 0)
    assert not (g["drawn"] & ~g["front"]).any()
    got = VC.emu_raster(xyz, e, mesh.triangles, mesh.halfedges, W, H, eye, fov, hh, ex, VC.SUN)
    want = VC.numpy_raster(xyz, e, mesh.triangles, mesh.halfedges, W, H, eye, fov, hh, ex, VC.SUN)
    assert np.array_equal(got["regionMap"], want["regionMap"]) and _same_bits(got["depth"], want["depth"]) and _same_bits(got["lambert"], want["lambert"])
    assert got["covered"] > (0.5 * W * H if which == "near" else 0)      # among the relief the eye sees a few facets and the sky


def nan_inf_field():
    """the golden case's relief with one NaN region and one +inf region, both in sight of the first shape's camera"""
    mesh, xyz, e = VC.golden_case()
    p = np.asarray(xyz, np.float32).reshape(-1, 3)
    toward = p @ np.array([0.0, 0.4, 2.8]) / math.hypot(0.4, 2.8)
    order = np.argsort(-toward)
    e = e.copy()
    e[order[3]], e[order[40]] = np.nan, np.inf
    return e, int(order[3]), int(order[40])


def test_nan_and_inf_elevation_leave_a_hole():
    W, H, eye, fov, hh = VC.CPU_SHAPES[0]
    mesh, xyz, clean = VC.golden_case()
    e, r_nan, r_inf = nan_inf_field()
    got = VC.emu_raster(xyz, e, mesh.triangles, mesh.halfedges, W, H, eye, fov, hh, 1.0, VC.SUN)
    want = VC.numpy_raster(xyz, e, mesh.triangles, mesh.halfedges, W, H, eye, fov, hh, 1.0, VC.SUN)
    assert np.array_equal(got["regionMap"], want["regionMap"]) and _same_bits(got["depth"], want["depth"]) and _same_bits(got["lambert"], want["lambert"])
    whole = VC.cpu_case(VC.CPU_SHAPES[0])
    assert (whole["regionMap"] == r_nan).any() and (whole["regionMap"] == r_inf).any()
    assert not np.isin(got["regionMap"], [r_nan, r_inf]).any()
    hole = (got["regionMap"] < 0) & (whole["regionMap"] >= 0)
    print(f"regions {r_nan} (NaN) and {r_inf} (+inf): a hole of {int(hole.sum())} pixels")
    assert hole.sum() > 0 and np.isnan(got["depth"][hole]).all()
    assert np.isfinite(got["depth"][got["regionMap"] >= 0]).all()
    assert np.array_equal(np.isnan(got["depth"]), got["regionMap"] < 0)


# ---- 4. shading ----------------------------------------------------------------------------------------------------------------------
def test_shade_formula():
    values = np.arange(256, dtype=np.uint8)
    for lam in (0.0, 0.5, 1.0):
        rgba = np.stack([values, values[::-1], (values.astype(np.int32) * 7 % 256).astype(np.uint8), np.full(256, 200, np.uint8)], axis=1)
        region, lambert = np.zeros(256, np.int32), np.full(256, lam, np.float32)
        got = VC.emu_shade(region, lambert, rgba)
        gain = 0.55 + 0.45 * lam
        want = rgba.copy()
        for ch in range(3):
            want[:, ch] = [min(255, math.floor(int(c) * gain + 0.5)) for c in rgba[:, ch]]
        assert np.array_equal(got, want), lam
        assert np.array_equal(got, VC.numpy_shade(rgba, lambert, region >= 0))
        assert (got[:, 3] == 200).all()
    full = VC.emu_shade(np.zeros(256, np.int32), np.ones(256, np.float32), np.stack([values] * 4, axis=1))
    assert np.array_equal(full[:, 0], values)                 # a facet that faces the light keeps its colour
    bright = VC.emu_shade(np.zeros(256, np.int32), np.ones(256, np.float32), np.stack([values] * 4, axis=1), ambient=1.0, diffuse=1.0)
    assert np.array_equal(bright[:, 0], np.minimum(255, 2 * values.astype(np.int32)))
    for background in (0, VC.BACKGROUND):                     # transparent and opaque: uncovered pixels are left as they are
        px = np.full((4, 1), background, np.uint32).view(np.uint8).reshape(4, 4)
        assert np.array_equal(VC.emu_shade(np.full(4, -1, np.int32), np.zeros(4, np.float32), px), px)
    assert np.array_equal(np.array([VC.BACKGROUND], np.uint32).view(np.uint8), [0x03, 0x03, 0x08, 0xFF])


# ---- 5. the host module without a device -----------------------------------------------------------------------------------------------
def test_host_module_pieces():
    from planet_heightmap_generation_amd import capi, view_export as VE
    assert capi.SIGNATURES["wo_view_raster"] == (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p])
    assert capi.SIGNATURES["wo_view_depth_download"] == (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64])
    L = capi.lib()
    assert hasattr(L, "wo_view_raster") and hasattr(L, "wo_view_depth_download")
    assert np.allclose(VE.camera(0.0, 0.0, 2.8)["eye"], (0.0, 0.0, 2.8)) and np.allclose(VE.camera(90.0, 0.0, 2.0)["eye"], (2.0, 0.0, 0.0), atol=1e-15)
    assert np.allclose(VE.camera(0.0, 90.0, 3.0)["eye"], (0.0, 3.0, 0.0), atol=1e-15) and VE.camera(10.0, 20.0)["fov"] == 50.0
    q = VE.request(VE.camera(30.0, 10.0), shade=True)
    assert q.fovY == 50.0 and q.shade == 1 and tuple(q.light) == VC.SUN and (q.ambient, q.diffuse) == (0.55, 0.45) and q.backgroundRgba == VC.BACKGROUND and q.exaggeration == 1.0
    assert VE.request(dict(eye=(0, 3, 0), fov=0, halfHeight=0.6), shade=False, background=0).backgroundRgba == 0
    assert VE.view_filename("biome", 7) == "orogen-globe-satellite-7.png" and VE.view_filename("tempSummer", 7) == "orogen-globe-layer-tempSummer-7.png"
    with pytest.raises(ValueError):
        VE.camera(0.0, 91.0)
    assert L.wo_view_raster(None, 0, None, None, 4, 4, None, None, None, None) != 0 and "wo_view_raster" in capi.last_error()
    assert L.wo_view_depth_download(None, None, 0) != 0 and "wo_view_depth_download" in capi.last_error()
