"""The relief contract of csrc/relief_ops.h on the host: the emulator's heights against independent numpy statements (barycentrics by
np.linalg.solve in the map plane; a 3-D ray-triangle intersection for the cube), properties that need no emulator arithmetic of
their own (a constant field, the range of the covering side, the region map, the frame of the pixel directions), the normals
against a numpy restatement of the finite-difference rule, the neighbour function across cube edges, and the 16-bit quantiser."""
import numpy as np
import pytest

import cube_common as CC
import map_common as MC
import map_layers_common as MLC
import relief_common as RC


def _report(tag, diff, bar, other_side):
    worst = float(np.nanmax(diff / bar))
    print(f"{tag}: max |emulator - numpy| {float(np.nanmax(diff)):.3e}, worst ratio to the bar {worst:.3f}; {int(other_side.sum())} pixels where the two pick different sides")


# ---- 1. heights against numpy ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,W,center_lon", RC.MAP_SHAPES)
def test_map_heights_equal_numpy_barycentrics(name, W, center_lon):
    mesh, xyz, e, side, region, h = RC.cpu_map_case(name, W, center_lon)
    n_side, n_h, shape, m = RC.numpy_map_heights(xyz, mesh.triangles, mesh.halfedges, W, center_lon, e)
    covered = side != RC.NO_SIDE
    assert np.array_equal(covered, n_side >= 0) and np.array_equal(np.isnan(h), ~covered)      # no NaN in this field: NaN marks uncovered
    diff = np.abs(h.astype(np.float64) - n_h)[covered]
    bar = RC.height_bar(m, shape)[covered]
    other = (side.astype(np.int64) != n_side)[covered]
    _report(f"{name} {W} x {W // 2} around {center_lon}", diff, bar, other)
    assert covered.sum() > 0.9 * covered.size
    assert (diff <= bar).all(), f"{int((diff > bar).sum())} pixels beyond the bar"                # no pixel left out, shared edges included


@pytest.mark.parametrize("name,S", CC.CPU_SHAPES)
def test_cube_heights_equal_numpy_ray_triangle(name, S):
    mesh, xyz, e, side, region, h = RC.cpu_cube_case(name, S)
    n_side, n_h = RC.numpy_cube_heights(xyz, mesh.triangles, mesh.halfedges, S, e)
    assert (side != RC.NO_SIDE).all() and (n_side >= 0).all() and not np.isnan(h).any()
    E = RC.numpy_side_elevations(mesh.triangles, mesh.halfedges, e).astype(np.float64)
    m = np.abs(E[side.astype(np.int64)]).max(axis=-1)
    bar = RC.height_bar(m, RC.cube_planar_shape(xyz, mesh.triangles, mesh.halfedges, side))
    diff = np.abs(h.astype(np.float64) - n_h)
    _report(f"{name} 6 x {S} x {S}", diff, bar, side.astype(np.int64) != n_side)
    assert (diff <= bar).all(), f"{int((diff > bar).sum())} pixels beyond the bar"


def test_side_elevations_equal_numpy():
    mesh, xyz = MC.golden_mesh("mesh_N2000_s1")
    e = RC.field(xyz, 3, nans=5)
    assert MC.same_bits(RC.emu_side_elevations(mesh.triangles, mesh.halfedges, e), RC.numpy_side_elevations(mesh.triangles, mesh.halfedges, e))


# ---- 2. properties -----------------------------------------------------------------------------------------------------------------
CONSTANTS = (0.25, -0.37, np.float32(1e-3), 0.0)


def test_constant_field_is_constant_in_every_bit():
    mesh, xyz = MC.golden_mesh("mesh_N2000_s1")
    for c in CONSTANTS:
        e = np.full(mesh.numRegions, c, np.float32)
        for W, lon in ((256, 0.0), (250, 0.0), (256, 1.0)):
            side, _, h = RC.emu_map(xyz, mesh.triangles, mesh.halfedges, W, lon, e)
            assert (h[side != RC.NO_SIDE].view(np.uint32) == np.float32(c).view(np.uint32)).all(), (c, W, lon)
            assert np.isnan(h[side == RC.NO_SIDE]).all()
        for S in (32, 50):
            side, _, h = RC.emu_cube(xyz, mesh.triangles, mesh.halfedges, S, e)
            assert (h.view(np.uint32) == np.float32(c).view(np.uint32)).all(), (c, S)


def test_heights_lie_within_the_covering_side():
    for name, W, lon in RC.MAP_SHAPES:
        mesh, xyz, e, side, _, h = RC.cpu_map_case(name, W, lon)
        E = RC.numpy_side_elevations(mesh.triangles, mesh.halfedges, e)
        covered = side != RC.NO_SIDE
        Es = E[side[covered].astype(np.int64)]
        assert (Es.min(axis=1) <= h[covered]).all() and (h[covered] <= Es.max(axis=1)).all(), (name, W, lon)
    for name, S in CC.CPU_SHAPES:
        mesh, xyz, e, side, _, h = RC.cpu_cube_case(name, S)
        Es = RC.numpy_side_elevations(mesh.triangles, mesh.halfedges, e)[side.astype(np.int64)]
        assert (Es.min(axis=-1) <= h).all() and (h <= Es.max(axis=-1)).all(), (name, S)


def test_region_map_is_the_plain_rasters():
    for name, W, lon in RC.MAP_SHAPES:
        mesh, xyz, e, side, region, _ = RC.cpu_map_case(name, W, lon)
        assert np.array_equal(region, MLC.emu_raster(xyz, mesh.triangles, mesh.halfedges, W, lon)[0]), (name, W, lon)
    for name, S in CC.CPU_SHAPES:
        mesh, xyz, e, side, region, _ = RC.cpu_cube_case(name, S)
        assert np.array_equal(region, CC.cpu_case(name, S)[2]), (name, S)


def _largest_angle_cos(xyz, tri, he):
    """per region: the cosine of the largest angle from the region to a vertex of its own sides"""
    v = CC.numpy_vertices(xyz, tri, he).astype(np.float64)
    u = v / np.linalg.norm(v, axis=2, keepdims=True)
    c = np.minimum((u[:, 0] * u[:, 2]).sum(axis=1), (u[:, 1] * u[:, 2]).sum(axis=1))
    out = np.ones(np.asarray(xyz).size // 3)
    np.minimum.at(out, np.asarray(tri, np.int64), c)
    return out


@pytest.mark.parametrize("name,W,lon", RC.MAP_SHAPES)
def test_map_pixel_directions_point_into_their_region(name, W, lon):
    """For every covered pixel, dhat . r_xyz[region] >= cos(A), A the largest angle from a region to a vertex of its own sides: ONE
    angle, the maximum over the mesh, computed from the mesh in numpy (6.76 degrees on mesh_N2000_s1; the worst pixel of the three
    shapes lies 6.17, 6.24 and 6.16 degrees from its region).  A frame that is mirrored, rotated or off by the centre meridian puts
    pixels tens of degrees from their regions, so this pins it.

    The sharper form, every pixel within its OWN region's largest angle, holds on the cube (below: gnomonic sides are great-circle
    arcs) and does not hold on this map, whatever the frame: the map's sides are straight in the (lon, lat) plane, so a pixel inside
    a side's planar triangle can lie outside the side's cone on the sphere.  Measured: 253, 274 and 312 of about 31 700 covered
    pixels exceed their own region's angle (about 3.8 degrees), by 0.004 to 0.2 degrees between latitudes 54 and 72 and by up to
    2.4 degrees within 4 degrees of a pole.  Those counts are printed, not asserted."""
    mesh, xyz, e, side, region, _ = RC.cpu_map_case(name, W, lon)
    d = RC.emu_directions(region.shape, lon)
    p = np.asarray(xyz, np.float64).reshape(-1, 3)
    p = p / np.linalg.norm(p, axis=1, keepdims=True)
    per_region = _largest_angle_cos(xyz, mesh.triangles, mesh.halfedges)
    cos_bound = per_region.min()
    ok = region >= 0
    got = (d[ok] * p[region[ok]]).sum(axis=1)
    own = got < per_region[region[ok]]
    print(f"{name} {W} around {lon}: largest angle of the mesh {np.degrees(np.arccos(cos_bound)):.3f} degrees, worst pixel {np.degrees(np.arccos(got.min())):.3f}; "
          f"{int(own.sum())} of {int(ok.sum())} covered pixels lie beyond their own region's largest angle")
    assert ok.sum() > 0.9 * ok.size and (got >= cos_bound).all(), (name, W, lon, int((got < cos_bound).sum()))


@pytest.mark.parametrize("name,W,lon", RC.MAP_SHAPES)
def test_map_pixel_directions_hit_their_regions(name, W, lon):
    """The frame of the map's directions against the mesh, without the sides: the directions are unit vectors, those of numpy's own
    sin and cos, and the pixel that holds a region's own map position (lon = atan2(x, z) less centerLon, lat = asin(y)) looks at the
    region to within half a pixel's diagonal on the map, which is no shorter than on the sphere."""
    mesh, xyz, e, side, region, _ = RC.cpu_map_case(name, W, lon)
    H = W // 2
    d = RC.emu_directions(region.shape, lon)
    assert np.abs(np.linalg.norm(d, axis=-1) - 1).max() < 1e-15
    assert np.abs(d - RC.numpy_map_directions(W, lon)[0]).max() < 1e-15
    p = np.asarray(xyz, np.float64).reshape(-1, 3)
    p = p / np.linalg.norm(p, axis=1, keepdims=True)
    rel = np.arctan2(p[:, 0], p[:, 2]) - lon
    rel = np.where(rel > np.pi, rel - 2 * np.pi, np.where(rel < -np.pi, rel + 2 * np.pi, rel))
    i = np.clip(np.floor((rel * 2 / np.pi + 2.0) * W / 4.0), 0, W - 1).astype(np.int64)
    j = np.clip(np.floor((1.0 - np.arcsin(p[:, 1]) * 2 / np.pi) * H / 2.0), 0, H - 1).astype(np.int64)
    half_diagonal = 0.5 * np.hypot(2 * np.pi / W, np.pi / H)
    assert ((d[j, i] * p).sum(axis=1) >= np.cos(half_diagonal) - 1e-12).all()


def test_cube_pixel_directions_point_into_their_region():
    for name, S in CC.CPU_SHAPES:
        mesh, xyz, e, side, region, _ = RC.cpu_cube_case(name, S)
        d = RC.emu_directions(region.shape)
        want = CC.numpy_directions(S)
        assert np.abs(d - want / np.linalg.norm(want, axis=-1, keepdims=True)).max() < 1e-15
        p = np.asarray(xyz, np.float64).reshape(-1, 3)
        p = p / np.linalg.norm(p, axis=1, keepdims=True)
        got = (d * p[region]).sum(axis=-1)
        assert (got >= _largest_angle_cos(xyz, mesh.triangles, mesh.halfedges)[region] - 1e-12).all(), (name, S)


# ---- 3. normals --------------------------------------------------------------------------------------------------------------------
FLAT = np.array([128, 128, 255, 255], np.uint8)


def _quantised(d):
    return np.clip(np.floor((d * 0.5 + 0.5) * 255.0 + 0.5), 0, 255).astype(np.uint8)


@pytest.mark.parametrize("c", (0.3, -0.5, 0.0))
def test_constant_field_gives_flat_normals(c):
    for S in (1, 2, 5, 50):
        h = np.full((6, S, S), c, np.float32)
        assert (RC.emu_normals(h, 0) == FLAT).all(), (c, S)
        obj = RC.emu_normals(h, 1)
        assert np.array_equal(obj[..., :3], _quantised(RC.emu_directions(h.shape))) and (obj[..., 3] == 255).all(), (c, S)
    for W, lon in ((2, 0.0), (4, 0.0), (64, 0.0), (250, 1.0)):
        h = np.full((W // 2, W), c, np.float32)
        assert (RC.emu_normals(h, 0, center_lon=lon) == FLAT).all(), (c, W, lon)
        obj = RC.emu_normals(h, 1, center_lon=lon)
        assert np.array_equal(obj[..., :3], _quantised(RC.emu_directions(h.shape, lon))), (c, W, lon)


def test_flat_ocean_and_zero_strength_give_flat_normals():
    mesh, xyz, e, side, region, h = RC.cpu_cube_case("mesh_N2000_s1", 32)
    _, _, _, _, _, hm = RC.cpu_map_case("mesh_N2000_s1", 256, 1.0)
    for heights, lon in ((h, 0.0), (hm, 1.0)):
        assert not (RC.emu_normals(heights, 0, center_lon=lon) == FLAT).all()                 # the field does tilt the normals
        assert (RC.emu_normals(heights, 0, strength=0.0, center_lon=lon) == FLAT).all()
        sea = -np.abs(np.where(np.isnan(heights), 1.0, heights)) - 0.01
        assert not (RC.emu_normals(sea, 0, center_lon=lon) == FLAT).all()
        assert (RC.emu_normals(sea, 0, flags=1, center_lon=lon) == FLAT).all()
        assert (RC.emu_normals(np.full_like(heights, np.nan), 0, center_lon=lon) == FLAT).all()


@pytest.mark.parametrize("space", (0, 1))
@pytest.mark.parametrize("flat_ocean", (False, True))
def test_normals_equal_numpy_finite_differences(space, flat_ocean):
    cases = [(RC.cpu_map_case("mesh_N2000_s1", 256, 1.0)[5], 1.0), (RC.cpu_map_case("mesh_N2000_s1", 250, 0.0)[5], 0.0), (RC.cpu_cube_case("mesh_N2000_s1", 32)[5], 0.0),
             (RC.cpu_cube_case("mesh_N2000_s1", 50)[5], 0.0)]
    for h, lon in cases:
        h = h.copy()
        if h.ndim == 3:
            h[2, 3, 4] = h[0, 0, 0] = np.nan                   # a NaN centre and NaN neighbours, one of them across an edge
        for strength in (1.0, 25.0):
            got = RC.emu_normals(h, space, strength, int(flat_ocean), lon).astype(np.int64)
            real = RC.numpy_normals(h, space, strength, flat_ocean, lon)
            want = np.clip(np.floor(real), 0, 255).astype(np.int64)
            differ = got[..., :3] != want
            print(f"space {space} flat_ocean {flat_ocean} {h.shape} strength {strength}: {int(differ.sum())} of {differ.size} bytes differ; {np.unique(got[..., :3]).size} distinct byte values")
            assert (got[..., 3] == 255).all()
            assert np.abs(got[..., :3] - want).max() <= 1
            assert (np.abs(real - np.round(real))[differ] < 1e-6).all()       # a differing byte sits on a rounding boundary
            assert np.unique(got[..., :3]).size > 20 or flat_ocean


@pytest.mark.parametrize("S", (1, 2, 5, 8))
def test_cube_neighbour_equals_numpy(S):
    seen = set()
    for f in range(6):
        for j in range(S):
            for i in range(S):
                for di, dj in ((1, 0), (-1, 0), (0, -1), (0, 1)):
                    if 0 <= i + di < S and 0 <= j + dj < S and S > 2:
                        continue
                    got = RC.emu_neighbor(f, i, j, di, dj, S)
                    assert got == RC.numpy_cube_neighbor(f, i, j, di, dj, S), (f, i, j, di, dj)
                    if not (0 <= i + di < S and 0 <= j + dj < S):
                        assert got[0] != f and got[0] // 2 != f // 2        # an adjacent face, never the opposite one
                        a = RC.emu_directions((6, S, S))[f, j, i]
                        b = RC.emu_directions((6, S, S))[got[0], got[2], got[1]]
                        assert (a * b).sum() > (-1e-12 if S == 1 else 0.5)  # and a pixel next to this one on the sphere
                        seen.add((f, got[0]))
    assert len(seen) == 24                                     # every face borders four others


# ---- 4. 16 bit ---------------------------------------------------------------------------------------------------------------------
def _km(e):
    if e <= 0:
        return e * 10.0
    t = min(e, 1.0)
    return 6.0 * (t * t) * (t * t) * (5.0 - 4.0 * t)


def _q16(kind, h):
    h = float(np.float32(h))
    if h != h:
        return 0
    shade = max(0.0, min(1.0, (_km(h) + 5.0) / 11.0)) if kind == 0 else (0.0 if h <= 0 else max(0.0, min(1.0, _km(h) / 6.0)))
    return int(np.floor(shade * 65535 + 0.5))


def test_quantiser_at_the_branch_points():
    points = []
    for b in (0.0, 1.0, -0.5, 0.6, -1.0, 0.5, 1e-3):           # sea level, the top, the floor of the shade (km = -5), its ceiling, and a few between
        x = np.float32(b)
        for _ in range(2):
            x = np.nextafter(x, np.float32(-np.inf))
        for _ in range(5):
            points.append(x)
            x = np.nextafter(x, np.float32(np.inf))
    points += [np.float32(0.0), np.float32(-0.0), np.float32(np.nan), np.float32(np.inf), np.float32(-np.inf)]
    h = np.array(points, np.float32)
    for kind in (0, 1):
        got = RC.emu_height16(kind, h)
        want = np.array([_q16(kind, x) for x in h], np.uint16)
        assert np.array_equal(got, want), (kind, h[got != want], got[got != want], want[got != want])
    assert RC.emu_height16(0, np.float32([np.nan, -np.inf, np.inf, 0.0, -0.0])).tolist() == [0, 0, 65535, 29789, 29789]
    assert RC.emu_height16(1, np.float32([np.nan, -np.inf, np.inf, 0.0, -0.0, 1.0])).tolist() == [0, 0, 65535, 0, 0, 65535]
    mono = np.linspace(-0.6, 1.1, 20001).astype(np.float32)
    for kind in (0, 1):
        q = RC.emu_height16(kind, mono).astype(np.int64)
        assert (np.diff(q) >= 0).all() and np.unique(q).size > 5000       # monotone, and far more than 256 levels
