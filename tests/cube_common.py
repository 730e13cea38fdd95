"""Shared pieces of the cube-map tests: the host emulator of csrc/cube_ops.h (tests/emu_cube), the projection and the coverage rule
stated independently in numpy (float64 point-in-triangle over the projected f32 triangles, per face), and a ray cast in 3-D that
knows neither the projection nor the face table."""
from __future__ import annotations

import ctypes as C
import functools
import subprocess

import numpy as np

import map_common as MC
from conftest import REPO

EMU_DIR = REPO / "tests" / "emu_cube"
FACES = ("px", "nx", "py", "ny", "pz", "nz")
# (mesh, face size) of the CPU tests: the shapes at which the contract's prototype found every pixel covered, none within 1e-9 of
# an edge, and the planar raster and the ray cast in agreement
CPU_SHAPES = [("mesh_N2000_s1", 32), ("mesh_N2000_s1", 50), ("mesh_N2000_s1", 64), ("mesh_N10000_s1", 48)]
_emu = None


def emu():
    global _emu
    if _emu is None:
        subprocess.run(["make", "-s", "-C", str(EMU_DIR)], check=True)
        _emu = C.CDLL(str(EMU_DIR / "_build" / "libemu_cube.so"))
        _emu.emu_cube_small_box.restype = C.c_int32
    return _emu


def small_box() -> int:
    return int(emu().emu_cube_small_box())


def emu_cube_raster(xyz, tri, he, S):
    """-> (regionMap int32 [6, S, S], covered, uncovered)"""
    xyz, tri, he = MC._mesh_args(xyz, tri, he)
    out, counts = np.empty((6, S, S), np.int32), np.zeros(2, np.int64)
    emu().emu_cube_raster(C.c_int32(xyz.size // 3), MC.ptr(xyz), C.c_int32(tri.size), MC.ptr(tri), MC.ptr(he), C.c_int32(S), MC.ptr(out), MC.ptr(counts))
    return out, int(counts[0]), int(counts[1])


def emu_cube_geometry(xyz, tri, he, S):
    """-> (raw float32 [ns, 3, 3]: the vertices of every side; drawn bool [ns, 6]; positions float32 [ns, 6, 3, 2]: (a, b) of every
    vertex where the side passes the face's test; boxPixels int64 [ns, 6]: the size of the pixel box where drawn)"""
    xyz, tri, he = MC._mesh_args(xyz, tri, he)
    ns = tri.size
    raw, drawn = np.empty(9 * ns, np.float32), np.empty(6 * ns, np.uint8)
    pos, box = np.empty(36 * ns, np.float32), np.empty(6 * ns, np.int64)
    emu().emu_cube_geometry(C.c_int32(xyz.size // 3), MC.ptr(xyz), C.c_int32(ns), MC.ptr(tri), MC.ptr(he), C.c_int32(S), MC.ptr(raw), MC.ptr(drawn), MC.ptr(pos), MC.ptr(box))
    return raw.reshape(ns, 3, 3), drawn.reshape(ns, 6).astype(bool), pos.reshape(ns, 6, 3, 2), box.reshape(ns, 6)


def emu_cube_direction(f, i, j, S):
    d = np.empty(3, np.float64)
    emu().emu_cube_direction(C.c_int32(f), C.c_int32(i), C.c_int32(j), C.c_int32(S), MC.ptr(d))
    return d


# ---- the contract restated in numpy ------------------------------------------------------------------------------------------------
def numpy_vertices(xyz, tri, he):
    """The three vertices of every side, float32 [ns, 3, 3]: the centres of the inner and the outer triangle (the sum left to right
    in float64, / 3, stored as f32) and the region's position."""
    p = np.asarray(xyz, np.float32).reshape(-1, 3)
    tri, he = np.asarray(tri, np.int64), np.asarray(he, np.int64)
    c = p[tri].astype(np.float64).reshape(-1, 3, 3)
    t_xyz = (((c[:, 0] + c[:, 1]) + c[:, 2]) / 3.0).astype(np.float32)
    s = np.arange(tri.size)
    return np.stack([t_xyz[s // 3], t_xyz[he // 3], p[tri]], axis=1)


def numpy_project(v, f):
    """(ma, a, b) of points v [..., 3] (f32) on face f by the table, the division in float64, a and b stored as f32"""
    x, y, z = v[..., 0], v[..., 1], v[..., 2]
    ma, sc, tc = ((x, -z, -y), (-x, z, -y), (y, x, z), (-y, x, -z), (z, x, -y), (-z, -x, -y))[f]
    with np.errstate(divide="ignore", invalid="ignore"):
        a = (sc.astype(np.float64) / ma.astype(np.float64)).astype(np.float32)
        b = (tc.astype(np.float64) / ma.astype(np.float64)).astype(np.float32)
    return ma, a, b


def numpy_cube_raster(xyz, tri, he, S, near=1e-9):
    """The contract stated independently: per face, the sides all of whose vertices have ma > 0, projected as above; float64
    point-in-triangle at the pixel centres; the lowest side index wins.  -> (regionMap [6, S, S], ambiguous [6, S, S]): ambiguous
    marks the pixels whose centre lies within `near` of an edge line of a triangle whose box holds them."""
    v = numpy_vertices(xyz, tri, he)
    tri = np.asarray(tri, np.int64)
    centre = -1.0 + 2.0 * (np.arange(S, dtype=np.float64) + 0.5) / S
    side_map = np.full((6, S, S), np.iinfo(np.int64).max, np.int64)
    ambiguous = np.zeros((6, S, S), bool)
    for f in range(6):
        ma, a, b = numpy_project(v, f)
        sides = np.flatnonzero((ma > 0).all(axis=1))
        A, B = a[sides].astype(np.float64), b[sides].astype(np.float64)
        area2 = (A[:, 1] - A[:, 0]) * (B[:, 2] - B[:, 0]) - (B[:, 1] - B[:, 0]) * (A[:, 2] - A[:, 0])
        keep = (area2 > 0) | (area2 < 0)
        sides, A, B, area2 = sides[keep], A[keep], B[keep], area2[keep]
        lo_a, hi_a = np.clip(A.min(axis=1), -1.5, 1.5), np.clip(A.max(axis=1), -1.5, 1.5)
        lo_b, hi_b = np.clip(B.min(axis=1), -1.5, 1.5), np.clip(B.max(axis=1), -1.5, 1.5)
        i0 = np.searchsorted(centre, lo_a - 1e-6)                      # the first centre that is not left of the box
        i1 = np.searchsorted(centre, hi_a + 1e-6)                      # one past the last centre in it
        j0, j1 = np.searchsorted(centre, lo_b - 1e-6), np.searchsorted(centre, hi_b + 1e-6)
        width = int(max((i1 - i0).max(), (j1 - j0).max(), 0))
        for dj in range(width):
            for di in range(width):
                i, j = i0 + di, j0 + dj
                m = (i < i1) & (j < j1)
                if not m.any():
                    continue
                X, Y = centre[i[m]], centre[j[m]]
                ax, ay, bx, by, cx, cy = A[m, 0], B[m, 0], A[m, 1], B[m, 1], A[m, 2], B[m, 2]
                e0 = (bx - ax) * (Y - ay) - (by - ay) * (X - ax)
                e1 = (cx - bx) * (Y - by) - (cy - by) * (X - bx)
                e2 = (ax - cx) * (Y - cy) - (ay - cy) * (X - cx)
                inside = np.where(area2[m] > 0, (e0 >= 0) & (e1 >= 0) & (e2 >= 0), (e0 <= 0) & (e1 <= 0) & (e2 <= 0))
                np.minimum.at(side_map[f], (j[m][inside], i[m][inside]), sides[m][inside])
                for e, ux, uy in ((e0, bx - ax, by - ay), (e1, cx - bx, cy - by), (e2, ax - cx, ay - cy)):
                    length = np.hypot(ux, uy)
                    close = (length > 0) & (np.abs(e) < near * length)
                    ambiguous[f][j[m][close], i[m][close]] = True
    covered = side_map != np.iinfo(np.int64).max
    return np.where(covered, tri[np.where(covered, side_map, 0)], -1), ambiguous


def numpy_directions(S):
    """cube_direction of every pixel centre, float64 [6, S, S, 3] (row j, column i), from the contract's sentence: the major axis is
    +-1, the other two come from ac and bc through the table"""
    c = -1.0 + 2.0 * (np.arange(S, dtype=np.float64) + 0.5) / S
    b, a = np.meshgrid(c, c, indexing="ij")
    one = np.ones_like(a)
    return np.stack([np.stack(d, axis=-1) for d in ((one, -b, -a), (-one, -b, a), (a, one, b), (a, -one, -b), (a, -b, one), (-a, -b, -one))])


def ray_cast(xyz, tri, he, S, chunk=1024):
    """For every pixel centre's direction d: the region of the lowest side whose triangle of raw vertices the ray from the origin
    hits, -1 when none does.  Hits: the three scalar triple products d . (v0 x v1), d . (v1 x v2), d . (v2 x v0) agree in sign, zero
    included, and the centroid lies in front (d . centroid > 0).  3-D arithmetic in float64: no projection, no face table beyond
    the directions.  Candidates come from a cone around every triangle's centroid that holds its three vertices.  -> [6, S, S]"""
    v = numpy_vertices(xyz, tri, he).astype(np.float64)
    tri = np.asarray(tri, np.int64)
    n01, n12, n20 = np.cross(v[:, 0], v[:, 1]), np.cross(v[:, 1], v[:, 2]), np.cross(v[:, 2], v[:, 0])
    cen = v.sum(axis=1) / 3.0
    cen_u = cen / np.linalg.norm(cen, axis=1, keepdims=True)
    v_u = v / np.linalg.norm(v, axis=2, keepdims=True)
    cone = np.einsum("skc,sc->sk", v_u, cen_u).min(axis=1) - 1e-3      # the cosine of the cone's half angle, widened
    d = numpy_directions(S).reshape(-1, 3)
    d_u = d / np.linalg.norm(d, axis=1, keepdims=True)
    best = np.full(d.shape[0], np.iinfo(np.int64).max, np.int64)
    for p0 in range(0, d.shape[0], chunk):
        px, sd = np.nonzero(d_u[p0:p0 + chunk] @ cen_u.T >= cone[None, :])
        px += p0
        D = d[px]
        t0, t1, t2 = (D * n01[sd]).sum(axis=1), (D * n12[sd]).sum(axis=1), (D * n20[sd]).sum(axis=1)
        hit = (((t0 >= 0) & (t1 >= 0) & (t2 >= 0)) | ((t0 <= 0) & (t1 <= 0) & (t2 <= 0))) & ((D * cen[sd]).sum(axis=1) > 0)
        np.minimum.at(best, px[hit], sd[hit])
    found = best != np.iinfo(np.int64).max
    return np.where(found, tri[np.where(found, best, 0)], -1).reshape(6, S, S)


@functools.lru_cache(maxsize=None)
def cpu_case(name, S):
    """One CPU shape: the mesh and the emulator's region map with its counts, computed once and left unchanged"""
    mesh, xyz = MC.golden_mesh(name)
    rm, covered, uncovered = emu_cube_raster(xyz, mesh.triangles, mesh.halfedges, S)
    rm.setflags(write=False)
    return mesh, xyz, rm, covered, uncovered
