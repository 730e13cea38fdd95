"""Shared pieces of the relief tests: the host emulator of csrc/relief_ops.h (tests/emu_relief) and the contract restated independently
in numpy: the height of a map pixel as float64 barycentrics by np.linalg.solve in the map plane, the height of a cube pixel as a 3-D
ray-triangle intersection that knows no face table beyond the directions, and the finite-difference rule of the normals."""
from __future__ import annotations

import ctypes as C
import functools
import subprocess

import numpy as np

import cube_common as CC
import map_common as MC
import map_layers_common as MLC
from conftest import REPO

EMU_DIR = REPO / "tests" / "emu_relief"
NO_SIDE = 0xFFFFFFFF
V = 0.04
# (mesh, width, centerLon) of the CPU map tests: the shapes the map tests vetted (no pixel centre within 1e-9 of an edge)
MAP_SHAPES = [("mesh_N2000_s1", 256, 0.0), ("mesh_N2000_s1", 250, 0.0), ("mesh_N2000_s1", 256, 1.0)]
_emu = None


def emu():
    global _emu
    if _emu is None:
        subprocess.run(["make", "-s", "-C", str(EMU_DIR)], check=True)
        _emu = C.CDLL(str(EMU_DIR / "_build" / "libemu_relief.so"))
    return _emu


def _f32(a):
    return np.ascontiguousarray(a, np.float32).reshape(-1)


def emu_map(xyz, tri, he, W, center_lon, e):
    """-> (sideMap uint32 [H, W], regionMap int32 [H, W], heights float32 [H, W])"""
    xyz, tri, he = MC._mesh_args(xyz, tri, he)
    e = _f32(e)
    shape = (W // 2, W)
    side, region, h = np.empty(shape, np.uint32), np.empty(shape, np.int32), np.empty(shape, np.float32)
    emu().emu_relief_map(C.c_int32(xyz.size // 3), MC.ptr(xyz), C.c_int32(tri.size), MC.ptr(tri), MC.ptr(he), C.c_int32(W), C.c_double(center_lon), MC.ptr(e), MC.ptr(side),
                         MC.ptr(region), MC.ptr(h))
    return side, region, h


def emu_cube(xyz, tri, he, S, e):
    """-> (sideMap uint32 [6, S, S], regionMap int32 [6, S, S], heights float32 [6, S, S])"""
    xyz, tri, he = MC._mesh_args(xyz, tri, he)
    e = _f32(e)
    shape = (6, S, S)
    side, region, h = np.empty(shape, np.uint32), np.empty(shape, np.int32), np.empty(shape, np.float32)
    emu().emu_relief_cube(C.c_int32(xyz.size // 3), MC.ptr(xyz), C.c_int32(tri.size), MC.ptr(tri), MC.ptr(he), C.c_int32(S), MC.ptr(e), MC.ptr(side), MC.ptr(region), MC.ptr(h))
    return side, region, h


def emu_side_elevations(tri, he, e):
    """-> float32 [ns, 3]: E0, E1, E2 of every side"""
    tri, he, e = np.ascontiguousarray(tri, np.int32), np.ascontiguousarray(he, np.int32), _f32(e)
    out = np.empty((tri.size, 3), np.float32)
    emu().emu_relief_side_elevations(C.c_int32(tri.size), MC.ptr(tri), MC.ptr(he), MC.ptr(e), MC.ptr(out))
    return out


def emu_height16(kind, h):
    h = np.ascontiguousarray(h, np.float32)
    out = np.empty(h.shape, np.uint16)
    emu().emu_relief_height16(C.c_int32(kind), C.c_int64(h.size), MC.ptr(h), MC.ptr(out))
    return out


def emu_normals(heights, space, strength=1.0, flags=0, center_lon=0.0):
    """heights [H, W] (a map) or [6, S, S] (a cube map) -> uint8 heights.shape + (4,)"""
    h = np.ascontiguousarray(heights, np.float32)
    cube = h.ndim == 3
    W, H = (h.shape[2], 6 * h.shape[2]) if cube else (h.shape[1], h.shape[0])
    out = np.empty(h.size, np.uint32)
    emu().emu_relief_normals(C.c_int32(cube), C.c_int32(W), C.c_int32(H), C.c_double(center_lon), MC.ptr(h), C.c_int32(space), C.c_double(strength), C.c_int32(flags), MC.ptr(out))
    return out.view(np.uint8).reshape(h.shape + (4,))


def emu_directions(shape, center_lon=0.0):
    """the unit directions of every pixel of a map [H, W] or a cube map [6, S, S] -> float64 shape + (3,)"""
    cube = len(shape) == 3
    W, H = (shape[2], 6 * shape[2]) if cube else (shape[1], shape[0])
    out = np.empty(tuple(shape) + (3,), np.float64)
    emu().emu_relief_directions(C.c_int32(cube), C.c_int32(W), C.c_int32(H), C.c_double(center_lon), MC.ptr(out))
    return out


def emu_neighbor(f, i, j, di, dj, S):
    out = np.empty(3, np.int32)
    emu().emu_relief_neighbor(C.c_int32(f), C.c_int32(i), C.c_int32(j), C.c_int32(di), C.c_int32(dj), C.c_int32(S), MC.ptr(out))
    return tuple(int(x) for x in out)


def field(xyz, seed=7, nans=0):
    """An fbm field of both signs, with a few NaN cells when asked"""
    e = MC.fbm_like(xyz, seed).copy()
    if nans:
        e[np.random.default_rng(seed).choice(e.size, nans, replace=False)] = np.nan
    return e


# ---- the contract restated in numpy ----------------------------------------------------------------------------------------------
def numpy_side_elevations(tri, he, e):
    """E0, E1, E2 of every side, float32 [ns, 3]: the triangle means summed left to right in float64, / 3, stored as f32"""
    tri, he = np.asarray(tri, np.int64), np.asarray(he, np.int64)
    c = np.asarray(e, np.float32)[tri].astype(np.float64).reshape(-1, 3)
    t_e = (((c[:, 0] + c[:, 1]) + c[:, 2]) / 3.0).astype(np.float32)
    s = np.arange(tri.size)
    return np.stack([t_e[s // 3], t_e[he // 3], np.asarray(e, np.float32)[tri]], axis=1)


def numpy_map_heights(xyz, tri, he, W, center_lon, e):
    """Per pixel of the W x W / 2 map: the lowest side with a triangle that holds the centre (float64 point-in-triangle), and the
    plane through the triangle's three (x, y, E) by np.linalg.solve evaluated at the centre.
    -> (side int64 [H, W] (-1: none), h float64 [H, W], shape float64 [H, W]: L^2 / |area2| of the triangle used, m float64 [H, W])"""
    H = W // 2
    pos, _, sides = MLC.emu_geometry(xyz, tri, he, center_lon)
    E = numpy_side_elevations(tri, he, e).astype(np.float64)
    P = pos.astype(np.float64)
    xc = -2.0 + 4.0 * (np.arange(W, dtype=np.float64) + 0.5) / W
    yc = 1.0 - 2.0 * (np.arange(H, dtype=np.float64) + 0.5) / H
    side = np.full((H, W), -1, np.int64)
    h, shape, m = np.full((H, W), np.nan), np.zeros((H, W)), np.zeros((H, W))
    for t in range(P.shape[0] - 1, -1, -1):                  # descending: the lowest index is written last
        (ax, ay), (bx, by), (cx, cy) = P[t]
        area2 = (bx - ax) * (cy - ay) - (by - ay) * (cx - ax)
        if not (area2 > 0 or area2 < 0):
            continue
        i0, i1 = np.searchsorted(xc, min(ax, bx, cx) - 1e-6), np.searchsorted(xc, max(ax, bx, cx) + 1e-6)
        j0, j1 = np.searchsorted(-yc, -(max(ay, by, cy) + 1e-6)), np.searchsorted(-yc, -(min(ay, by, cy) - 1e-6))
        if i0 >= i1 or j0 >= j1:
            continue
        X, Y = xc[None, i0:i1], yc[j0:j1, None]
        e0 = (bx - ax) * (Y - ay) - (by - ay) * (X - ax)
        e1 = (cx - bx) * (Y - by) - (cy - by) * (X - bx)
        e2 = (ax - cx) * (Y - cy) - (ay - cy) * (X - cx)
        inside = ((e0 >= 0) & (e1 >= 0) & (e2 >= 0)) if area2 > 0 else ((e0 <= 0) & (e1 <= 0) & (e2 <= 0))
        if not inside.any():
            continue
        Es = E[sides[t]]
        with np.errstate(invalid="ignore"):
            plane = np.linalg.solve(np.array([[ax, ay, 1.0], [bx, by, 1.0], [cx, cy, 1.0]]), Es) if np.isfinite(Es).all() else np.full(3, np.nan)
        L2 = max((bx - ax) ** 2 + (by - ay) ** 2, (cx - bx) ** 2 + (cy - by) ** 2, (ax - cx) ** 2 + (ay - cy) ** 2)
        side[j0:j1, i0:i1][inside] = sides[t]
        h[j0:j1, i0:i1][inside] = (plane[0] * X + plane[1] * Y + plane[2] + 0 * Y)[inside]
        shape[j0:j1, i0:i1][inside] = L2 / abs(area2)
        m[j0:j1, i0:i1][inside] = np.nanmax(np.abs(Es)) if np.isfinite(Es).any() else 0.0
    return side, h, shape, m


def numpy_cube_heights(xyz, tri, he, S, e, chunk=1024):
    """Per pixel of the six faces: the lowest side whose raw 3-D triangle the ray through the pixel centre hits (cube_common.ray_cast's
    rule), and the elevation where it meets the triangle's plane: [v0 v1 v2] w = d by np.linalg.solve, h = w . E / sum(w).
    -> (side int64 [6, S, S] (-1: none), h float64 [6, S, S])"""
    v = CC.numpy_vertices(xyz, tri, he).astype(np.float64)
    E = numpy_side_elevations(tri, he, e).astype(np.float64)
    n01, n12, n20 = np.cross(v[:, 0], v[:, 1]), np.cross(v[:, 1], v[:, 2]), np.cross(v[:, 2], v[:, 0])
    cen = v.sum(axis=1) / 3.0
    cen_u = cen / np.linalg.norm(cen, axis=1, keepdims=True)
    v_u = v / np.linalg.norm(v, axis=2, keepdims=True)
    cone = np.einsum("skc,sc->sk", v_u, cen_u).min(axis=1) - 1e-3
    d = CC.numpy_directions(S).reshape(-1, 3)
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
    s = np.where(found, best, 0)
    w = np.linalg.solve(np.swapaxes(v[s], 1, 2), d[:, :, None])[:, :, 0]
    with np.errstate(invalid="ignore"):
        h = (w * E[s]).sum(axis=1) / w.sum(axis=1)
    return np.where(found, best, -1).reshape(6, S, S), np.where(found, h, np.nan).reshape(6, S, S)


def cube_planar_shape(xyz, tri, he, side_map):
    """L^2 / |area2| of the planar triangle of every pixel's side on the pixel's face, and m = max |E_k| is left to the caller
    -> float64 [6, S, S]"""
    v = CC.numpy_vertices(xyz, tri, he)
    out = np.zeros(side_map.shape)
    for f in range(6):
        s = side_map[f].astype(np.int64)
        _, a, b = CC.numpy_project(v[s], f)
        a, b = a.astype(np.float64), b.astype(np.float64)
        area2 = (a[..., 1] - a[..., 0]) * (b[..., 2] - b[..., 0]) - (b[..., 1] - b[..., 0]) * (a[..., 2] - a[..., 0])
        L2 = np.maximum.reduce([(a[..., k] - a[..., (k + 1) % 3]) ** 2 + (b[..., k] - b[..., (k + 1) % 3]) ** 2 for k in range(3)])
        out[f] = L2 / np.abs(area2)
    return out


def height_bar(m, shape):
    """The issue's bar per pixel: one f32 rounding of the result, and the double rounding of the edge functions amplified by the
    triangle's shape"""
    return 2.0 ** -23 * m + 2.0 ** -40 * m * shape


def numpy_map_directions(W, center_lon=0.0):
    """d = (cos lat sin lon, sin lat, cos lat cos lon) at every pixel centre, lat = yc pi / 2, lon = xc pi / 2 + centerLon, with numpy's
    own sin and cos -> float64 [H, W, 3], and the frame (east, north) [H, W, 3] each"""
    H = W // 2
    lon = (-2.0 + 4.0 * (np.arange(W, dtype=np.float64) + 0.5) / W) * (np.pi / 2) + center_lon
    lat = (1.0 - 2.0 * (np.arange(H, dtype=np.float64) + 0.5) / H) * (np.pi / 2)
    lat, lon = np.meshgrid(lat, lon, indexing="ij")
    d = np.stack([np.cos(lat) * np.sin(lon), np.sin(lat), np.cos(lat) * np.cos(lon)], axis=-1)
    east = np.stack([np.cos(lon), 0 * lon, -np.sin(lon)], axis=-1)
    north = np.stack([-np.sin(lat) * np.sin(lon), np.cos(lat), -np.sin(lat) * np.cos(lon)], axis=-1)
    return d, east, north


def numpy_cube_neighbor(f, i, j, di, dj, S):
    """extended direction -> dominant axis -> floor"""
    ni, nj = i + di, j + dj
    if 0 <= ni < S and 0 <= nj < S:
        return f, ni, nj
    a, b = -1.0 + 2.0 * (ni + 0.5) / S, -1.0 + 2.0 * (nj + 0.5) / S
    d = np.array(((1.0, -b, -a), (-1.0, -b, a), (a, 1.0, b), (a, -1.0, -b), (a, -b, 1.0), (-a, -b, -1.0))[f])
    k = int(np.argmax(np.abs(d)))
    g = 2 * k + (0 if d[k] > 0 else 1)
    x, y, z = d
    ma, sc, tc = ((x, -z, -y), (-x, z, -y), (y, x, z), (-y, x, -z), (z, x, -y), (-z, -x, -y))[g]
    clamp = lambda c: int(min(max(np.floor((c + 1.0) * S / 2.0), 0), S - 1))
    return g, clamp(sc / ma), clamp(tc / ma)


def _radius(h, strength, flat_ocean):
    h = np.where(flat_ocean & (h <= 0), 0.0, h) if flat_ocean else h
    return 1.0 + strength * np.where(h > 0, h * V, h * V * 0.3)


def numpy_normals(heights, space, strength=1.0, flat_ocean=False, center_lon=0.0):
    """The finite-difference rule restated: the four neighbours' points d(q) R(h(q)), N = Tu x Tv, N0 the same with every R the
    centre's, t = ((N - N0) . right, (N - N0) . up, (N - N0) . d + |N0|), normalised -> the real-valued bytes before the floor,
    float64 heights.shape + (3,)"""
    h = np.asarray(heights, np.float32).astype(np.float64)
    if h.ndim == 2:
        Hh, W = h.shape
        d, right, up = numpy_map_directions(W, center_lon)
        jj, ii = np.meshgrid(np.arange(Hh), np.arange(W), indexing="ij")
        nb = [(jj, (ii + 1) % W), (jj, (ii - 1) % W), (np.maximum(jj - 1, 0), ii), (np.minimum(jj + 1, Hh - 1), ii)]
    else:
        S = h.shape[1]
        d = CC.numpy_directions(S)
        d = d / np.linalg.norm(d, axis=-1, keepdims=True)
        A = np.array([(0, 0, -1), (0, 0, 1), (1, 0, 0), (1, 0, 0), (1, 0, 0), (-1, 0, 0)], np.float64)[:, None, None, :]
        right = A - (A * d).sum(axis=-1, keepdims=True) * d
        right = right / np.linalg.norm(right, axis=-1, keepdims=True)
        up = np.cross(d, right)
        nb = []
        for di, dj in ((1, 0), (-1, 0), (0, -1), (0, 1)):
            idx = np.empty((3, 6, S, S), np.int64)
            for f in range(6):
                for j in range(S):
                    for i in range(S):
                        interior = 0 <= i + di < S and 0 <= j + dj < S
                        g, ni, nj = (f, i + di, j + dj) if interior else numpy_cube_neighbor(f, i, j, di, dj, S)
                        idx[:, f, j, i] = (g, nj, ni)
            nb.append(tuple(idx))
    hc = h
    Rc = _radius(hc, strength, flat_ocean)
    P, P0 = [], []
    for q in nb:
        hq = h[q]
        hq = np.where(np.isnan(hq), hc, hq)
        P.append(d[q] * _radius(hq, strength, flat_ocean)[..., None])
        P0.append(d[q] * Rc[..., None])
    N, N0 = np.cross(P[0] - P[1], P[2] - P[3]), np.cross(P0[0] - P0[1], P0[2] - P0[3])
    D = N - N0
    t = np.stack([(D * right).sum(-1), (D * up).sum(-1), (D * d).sum(-1) + np.linalg.norm(N0, axis=-1)], axis=-1)
    t = np.where(t[..., 2:3] < 0, -t, t)
    with np.errstate(invalid="ignore", divide="ignore"):
        t = t / np.linalg.norm(t, axis=-1, keepdims=True)
    flat = np.isnan(t).any(axis=-1) | np.isnan(hc)
    t[flat] = (0.0, 0.0, 1.0)
    n = t if space == 0 else right * t[..., 0:1] + up * t[..., 1:2] + d * t[..., 2:3]
    return (n * 0.5 + 0.5) * 255.0 + 0.5


@functools.lru_cache(maxsize=None)
def cpu_map_case(name, W, center_lon):
    mesh, xyz = MC.golden_mesh(name)
    e = field(xyz)
    out = (mesh, xyz, e) + emu_map(xyz, mesh.triangles, mesh.halfedges, W, center_lon, e)
    for a in out[2:]:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def cpu_cube_case(name, S):
    mesh, xyz = MC.golden_mesh(name)
    e = field(xyz)
    out = (mesh, xyz, e) + emu_cube(xyz, mesh.triangles, mesh.halfedges, S, e)
    for a in out[2:]:
        a.setflags(write=False)
    return out
