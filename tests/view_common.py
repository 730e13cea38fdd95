"""Shared pieces of the globe-view tests: the host emulator of csrc/view_ops.h (tests/emu_view), the contract stated independently in
numpy (the camera, the per-side rules, float64 point-in-triangle over the projected f32 triangles, the f32 depth and the lowest side
on a tie), and a ray cast in 3-D (Moeller-Trumbore in float64, nearest hit) that knows neither the projection nor the culling."""
from __future__ import annotations

import ctypes as C
import functools
import math
import subprocess

import numpy as np

import map_common as MC
from conftest import REPO
from map_common import ptr

EMU_DIR = REPO / "tests" / "emu_view"
SUN = (5.0, 3.0, 4.0)
AMBIENT, DIFFUSE = 0.55, 0.45
BACKGROUND = 0xFF080303                                    # 0x030308 opaque, R first in memory
NAN_BITS = 0x7FC00000
# (width, height, eye, fovY, halfHeight) of the CPU tests: the shapes at which the contract's prototype found the planar raster and
# the ray cast in agreement in every pixel and no pixel centre within 1e-9 of an edge line
CPU_SHAPES = [
    (64, 64, (0.0, 0.4, 2.8), 50.0, 1.1),
    (48, 32, (2.0, -1.0, 0.5), 50.0, 1.1),
    (50, 50, (0.0, 3.0, 0.0), 0.0, 1.1),                   # the pole: the degenerate basis
    (33, 64, (-1.5, 0.2, -0.1), 0.0, 0.6),                 # every pixel covered, boxes clipped at all four borders
]
_TOWARDS = tuple(c / math.sqrt(0.4 * 0.4 + 2.8 * 2.8) for c in (0.0, 0.4, 2.8))
NEAR_EYE = (64, 64, tuple(1.2 * c for c in _TOWARDS), 100.0, 1.1)        # the eye at distance 1.2
SURFACE_EYE = (64, 64, tuple(1.15 * c for c in _TOWARDS), 100.0, 1.1)    # at 1.15 under SURFACE_EXAGGERATION: lower than the relief around it
SURFACE_EXAGGERATION = 8.0
_emu = None


def emu():
    global _emu
    if _emu is None:
        subprocess.run(["make", "-s", "-C", str(EMU_DIR)], check=True)
        _emu = C.CDLL(str(EMU_DIR / "_build" / "libemu_view.so"))
        for name in ("emu_view_small_box", "emu_view_camera", "emu_view_geometry", "emu_view_raster"):
            getattr(_emu, name).restype = C.c_int32
        _emu.emu_view_shade.restype = None
    return _emu


def small_box() -> int:
    return int(emu().emu_view_small_box())


def relief_field(xyz) -> np.ndarray:
    """the synthetic relief of the tests, within +-1: e = 0.7 sin(3 x + 1) cos(2 y) + 0.3 sin(9 z), as f32"""
    p = np.asarray(xyz, np.float32).reshape(-1, 3).astype(np.float64)
    return (0.7 * np.sin(3.0 * p[:, 0] + 1.0) * np.cos(2.0 * p[:, 1]) + 0.3 * np.sin(9.0 * p[:, 2])).astype(np.float32)


def _args(xyz, e, tri, he):
    xyz, tri, he = MC._mesh_args(xyz, tri, he)
    e = np.ascontiguousarray(e, np.float32)
    assert e.size * 3 == xyz.size
    return xyz, e, tri, he


def _camera_args(eye, fov, half_height, exaggeration=None):
    eye = np.ascontiguousarray(eye, np.float64)
    args = [ptr(eye), C.c_double(fov), C.c_double(half_height)]
    return args if exaggeration is None else args + [C.c_double(exaggeration)]


def emu_camera(eye, fov, half_height):
    """-> dict(origin, x, y, z, f, ortho), or None for a camera that is refused"""
    out = np.empty(14, np.float64)
    if not emu().emu_view_camera(*_camera_args(eye, fov, half_height), ptr(out)):
        return None
    return dict(origin=out[0:3], x=out[3:6], y=out[6:9], z=out[9:12], f=float(out[12]), ortho=bool(out[13]))


def emu_geometry(xyz, e, tri, he, W, H, eye, fov, half_height, exaggeration=1.0):
    """-> dict(positions f32 [ns, 9], zc f64 [ns, 3], screen f32 [ns, 3, 2], front, facing, drawn bool [ns], box int64 [ns])"""
    xyz, e, tri, he = _args(xyz, e, tri, he)
    ns = tri.size
    pos, zc, screen = np.empty(9 * ns, np.float32), np.empty(3 * ns, np.float64), np.empty(6 * ns, np.float32)
    front, facing, drawn, box = np.empty(ns, np.uint8), np.empty(ns, np.uint8), np.empty(ns, np.uint8), np.empty(ns, np.int64)
    ok = emu().emu_view_geometry(ptr(xyz), ptr(e), C.c_int32(ns), ptr(tri), ptr(he), C.c_int32(W), C.c_int32(H), *_camera_args(eye, fov, half_height, exaggeration), ptr(pos), ptr(zc),
                                 ptr(screen), ptr(front), ptr(facing), ptr(drawn), ptr(box))
    assert ok
    return dict(positions=pos.reshape(ns, 9), zc=zc.reshape(ns, 3), screen=screen.reshape(ns, 3, 2), front=front.astype(bool), facing=facing.astype(bool), drawn=drawn.astype(bool), box=box)


def emu_raster(xyz, e, tri, he, W, H, eye, fov, half_height, exaggeration=1.0, light=None):
    """-> dict(regionMap int32 [H, W], depth f32 [H, W], lambert f32 [H, W] or None, covered, uncovered)"""
    xyz, e, tri, he = _args(xyz, e, tri, he)
    rm, depth, counts = np.empty((H, W), np.int32), np.empty((H, W), np.float32), np.zeros(2, np.int64)
    lam = None if light is None else np.empty((H, W), np.float32)
    light = None if light is None else np.ascontiguousarray(light, np.float64)
    ok = emu().emu_view_raster(ptr(xyz), ptr(e), C.c_int32(tri.size), ptr(tri), ptr(he), C.c_int32(W), C.c_int32(H), *_camera_args(eye, fov, half_height, exaggeration), ptr(light), ptr(rm),
                               ptr(depth), ptr(lam), ptr(counts))
    assert ok
    return dict(regionMap=rm, depth=depth, lambert=lam, covered=int(counts[0]), uncovered=int(counts[1]))


def emu_shade(region_map, lambert, rgba, ambient=AMBIENT, diffuse=DIFFUSE):
    """the shade pass over uint8 [..., 4] pixels: covered pixels shaded, the others left -> a new array"""
    rm = np.ascontiguousarray(region_map, np.int32).reshape(-1)
    lam = np.ascontiguousarray(lambert, np.float32).reshape(-1)
    out = np.ascontiguousarray(rgba, np.uint8).copy()
    words = out.reshape(-1).view(np.uint32)
    assert words.size == rm.size == lam.size
    emu().emu_view_shade(ptr(rm), ptr(lam), C.c_int64(rm.size), C.c_double(ambient), C.c_double(diffuse), ptr(words))
    return out


# ---- the contract restated in numpy ------------------------------------------------------------------------------------------------
def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def numpy_camera(eye, fov, half_height):
    eye = np.asarray(eye, np.float64)
    z = eye / math.sqrt((eye[0] * eye[0] + eye[1] * eye[1]) + eye[2] * eye[2])
    xl = math.sqrt(z[2] * z[2] + z[0] * z[0])
    x = np.array([1.0, 0.0, 0.0]) if xl < 1e-12 else np.array([z[2] / xl, 0.0, -z[0] / xl])
    y = np.cross(z, x)
    ortho = fov == 0
    f = 1.0 / half_height if ortho else 1.0 / math.tan(fov * 3.141592653589793 / 180.0 / 2.0)
    return dict(origin=10.0 * z if ortho else eye, x=x, y=y, z=z, f=f, ortho=ortho)


def numpy_positions(xyz, e, tri, he, exaggeration=1.0):
    """The globe mesh's position rule (globe_common.numpy_positions) with 0.04 * exaggeration in the place of 0.04: float64 on the
    f32 inputs, stored as f32.  -> float32 [ns, 3, 3]"""
    f64 = np.float64
    P, E = np.asarray(xyz, np.float32).reshape(-1, 3).astype(f64), np.asarray(e, np.float32).astype(f64)
    tri, he = np.asarray(tri, np.int64), np.asarray(he, np.int64)
    c = tri.reshape(-1, 3)
    v = 0.04 * float(exaggeration)
    with np.errstate(all="ignore"):
        t_xyz = (((P[c[:, 0]] + P[c[:, 1]]) + P[c[:, 2]]) / 3.0).astype(np.float32).astype(f64)
        t_e = (((E[c[:, 0]] + E[c[:, 1]]) + E[c[:, 2]]) / 3.0).astype(np.float32).astype(f64)
        disp = lambda h: 1.0 + np.where(h > 0, h * v, h * v * 0.3)  # noqa: E731
        it, ot = np.arange(tri.size) // 3, he // 3
        v0, v1, v2 = t_xyz[it] * disp(t_e[it])[:, None], t_xyz[ot] * disp(t_e[ot])[:, None], P[tri] * disp(E[tri])[:, None]
        n = np.cross(v1 - v0, v2 - v0)
        swap = _dot(n, ((v0 + v1) + v2) / 3.0) < 0
        second, third = np.where(swap[:, None], v2, v1), np.where(swap[:, None], v1, v2)
        return np.stack([v0, second, third], axis=1).astype(np.float32)


def numpy_sides(pos, cam):
    """The per-side rules on the stored positions pos [ns, 3, 3] (f32): -> dict(zc f64 [ns, 3], a, b f32 [ns, 3], front, facing,
    area2, drawn)"""
    p = pos.astype(np.float64)
    with np.errstate(all="ignore"):
        d = p - cam["origin"]
        xr, yu, zc = _dot(d, cam["x"]), _dot(d, cam["y"]), -_dot(d, cam["z"])
        if cam["ortho"]:
            a, b = (cam["f"] * xr).astype(np.float32), (-(cam["f"] * yu)).astype(np.float32)
        else:
            a, b = ((cam["f"] * xr) / zc).astype(np.float32), (-((cam["f"] * yu) / zc)).astype(np.float32)
        n = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
        facing = (_dot(n, cam["z"]) > 0) if cam["ortho"] else (_dot(n, cam["origin"] - p[:, 0]) > 0)
        front = (zc > 0).all(axis=1)
        A, B = a.astype(np.float64), b.astype(np.float64)
        area2 = (A[:, 1] - A[:, 0]) * (B[:, 2] - B[:, 0]) - (B[:, 1] - B[:, 0]) * (A[:, 2] - A[:, 0])
        drawn = front & facing & ((area2 > 0) | (area2 < 0))
    return dict(zc=zc, a=a, b=b, n=n, front=front, facing=facing, area2=area2, drawn=drawn)


def pixel_centres(W, H):
    return (2.0 * (np.arange(W, dtype=np.float64) + 0.5) - W) / H, (2.0 * (np.arange(H, dtype=np.float64) + 0.5) - H) / H


def numpy_raster(xyz, e, tri, he, W, H, eye, fov, half_height, exaggeration=1.0, light=None, near=1e-9):
    """The contract stated independently.  -> dict(regionMap [H, W], depth f32 [H, W], lambert f32 [H, W] or None, side int64 [H, W]
    (-1: none), ambiguous bool [H, W]: the pixels whose centre lies within `near` of an edge line of a drawn triangle whose box
    holds them)"""
    cam = numpy_camera(eye, fov, half_height)
    pos = numpy_positions(xyz, e, tri, he, exaggeration)
    S = numpy_sides(pos, cam)
    tri = np.asarray(tri, np.int64)
    ca, cb = pixel_centres(W, H)
    sides = np.flatnonzero(S["drawn"])
    A, B, ZC, area2 = S["a"][sides].astype(np.float64), S["b"][sides].astype(np.float64), S["zc"][sides], S["area2"][sides]
    NONE = np.iinfo(np.uint64).max
    keys = np.full((H, W), NONE, np.uint64)
    ambiguous = np.zeros((H, W), bool)
    if sides.size:
        lim = W / H
        i0, i1 = np.searchsorted(ca, np.clip(A.min(axis=1), -lim - 1, lim + 1) - 1e-6), np.searchsorted(ca, np.clip(A.max(axis=1), -lim - 1, lim + 1) + 1e-6)
        j0, j1 = np.searchsorted(cb, np.clip(B.min(axis=1), -2, 2) - 1e-6), np.searchsorted(cb, np.clip(B.max(axis=1), -2, 2) + 1e-6)
        for dj in range(int(max((j1 - j0).max(), 0))):
            for di in range(int(max((i1 - i0).max(), 0))):
                i, j = i0 + di, j0 + dj
                m = (i < i1) & (j < j1)
                if not m.any():
                    continue
                X, Y = ca[i[m]], cb[j[m]]
                ax, ay, bx, by, cx, cy = A[m, 0], B[m, 0], A[m, 1], B[m, 1], A[m, 2], B[m, 2]
                e0 = (bx - ax) * (Y - ay) - (by - ay) * (X - ax)
                e1 = (cx - bx) * (Y - by) - (cy - by) * (X - bx)
                e2 = (ax - cx) * (Y - cy) - (ay - cy) * (X - cx)
                ar, zc = area2[m], ZC[m]
                inside = np.where(ar > 0, (e0 >= 0) & (e1 >= 0) & (e2 >= 0), (e0 <= 0) & (e1 <= 0) & (e2 <= 0))
                with np.errstate(all="ignore"):
                    if cam["ortho"]:
                        depth = (((e1 * zc[:, 0] + e2 * zc[:, 1]) + e0 * zc[:, 2]) / ar).astype(np.float32)
                    else:
                        w0, w1, w2 = (e1 / ar) / zc[:, 0], (e2 / ar) / zc[:, 1], (e0 / ar) / zc[:, 2]
                        depth = (1.0 / ((w0 + w1) + w2)).astype(np.float32)
                    take = inside & (depth > 0)
                key = (depth.view(np.uint32).astype(np.uint64) << np.uint64(32)) | sides[m].astype(np.uint64)
                np.minimum.at(keys, (j[m][take], i[m][take]), key[take])
                for ef, ux, uy in ((e0, bx - ax, by - ay), (e1, cx - bx, cy - by), (e2, ax - cx, ay - cy)):
                    length = np.hypot(ux, uy)
                    close = (length > 0) & (np.abs(ef) < near * length)
                    ambiguous[j[m][close], i[m][close]] = True
    covered = keys != NONE
    side = np.where(covered, (keys & np.uint64(0xFFFFFFFF)).astype(np.int64), -1)
    depth = np.where(covered, (keys >> np.uint64(32)).astype(np.uint32), np.uint32(NAN_BITS)).astype(np.uint32).view(np.float32)
    lam = None
    if light is not None:
        l = np.asarray(light, np.float64)
        l = l / math.sqrt((l[0] * l[0] + l[1] * l[1]) + l[2] * l[2])
        n = S["n"][np.where(covered, side, 0)]
        with np.errstate(all="ignore"):
            nh = n / np.sqrt(_dot(n, n))[..., None]
            d = _dot(nh, l)
        lam = np.where(covered & (d > 0), d, 0.0).astype(np.float32)
    return dict(regionMap=np.where(covered, tri[np.where(covered, side, 0)], -1).astype(np.int32), depth=depth, lambert=lam, side=side, ambiguous=ambiguous)


def numpy_shade(rgba, lambert, covered, ambient=AMBIENT, diffuse=DIFFUSE):
    """min(255, floor(c * (ambient + diffuse * lambert) + 0.5)) on R, G, B of the covered pixels; alpha and the others are kept"""
    px = np.asarray(rgba, np.uint8)
    gain = ambient + diffuse * np.asarray(lambert, np.float32).astype(np.float64)
    shaded = np.minimum(255.0, np.floor(px[..., :3].astype(np.float64) * gain[..., None] + 0.5)).astype(np.uint8)
    out = px.copy()
    out[..., :3] = np.where(np.asarray(covered, bool)[..., None], shaded, px[..., :3])
    return out


# ---- the ray cast ------------------------------------------------------------------------------------------------------------------
def ray_cast(xyz, e, tri, he, W, H, eye, fov, half_height, exaggeration=1.0, chunk=128):
    """For every pixel centre the region of the side whose flat 3-D triangle the pixel's ray hits first (Moeller-Trumbore in float64
    on the stored positions; no projection, no culling, either winding), -1 when it hits none.  The ray: perspective from the eye
    through x a / f - y b / f - z; orthographic from 10 z + x a / f - y b / f along -z.  -> int32 [H, W]"""
    cam = numpy_camera(eye, fov, half_height)
    v = numpy_positions(xyz, e, tri, he, exaggeration).astype(np.float64)
    good = np.isfinite(v).all(axis=(1, 2))
    ids = np.flatnonzero(good)
    v0, E1, E2 = v[ids, 0], v[ids, 1] - v[ids, 0], v[ids, 2] - v[ids, 0]
    tri = np.asarray(tri, np.int64)
    ca, cb = pixel_centres(W, H)
    bb, aa = np.meshgrid(cb, ca, indexing="ij")
    off = aa.reshape(-1, 1) / cam["f"] * cam["x"] - bb.reshape(-1, 1) / cam["f"] * cam["y"]
    if cam["ortho"]:
        O, D = cam["origin"] + off, np.broadcast_to(-cam["z"], off.shape)
    else:
        O, D = np.broadcast_to(cam["origin"], off.shape), off - cam["z"]
    out = np.full(W * H, -1, np.int32)
    for p0 in range(0, W * H, chunk):
        o, d = O[p0:p0 + chunk, None, :], D[p0:p0 + chunk, None, :]
        with np.errstate(all="ignore"):
            pv = np.cross(d, E2[None])
            det = (E1[None] * pv).sum(axis=2)
            tv = o - v0[None]
            u = (tv * pv).sum(axis=2) / det
            qv = np.cross(tv, E1[None])
            w = (d * qv).sum(axis=2) / det
            t = (E2[None] * qv).sum(axis=2) / det
            hit = (det != 0) & (u >= 0) & (w >= 0) & (u + w <= 1) & (t > 0)
        t = np.where(hit, t, np.inf)
        best = t.argmin(axis=1)
        found = np.isfinite(t[np.arange(t.shape[0]), best])
        out[p0:p0 + chunk] = np.where(found, tri[ids[best]], -1)
    return out.reshape(H, W)


@functools.lru_cache(maxsize=None)
def golden_case():
    """mesh_N2000_s1 under the synthetic relief: (mesh, xyz, e), computed once and left unchanged"""
    mesh, xyz = MC.golden_mesh("mesh_N2000_s1")
    e = relief_field(xyz)
    e.setflags(write=False)
    return mesh, xyz, e


@functools.lru_cache(maxsize=None)
def cpu_case(shape, shaded=True):
    """One shape of the golden case: the emulator's raster, computed once and left unchanged"""
    W, H, eye, fov, hh = shape
    mesh, xyz, e = golden_case()
    r = emu_raster(xyz, e, mesh.triangles, mesh.halfedges, W, H, eye, fov, hh, 1.0, SUN if shaded else None)
    for a in r.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return r
