"""Shared pieces of the editor tests: the golden fixtures of the reference's findNearestRegion, getHitInfoGlobe / getHitInfoMap and
highlight functions (tests/golden/editor_N2000_s1.npz, editor_crafted.npz), the host emulator of csrc/pick_ops.h (tests/emu_editor),
and a numpy statement of the class-byte rule."""
from __future__ import annotations

import ctypes as C
import functools
import json
import subprocess

import numpy as np

import map_common as MC
from conftest import GOLDEN, REPO
from map_common import ptr

EMU_DIR = REPO / "tests" / "emu_editor"
VIEWS = ("color", "plates")
_emu = None


@functools.lru_cache(maxsize=None)
def golden():
    g = dict(np.load(GOLDEN / "editor_N2000_s1.npz"))
    g["states"] = json.loads(bytes(g["states_json"]).decode())
    return g


@functools.lru_cache(maxsize=None)
def crafted():
    return dict(np.load(GOLDEN / "editor_crafted.npz"))


def emu():
    global _emu
    if _emu is None:
        subprocess.run(["make", "-s", "-C", str(EMU_DIR)], check=True)
        _emu = C.CDLL(str(EMU_DIR / "_build" / "libemu_editor.so"))
        _emu.emu_editor_tile.restype = C.c_int32
    return _emu


def tile():
    return int(emu().emu_editor_tile())


def _pick_args(xyz, dirs):
    xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1)
    dirs = np.ascontiguousarray(dirs, np.float64).reshape(-1, 3)
    return xyz, dirs, np.empty(dirs.shape[0], np.int32), np.empty(dirs.shape[0], np.float64)


def emu_pick_loop(xyz, dirs):
    """the reference's loop: -> (regions int32, dots float64)"""
    xyz, dirs, regions, dots = _pick_args(xyz, dirs)
    emu().emu_editor_pick_loop(C.c_int32(xyz.size // 3), ptr(xyz), C.c_int32(dirs.shape[0]), ptr(dirs), ptr(regions), ptr(dots))
    return regions, dots


def emu_pick_reduce(xyz, dirs, lanes):
    """the reduction form with `lanes` lanes: -> (regions int32, dots float64)"""
    xyz, dirs, regions, dots = _pick_args(xyz, dirs)
    emu().emu_editor_pick_reduce(C.c_int32(xyz.size // 3), ptr(xyz), C.c_int32(dirs.shape[0]), ptr(dirs), C.c_int32(lanes), ptr(regions), ptr(dots))
    return regions, dots


def emu_directions_globe(rays):
    rays = np.ascontiguousarray(rays, np.float64).reshape(-1, 6)
    out, valid = np.empty((rays.shape[0], 3), np.float64), np.empty(rays.shape[0], np.uint8)
    emu().emu_editor_directions_globe(C.c_int32(rays.shape[0]), ptr(rays), ptr(out), ptr(valid))
    return out, valid


def emu_directions_map(points, center):
    points = np.ascontiguousarray(points, np.float64).reshape(-1, 2)
    out, valid = np.empty((points.shape[0], 3), np.float64), np.empty(points.shape[0], np.uint8)
    emu().emu_editor_directions_map(C.c_int32(points.shape[0]), ptr(points), C.c_double(center), ptr(out), ptr(valid))
    return out, valid


def emu_classes(r_plate, pending, is_ocean, hovered_plate, koppen, hovered_koppen):
    """-> (class bytes uint8 [N], counts int64 [4])"""
    r_plate = np.ascontiguousarray(r_plate, np.int32)
    pending, is_ocean = np.ascontiguousarray(pending, np.int32), np.ascontiguousarray(is_ocean, np.uint8)
    koppen = None if koppen is None else np.ascontiguousarray(koppen, np.uint8)
    cls, counts = np.empty(r_plate.size, np.uint8), np.zeros(4, np.int64)
    emu().emu_editor_classes(C.c_int32(r_plate.size), ptr(r_plate), C.c_int32(pending.size), ptr(pending), ptr(is_ocean), C.c_int32(hovered_plate), ptr(koppen),
                             C.c_int32(hovered_koppen), ptr(cls), ptr(counts))
    return cls, counts


def emu_tint(rgb, cls):
    """-> the tinted copy of rgb (float32 [3 N])"""
    out = np.ascontiguousarray(rgb, np.float32).reshape(-1).copy()
    cls = np.ascontiguousarray(cls, np.uint8)
    assert out.size == 3 * cls.size
    emu().emu_editor_tint(C.c_int32(cls.size), ptr(cls), ptr(out))
    return out


def emu_pack(rgb):
    """quantise and the gamma table: -> uint8 [N, 4]"""
    rgb = np.ascontiguousarray(rgb, np.float32).reshape(-1)
    out = np.empty(rgb.size // 3, np.uint32)
    emu().emu_editor_pack(C.c_int32(out.size), ptr(rgb), ptr(out))
    return out.view(np.uint8).reshape(-1, 4)


def numpy_classes(r_plate, n, pending, is_ocean, hovered_plate, koppen, hovered_koppen):
    """the rule of include/worogen.h stated in numpy: -> (class bytes, counts)"""
    r_plate = np.asarray(r_plate, np.int64)
    inside = (r_plate >= 0) & (r_plate < n)
    cls = np.zeros(r_plate.size, np.uint8)
    for pid, oc in zip(pending, is_ocean):
        cls[inside & (r_plate == pid)] |= 1 if oc else 2
    if hovered_plate >= 0:
        cls[inside & (r_plate == hovered_plate)] |= 4
    if hovered_koppen >= 0:
        cls[np.asarray(koppen, np.int64) == hovered_koppen] |= 8
    return cls, np.array([int(((cls >> b) & 1).sum()) for b in range(4)], np.int64)


def state_args(st, g=None):
    """a golden state as set_highlight takes it: (pending ids, their plateIsOcean bytes, hoveredPlate, hoveredKoppen)"""
    g = g or golden()
    ocean = set(int(i) for i in g["plateIsOcean"])
    return [int(i) for i in st["pending"]], [1 if int(i) in ocean else 0 for i in st["pending"]], int(st["hoveredPlate"]), int(st["hoveredKoppen"])


def state_classes(st):
    g = golden()
    pending, is_ocean, hp, hk = state_args(st)
    return emu_classes(g["r_plate"], pending, is_ocean, hp, g["koppen"], hk)[0]


def same_f32(a, b):
    return MC.same_bits(np.ascontiguousarray(a, np.float32).reshape(-1), np.ascontiguousarray(b, np.float32).reshape(-1))


def same_f64(a, b):
    """bit for bit, NaN with NaN"""
    a, b = np.ascontiguousarray(a, np.float64).reshape(-1), np.ascontiguousarray(b, np.float64).reshape(-1)
    return a.shape == b.shape and bool(np.all((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))))


def random_planet(n, seed, ties=True):
    """unit positions with planted ties: copies of one position at several indices, and queries that point at them"""
    rng = np.random.default_rng(seed)
    p = rng.normal(size=(n, 3))
    p = (p / np.linalg.norm(p, axis=1)[:, None]).astype(np.float32)
    q = rng.normal(size=(12, 3))
    q /= np.linalg.norm(q, axis=1)[:, None]
    if ties and n >= 8:
        for k in range(4):
            idx = rng.choice(n, size=min(n, 3 + k), replace=False)
            p[idx] = p[idx[0]]
            q[k] = p[idx[0]].astype(np.float64)
    q[4] = 0.0
    q[5] = -0.0
    q[6] = np.nan
    return p, np.ascontiguousarray(q)
