"""Shared pieces of the heightmap-import tests: the golden fixture, the host emulator of csrc/import_ops.h
(tests/emu_import), the host component composition and a numpy restatement of the region classification."""
from __future__ import annotations

import ctypes as C
import json
import subprocess

import numpy as np

from conftest import GOLDEN, REPO

EMU_DIR = REPO / "tests" / "emu_import"
IMAGES = ("512x256", "333x97", "4x2", "zero", "full")
_emu = None


def golden():
    return np.load(GOLDEN / "import_N10000_s1.npz")


def meta(g):
    return json.loads(bytes(g["meta_json"]).decode())


def emu():
    global _emu
    if _emu is None:
        subprocess.run(["make", "-s", "-C", str(EMU_DIR)], check=True)
        _emu = C.CDLL(str(EMU_DIR / "_build" / "libemu_import.so"))
    return _emu


def ptr(a):
    assert a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(C.c_void_p)


def emu_sample(xyz, img):
    xyz = np.ascontiguousarray(xyz, np.float32)
    img = np.ascontiguousarray(img, np.uint8)
    n = xyz.size // 3
    out = np.empty(n, np.float32)
    emu().emu_sample(C.c_int32(n), ptr(xyz), ptr(img), C.c_int32(img.shape[1]), C.c_int32(img.shape[0]), ptr(out))
    return out


def emu_components(off, adj, e, seed):
    off, adj, e = (np.ascontiguousarray(a) for a in (off, adj, e))
    out = np.empty(off.size - 1, np.int32)
    emu().emu_components(C.c_int32(off.size - 1), ptr(off), ptr(adj), ptr(e), C.c_uint64(seed), ptr(out))
    return out


def host_components(off, adj, e):
    """min id per same-class component from the host's wo_land_components, once per class"""
    from planet_heightmap_generation_amd import capi
    off, adj = np.ascontiguousarray(off, np.int32), np.ascontiguousarray(adj, np.int32)
    ocean = (np.asarray(e) <= 0).astype(np.uint8)
    n = off.size - 1
    lab_land, lab_ocean = np.empty(n, np.int32), np.empty(n, np.int32)
    capi.check(capi.lib().wo_land_components(n, ptr(off), ptr(adj), ptr(ocean), ptr(lab_land)), "wo_land_components")
    inv = np.ascontiguousarray(1 - ocean)
    capi.check(capi.lib().wo_land_components(n, ptr(off), ptr(adj), ptr(inv), ptr(lab_ocean)), "wo_land_components")
    return np.where(ocean == 1, lab_ocean, lab_land).astype(np.int32)


def numpy_regions(off, adj, e):
    """js/planet-worker.js:811-831 restated: (mountain_r, coastline_r, ocean_r), ascending"""
    e = np.asarray(e, np.float32)
    ocean = e <= 0
    row = np.repeat(np.arange(off.size - 1), np.diff(off))
    nb_ocean = np.zeros(e.size, bool)
    np.logical_or.at(nb_ocean, row, ocean[adj])
    return (np.nonzero(~ocean & (e > 0.5))[0].astype(np.int32), np.nonzero((e > 0) & nb_ocean)[0].astype(np.int32),
            np.nonzero(ocean)[0].astype(np.int32))


def seeds_of(label, e):
    seeds = np.nonzero(label == np.arange(label.size))[0].astype(np.int32)
    return seeds, seeds[np.asarray(e)[seeds] <= 0]


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape:
        return False
    ua, ub = a.view(np.uint32 if a.dtype == np.float32 else np.uint64), b.view(np.uint32 if b.dtype == np.float32 else np.uint64)
    return bool(np.all((ua == ub) | (np.isnan(a) & np.isnan(b))))


def ring_csr(n):
    """A ring: cell i joined to i +- 1 (the sampler reads positions only)."""
    i = np.arange(n)
    adj = np.stack([(i - 1) % n, (i + 1) % n], 1).reshape(-1).astype(np.int32)
    return np.arange(0, 2 * n + 1, 2, dtype=np.int32), adj


def canonical_triangles(tri):
    """Triangles as sorted rows of their corner triples, rotation-invariant (for comparing two orders of one triangulation)."""
    t = np.asarray(tri).reshape(-1, 3)
    k = np.argmin(t, axis=1)
    rot = np.stack([t[np.arange(t.shape[0]), (k + j) % 3] for j in range(3)], 1)
    return rot[np.lexsort(rot.T[::-1])]
