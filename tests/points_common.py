"""Shared by the tests of the device point generator (csrc/points_ops.h, csrc/points.hip): the host emulator of the shared bodies
(tests/emu_points), the inputs the GPU tests use, and the fixtures."""
from __future__ import annotations

import ctypes as C
import json
import subprocess
import zlib
from functools import lru_cache

import numpy as np

from conftest import GOLDEN, REPO

EMU_DIR = REPO / "tests" / "emu_points"
# the sizes at which the chain tables were checked against the serial loop
CHAIN_SIZES = (1, 2, 3, 4, 7, 63, 2000, 5000, 12345, 65536, 999983, 10 ** 6, 2 ** 20, 10 ** 7, 10 ** 7 + 1, 2 ** 24, 4 * 10 ** 7)
SEEDS = (1, 7, 0.5, -3, 2147483645)
# the device test's inputs: 700 000 is the smallest size at which the large reduction runs; 255, 256 and 257 straddle a workgroup
GPU_SIZES = (1, 2, 3, 7, 63, 255, 256, 257, 2000, 5000, 65536, 700000, 1000000)
JITTERS = (0.0, 0.75, 1.0)
SMALL = (1, 7, 257, 2000)
GPU_CASES = tuple((N, j, 1) for N in GPU_SIZES for j in JITTERS) + tuple((N, 0.75, s) for N in SMALL for s in SEEDS[1:])
_emu = None


def emu():
    global _emu
    if _emu is None:
        subprocess.run(["make", "-s", "-C", str(EMU_DIR)], check=True)
        _emu = C.CDLL(str(EMU_DIR / "_build" / "libemu_points.so"))
        for f in ("emu_chain_mismatches", "emu_chain_mismatches_of", "emu_jump_mismatches", "emu_lonr_samples"):
            getattr(_emu, f).restype = C.c_int64
        _emu.emu_seed_state.restype = C.c_uint32
    return _emu


def ptr(a):
    assert a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(C.c_void_p)


@lru_cache(maxsize=None)
def emu_points(N, jitter, seed):
    """3 (N + 1) floats of the shared body, the pole last; read-only, shared among the tests"""
    out = np.empty(3 * (N + 1), np.float32)
    assert emu().emu_fib_points(C.c_int32(N), C.c_double(jitter), C.c_double(seed), ptr(out)) == 0
    out.flags.writeable = False
    return out


def emu_trig(name, x):
    x = np.ascontiguousarray(x, np.float64)
    out = np.empty_like(x)
    getattr(emu(), name)(C.c_int64(x.size), ptr(x), ptr(out))
    return out


def lonr_samples(N, jitter, seed, stride):
    out = np.empty((N + stride - 1) // stride, np.float64)
    assert emu().emu_lonr_samples(C.c_int32(N), C.c_double(jitter), C.c_double(seed), C.c_int32(stride), ptr(out)) == out.size
    return out


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    u = np.uint32 if a.dtype == np.float32 else np.uint64
    return a.shape == b.shape and a.dtype == b.dtype and bool(np.all((a.view(u) == b.view(u)) | (np.isnan(a) & np.isnan(b))))


def differing(a, b):
    u = np.uint32 if a.dtype == np.float32 else np.uint64
    return int(np.count_nonzero(np.ascontiguousarray(a).view(u) != np.ascontiguousarray(b).view(u)))


def large_cases():
    g = np.load(GOLDEN / "points_large.npz")
    return g, json.loads(bytes(g["meta_json"]).decode())


def crc32(a):
    return zlib.crc32(np.ascontiguousarray(a).tobytes()) & 0xFFFFFFFF
