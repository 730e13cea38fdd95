"""Shared pieces of the overlay tests: the golden fixtures of the reference's buildWindArrows, buildOceanCurrentArrows and rebuildGrids
(tests/golden/overlays_N2000_s1.npz, overlays_crafted.npz) and the host emulator of csrc/overlay_ops.h (tests/emu_overlay)."""
from __future__ import annotations

import ctypes as C
import functools
import json
import subprocess

import numpy as np

from conftest import GOLDEN, REPO
from map_common import ptr

EMU_DIR = REPO / "tests" / "emu_overlay"
BINS, ARROW_FLOATS = 7200, 18
WIND, OCEAN = 0, 1
SEASONS = ("summer", "winter")
WIND_KEYS = ("r_wind_east_{s}", "r_wind_north_{s}")
OCEAN_KEYS = ("r_ocean_current_east_{s}", "r_ocean_current_north_{s}", "r_ocean_speed_{s}", "r_ocean_warmth_{s}")
_emu = None


@functools.lru_cache(maxsize=None)
def golden():
    g = dict(np.load(GOLDEN / "overlays_N2000_s1.npz"))
    g["meta"] = json.loads(bytes(g["meta_json"]).decode())
    return g


@functools.lru_cache(maxsize=None)
def crafted():
    return dict(np.load(GOLDEN / "overlays_crafted.npz"))


def golden_fields(kind: int, season: str) -> list:
    """the golden's fields of one kind and season in the order the arrow pass reads them"""
    return [golden()["field_" + k.format(s=season)] for k in (OCEAN_KEYS if kind == OCEAN else WIND_KEYS)]


def emu():
    global _emu
    if _emu is None:
        subprocess.run(["make", "-s", "-C", str(EMU_DIR)], check=True)
        _emu = C.CDLL(str(EMU_DIR / "_build" / "libemu_overlay.so"))
        _emu.emu_overlay_arrows.restype = C.c_int64
    return _emu


def _f32(a):
    return None if a is None else np.ascontiguousarray(a, np.float32).reshape(-1)


def emu_candidates(xyz, e=None, skip_land=False):
    """-> (bin int32 [N] (-1: none), d2 float64 [N])"""
    xyz, e = _f32(xyz), _f32(e)
    n = xyz.size // 3
    assert not skip_land or e.size == n
    idx, d2 = np.empty(n, np.int32), np.empty(n, np.float64)
    emu().emu_overlay_candidates(C.c_int32(n), ptr(xyz), ptr(e), C.c_int32(1 if skip_land else 0), ptr(idx), ptr(d2))
    return idx, d2


def emu_pick(idx, d2, bins=BINS, form="keys"):
    """the winners of candidates (idx, d2) by the reference's loop (form 'loop') or by the minimum of the keys"""
    idx, d2 = np.ascontiguousarray(idx, np.int32), np.ascontiguousarray(d2, np.float64)
    assert idx.size == d2.size and (idx < bins).all()
    out = np.empty(bins, np.int32)
    getattr(emu(), "emu_overlay_pick_" + form)(C.c_int32(idx.size), ptr(idx), ptr(d2), C.c_int32(bins), ptr(out))
    return out


def emu_winners(xyz, e=None, skip_land=False, form="keys"):
    return emu_pick(*emu_candidates(xyz, e, skip_land), BINS, form)


def emu_arrows(kind, xyz, winners, fields, center_lon=0.0, outputs=(True, True, True, True)):
    """-> (count, [globe position, globe colour, map position, map colour]: float32 [count * 18] or None where not asked for)"""
    xyz, winners = _f32(xyz), np.ascontiguousarray(winners, np.int32)
    f = [_f32(a) for a in fields] + [None] * (4 - len(fields))
    assert winners.size == BINS and len(fields) == (4 if kind == OCEAN else 2)
    bufs = [np.empty(BINS * ARROW_FLOATS, np.float32) if o else None for o in outputs]
    n = emu().emu_overlay_arrows(C.c_int32(kind), ptr(xyz), ptr(winners), ptr(f[0]), ptr(f[1]), ptr(f[2]), ptr(f[3]), C.c_double(center_lon), *[ptr(b) for b in bufs])
    return int(n), [None if b is None else b[: n * ARROW_FLOATS].copy() for b in bufs]


def emu_call(kind, xyz, e, fields, center_lon=0.0, form="keys"):
    """a whole call as wo_overlay_arrows makes it: the bins (the ocean form skips land), then the arrows"""
    winners = emu_winners(xyz, e, kind == OCEAN, form)
    n, arrays = emu_arrows(kind, xyz, winners, fields, center_lon)
    return winners, n, arrays


def round_kinds(d2):
    """per candidate whether its d2 rounds up when it is stored as f32"""
    d2 = np.asarray(d2, np.float64)
    return d2 < d2.astype(np.float32).astype(np.float64)
