"""What the climate stages share on the Python side: the result blocks a planet keeps on the device (wind, ocean, precipitation,
temperature), one field of a block down to the host or up from it by the reference's result key, a caller's result dict checked
and uploaded, and the two argument checks every stage makes.  The C side of the same path is csrc/stage_block.h.
"""
from __future__ import annotations

from typing import NamedTuple

import numpy as np

from . import capi
from . import terrain_post as TP

ITCZ_SAMPLES = 360


class Block(NamedTuple):
    prefix: str         # of its C entry points: <prefix>_download, <prefix>_upload
    fields: tuple       # (result key, dtype) in the order of the block's fields


def size_of(n: int, field: str) -> int:
    """Entries of a field on a planet of n cells: the ITCZ arrays are per longitude sample, everything else per cell."""
    return ITCZ_SAMPLES if field.startswith("itcz") else n


def _dtype(block: Block, field: str):
    ty = dict(block.fields).get(field)
    if ty is None:
        raise KeyError(field)
    return ty


def checked_field(n: int, block: Block, field: str, data) -> np.ndarray:
    """data as the block takes the field: contiguous, of the field's dtype and size."""
    a = np.ascontiguousarray(data, dtype=_dtype(block, field)).reshape(-1)
    if a.size != size_of(n, field):
        raise ValueError(f"{field} has {a.size} values, expected {size_of(n, field)}")
    return a


def download(planet: TP.Planet, block: Block, field: str) -> np.ndarray:
    """One field of the planet's block by the reference's result key."""
    out = np.empty(size_of(planet.numRegions, field), _dtype(block, field))
    fn = f"{block.prefix}_download"
    capi.check(getattr(capi.lib(), fn)(planet.handle, field.encode(), capi.ptr(out), out.nbytes), fn)
    return out


def upload(planet: TP.Planet, block: Block, field: str, data) -> None:
    """Set one field of the planet's block from the host by its result key."""
    a = checked_field(planet.numRegions, block, field, data)
    fn = f"{block.prefix}_upload"
    capi.check(getattr(capi.lib(), fn)(planet.handle, field.encode(), capi.ptr(a), a.nbytes), fn)


def checked_inputs(n: int, result, required, block: Block, what: str) -> dict:
    """The fields of a caller's result dict that the block knows, checked; the required ones must be there.  None: {}."""
    if result is None:
        return {}
    missing = [k for k in required if result.get(k) is None]
    if missing:
        raise ValueError(f"{what} lacks {missing}")
    known = dict(block.fields)
    return {k: checked_field(n, block, k, v) for k, v in result.items() if k in known and v is not None}


def upload_inputs(planet: TP.Planet, block: Block, checked: dict) -> None:
    for k, a in checked.items():
        upload(planet, block, k, a)


def check_xyz(n: int, r_xyz) -> None:
    """r_xyz is the planet's: only its size is checked; None is accepted."""
    if r_xyz is not None and np.asarray(r_xyz).size != 3 * n:
        raise ValueError(f"r_xyz has {np.asarray(r_xyz).size} values, expected 3 * {n}")


def elevation_arg(n: int, r_elevation):
    """r_elevation as the C ABI takes it: contiguous float32 of n values, or None for the planet's resident field."""
    if r_elevation is None:
        return None
    e = np.ascontiguousarray(r_elevation, dtype=np.float32).reshape(-1)
    if e.size != n:
        raise ValueError(f"r_elevation has {e.size} values, expected {n}")
    return e
