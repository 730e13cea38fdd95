"""Rivers and lakes over the C ABI, on a device-resident planet (ours: the reference keeps no drainage; csrc/rivers.hip, the contract
is in csrc/rivers_ops.h).

``compute_rivers`` drains the final terrain: every land cell (elevation > 0) to its lowest neighbour, depressions resolved by
spilling over their lowest pass so that rivers reach the sea, lakes where a basin lies below its water level, and the runoff
accumulated down the receivers in exact fixed point.  The five fields stay on the planet; ``download`` fetches one,
``river_lines`` gives the segments of the cells whose flow reaches a threshold, ``color_map_rivers`` paints them and the lakes over
``map_export.color``.  ``r_river_flow`` is an ordinary per-region field: ``map_export.color_layer(planet, 'debug', flow)`` shows it.
There is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import capi
from . import climate_blocks as CB
from . import map_export as ME
from . import terrain_post as TP

# the runoff sources in the order of WO_RIVERS_RUNOFF_PRECIP, _UNIFORM, _VALUES (include/worogen.h)
RUNOFF = ("precip", "uniform", "values")
BLOCK = CB.Block("wo_rivers", (("r_river_receiver", np.int32), ("r_river_basin", np.int32), ("r_lake_level", np.float32), ("r_river_discharge", np.uint64),
                               ("r_river_flow", np.float32)))
FIELDS = tuple(k for k, _ in BLOCK.fields)
TINT = (41, 98, 168, 255)


class RiversInfo(C.Structure):
    _fields_ = [(k, C.c_int32) for k in ("landCells", "pits", "spilledBasins", "endorheicBasins", "lakeCells", "rounds", "launches")]


def compute_rivers(planet: TP.Planet, r_elevation=None, runoff="precip", download: bool = False) -> dict:
    """The drainage of r_elevation (None: the planet's resident field).  runoff: 'precip' (the mean of the planet's two resident
    precipitation fields, computed or uploaded), 'uniform' (1 per land cell) or an array of numRegions floats.
    -> the counts of wo_rivers_info, and with download the five fields under their keys."""
    n = planet.numRegions
    e = CB.elevation_arg(n, r_elevation)
    values = None
    if isinstance(runoff, str):
        if runoff not in RUNOFF[:2]:
            raise ValueError(f"unknown runoff source '{runoff}' (one of precip, uniform, or an array of values)")
        source = RUNOFF.index(runoff)
    else:
        values = np.ascontiguousarray(runoff, dtype=np.float32).reshape(-1)
        if values.size != n:
            raise ValueError(f"runoff has {values.size} values, expected {n}")
        source = 2
    info = RiversInfo()
    capi.check(capi.lib().wo_compute_rivers(planet.handle, n, capi.ptr(e), source, capi.ptr(values), C.byref(info)), "computeRivers")
    res = {k: int(getattr(info, k)) for k, _ in RiversInfo._fields_}
    if download:
        res.update({k: CB.download(planet, BLOCK, k) for k in FIELDS})
    return res


def download(planet: TP.Planet, field: str) -> np.ndarray:
    """One field of the planet's rivers block by its key (FIELDS)."""
    return CB.download(planet, BLOCK, field)


def river_lines(planet: TP.Planet, min_flow: float, r_elevation=None) -> dict:
    """The segments of the river cells under min_flow, in ascending cell order -> {segments float32 (count, 2, 3), flows float32
    (count,)}; r_elevation (None: the resident field) displaces the ends."""
    n = planet.numRegions
    e = CB.elevation_arg(n, r_elevation)
    seg, flows = np.empty((n, 2, 3), np.float32), np.empty(n, np.float32)
    count = np.zeros(1, np.int64)
    capi.check(capi.lib().wo_river_lines(planet.handle, float(min_flow), capi.ptr(e), capi.ptr(seg), capi.ptr(flows), n, capi.ptr(count)), "riverLines")
    k = int(count[0])
    return dict(segments=seg[:k].copy(), flows=flows[:k].copy())


def color_map_rivers(planet: TP.Planet, type, min_flow: float, r_elevation=None, width: int | None = None) -> np.ndarray:
    """map_export.color with the river cells under min_flow and the lakes painted TINT."""
    e = CB.elevation_arg(planet.numRegions, r_elevation)
    out = np.empty(ME._map_shape(planet, width) + (4,), np.uint8)
    capi.check(capi.lib().wo_map_color_rivers(planet.handle, ME.type_id(type), capi.ptr(e), float(min_flow), capi.ptr(out), out.nbytes), "mapColorRivers")
    return out
