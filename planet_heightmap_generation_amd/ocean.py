"""Ocean surface currents (js/ocean.js) over the C ABI: the reference's names, snake-cased, on a device-resident planet.

``compute_ocean_currents`` is the reference's ``computeOceanCurrents`` (js/ocean.js:204-382): the coast seeds, the west and east
hop-distance fields, the circumpolar test, the band and deflection loop, the masked smoothing passes, classifyWarmth, the speeds
and their percentile run in HIP kernels (csrc/ocean.hip; exactness contract in csrc/ocean_ops.h).  The stage reads the planet's
wind block (left there by ``wind.compute_wind``, or filled from a caller's ``windResult`` by ``wind.upload``); its result stays
on the device in the planet's ocean block, and the returned dict holds host copies under the reference's result keys (without
``_oceanTiming``).  There is no CPU fallback.
"""
from __future__ import annotations

import numpy as np

from . import capi
from . import climate_blocks as CB
from . import terrain_post as TP
from . import wind as WD

# the reference's result keys in the order it sets them (js/ocean.js:374-377), all Float32Array
RESULT_FIELDS = tuple((f"r_ocean_{k}_{s}", np.float32) for s in ("summer", "winter") for k in ("current_east", "current_north", "speed", "warmth"))
BLOCK = CB.Block("wo_ocean", RESULT_FIELDS)
# the keys of windResult the stage reads
WIND_INPUTS = ("r_lat", "r_lon", "r_isLand", "r_eastX", "r_eastY", "r_eastZ", "itczLons", "itczLatsSummer", "itczLatsWinter")
INFO_FIELDS = ("circumpolarNH", "circumpolarSH", "coastThreshold", "warmthRange", "currentSmoothPasses", "warmthSmoothPasses",
               "oceanCellsSummer", "oceanCellsWinter", "p95Summer", "p95Winter")


def download(planet: TP.Planet, field: str) -> np.ndarray:
    """One field of the planet's ocean block by the reference's result key."""
    return CB.download(planet, BLOCK, field)


def upload(planet: TP.Planet, field: str, data) -> None:
    """Set one field of the planet's ocean block from the host by its result key."""
    CB.upload(planet, BLOCK, field, data)


def info(planet: TP.Planet) -> dict:
    """What the planet's last compute_ocean_currents found: the flags, thresholds, pass counts, ocean-speed counts and p95 values
    the reference logs."""
    return dict(planet.ocean_info)


def compute_ocean_currents(planet: TP.Planet, r_xyz, r_elevation, wind_result=None, fields=None) -> dict:
    """computeOceanCurrents(mesh, r_xyz, r_elevation, windResult) on the planet's mesh.

    r_xyz is the planet's (only its size is checked; None is accepted); r_elevation is accepted and unused, as in the reference.
    wind_result None means the planet's resident wind block; a dict is uploaded first (the keys of WIND_INPUTS are required,
    other keys of wind.RESULT_FIELDS are uploaded too, anything else is ignored).  fields: the result keys to bring back
    (default: all)."""
    n = planet.numRegions
    CB.check_xyz(n, r_xyz)
    CB.elevation_arg(n, r_elevation)
    wind_up = CB.checked_inputs(n, wind_result, WIND_INPUTS, WD.BLOCK, "wind_result")      # all refused before any device work
    CB.upload_inputs(planet, WD.BLOCK, wind_up)
    raw = np.zeros(10, np.int32)
    capi.check(capi.lib().wo_compute_ocean_currents(planet.handle, n, capi.ptr(raw)), "computeOceanCurrents")
    vals = [bool(raw[0]), bool(raw[1])] + [int(v) for v in raw[2:8]] + [float(v) for v in raw[8:10].view(np.float32)]
    planet.ocean_info = dict(zip(INFO_FIELDS, vals))
    return {k: download(planet, k) for k, _ in RESULT_FIELDS if fields is None or k in fields}
