"""Seasonal precipitation (js/precipitation.js) over the C ABI: the reference's names, snake-cased, on a device-resident planet.

``compute_precipitation`` is the reference's ``computePrecipitation`` (js/precipitation.js:196-684 with js/heuristic-precip.js):
the smoothed elevation's gradient, the blended winds, convergence, moisture advection, the mechanisms loop, the rain-shadow
propagations, the heuristic model, the blend and its percentile run in HIP kernels (csrc/precip.hip; exactness contract in
csrc/precip_ops.h).  The stage reads the planet's wind block (``wind.compute_wind``, or a caller's ``windResult`` uploaded key
by key) and the two warmth fields of its ocean block (``ocean.compute_ocean_currents``, or ``ocean.upload``); its result stays
on the device in the planet's precipitation block, and the returned dict holds host copies under the reference's result keys
(without ``_precipTiming``).  There is no CPU fallback.
"""
from __future__ import annotations

import numpy as np

from . import capi
from . import climate_blocks as CB
from . import ocean as OD
from . import terrain_post as TP
from . import wind as WD

# the reference's result keys (js/precipitation.js:640-641, :678), all Float32Array
RESULT_FIELDS = tuple((k, np.float32) for k in ("r_precip_summer", "r_precip_winter", "r_rainshadow_summer", "r_rainshadow_winter"))
BLOCK = CB.Block("wo_precip", RESULT_FIELDS)
# the keys of windResult and of oceanResult the stage reads
WIND_INPUTS = ("r_lat", "r_lon", "r_isLand", "r_continentality", "r_coastDistLand", "r_eastX", "r_eastY", "r_eastZ", "r_northX", "r_northY", "r_northZ",
               "itczLons", "itczLatsSummer", "itczLatsWinter", "r_wind_east_summer", "r_wind_north_summer", "r_pressure_summer",
               "r_wind_east_winter", "r_wind_north_winter", "r_pressure_winter")
OCEAN_INPUTS = ("r_ocean_warmth_summer", "r_ocean_warmth_winter")
INFO_FIELDS = ("maxHops", "elevSmoothPasses", "convSmoothPasses", "shadowHops", "windwardHops", "rsSmoothPasses", "precipSmoothPasses", "wcPasses", "leeCoastHops",
               "upCountSummer", "downCountSummer", "upCountWinter", "downCountWinter", "depletionBase", "shadowDecay", "windwardDecay", "p95Summer", "p95Winter")
# wo_precip_info: 13 int32 and one reserved, three doubles, two floats
_INFO_DTYPE = np.dtype([("counts", np.int32, 13), ("reserved", np.int32), ("decay", np.float64, 3), ("p95", np.float32, 2)])
assert _INFO_DTYPE.itemsize == 88


def download(planet: TP.Planet, field: str) -> np.ndarray:
    """One field of the planet's precipitation block by the reference's result key."""
    return CB.download(planet, BLOCK, field)


def upload(planet: TP.Planet, field: str, data) -> None:
    """Set one field of the planet's precipitation block from the host by its result key."""
    CB.upload(planet, BLOCK, field, data)


def info(planet: TP.Planet) -> dict:
    """The scalars of the planet's last compute_precipitation: pass counts, list lengths, the three decay scalars, both maxPrecip."""
    return dict(planet.precip_info)


def compute_precipitation(planet: TP.Planet, r_xyz, r_elevation, wind_result=None, ocean_result=None, precipitation_offset=0, land_coverage=0.3,
                          fields=None) -> dict:
    """computePrecipitation(mesh, r_xyz, r_elevation, windResult, oceanResult, precipitationOffset, landCoverage) on the planet's mesh.

    r_xyz is the planet's (only its size is checked; None is accepted); r_elevation None means the planet's resident field.
    wind_result / ocean_result None mean the planet's resident blocks; a dict is uploaded first (the keys of WIND_INPUTS /
    OCEAN_INPUTS are required, other result keys are uploaded too, anything else is ignored).  fields: the result keys to bring
    back (default: all).  Every argument is checked before any device work."""
    n = planet.numRegions
    CB.check_xyz(n, r_xyz)
    e = CB.elevation_arg(n, r_elevation)
    offset, coverage = float(precipitation_offset), float(land_coverage)
    if offset != offset or coverage != coverage:
        raise ValueError("precipitation_offset and land_coverage must be numbers")
    if fields is not None:
        unknown = [k for k in fields if k not in dict(RESULT_FIELDS)]
        if unknown:
            raise KeyError(unknown[0])
    wind_up = CB.checked_inputs(n, wind_result, WIND_INPUTS, WD.BLOCK, "wind_result")
    ocean_up = CB.checked_inputs(n, ocean_result, OCEAN_INPUTS, OD.BLOCK, "ocean_result")
    CB.upload_inputs(planet, WD.BLOCK, wind_up)
    CB.upload_inputs(planet, OD.BLOCK, ocean_up)
    raw = np.zeros(1, _INFO_DTYPE)
    capi.check(capi.lib().wo_compute_precipitation(planet.handle, n, capi.ptr(e), offset, coverage, capi.ptr(raw)), "computePrecipitation")
    vals = [int(v) for v in raw["counts"][0]] + [float(v) for v in raw["decay"][0]] + [float(v) for v in raw["p95"][0]]
    planet.precip_info = dict(zip(INFO_FIELDS, vals))
    return {k: download(planet, k) for k, _ in RESULT_FIELDS if fields is None or k in fields}
