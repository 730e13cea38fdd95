"""Seasonal precipitation (js/precipitation.js) over the C ABI: the reference's names, snake-cased, on a device-resident planet.

``compute_precipitation`` is the reference's ``computePrecipitation`` (js/precipitation.js:196-684 with js/heuristic-precip.js):
the smoothed elevation's gradient, the blended winds, convergence, moisture advection, the mechanisms loop, the rain-shadow
propagations, the heuristic model, the blend and its percentile run in HIP kernels (csrc/precip.hip; exactness contract in
csrc/precip_ops.h).  The stage reads the planet's wind block (``wind.compute_wind``, or a caller's ``windResult`` uploaded key
by key) and the two warmth fields of its ocean block (``ocean.compute_ocean_currents``, or ``upload_ocean``); its result stays
on the device in the planet's precipitation block, and the returned dict holds host copies under the reference's result keys
(without ``_precipTiming``).  There is no CPU fallback.
"""
from __future__ import annotations

import numpy as np

from . import capi
from . import ocean as OD
from . import terrain_post as TP
from . import wind as WD

# the reference's result keys (js/precipitation.js:640-641, :678), all Float32Array
RESULT_FIELDS = tuple((k, np.float32) for k in ("r_precip_summer", "r_precip_winter", "r_rainshadow_summer", "r_rainshadow_winter"))
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


def _ocean_field(n: int, field: str, data) -> np.ndarray:
    if field not in dict(OD.RESULT_FIELDS):
        raise KeyError(field)
    a = np.ascontiguousarray(data, dtype=np.float32).reshape(-1)
    if a.size != n:
        raise ValueError(f"{field} has {a.size} values, expected {n}")
    return a


def upload_ocean(planet: TP.Planet, field: str, data) -> None:
    """Set one field of the planet's ocean block from the host by its result key (ocean.RESULT_FIELDS)."""
    a = _ocean_field(planet.numRegions, field, data)
    capi.check(capi.lib().wo_ocean_upload(planet.handle, field.encode(), capi.ptr(a), a.nbytes), "wo_ocean_upload")


def download(planet: TP.Planet, field: str) -> np.ndarray:
    """One field of the planet's precipitation block by the reference's result key."""
    ty = dict(RESULT_FIELDS).get(field)
    if ty is None:
        raise KeyError(field)
    out = np.empty(planet.numRegions, ty)
    capi.check(capi.lib().wo_precip_download(planet.handle, field.encode(), capi.ptr(out), out.nbytes), "wo_precip_download")
    return out


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
    if r_xyz is not None and np.asarray(r_xyz).size != 3 * n:
        raise ValueError(f"r_xyz has {np.asarray(r_xyz).size} values, expected 3 * {n}")
    e = None
    if r_elevation is not None:
        e = np.ascontiguousarray(r_elevation, dtype=np.float32).reshape(-1)
        if e.size != n:
            raise ValueError(f"r_elevation has {e.size} values, expected {n}")
    offset, coverage = float(precipitation_offset), float(land_coverage)
    if offset != offset or coverage != coverage:
        raise ValueError("precipitation_offset and land_coverage must be numbers")
    if fields is not None:
        unknown = [k for k in fields if k not in dict(RESULT_FIELDS)]
        if unknown:
            raise KeyError(unknown[0])
    wind_up, ocean_up = {}, {}
    if wind_result is not None:
        missing = [k for k in WIND_INPUTS if wind_result.get(k) is None]
        if missing:
            raise ValueError(f"wind_result lacks {missing}")
        known = dict(WD.RESULT_FIELDS)
        wind_up = {k: OD._wind_field(n, k, v) for k, v in wind_result.items() if k in known and v is not None}
    if ocean_result is not None:
        missing = [k for k in OCEAN_INPUTS if ocean_result.get(k) is None]
        if missing:
            raise ValueError(f"ocean_result lacks {missing}")
        known = dict(OD.RESULT_FIELDS)
        ocean_up = {k: _ocean_field(n, k, v) for k, v in ocean_result.items() if k in known and v is not None}
    for k, a in wind_up.items():
        OD.upload_wind(planet, k, a)
    for k, a in ocean_up.items():
        upload_ocean(planet, k, a)
    raw = np.zeros(1, _INFO_DTYPE)
    capi.check(capi.lib().wo_compute_precipitation(planet.handle, n, capi.ptr(e), offset, coverage, capi.ptr(raw)), "computePrecipitation")
    vals = [int(v) for v in raw["counts"][0]] + [float(v) for v in raw["decay"][0]] + [float(v) for v in raw["p95"][0]]
    planet.precip_info = dict(zip(INFO_FIELDS, vals))
    return {k: download(planet, k) for k, _ in RESULT_FIELDS if fields is None or k in fields}
