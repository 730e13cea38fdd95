"""Seasonal pressure and wind (js/wind.js) over the C ABI: the reference's names, snake-cased, on a device-resident planet.

``compute_wind`` is the reference's ``computeWind`` (js/wind.js:394-687): every per-cell stage, the geographic index with its
disc samples, the ocean components, the two hop-distance fields, the smoothing passes and the percentile run in HIP kernels
(csrc/wind.hip; exactness contract in csrc/wind_ops.h).  The result stays on the device in the planet's wind block; the
returned dict holds host copies under the reference's result keys (without ``_windTiming``).  There is no CPU fallback.
"""
from __future__ import annotations

import numpy as np

from . import capi
from . import climate_blocks as CB
from . import terrain_post as TP

# the reference's result keys in the order it sets them (js/wind.js:649-683), with the dtype of each typed array
RESULT_FIELDS = (
    ("r_pressure_summer", np.float32), ("r_wind_east_summer", np.float32), ("r_wind_north_summer", np.float32), ("r_wind_speed_summer", np.float32),
    ("r_pressure_winter", np.float32), ("r_wind_east_winter", np.float32), ("r_wind_north_winter", np.float32), ("r_wind_speed_winter", np.float32),
    ("itczLons", np.float32), ("itczLatsSummer", np.float32), ("itczLatsWinter", np.float32),
    ("r_lat", np.float32), ("r_lon", np.float32), ("r_sinLat", np.float32), ("r_isLand", np.uint8),
    ("r_continentality", np.float32), ("r_coastDistLand", np.int32), ("r_plateContinentality", np.float32),
    ("r_eastX", np.float32), ("r_eastY", np.float32), ("r_eastZ", np.float32), ("r_northX", np.float32), ("r_northY", np.float32), ("r_northZ", np.float32),
)
BLOCK = CB.Block("wo_wind", RESULT_FIELDS)
ITCZ_SAMPLES = CB.ITCZ_SAMPLES


def smoothstep(edge0, edge1, x):
    """js/wind.js:75-79"""
    if edge0 == edge1:
        return 1 if x >= edge1 else 0
    t = max(0.0, min(1.0, (x - edge0) / (edge1 - edge0)))
    return t * t * (3 - 2 * t)


def _ocean_ids(plate_is_ocean) -> np.ndarray:
    if isinstance(plate_is_ocean, np.ndarray):
        ids = plate_is_ocean.reshape(-1)
        if ids.size and not np.issubdtype(ids.dtype, np.integer):
            raise TypeError("plate_is_ocean must hold integer plate ids")
    else:
        ids = list(plate_is_ocean)
        if any(not isinstance(v, (int, np.integer)) for v in ids):
            raise TypeError("plate_is_ocean must hold integer plate ids")
    return np.ascontiguousarray(ids, dtype=np.int32).reshape(-1)


def check_wind_args(n: int, r_xyz, r_elevation, plate_is_ocean, r_plate, seed, axial_tilt):
    """The arguments as the C ABI takes them; refused before any device work otherwise."""
    CB.check_xyz(n, r_xyz)
    e = CB.elevation_arg(n, r_elevation)
    if r_plate is None:
        raise ValueError("r_plate is required")
    plate = np.asarray(r_plate)
    if not np.issubdtype(plate.dtype, np.integer):
        raise TypeError("r_plate must hold integer plate ids (Int32Array in the reference)")
    plate = np.ascontiguousarray(plate, dtype=np.int32).reshape(-1)
    if plate.size != n:
        raise ValueError(f"r_plate has {plate.size} values, expected {n}")
    ids = _ocean_ids(plate_is_ocean)
    seed, axial_tilt = float(seed), float(axial_tilt)
    if seed != seed or axial_tilt != axial_tilt:
        raise ValueError("seed and axial_tilt must be numbers")
    return e, plate, ids, seed, axial_tilt


def download(planet: TP.Planet, field: str) -> np.ndarray:
    """One field of the planet's wind block by the reference's result key."""
    return CB.download(planet, BLOCK, field)


def upload(planet: TP.Planet, field: str, data) -> None:
    """Set one field of the planet's wind block from the host by its result key."""
    CB.upload(planet, BLOCK, field, data)


def compute_wind(planet: TP.Planet, r_xyz, r_elevation, plate_is_ocean, r_plate, seed, axial_tilt=23.5, fields=None) -> dict:
    """computeWind(mesh, r_xyz, r_elevation, plateIsOcean, r_plate, noise, axialTilt) on the planet's mesh.

    r_xyz is the planet's (only its size is checked; None is accepted); r_elevation None means the planet's resident field;
    plate_is_ocean is the reference's Set of ocean plate ids (any iterable of ints); seed is the seed of the reference's
    SimplexNoise instance.  fields: the result keys to bring back (default: all)."""
    e, plate, ids, seed, axial_tilt = check_wind_args(planet.numRegions, r_xyz, r_elevation, plate_is_ocean, r_plate, seed, axial_tilt)
    levels = np.zeros(2, np.int32)
    capi.check(capi.lib().wo_compute_wind(planet.handle, planet.numRegions, capi.ptr(e), capi.ptr(plate), capi.ptr(ids) if ids.size else None,
                                          int(ids.size), seed, axial_tilt, capi.ptr(levels)), "computeWind")
    planet.wind_bfs_levels = (int(levels[0]), int(levels[1]))
    return {k: download(planet, k) for k, _ in RESULT_FIELDS if fields is None or k in fields}


def bfs_levels(planet: TP.Planet) -> tuple[int, int]:
    """Levels the coast / plate distance fields of the planet's last compute_wind took."""
    return planet.wind_bfs_levels


def compute_gradients(planet: TP.Planet, r_pressure, r_eastX, r_eastY, r_eastZ, r_northX, r_northY, r_northZ):
    """computeGradients (js/wind.js:306-339) on the planet's mesh; returns (r_gradE, r_gradN)."""
    n = planet.numRegions
    arrs = [np.ascontiguousarray(a, dtype=np.float32).reshape(-1) for a in (r_pressure, r_eastX, r_eastY, r_eastZ, r_northX, r_northY, r_northZ)]
    for a in arrs:
        if a.size != n:
            raise ValueError(f"an array has {a.size} values, expected {n}")
    east, north = np.concatenate(arrs[1:4]), np.concatenate(arrs[4:7])
    ge, gn = np.empty(n, np.float32), np.empty(n, np.float32)
    capi.check(capi.lib().wo_compute_gradients(planet.handle, n, capi.ptr(arrs[0]), capi.ptr(east), capi.ptr(north), capi.ptr(ge), capi.ptr(gn)),
               "computeGradients")
    return ge, gn
