"""Seasonal temperature (js/temperature.js) over the C ABI: the reference's names, snake-cased, on a device-resident planet.

``compute_temperature`` is the reference's ``computeTemperature`` (js/temperature.js:69-237): the diffusion of ocean warmth onto
coastal land, the per-cell loop, the smoothing pass and the normalisation run in HIP kernels (csrc/temp.hip; contract in
csrc/temp_ops.h).  The stage reads the planet's wind block (``wind.compute_wind``, or a caller's ``windResult`` uploaded key by
key), the warmth and speed fields of its ocean block (``ocean.compute_ocean_currents``, or ``ocean.upload``) and
``r_precip_*`` of its precipitation block (``precipitation.compute_precipitation``, or ``precipitation.upload``); its result stays on the
device in the planet's temperature block, and the returned dict holds host copies under the reference's result keys (without
``_tempTiming``).  The reference's branches for missing inputs are not offered: a missing field is refused.  There is no CPU
fallback.
"""
from __future__ import annotations

import numpy as np

from . import capi
from . import climate_blocks as CB
from . import ocean as OD
from . import precipitation as PD
from . import terrain_post as TP
from . import wind as WD

# the reference's result keys (js/temperature.js:232), both Float32Array
RESULT_FIELDS = (("r_temperature_summer", np.float32), ("r_temperature_winter", np.float32))
BLOCK = CB.Block("wo_temperature", RESULT_FIELDS)
# the keys of windResult, oceanResult and precipResult the stage reads
WIND_INPUTS = ("r_lat", "r_lon", "r_isLand", "r_continentality", "r_plateContinentality", "itczLons", "itczLatsSummer", "itczLatsWinter")
OCEAN_INPUTS = ("r_ocean_warmth_summer", "r_ocean_speed_summer", "r_ocean_warmth_winter", "r_ocean_speed_winter")
PRECIP_INPUTS = ("r_precip_summer", "r_precip_winter")
INFO_FIELDS = ("oceanWarmthPasses", "smoothPasses", "launches")


def upload(planet: TP.Planet, field: str, data) -> None:
    """Set one field of the planet's temperature block from the host by its result key."""
    CB.upload(planet, BLOCK, field, data)


def download(planet: TP.Planet, field: str) -> np.ndarray:
    """One field of the planet's temperature block by the reference's result key."""
    return CB.download(planet, BLOCK, field)


def info(planet: TP.Planet) -> dict:
    """The scalars of the planet's last compute_temperature: oceanWarmthPasses, smoothPasses, the kernel launches of the call."""
    return dict(getattr(planet, "temperature_info", {}))


def compute_temperature(planet: TP.Planet, r_xyz, r_elevation, wind_result=None, ocean_result=None, precip_result=None, temperature_offset=0,
                        fields=None) -> dict:
    """computeTemperature(mesh, r_xyz, r_elevation, windResult, oceanResult, precipResult, temperatureOffset) on the planet's mesh.

    r_xyz is the planet's (only its size is checked; None is accepted); r_elevation None means the planet's resident field.
    wind_result / ocean_result / precip_result None mean the planet's resident blocks; a dict is uploaded first (the keys of
    WIND_INPUTS / OCEAN_INPUTS / PRECIP_INPUTS are required, other result keys are uploaded too, anything else is ignored).
    fields: the result keys to bring back (default: all).  Every argument is checked before any device work."""
    n = planet.numRegions
    CB.check_xyz(n, r_xyz)
    e = CB.elevation_arg(n, r_elevation)
    offset = float(temperature_offset)
    if offset != offset:
        raise ValueError("temperature_offset must be a number")
    if fields is not None:
        unknown = [k for k in fields if k not in dict(RESULT_FIELDS)]
        if unknown:
            raise KeyError(unknown[0])
    wind_up = CB.checked_inputs(n, wind_result, WIND_INPUTS, WD.BLOCK, "wind_result")
    ocean_up = CB.checked_inputs(n, ocean_result, OCEAN_INPUTS, OD.BLOCK, "ocean_result")
    precip_up = CB.checked_inputs(n, precip_result, PRECIP_INPUTS, PD.BLOCK, "precip_result")
    CB.upload_inputs(planet, WD.BLOCK, wind_up)
    CB.upload_inputs(planet, OD.BLOCK, ocean_up)
    CB.upload_inputs(planet, PD.BLOCK, precip_up)
    raw = np.zeros(4, np.int32)
    capi.check(capi.lib().wo_compute_temperature(planet.handle, n, capi.ptr(e), offset, capi.ptr(raw)), "computeTemperature")
    planet.temperature_info = dict(zip(INFO_FIELDS, (int(v) for v in raw[:3])))
    return {k: download(planet, k) for k, _ in RESULT_FIELDS if fields is None or k in fields}
