"""Koppen climate classes (js/koppen.js) over the C ABI: the reference's names, snake-cased, on a device-resident planet.

``classify_koppen`` is the reference's ``classifyKoppen`` (js/koppen.js:67-288): one HIP kernel, one thread per cell
(csrc/temp.hip; the body is csrc/temp_ops.h's koppen_cell).  It reads the elevation, the planet's temperature block
(``temperature.compute_temperature``, or a caller's ``tempResult`` uploaded) and ``r_precip_*`` of its precipitation block, and
returns the class ids as a uint8 array; they also stay on the device in the planet's Koppen block.  Given the same inputs every
cell has the reference's class.  ``KOPPEN_CLASSES`` is the reference's table: id -> code, name, colour.  There is no CPU fallback.
"""
from __future__ import annotations

import numpy as np

from . import capi
from . import climate_blocks as CB
from . import precipitation as PD
from . import temperature as TD
from . import terrain_post as TP

# js/koppen.js:19-51: index = class id
KOPPEN_CLASSES = (
    dict(code="Ocean", name="Ocean", color=(0.29, 0.44, 0.65)),
    dict(code="Af", name="Tropical rainforest", color=(0.00, 0.00, 1.00)),
    dict(code="Am", name="Tropical monsoon", color=(0.00, 0.47, 1.00)),
    dict(code="Aw", name="Tropical savanna", color=(0.27, 0.67, 0.98)),
    dict(code="BWh", name="Hot desert", color=(1.00, 0.00, 0.00)),
    dict(code="BWk", name="Cold desert", color=(1.00, 0.59, 0.59)),
    dict(code="BSh", name="Hot steppe", color=(0.96, 0.65, 0.00)),
    dict(code="BSk", name="Cold steppe", color=(1.00, 0.86, 0.39)),
    dict(code="Cfa", name="Humid subtropical", color=(0.78, 1.00, 0.31)),
    dict(code="Cfb", name="Oceanic", color=(0.39, 1.00, 0.31)),
    dict(code="Cfc", name="Subpolar oceanic", color=(0.20, 0.78, 0.00)),
    dict(code="Csa", name="Hot-summer Mediterranean", color=(1.00, 1.00, 0.00)),
    dict(code="Csb", name="Warm-summer Mediterranean", color=(0.78, 0.78, 0.00)),
    dict(code="Csc", name="Cold-summer Mediterranean", color=(0.59, 0.59, 0.00)),
    dict(code="Cwa", name="Humid subtropical (monsoon)", color=(0.59, 1.00, 0.59)),
    dict(code="Cwb", name="Subtropical highland", color=(0.39, 0.78, 0.39)),
    dict(code="Cwc", name="Cold subtropical highland", color=(0.20, 0.59, 0.20)),
    dict(code="Dfa", name="Hot-summer continental", color=(0.00, 1.00, 1.00)),
    dict(code="Dfb", name="Warm-summer continental", color=(0.22, 0.78, 1.00)),
    dict(code="Dfc", name="Subarctic", color=(0.00, 0.49, 0.49)),
    dict(code="Dfd", name="Extremely cold subarctic", color=(0.00, 0.27, 0.37)),
    dict(code="Dsa", name="Hot-summer continental (dry summer)", color=(0.90, 0.50, 1.00)),
    dict(code="Dsb", name="Warm-summer continental (dry summer)", color=(0.70, 0.35, 0.85)),
    dict(code="Dsc", name="Subarctic (dry summer)", color=(0.50, 0.20, 0.65)),
    dict(code="Dsd", name="Extremely cold subarctic (dry summer)", color=(0.35, 0.10, 0.45)),
    dict(code="Dwa", name="Hot-summer continental (monsoon)", color=(0.67, 0.69, 1.00)),
    dict(code="Dwb", name="Warm-summer continental (monsoon)", color=(0.43, 0.47, 0.78)),
    dict(code="Dwc", name="Subarctic (monsoon)", color=(0.29, 0.31, 0.78)),
    dict(code="Dwd", name="Extremely cold subarctic (monsoon)", color=(0.20, 0.00, 0.53)),
    dict(code="ET", name="Tundra", color=(0.70, 0.70, 0.70)),
    dict(code="EF", name="Ice cap", color=(0.41, 0.41, 0.41)),
)
TEMP_INPUTS = ("r_temperature_summer", "r_temperature_winter")
PRECIP_INPUTS = ("r_precip_summer", "r_precip_winter")


def download(planet: TP.Planet) -> np.ndarray:
    """The class ids of the planet's Koppen block."""
    out = np.empty(planet.numRegions, np.uint8)
    capi.check(capi.lib().wo_koppen_download(planet.handle, capi.ptr(out), out.nbytes), "wo_koppen_download")
    return out


def classify_koppen(planet: TP.Planet, r_elevation, temp_result=None, precip_result=None) -> np.ndarray:
    """classifyKoppen(mesh, r_elevation, tempResult, precipResult) on the planet's mesh: a uint8 array of class ids.

    r_elevation None means the planet's resident field.  temp_result / precip_result None mean the planet's resident blocks; a
    dict is uploaded first (both keys of TEMP_INPUTS / PRECIP_INPUTS are required).  Every argument is checked before any device
    work."""
    n = planet.numRegions
    e = CB.elevation_arg(n, r_elevation)
    temp_up = CB.checked_inputs(n, temp_result, TEMP_INPUTS, TD.BLOCK, "temp_result")
    precip_up = CB.checked_inputs(n, precip_result, PRECIP_INPUTS, PD.BLOCK, "precip_result")
    CB.upload_inputs(planet, TD.BLOCK, temp_up)
    CB.upload_inputs(planet, PD.BLOCK, precip_up)
    capi.check(capi.lib().wo_classify_koppen(planet.handle, n, capi.ptr(e)), "classifyKoppen")
    return download(planet)
