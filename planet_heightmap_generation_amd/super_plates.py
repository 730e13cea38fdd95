"""Python mirror of the reference's ``buildSuperPlates`` (js/super-plates.js:16-273) over the C ABI.

``build_super_plates(mesh, r_plate, plateSeeds, plateVec, plateIsOcean, plateDensity)`` takes the reference's argument list
(Sets -> iterables in insertion order, keyed objects -> dicts) and returns the reference's result object as a dict — the shape
``elevation.assign_elevation`` accepts as ``superPlateData``.  The per-cell passes (plate areas, plate adjacency, the final
gather) run in HIP kernels on the planet's CSR, the plate-level part in native host code (csrc/super_plates_host.cc).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import capi
from .elevation import _table
from .terrain_post import Planet, _planet_for

MAX_PLATES = 1024          # include/worogen.h: WO_SUPER_MAX_PLATES


def super_plate_tables(planet: Planet, r_plate, plateSeeds):
    """The device half alone: (area int32[P], firstSlot uint32[P, P]) by position in plateSeeds (wo_super_plate_tables)."""
    r_plate = np.ascontiguousarray(r_plate, np.int32)
    seeds = np.ascontiguousarray(list(plateSeeds), np.int32)
    if r_plate.size != planet.numRegions:
        raise ValueError("r_plate must have numRegions entries")
    P = max(1, min(int(seeds.size), MAX_PLATES))          # (a count outside the limits is the library's to report)
    area = np.zeros(P, np.int32); first = np.zeros(P * P, np.uint32)
    capi.check(capi.lib().wo_super_plate_tables(planet.handle, capi.ptr(r_plate), capi.ptr(seeds), seeds.size, capi.ptr(area), capi.ptr(first)),
               "superPlateTables")
    return area, first.reshape(P, P)


def build_super_plates(mesh, r_plate, plateSeeds, plateVec, plateIsOcean, plateDensity, planet: Planet | None = None):
    pl = planet or _planet_for(mesh)
    r_plate = np.ascontiguousarray(r_plate, np.int32)
    if r_plate.size != pl.numRegions:
        raise ValueError("r_plate must have numRegions entries")
    seeds = np.ascontiguousarray(list(plateSeeds), np.int32)
    P = int(seeds.size)
    # dense by plate id, wide enough for every seed
    t, keep = _table(set(plateIsOcean), plateVec, plateDensity, ids=[s for s in seeds.tolist() if s >= 0])
    room = max(P, 1)
    r_super = np.empty(pl.numRegions, np.int32); ns = np.zeros(1, np.int32)
    pole = np.zeros(3 * room); omega = np.zeros(room); is_ocean = np.zeros(room, np.uint8); dens = np.zeros(room)
    capi.check(capi.lib().wo_build_super_plates(pl.handle, capi.ptr(r_plate), C.byref(t), capi.ptr(seeds), P, capi.ptr(r_super), capi.ptr(ns),
                                                capi.ptr(pole), capi.ptr(omega), capi.ptr(is_ocean), capi.ptr(dens)), "buildSuperPlates")
    n = int(ns[0])
    return {"r_superPlate": r_super,
            "superPlateVec": {s: {"pole": pole[3 * s:3 * s + 3].tolist(), "omega": float(omega[s])} for s in range(n)},
            "superPlateIsOcean": {s for s in range(n) if is_ocean[s]},
            "superPlateDensity": {s: float(dens[s]) for s in range(n)},
            "numSuperPlates": n,
            "_timing": [{"stage": k, "ms": v} for k, v in pl.last_stage_timing().items()]}
