"""The editor's hit test and highlights (js/edit-mode.js:18-93, js/planet-mesh.js:953-1244) over the C ABI, on a device-resident
planet.

``pick`` is the reference's findNearestRegion for many directions at once: per direction the region of the planet's resident
positions with the greatest dot product, the lowest index among equals, -1 where no dot is above -2.  ``pick_globe`` and
``pick_map`` put the arithmetic of getHitInfoGlobe (a ray in the planet's local space against the sphere of radius 1.08) and of
getHitInfoMap (the inverse equirectangular projection around a centre meridian) in front of it.  ``set_highlight`` sets the editor
state the reference's updatePendingHighlight, updateHoverHighlight and updateKoppenHoverHighlight draw: while it is set,
``globe_export`` and ``map_export`` give the tinted colours with no further option; ``clear_highlight`` drops it.  Everything is
the reference's own bit for bit (csrc/pick_ops.h).  There is no CPU fallback.
"""
from __future__ import annotations

import numpy as np

from . import capi
from . import terrain_post as TP

MAX_QUERIES = 65536                                           # include/worogen.h: WO_PICK_MAX_QUERIES
PENDING_OCEAN, PENDING_LAND, HOVER_PLATE, HOVER_KOPPEN = 1, 2, 4, 8      # the bits of a region's class byte


def _queries(a, width: int, what: str) -> np.ndarray:
    q = np.ascontiguousarray(a, dtype=np.float64)
    if q.ndim == 1 and q.size == width:
        q = q.reshape(1, width)
    if q.ndim != 2 or q.shape[1] != width:
        raise ValueError(f"{what} must hold {width} doubles per query, got shape {q.shape}")
    if q.shape[0] > MAX_QUERIES:
        raise ValueError(f"{q.shape[0]} queries in one call, at most {MAX_QUERIES}")
    return q


def pick(planet: TP.Planet, directions, dots: bool = False):
    """findNearestRegion per direction (n x 3 doubles): int32 regions, -1 for none; with dots=True -> (regions, float64 dots), the
    winning dot or -2."""
    q = _queries(directions, 3, "directions")
    regions = np.full(q.shape[0], -1, np.int32)
    d = np.full(q.shape[0], -2.0, np.float64) if dots else None
    capi.check(capi.lib().wo_pick_regions(planet.handle, q.shape[0], capi.ptr(q), capi.ptr(regions), capi.ptr(d)), "pick")
    return (regions, d) if dots else regions


def directions_globe(rays):
    """getHitInfoGlobe's arithmetic on the host: rays n x 6 (origin, normalised direction) -> (directions n x 3, valid bool n)"""
    q = _queries(rays, 6, "rays")
    out, valid = np.empty((q.shape[0], 3), np.float64), np.zeros(q.shape[0], np.uint8)
    capi.check(capi.lib().wo_pick_directions_globe(q.shape[0], capi.ptr(q), capi.ptr(out), capi.ptr(valid)), "pickDirectionsGlobe")
    return out, valid.astype(bool)


def directions_map(points, center_lon: float = 0.0):
    """getHitInfoMap's arithmetic on the host: points n x 2 (wx, wy on the map plane) -> (directions n x 3, valid bool n)"""
    q = _queries(points, 2, "points")
    out, valid = np.empty((q.shape[0], 3), np.float64), np.zeros(q.shape[0], np.uint8)
    capi.check(capi.lib().wo_pick_directions_map(q.shape[0], capi.ptr(q), float(center_lon), capi.ptr(out), capi.ptr(valid)), "pickDirectionsMap")
    return out, valid.astype(bool)


def pick_globe(planet: TP.Planet, rays) -> np.ndarray:
    """getHitInfoGlobe for rays in the planet's local space: the region under each ray, -1 where it misses the sphere."""
    return pick(planet, directions_globe(rays)[0])


def pick_map(planet: TP.Planet, points, center_lon: float = 0.0) -> np.ndarray:
    """getHitInfoMap for points of the map plane: the region under each point, -1 outside the map."""
    return pick(planet, directions_map(points, center_lon)[0])


def set_highlight(planet: TP.Planet, r_plate, pending=(), plate_is_ocean=(), hovered_plate: int = -1, hovered_koppen: int = -1) -> dict:
    """The editor state: `pending` the plates queued for a rebuild (the reference's pendingToggles), `plate_is_ocean` the plates that
    are ocean now, hovered_plate and hovered_koppen as the reference's state holds them (-1: none).
    -> the regions per tint {pendingOcean, pendingLand, hoveredPlate, hoveredKoppen}"""
    n = planet.numRegions
    rp = np.ascontiguousarray(r_plate, dtype=np.int32).reshape(-1)
    if rp.size != n:
        raise ValueError(f"r_plate has {rp.size} values, expected {n}")
    ocean = set(int(i) for i in plate_is_ocean)
    ids = np.ascontiguousarray([int(i) for i in pending], dtype=np.int32)
    is_ocean = np.ascontiguousarray([1 if int(i) in ocean else 0 for i in ids], dtype=np.uint8)
    counts = np.zeros(4, np.int64)
    capi.check(capi.lib().wo_highlight_set(planet.handle, capi.ptr(rp), ids.size, capi.ptr(ids) if ids.size else None, capi.ptr(is_ocean) if ids.size else None,
                                           int(hovered_plate), int(hovered_koppen), capi.ptr(counts)), "setHighlight")
    return dict(zip(("pendingOcean", "pendingLand", "hoveredPlate", "hoveredKoppen"), (int(c) for c in counts)))


def clear_highlight(planet: TP.Planet) -> None:
    capi.check(capi.lib().wo_highlight_clear(planet.handle), "clearHighlight")
