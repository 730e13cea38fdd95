"""The line overlays of the reference's views (js/planet-mesh.js): the wind and ocean-current arrows (buildWindArrows :1289-1465,
buildOceanCurrentArrows :1545-1720) over the C ABI on a device-resident planet, and on the host the ITCZ line of the pressure views
(:1498-1538) and the latitude / longitude grids (buildGlobeGrid :427-469, buildMapGrid :385-412).

Every array is the Float32Array the reference hands to three.js, bit for bit: the arrows by csrc/overlay_ops.h, the host parts by
numpy float64 arithmetic in the reference's operation order with V8's sin and cos (wo_v8_math).  Each overlay comes in the globe
form and the map form.  The map form of the ITCZ line does not subtract the centre meridian: that is the reference's behaviour and
it is kept.  There is no CPU fallback for the arrows.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import capi
from . import climate_blocks as CB
from . import terrain_post as TP

BINS = 7200                                                   # WO_OVERLAY_BINS: 60 x 120 cells of 3 x 3 degrees
ARROW_FLOATS = 18
SEASONS = ("summer", "winter")
WIND, OCEAN = 0, 1
# how the reference's materials draw them (js/planet-mesh.js:1474, :1516, :474): the arrows by vertex colour at opacity 0.6, the ITCZ
# line 0x00ff88 opaque, the grid white at 0.12
ARROW_OPACITY = 0.6
ITCZ_COLOR = (0.0, 1.0, 0x88 / 255)
GRID_OPACITY = 0.12
R_ITCZ, R_GRID, GRID_SEGMENTS = 1.01, 1.002, 120
Z_ITCZ, Z_GRID = 0.003, 0.001


def _season(season) -> int:
    if season not in SEASONS:
        raise ValueError(f"unknown season {season!r} (one of {', '.join(SEASONS)})")
    return SEASONS.index(season)


def _v8(fn: int, x) -> np.ndarray:
    x = np.ascontiguousarray(x, np.float64).reshape(-1)
    out = np.empty_like(x)
    capi.check(capi.lib().wo_v8_math(fn, x.size, capi.ptr(x), capi.ptr(out)), "wo_v8_math")
    return out


def v8_sin(x) -> np.ndarray:
    return _v8(0, x)


def v8_cos(x) -> np.ndarray:
    return _v8(1, x)


# ---- the device calls ----------------------------------------------------------------------------------------------------------------
def grid_regions(planet: TP.Planet, skip_land: bool = False, r_elevation=None) -> np.ndarray:
    """The reference's gridRegions: per 3 x 3 degree cell the region closest to its centre, -1 for an empty cell.  skip_land is the
    ocean form (regions with r_elevation > 0 take no part; None means the planet's resident field).  -> int32 (7200)"""
    e = CB.elevation_arg(planet.numRegions, r_elevation) if skip_land else None
    out = np.empty(BINS, np.int32)
    capi.check(capi.lib().wo_overlay_bins(planet.handle, 1 if skip_land else 0, capi.ptr(e), capi.ptr(out)), "overlayBins")
    return out


def _arrows(planet: TP.Planet, kind: int, season, center_lon, r_elevation) -> dict:
    e = CB.elevation_arg(planet.numRegions, r_elevation)
    bufs = [np.empty(BINS * ARROW_FLOATS, np.float32) for _ in range(4)]
    count = C.c_int64(0)
    capi.check(capi.lib().wo_overlay_arrows(planet.handle, kind, _season(season), float(center_lon), capi.ptr(e), *[capi.ptr(b) for b in bufs], BINS, C.byref(count)),
               "overlayArrows")
    n = count.value * ARROW_FLOATS
    gp, gc, mp, mc = (b[:n].copy() for b in bufs)
    return dict(globe=dict(position=gp, color=gc), map=dict(position=mp, color=mc), count=count.value)


def wind_arrows(planet: TP.Planet, season, center_lon: float = 0.0) -> dict:
    """buildWindArrows of one season from the planet's wind block: dict(globe=dict(position, color), map=dict(position, color),
    count), 18 floats per arrow and array.  center_lon is the map view's centre meridian."""
    return _arrows(planet, WIND, season, center_lon, None)


def ocean_current_arrows(planet: TP.Planet, season, center_lon: float = 0.0, r_elevation=None) -> dict:
    """buildOceanCurrentArrows of one season from the planet's ocean block, land (r_elevation > 0; None: the resident field) left out."""
    return _arrows(planet, OCEAN, season, center_lon, r_elevation)


# ---- the ITCZ line -----------------------------------------------------------------------------------------------------------------
def itcz_line(itcz_lons, itcz_lats) -> dict:
    """The green line of the pressure views from the wind result's itczLons and one season's itczLats: dict(globe, map) of float32
    positions, six per segment.  The globe polyline closes; the map form leaves out the segment across the antimeridian."""
    lon = np.ascontiguousarray(itcz_lons, np.float32).reshape(-1).astype(np.float64)
    lat = np.ascontiguousarray(itcz_lats, np.float32).reshape(-1).astype(np.float64)
    if lon.size != lat.size:
        raise ValueError(f"itczLons has {lon.size} values and itczLats {lat.size}")
    n = lon.size
    if n == 0:
        return dict(globe=np.empty(0, np.float32), map=np.empty(0, np.float32))
    cos_lat = v8_cos(lat)
    p = np.stack([v8_sin(lon) * cos_lat * R_ITCZ, v8_sin(lat) * R_ITCZ, v8_cos(lon) * cos_lat * R_ITCZ], axis=1)
    nxt = (np.arange(n) + 1) % n
    with np.errstate(over="ignore", invalid="ignore"):
        globe = np.concatenate([p, p[nxt]], axis=1).astype(np.float32).reshape(-1)
        sx = 2 / math.pi
        mx, my = lon * sx, lat * sx
        keep = ~(np.abs(mx[nxt] - mx) > 1)
        z = np.full(n, Z_ITCZ)
        flat = np.stack([mx, my, z, mx[nxt], my[nxt], z], axis=1)[keep].astype(np.float32).reshape(-1)
    return dict(globe=globe, map=flat)


def itcz(planet: TP.Planet, season) -> dict:
    """itcz_line of the planet's wind block."""
    from . import wind as W
    _season(season)
    return itcz_line(CB.download(planet, W.BLOCK, "itczLons"), CB.download(planet, W.BLOCK, "itczLats" + season.capitalize()))


# ---- the grids ---------------------------------------------------------------------------------------------------------------------
def _steps(first: float, last: float, spacing: float, closed: bool) -> list:
    """for (deg = first; deg <= last (or < last); deg += spacing), with the loop's own running sum"""
    spacing = float(spacing)
    if not (math.isfinite(spacing) and spacing > 0) or (last - first) / spacing > 100000:
        raise ValueError(f"the grid spacing is {spacing} degrees: it must be a positive number that gives at most 100000 lines")
    out, deg = [], float(first)
    while deg <= last if closed else deg < last:
        out.append(deg)
        deg += spacing
    return out


def globe_grid(spacing: float) -> np.ndarray:
    """buildGlobeGrid for a spacing in degrees: float32 positions, six per segment, circles of latitude (the poles left out), then
    meridians, 120 segments each, at radius 1.002."""
    R, SEG, PI = R_GRID, GRID_SEGMENTS, math.pi
    i = np.arange(SEG, dtype=np.float64)
    parts = []
    lats = np.array([d for d in _steps(-90, 90, spacing, True) if d != -90 and d != 90], np.float64)
    if lats.size:
        lat = lats * PI / 180
        cos_lat, y = v8_cos(lat)[:, None], (v8_sin(lat) * R)[:, None]
        lon0, lon1 = (i / SEG) * PI * 2, ((i + 1) / SEG) * PI * 2
        ys = np.broadcast_to(y, (lats.size, SEG))
        parts.append(np.stack([v8_sin(lon0)[None, :] * cos_lat * R, ys, v8_cos(lon0)[None, :] * cos_lat * R,
                               v8_sin(lon1)[None, :] * cos_lat * R, ys, v8_cos(lon1)[None, :] * cos_lat * R], axis=2).reshape(-1))
    lons = np.array(_steps(-180, 180, spacing, False), np.float64)
    if lons.size:
        lon = lons * PI / 180
        sin_lon, cos_lon = v8_sin(lon)[:, None], v8_cos(lon)[:, None]
        lat0, lat1 = -PI / 2 + (i / SEG) * PI, -PI / 2 + ((i + 1) / SEG) * PI
        c0, c1, s0, s1 = v8_cos(lat0)[None, :], v8_cos(lat1)[None, :], v8_sin(lat0)[None, :], v8_sin(lat1)[None, :]
        parts.append(np.stack([sin_lon * c0 * R, np.broadcast_to(s0 * R, (lons.size, SEG)), cos_lon * c0 * R,
                               sin_lon * c1 * R, np.broadcast_to(s1 * R, (lons.size, SEG)), cos_lon * c1 * R], axis=2).reshape(-1))
    return np.concatenate(parts).astype(np.float32) if parts else np.empty(0, np.float32)


def map_grid(spacing: float, center_lon: float = 0.0) -> np.ndarray:
    """buildMapGrid for a spacing in degrees around the centre meridian center_lon: float32 positions, six per segment, parallels then
    meridians, at z = 0.001."""
    PI, Z = math.pi, Z_GRID
    sx = 2 / PI
    center_lon = float(center_lon)
    center_deg = (0.0 if (center_lon != center_lon or center_lon == 0) else center_lon) * 180 / PI
    out = []
    for deg in _steps(-90, 90, spacing, True):
        y = (deg * PI / 180) * sx
        out += [-2, y, Z, 2, y, Z]
    for deg in _steps(-180, 180, spacing, True):
        off = deg - center_deg
        if off > 180:
            off -= 360
        elif off < -180:
            off += 360
        x = (off * PI / 180) * sx
        out += [x, -1, Z, x, 1, Z]
    return np.array(out, np.float64).astype(np.float32)


def grids(spacing: float, center_lon: float = 0.0) -> dict:
    return dict(globe=globe_grid(spacing), map=map_grid(spacing, center_lon))
