"""Region outlines as ordered closed rings over the C ABI, on a device-resident planet, and their export as GeoJSON and SVG.

``build_outline`` traces the line where one class of cells ends and another begins (a coastline, a lake shore, a plate, a Koppen
zone, an elevation band) into rings on the device (csrc/outline.hip; the contract is in csrc/outline_ops.h): the directed boundary
sides of the Voronoi cells, ring after ring, every ring from its lowest side on, its class on the side of the side's own cell.
``outline_rings`` cuts the result into per-ring views, ``to_geojson`` and ``to_svg`` write them out, cut where a ring crosses the
map's edge.  Ours: the reference exports no outline.  There is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import json
import math

import numpy as np

from . import capi
from . import climate_blocks as CB
from . import terrain_post as TP

SOURCES = ("coast", "lakes", "koppen", "levels", "values")    # WO_OUTLINE_* of include/worogen.h, in order
FIELDS = ("sides", "ring_start", "ring_class", "ring_of_side")
GLOBE_BASE = 1.002                                            # where export_globe draws the rings: the base of the super-plate borders


class OutlineInfo(C.Structure):
    _fields_ = [(k, C.c_int32) for k in ("boundarySides", "rings", "longestRing", "rounds", "launches")]


def source_id(source) -> int:
    if isinstance(source, str):
        if source not in SOURCES:
            raise ValueError(f"unknown outline source '{source}' (one of {', '.join(SOURCES)})")
        return SOURCES.index(source)
    return int(source)


def outline_filename(source: str, seed, ext: str = "geojson") -> str:
    """The file name of an outline export.  Ours: the reference exports no outline."""
    return f"orogen-outline-{source}-{seed}.{ext}"


def _sides(mesh):
    tri = np.ascontiguousarray(mesh.triangles, dtype=np.int32)
    he = np.ascontiguousarray(mesh.halfedges, dtype=np.int32)
    if tri.shape != he.shape or tri.ndim != 1:
        raise ValueError("mesh.triangles and mesh.halfedges must be int32 arrays of numSides entries")
    return tri, he


def download(planet: TP.Planet, field: str, count: int) -> np.ndarray:
    """One field of the planet's outline block: int32 (count)."""
    out = np.empty(count, np.int32)
    capi.check(capi.lib().wo_outline_download(planet.handle, field.encode(), capi.ptr(out), out.nbytes), "outlineDownload")
    return out


def positions(planet: TP.Planet, count: int, base: float = GLOBE_BASE, r_elevation=None) -> np.ndarray:
    """The vertices of the planet's outline block on the globe: float32 (count, 3), the centres of the entries' triangles displaced
    as the globe's lines are, at `base` (0: the undisplaced centres)."""
    e = CB.elevation_arg(planet.numRegions, r_elevation)
    out = np.empty((count, 3), np.float32)
    capi.check(capi.lib().wo_outline_positions(planet.handle, float(base), capi.ptr(e), capi.ptr(out), out.size), "outlinePositions")
    return out


def lonlat(planet: TP.Planet, count: int) -> np.ndarray:
    """The vertices of the planet's outline block on the map: float64 (count, 2), longitude and latitude in radians."""
    out = np.empty((count, 2), np.float64)
    capi.check(capi.lib().wo_outline_lonlat(planet.handle, capi.ptr(out), out.size), "outlineLonLat")
    return out


def free(planet: TP.Planet) -> None:
    capi.check(capi.lib().wo_outline_free(planet.handle), "outlineFree")


def build_outline(planet: TP.Planet, mesh, source, r_elevation=None, values=None, levels=None, only_class=None, base=None, want_lonlat: bool = False) -> dict:
    """The rings of `source` ('coast', 'lakes', 'koppen', 'levels' with levels=[...], 'values' with values=int32 per region):
    {source, sides, ring_start, ring_class, ring_of_side, info[, xyz][, lonlat]}.  only_class: trace the rings of that class alone
    (None: of every class; every boundary edge then appears twice, once per class).  base: also give xyz, float32 (M, 3), at that
    base (r_elevation None: the resident field).  want_lonlat: also give lonlat, float64 (M, 2) in radians."""
    tri, he = _sides(mesh)
    n = planet.numRegions
    sid = source_id(source)
    e = CB.elevation_arg(n, r_elevation)
    v = None
    if values is not None:
        v = np.ascontiguousarray(values, dtype=np.int32).reshape(-1)
        if v.size != n:
            raise ValueError(f"values has {v.size} entries, expected {n}")
    lv = None if levels is None else np.ascontiguousarray(levels, dtype=np.float32).reshape(-1)
    info = OutlineInfo()
    only = -1 if only_class is None else int(only_class)
    capi.check(capi.lib().wo_outline_build(planet.handle, tri.size, capi.ptr(tri), capi.ptr(he), sid, capi.ptr(e if sid in (0, 3) else None), capi.ptr(v), capi.ptr(lv),
                                           0 if lv is None else lv.size, only, C.byref(info)), "outlineBuild")
    M, R = info.boundarySides, info.rings
    res = dict(source=SOURCES[sid] if 0 <= sid < len(SOURCES) else sid, info={k: getattr(info, k) for k, _ in OutlineInfo._fields_})
    for f, count in zip(FIELDS, (M, R + 1, R, M)):
        res[f] = download(planet, f, count)
    if base is not None:
        res["xyz"] = positions(planet, M, base, r_elevation)
    if want_lonlat:
        res["lonlat"] = lonlat(planet, M)
    return res


def outline_rings(result: dict) -> list:
    """One dict per ring, views into the result's arrays: {ring, class, sides[, xyz][, lonlat]}."""
    start = result["ring_start"]
    out = []
    for r in range(len(start) - 1):
        a, b = int(start[r]), int(start[r + 1])
        ring = {"ring": r, "class": int(result["ring_class"][r]), "sides": result["sides"][a:b]}
        for k in ("xyz", "lonlat"):
            if result.get(k) is not None:
                ring[k] = result[k][a:b]
        out.append(ring)
    return out


def ring_segments(result: dict) -> np.ndarray:
    """The rings as line segments, float32 (M * 6), every vertex joined to the next of its ring: what a LINES primitive draws.  The
    result must hold xyz (build_outline(base=...))."""
    if result.get("xyz") is None:
        raise ValueError("ring_segments needs the result's xyz (build_outline(..., base=...))")
    xyz, start = np.asarray(result["xyz"], np.float32).reshape(-1, 3), np.asarray(result["ring_start"], np.int64)
    follower = np.arange(xyz.shape[0]) + 1
    follower[start[1:] - 1] = start[:-1]
    return np.concatenate([xyz, xyz[follower]], axis=1).reshape(-1)


def ring_pieces(lon) -> list:
    """A closed ring of longitudes (radians) cut where two consecutive vertices differ by more than pi: index arrays into the ring,
    one per piece.  An uncut ring gives one piece that ends with its first vertex again; a cut one gives its pieces in ring order, the
    one that holds vertex 0 last."""
    lon = np.asarray(lon, np.float64)
    n = lon.size
    if n == 0:
        return []
    cut = np.flatnonzero(np.abs(lon - np.roll(lon, -1)) > math.pi)        # cut[i]: between vertex i and vertex i + 1 (cyclically)
    if cut.size == 0:
        return [np.append(np.arange(n), 0)]
    pieces = []
    for a, b in zip(cut, np.roll(cut, -1)):
        first, last = int(a) + 1, int(b)
        if last < first:
            last += n
        pieces.append(np.arange(first, last + 1) % n)
    return pieces


def _degrees(x: float) -> float:
    return x * 180.0 / math.pi


def to_geojson(result: dict, properties=None) -> str:
    """A FeatureCollection with one feature per ring, in degrees (longitude, latitude): a closed LineString; for a ring that crosses
    the map's edge the pieces between its cuts (a LineString for one, a MultiLineString for more), so that nothing streaks across
    the map.  Properties: ring, class, and
    the entries of `properties`.  The result must hold lonlat (build_outline(want_lonlat=True))."""
    if result.get("lonlat") is None:
        raise ValueError("to_geojson needs the result's lonlat (build_outline(..., want_lonlat=True))")
    features = []
    for ring in outline_rings(result):
        ll = ring["lonlat"]
        lines = []
        for idx in ring_pieces(ll[:, 0]):
            if idx.size == 1:
                idx = np.repeat(idx, 2)                           # a LineString has two positions at least
            lines.append([[_degrees(float(ll[i, 0])), _degrees(float(ll[i, 1]))] for i in idx])
        geometry = {"type": "LineString", "coordinates": lines[0]} if len(lines) == 1 else {"type": "MultiLineString", "coordinates": lines}
        props = {"ring": ring["ring"], "class": ring["class"]}
        props.update(properties or {})
        features.append({"type": "Feature", "properties": props, "geometry": geometry})
    return json.dumps({"type": "FeatureCollection", "features": features})


def map_pixels(lonlat_rad, width: int, center_lon: float = 0.0) -> tuple:
    """(x, y, shifted longitude) of vertices in the pixel frame of export_map at `width` x width / 2, row 0 north, the centre
    meridian at center_lon (radians)."""
    ll = np.asarray(lonlat_rad, np.float64).reshape(-1, 2)
    lon = ll[:, 0] - float(center_lon)
    lon = np.where(lon > math.pi, lon - 2 * math.pi, np.where(lon < -math.pi, lon + 2 * math.pi, lon))
    x = (lon / math.pi + 1.0) * 0.5 * width
    y = (1.0 - ll[:, 1] / (math.pi / 2)) * 0.5 * (width // 2)
    return x, y, lon


def to_svg(result: dict, width: int, center_lon: float = 0.0) -> str:
    """An SVG of width x width / 2 in the pixel frame of export_map: one path per ring with its class and ring number as data
    attributes, cut like to_geojson's, in the frame shifted to center_lon."""
    if result.get("lonlat") is None:
        raise ValueError("to_svg needs the result's lonlat (build_outline(..., want_lonlat=True))")
    width = int(width)
    if width < 2 or width % 2:
        raise ValueError(f"width is {width}, it must be even and at least 2")
    out = [f'<svg xmlns="http://www.w3.org/2000/svg" width="{width}" height="{width // 2}" viewBox="0 0 {width} {width // 2}" fill="none" stroke="black" stroke-width="1">']
    for ring in outline_rings(result):
        x, y, lon = map_pixels(ring["lonlat"], width, center_lon)
        pieces = ring_pieces(lon)
        d = []
        for idx in pieces:
            closed = idx.size > 1 and idx[0] == idx[-1]           # the one piece of an uncut ring
            pts = idx[:-1] if closed else idx
            d.append("M" + "L".join(f"{x[i]:.3f} {y[i]:.3f}" for i in pts) + ("Z" if closed else ""))
        out.append(f'<path data-ring="{ring["ring"]}" data-class="{ring["class"]}" d="{" ".join(d)}"/>')
    out.append("</svg>")
    return "\n".join(out)
