"""Relief export over the C ABI, on a device-resident planet: a smooth height per pixel, its 16-bit encoding and the normals of the
displaced surface, on the equirectangular map or on the cube map (ours: the reference exports neither; csrc/relief.hip, the contract
is in csrc/relief_ops.h).

``raster`` / ``raster_cube`` are map_export's rasters with one more pass: they leave the same region map in the planet's map block,
so ``map_export.color`` and the rest serve it, and beside it a height map of the same shape, the globe mesh's own flat triangles
sampled at every pixel centre.  ``heights`` downloads it, ``height16`` encodes it in 16 bits (linear in the reference's heightmap or
land-heightmap shade, no gamma), ``normals`` gives RGBA8 normals in tangent or object space.  ``export_relief`` does a raster and any
of those.  Any later raster of either kind ends the relief.  There is no CPU fallback.
"""
from __future__ import annotations

import numpy as np

from . import capi
from . import climate_blocks as CB
from . import map_export as ME
from . import terrain_post as TP

# the 16-bit kinds in the order of WO_RELIEF_HEIGHT, WO_RELIEF_LAND_HEIGHT, the normal spaces in that of WO_RELIEF_NORMAL_TANGENT,
# WO_RELIEF_NORMAL_OBJECT (include/worogen.h)
HEIGHT_KINDS = ("height16", "landHeight16")
NORMAL_KINDS = ("normal", "normalObject")
KINDS = HEIGHT_KINDS + NORMAL_KINDS
FLAT_OCEAN = 1
_STEMS = dict(height16="height16", landHeight16="land-height16", normal="normal", normalObject="normal-object")


def _kind(kind: str) -> str:
    if kind not in KINDS:
        raise ValueError(f"unknown relief kind '{kind}' (one of {', '.join(KINDS)})")
    return kind


def relief_filename(kind: str, seed, face: str | None = None) -> str:
    """orogen-<kind>-<seed>.png, and for one face of a cube map orogen-cube-<kind>-<face>-<seed>.png"""
    stem = _STEMS[_kind(kind)]
    if face is None:
        return f"orogen-{stem}-{seed}.png"
    return f"orogen-cube-{stem}-{ME.FACES[ME._face_id(face)]}-{seed}.png"


def _sides(mesh):
    tri = np.ascontiguousarray(mesh.triangles, dtype=np.int32)
    he = np.ascontiguousarray(mesh.halfedges, dtype=np.int32)
    if tri.shape != he.shape or tri.ndim != 1:
        raise ValueError("mesh.triangles and mesh.halfedges must be int32 arrays of numSides entries")
    return tri, he


def raster(planet: TP.Planet, mesh, width: int, r_elevation=None, center_lon: float | None = 0.0, download: bool = False) -> dict:
    """map_export.raster around center_lon, and the height map beside its region map: {width, height, covered, uncovered, heights};
    heights is the float32 (height, width) array (NaN: nothing covers the pixel) when download is set, else None.  r_elevation None
    means the planet's resident field."""
    width = int(width)
    tri, he = _sides(mesh)
    e = CB.elevation_arg(planet.numRegions, r_elevation)
    ok = 2 <= width <= 32768 and width % 2 == 0
    out = np.empty((width // 2, width), np.float32) if (download and ok) else None
    counts = np.zeros(2, np.int64)
    capi.check(capi.lib().wo_relief_raster(planet.handle, tri.size, capi.ptr(tri), capi.ptr(he), width, float(center_lon or 0.0), capi.ptr(e), capi.ptr(out), capi.ptr(counts)),
               "reliefRaster")
    planet._map_width = width
    planet._map_shape = (width // 2, width)
    return dict(width=width, height=width // 2, covered=int(counts[0]), uncovered=int(counts[1]), heights=out)


def raster_cube(planet: TP.Planet, mesh, face_size: int, r_elevation=None, download: bool = False) -> dict:
    """map_export.raster_cube, and the height map beside its region map: {faceSize, covered, uncovered, heights}; heights is the
    float32 (6, faceSize, faceSize) array in the order of map_export.FACES when download is set, else None."""
    S = int(face_size)
    tri, he = _sides(mesh)
    e = CB.elevation_arg(planet.numRegions, r_elevation)
    ok = 1 <= S <= ME.MAX_FACE_SIZE
    out = np.empty((6, S, S), np.float32) if (download and ok) else None
    counts = np.zeros(2, np.int64)
    capi.check(capi.lib().wo_relief_raster_cube(planet.handle, tri.size, capi.ptr(tri), capi.ptr(he), S, capi.ptr(e), capi.ptr(out), capi.ptr(counts)), "reliefRasterCube")
    planet._map_width = None
    planet._map_shape = (6, S, S)
    return dict(faceSize=S, covered=int(counts[0]), uncovered=int(counts[1]), heights=out)


def _shape(planet: TP.Planet) -> tuple:
    shape = getattr(planet, "_map_shape", None)
    if shape is not None:
        return shape
    w, h = ME.map_dims(planet)                              # a raster made elsewhere
    return (6, w, w) if h == 6 * w and w > 0 else (max(h, 1), max(w, 2))


def heights(planet: TP.Planet) -> np.ndarray:
    """The planet's resident height map: float32 (height, width), or (6, S, S) after raster_cube"""
    out = np.empty(_shape(planet), np.float32)
    capi.check(capi.lib().wo_relief_download(planet.handle, capi.ptr(out), out.nbytes), "reliefDownload")
    return out


def height16(planet: TP.Planet, kind="height16") -> np.ndarray:
    """The height map in 16 bits, uint16 of the shape of heights: `height16` or `landHeight16` (or 0, 1)"""
    k = HEIGHT_KINDS.index(kind) if isinstance(kind, str) and kind in HEIGHT_KINDS else kind
    if isinstance(k, str):
        raise ValueError(f"unknown 16-bit kind '{kind}' (one of {', '.join(HEIGHT_KINDS)})")
    out = np.empty(_shape(planet), np.uint16)
    capi.check(capi.lib().wo_relief_height16(planet.handle, int(k), capi.ptr(out), out.nbytes), "reliefHeight16")
    return out


def normals(planet: TP.Planet, space="normal", strength: float = 1.0, flat_ocean: bool = False) -> np.ndarray:
    """RGBA8 normals of the displaced surface, uint8 of the shape of heights + (4,): `normal` (tangent space) or `normalObject` (or
    0, 1).  strength scales the globe's displacement (finite, >= 0); flat_ocean: elevations <= 0 count as 0."""
    k = NORMAL_KINDS.index(space) if isinstance(space, str) and space in NORMAL_KINDS else space
    if isinstance(k, str):
        raise ValueError(f"unknown normal space '{space}' (one of {', '.join(NORMAL_KINDS)})")
    out = np.empty(_shape(planet) + (4,), np.uint8)
    capi.check(capi.lib().wo_relief_normals(planet.handle, int(k), float(strength), FLAT_OCEAN if flat_ocean else 0, capi.ptr(out), out.nbytes), "reliefNormals")
    return out


def export_relief(planet: TP.Planet, mesh, kinds, width: int | None = None, face_size: int | None = None, projection: str = "map", r_elevation=None, center_lon: float = 0.0,
                  strength: float = 1.0, flat_ocean: bool = False) -> dict:
    """One relief raster (projection 'map' at width, or 'cube' at face_size), then one pass per kind of KINDS.
    -> the raster's dict without `heights`, with maps: {kind: uint16 array, or uint8 (..., 4) for the normals}"""
    names = [kinds] if isinstance(kinds, str) else list(kinds)
    for k in names:
        _kind(k)
    if projection == "map":
        if width is None:
            raise ValueError("projection 'map' takes a width")
        res = raster(planet, mesh, width, r_elevation, center_lon)
    elif projection == "cube":
        if face_size is None:
            raise ValueError("projection 'cube' takes a face_size")
        res = raster_cube(planet, mesh, face_size, r_elevation)
    else:
        raise ValueError(f"unknown projection '{projection}' (one of map, cube)")
    res["maps"] = {k: height16(planet, k) if k in HEIGHT_KINDS else normals(planet, k, strength, flat_ocean) for k in names}
    del res["heights"]
    return res
