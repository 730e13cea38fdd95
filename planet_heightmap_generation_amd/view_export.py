"""The globe view over the C ABI, on a device-resident planet: the displaced globe mesh seen through a camera (ours; csrc/view.hip,
the contract is in csrc/view_ops.h).

``raster_view`` rasters the mesh's sides through a perspective or orthographic camera that looks at the planet's centre, keeps the
nearest side per pixel and leaves the region map in the planet's map block, where ``map_export.color``, ``color_layer``, ``download``
and ``free`` and the editor's tints serve it; ``depth`` gives the depth per pixel.  With ``shade`` every facet is lit by one Lambert
term, ``min(255, floor(c * (ambient + diffuse * lambert) + 0.5))`` per channel; the pixels nothing covers take the background.
``render_globe`` does the raster and the colour passes.  The reference draws this picture with three.js (js/scene.js); its camera
and sun are the defaults here, its lighting and tone pipeline are not reproduced.  There is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import capi
from . import climate_blocks as CB
from . import map_export as ME
from . import terrain_post as TP

MAX_SIZE = 16384
SUN = (5.0, 3.0, 4.0)                                      # js/scene.js: the directional light's position
BACKGROUND = 0xFF080303                                    # the scene colour 0x030308, opaque: R | G << 8 | B << 16 | A << 24
DEFAULT_FOV, DEFAULT_DISTANCE, DEFAULT_HALF_HEIGHT = 50.0, 2.8, 1.1


class ViewRequest(C.Structure):
    """wo_view_request of include/worogen.h"""
    _fields_ = [("eye", C.c_double * 3), ("fovY", C.c_double), ("halfHeight", C.c_double), ("exaggeration", C.c_double), ("r_elevation", C.c_void_p), ("shade", C.c_int32),
                ("light", C.c_double * 3), ("ambient", C.c_double), ("diffuse", C.c_double), ("backgroundRgba", C.c_uint32)]


def camera(lon: float, lat: float, distance: float = DEFAULT_DISTANCE, fov: float = DEFAULT_FOV, half_height: float = DEFAULT_HALF_HEIGHT) -> dict:
    """The camera above longitude lon and latitude lat (degrees; north is +Y, longitude 0 is +Z, as everywhere else) at `distance`
    from the centre: {eye, fov, halfHeight}.  fov 0 is the orthographic camera of half height half_height."""
    if not -90.0 <= lat <= 90.0:
        raise ValueError(f"lat is {lat}, it must be from -90 to 90 degrees")
    lo, la = math.radians(lon), math.radians(lat)
    eye = (distance * math.cos(la) * math.sin(lo), distance * math.sin(la), distance * math.cos(la) * math.cos(lo))
    return dict(eye=eye, fov=float(fov), halfHeight=float(half_height))


def request(cam: dict | None = None, shade: bool = True, exaggeration: float = 1.0, light=SUN, ambient: float = 0.55, diffuse: float = 0.45, background: int = BACKGROUND,
            r_elevation=None) -> ViewRequest:
    """The request of wo_view_raster.  cam: {eye, fov, halfHeight} (None: the reference's camera, 50 degrees at (0, 0.4, 2.8));
    r_elevation: a contiguous float32 array that the caller keeps alive, or None."""
    cam = dict(eye=(0.0, 0.4, 2.8), fov=DEFAULT_FOV) if cam is None else cam
    q = ViewRequest()
    q.eye = (C.c_double * 3)(*[float(c) for c in cam["eye"]])
    q.fovY = float(cam.get("fov", DEFAULT_FOV))
    q.halfHeight = float(cam.get("halfHeight", DEFAULT_HALF_HEIGHT))
    q.exaggeration = float(exaggeration)
    q.r_elevation = None if r_elevation is None else r_elevation.ctypes.data
    q.shade = 1 if shade else 0
    q.light = (C.c_double * 3)(*[float(c) for c in light])
    q.ambient, q.diffuse = float(ambient), float(diffuse)
    q.backgroundRgba = int(background) & 0xFFFFFFFF
    return q


def view_filename(name: str, seed) -> str:
    """The file name the Node host gives a render's PNG (js/view-export.js: viewFilename): export_filename's stems (a name that is
    no type's: the layer's) behind `orogen-globe-`.  Nothing here encodes a file; the name is for a caller that does."""
    stem = ME.export_filename(name, seed) if name in ME.TYPES else ME.layer_filename(name, seed)
    return "orogen-globe-" + stem[len("orogen-"):]


def raster_view(planet: TP.Planet, mesh, width: int, height: int, cam: dict | None = None, r_elevation=None, download: bool = False, depth: bool = False, **shading) -> dict:
    """The region map of the planet seen through cam at width x height: {width, height, covered, uncovered, regionMap, depth};
    regionMap is the int32 (height, width) array (-1: nothing covers the pixel) when download is set and depth the float32 one (NaN:
    nothing covers) when depth is set, else None.  The map stays on the device.  shading: request's keywords."""
    W, H = int(width), int(height)
    tri = np.ascontiguousarray(mesh.triangles, dtype=np.int32)
    he = np.ascontiguousarray(mesh.halfedges, dtype=np.int32)
    if tri.shape != he.shape or tri.ndim != 1:
        raise ValueError("mesh.triangles and mesh.halfedges must be int32 arrays of numSides entries")
    e = CB.elevation_arg(planet.numRegions, r_elevation)
    q = request(cam, r_elevation=e, **shading)
    ok = 1 <= W <= MAX_SIZE and 1 <= H <= MAX_SIZE
    out = np.empty((H, W), np.int32) if (download and ok) else None
    dep = np.empty((H, W), np.float32) if (depth and ok) else None
    counts = np.zeros(2, np.int64)
    capi.check(capi.lib().wo_view_raster(planet.handle, tri.size, capi.ptr(tri), capi.ptr(he), W, H, C.byref(q), capi.ptr(out), capi.ptr(dep), capi.ptr(counts)), "viewRaster")
    planet._map_width = None
    planet._map_shape = (H, W)                             # what map_export.color sizes its result by
    return dict(width=W, height=H, covered=int(counts[0]), uncovered=int(counts[1]), regionMap=out, depth=dep)


def depth(planet: TP.Planet) -> np.ndarray:
    """The depth map of the planet's last view raster: float32 (height, width), NaN where nothing covers the pixel."""
    w, h = ME.map_dims(planet)
    out = np.empty((max(h, 1), max(w, 1)), np.float32)
    capi.check(capi.lib().wo_view_depth_download(planet.handle, capi.ptr(out), out.nbytes), "viewDepth")
    return out


def lambert(planet: TP.Planet) -> np.ndarray:
    """The Lambert terms of the planet's last shaded view raster: float32 (height, width), 0 where nothing covers the pixel."""
    w, h = ME.map_dims(planet)
    out = np.empty((max(h, 1), max(w, 1)), np.float32)
    capi.check(capi.lib().wo_view_lambert_download(planet.handle, capi.ptr(out), out.nbytes), "viewLambert")
    return out


def render_globe(planet: TP.Planet, mesh, types, width: int, height: int, camera: dict | None = None, layers=(), rivers: float | None = None, shade: bool = True,
                 r_elevation=None, **shading) -> dict:
    """One view raster, one colour pass per type, then one per layer (types, layers and rivers as for map_export.export_map).
    -> {width, height, covered, uncovered, maps: {name: uint8 (height, width, 4)}}.  RGBA arrays only: this package has no PNG
    encoder (the Node host's js/map-export.js has one, and its worker's renderGlobe command answers with PNG files)."""
    names = [types] if isinstance(types, str) else list(types)
    wanted = ME._wanted_layers(names, layers)
    res = raster_view(planet, mesh, width, height, camera, r_elevation, shade=shade, **shading)
    res["maps"] = {t: ME.color(planet, t, r_elevation, rivers=rivers) for t in names}
    for name, values in wanted.items():
        res["maps"][name] = ME.color_layer(planet, name if name in ME.LAYERS else "debug", values, r_elevation)
    del res["regionMap"], res["depth"]
    return res
