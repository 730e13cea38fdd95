"""Equirectangular map export (js/planet-mesh.js:1752-2180) over the C ABI, on a device-resident planet.

``raster`` builds the region map of the planet's positions for a mesh's sides (csrc/map.hip: forward rasterisation with the lowest
side index per pixel) and leaves it on the device; ``color`` turns it into RGBA8 in one of the reference's six kinds through the
reference's colour function per region, its quantiser and its gamma table; ``export_map`` does both.  The triangle list and the
region colours are the reference's bit for bit; the coverage rule is the one csrc/map_ops.h fixes (WebGL's own pixels differ
between GPUs).  ``biome`` and ``koppen`` need the planet's Koppen block (``koppen.classify_koppen``).  There is no CPU fallback.

The reference's map view (buildMapMesh, js/planet-mesh.js:200-382) shows more than its export button: ``raster(center_lon=...)`` draws
the map around a centre meridian (its wrapLon), ``color_layer`` colours it as one of the layers of its debugLayer switch, from the
planet's resident climate blocks or from values of the caller's, and ``export_map(layers=..., center_lon=...)`` adds those maps.

``raster_cube`` / ``export_cube`` give the cube map instead (ours; csrc/cube.hip, the contract is in csrc/cube_ops.h): six square faces
by gnomonic projection, ``FACES`` in the OpenGL order, exactly the globe mesh seen from its centre.  The faces lie stacked in the same
map block, so ``color``, ``color_layer``, ``download`` and ``free`` serve them and return arrays of shape (6, S, S, ...).
"""
from __future__ import annotations

import numpy as np

from . import capi
from . import climate_blocks as CB
from . import terrain_post as TP

# the reference's type names in the order of WO_MAP_COLOR .. WO_MAP_KOPPEN (include/worogen.h)
TYPES = ("color", "heightmap", "landheightmap", "landmask", "biome", "koppen")
# the reference's debugLayer names in the order of WO_MAP_LAYER_DEBUG .. WO_MAP_LAYER_WINDSPEED_WINTER; `debug` is any other array of
# its debugLayers, coloured by debugValueToColor over its own range
LAYERS = ("debug", "continentality", "tempSummer", "tempWinter", "precipSummer", "precipWinter", "rainShadowSummer", "rainShadowWinter", "oceanCurrentSummer",
          "oceanCurrentWinter", "pressureSummer", "pressureWinter", "windSpeedSummer", "windSpeedWinter")


# the cube map's faces in the order +X, -X, +Y, -Y, +Z, -Z (the OpenGL cube-map table; north is +Y, longitude 0 is +Z)
FACES = ("px", "nx", "py", "ny", "pz", "nz")
MAX_FACE_SIZE = 16384


def type_id(type) -> int:
    if isinstance(type, str):
        if type not in TYPES:
            raise ValueError(f"unknown map type '{type}' (one of {', '.join(TYPES)})")
        return TYPES.index(type)
    return int(type)


def layer_id(layer) -> int:
    if isinstance(layer, str):
        if layer not in LAYERS:
            raise ValueError(f"unknown map layer '{layer}' (one of {', '.join(LAYERS)})")
        return LAYERS.index(layer)
    return int(layer)


def layer_filename(name: str, seed) -> str:
    """The file name of a layer's map.  Ours: the reference exports no layer."""
    return f"orogen-layer-{name}-{seed}.png"


def export_filename(type: str, seed) -> str:
    """exportFilename(type, seed) (js/planet-mesh.js:1952-1961)."""
    stem = dict(landmask="landmask", landheightmap="land-heightmap", heightmap="heightmap", biome="satellite", koppen="climate").get(type, "colormap")
    return f"orogen-{stem}-{seed}.png"


def _face_id(face) -> int:
    if isinstance(face, str):
        if face not in FACES:
            raise ValueError(f"unknown cube face '{face}' (one of {', '.join(FACES)})")
        return FACES.index(face)
    if not 0 <= int(face) < 6:
        raise ValueError(f"cube face {face} is not one of 0 .. 5")
    return int(face)


def cube_direction(face, i: int, j: int, face_size: int) -> np.ndarray:
    """The direction of the centre of pixel (column i, row j) of a face (a name of FACES or 0 .. 5): three doubles, the major axis +-1
    (csrc/cube_ops.h: cube_direction).  Not normalised."""
    f, S = _face_id(face), int(face_size)
    a = -1.0 + 2.0 * (float(i) + 0.5) / float(S)
    b = -1.0 + 2.0 * (float(j) + 0.5) / float(S)
    return np.array(((1.0, -b, -a), (-1.0, -b, a), (a, 1.0, b), (a, -1.0, -b), (a, -b, 1.0), (-a, -b, -1.0))[f], np.float64)


def cube_filename(type: str, face: str, seed) -> str:
    """The file name of one face of a cube map: export_filename's stems (a name that is no type's: the layer's), then the face.
    Ours: the reference exports no cube map."""
    FACES[_face_id(face)]
    name = export_filename(type, seed) if type in TYPES else layer_filename(type, seed)
    return f"{name[:-len('.png')]}-{face}.png"


def map_dims(planet: TP.Planet) -> tuple[int, int]:
    """(width, height) of the planet's resident region map, (0, 0) without one.  After raster_cube: (S, 6 S)."""
    dims = np.zeros(2, np.int32)
    capi.check(capi.lib().wo_map_dims(planet.handle, capi.ptr(dims)), "mapDims")
    return int(dims[0]), int(dims[1])


def _map_shape(planet: TP.Planet, width) -> tuple:
    """The shape of the planet's region map as color returns it: what the last raster made here left on the planet, or width x
    width / 2 for an explicit width."""
    if width is not None:
        return (int(width) // 2, int(width))
    shape = getattr(planet, "_map_shape", None)
    return shape if shape is not None else (1, 2)          # no raster made here: the library says what is missing


def raster(planet: TP.Planet, mesh, width: int, download: bool = False, center_lon: float | None = 0.0) -> dict:
    """The region map of the planet at width x width / 2: {width, height, covered, uncovered, regionMap}; regionMap is the int32
    (height, width) array (-1: nothing covers the pixel) when download is set, else None.  The map stays on the device.
    center_lon: the centre meridian in radians, within [-pi, pi] (0 or None: the export's own raster, the same map)."""
    width = int(width)
    tri = np.ascontiguousarray(mesh.triangles, dtype=np.int32)
    he = np.ascontiguousarray(mesh.halfedges, dtype=np.int32)
    if tri.shape != he.shape or tri.ndim != 1:
        raise ValueError("mesh.triangles and mesh.halfedges must be int32 arrays of numSides entries")
    ok = 2 <= width <= 32768 and width % 2 == 0
    out = np.empty((width // 2, width), np.int32) if (download and ok) else None
    counts = np.zeros(2, np.int64)
    if center_lon is None or (isinstance(center_lon, (int, float)) and center_lon == 0):
        capi.check(capi.lib().wo_map_raster(planet.handle, tri.size, capi.ptr(tri), capi.ptr(he), width, capi.ptr(out), capi.ptr(counts)), "mapRaster")
    else:
        capi.check(capi.lib().wo_map_raster_centered(planet.handle, tri.size, capi.ptr(tri), capi.ptr(he), width, float(center_lon), capi.ptr(out), capi.ptr(counts)),
                   "mapRasterCentered")
    planet._map_width = width
    planet._map_shape = (width // 2, width)                # what color sizes its result by
    return dict(width=width, height=width // 2, covered=int(counts[0]), uncovered=int(counts[1]), regionMap=out)


def raster_cube(planet: TP.Planet, mesh, face_size: int, download: bool = False) -> dict:
    """The cube map's region map at six faces of face_size x face_size: {faceSize, covered, uncovered, regionMap}; regionMap is the
    int32 (6, faceSize, faceSize) array in the order of FACES (-1: nothing covers the pixel) when download is set, else None.  The
    map stays on the device, in the block raster uses."""
    S = int(face_size)
    tri = np.ascontiguousarray(mesh.triangles, dtype=np.int32)
    he = np.ascontiguousarray(mesh.halfedges, dtype=np.int32)
    if tri.shape != he.shape or tri.ndim != 1:
        raise ValueError("mesh.triangles and mesh.halfedges must be int32 arrays of numSides entries")
    ok = 1 <= S <= MAX_FACE_SIZE
    out = np.empty((6, S, S), np.int32) if (download and ok) else None
    counts = np.zeros(2, np.int64)
    capi.check(capi.lib().wo_map_raster_cube(planet.handle, tri.size, capi.ptr(tri), capi.ptr(he), S, capi.ptr(out), capi.ptr(counts)), "mapRasterCube")
    planet._map_width = None
    planet._map_shape = (6, S, S)
    return dict(faceSize=S, covered=int(counts[0]), uncovered=int(counts[1]), regionMap=out)


def download(planet: TP.Planet, width: int | None = None) -> np.ndarray:
    """The planet's resident region map: int32 (height, width) at the width of its last raster, (6, S, S) after raster_cube
    (width None: the shape that the last raster made here left)."""
    out = np.empty(_map_shape(planet, width), np.int32)
    capi.check(capi.lib().wo_map_download(planet.handle, capi.ptr(out), out.nbytes), "mapDownload")
    return out


def color(planet: TP.Planet, type, r_elevation=None, width: int | None = None, rivers: float | None = None) -> np.ndarray:
    """The planet's region map coloured as `type`: uint8 (height, width, 4), after raster_cube (6, S, S, 4).  r_elevation None means
    the planet's resident field.  width: the width of the planet's last raster; raster and raster_cube remember the shape on the
    planet, so it is only needed after a raster made elsewhere.  rivers: a minimum flow; the river cells that reach it and the lakes
    of the planet's rivers block (rivers.compute_rivers) are painted over the type's colours (None: off)."""
    e = CB.elevation_arg(planet.numRegions, r_elevation)
    out = np.empty(_map_shape(planet, width) + (4,), np.uint8)
    if rivers is None:
        capi.check(capi.lib().wo_map_color(planet.handle, type_id(type), capi.ptr(e), capi.ptr(out), out.nbytes), "mapColor")
    else:
        capi.check(capi.lib().wo_map_color_rivers(planet.handle, type_id(type), capi.ptr(e), float(rivers), capi.ptr(out), out.nbytes), "mapColorRivers")
    return out


def color_layer(planet: TP.Planet, layer, values=None, r_elevation=None, width: int | None = None) -> np.ndarray:
    """The planet's region map coloured as `layer` (a name of LAYERS): uint8 (height, width, 4).  values None reads the layer's field
    from the planet's resident climate block; otherwise numRegions floats take its place (required for `debug`, refused for the two
    ocean-current layers, which read two fields: ocean.upload sets those).  r_elevation (None: the resident field) is read by the
    ocean-current layers only.  width: as for color."""
    lid = layer_id(layer)
    v = None
    if values is not None:
        v = np.ascontiguousarray(values, dtype=np.float32)
        if v.shape != (planet.numRegions,):
            raise ValueError(f"values must hold numRegions = {planet.numRegions} floats, got shape {v.shape}")
    e = CB.elevation_arg(planet.numRegions, r_elevation)
    out = np.empty(_map_shape(planet, width) + (4,), np.uint8)
    capi.check(capi.lib().wo_map_color_layer(planet.handle, lid, capi.ptr(v), capi.ptr(e), capi.ptr(out), out.nbytes), "mapColorLayer")
    return out


def free(planet: TP.Planet) -> None:
    capi.check(capi.lib().wo_map_free(planet.handle), "mapFree")
    planet._map_width = None
    planet._map_shape = None


def _wanted_layers(names, layers) -> dict:
    """export_map's and export_cube's checks of the types and layers asked for -> {layer name: values or None}"""
    for t in names:
        type_id(t)
    wanted = dict(layers) if hasattr(layers, "keys") else {name: None for name in ([layers] if isinstance(layers, str) else layers)}
    for name, values in wanted.items():
        if values is None or name in LAYERS:
            layer_id(name)
            if name == "debug" and values is None:
                raise ValueError("the map layer 'debug' takes its values from the caller")
        if name in names:
            raise ValueError(f"'{name}' is asked for as a type and as a layer")
    return wanted


def export_cube(planet: TP.Planet, mesh, types, face_size: int, r_elevation=None, layers=(), rivers: float | None = None) -> dict:
    """export_map for the cube map: one raster of the six faces, one colour pass per type, then one per layer (types, layers and
    rivers as for export_map).  -> {faceSize, covered, uncovered, maps: {name: uint8 (6, S, S, 4)}}; maps[name][f] is face FACES[f]."""
    names = [types] if isinstance(types, str) else list(types)
    wanted = _wanted_layers(names, layers)
    res = raster_cube(planet, mesh, face_size)
    res["maps"] = {t: color(planet, t, r_elevation, rivers=rivers) for t in names}
    for name, values in wanted.items():
        res["maps"][name] = color_layer(planet, name if name in LAYERS else "debug", values, r_elevation)
    del res["regionMap"]
    return res


def export_map(planet: TP.Planet, mesh, types, width: int, r_elevation=None, layers=(), center_lon: float = 0.0, rivers: float | None = None) -> dict:
    """exportMapBatch: one raster, one colour pass per type.  types: one name or a sequence of names.
    layers: names of LAYERS other than `debug` (read from the planet's resident blocks), or a mapping name -> values (None: the
    resident block; an array: these values, under any name that is no climate layer's coloured as `debug`); their maps follow the
    types' in `maps`.  center_lon: the centre meridian of the raster.  rivers: a minimum flow; the types' maps get the rivers and
    lakes of the planet's rivers block painted over them (None: off; the layers stay as they are).
    -> {width, height, covered, uncovered, maps: {name: uint8 (height, width, 4)}}"""
    names = [types] if isinstance(types, str) else list(types)
    wanted = _wanted_layers(names, layers)
    res = raster(planet, mesh, width, center_lon=center_lon)
    res["maps"] = {t: color(planet, t, r_elevation, res["width"], rivers) for t in names}
    for name, values in wanted.items():
        res["maps"][name] = color_layer(planet, name if name in LAYERS else "debug", values, r_elevation, res["width"])
    del res["regionMap"]
    return res
