"""Shared pieces of the map-layer tests: the golden fixture of the reference's map view (tests/golden/map_layers_N2000_s1.npz), the
host emulator of csrc/map_layer_ops.h (tests/emu_map_layers) and the sweep arrays the golden records, laid out per colour function."""
from __future__ import annotations

import ctypes as C
import functools
import subprocess

import numpy as np

from conftest import GOLDEN, REPO
from map_common import _mesh_args, ptr

EMU_DIR = REPO / "tests" / "emu_map_layers"
# the reference's debugLayer names in the order of WO_MAP_LAYER_DEBUG .. (include/worogen.h); map_export.LAYERS must equal it
LAYERS = ("debug", "continentality", "tempSummer", "tempWinter", "precipSummer", "precipWinter", "rainShadowSummer", "rainShadowWinter", "oceanCurrentSummer",
          "oceanCurrentWinter", "pressureSummer", "pressureWinter", "windSpeedSummer", "windSpeedWinter")
NAMED = LAYERS[1:]
OCEAN_CURRENT = ("oceanCurrentSummer", "oceanCurrentWinter")
RANGE_CASES = ("positive", "negative", "zero", "nan", "inf")
# the block and the reference's result key(s) behind every named layer
SOURCE = {
    "continentality": ("wind", ("r_continentality",)), "tempSummer": ("temperature", ("r_temperature_summer",)), "tempWinter": ("temperature", ("r_temperature_winter",)),
    "precipSummer": ("precip", ("r_precip_summer",)), "precipWinter": ("precip", ("r_precip_winter",)), "rainShadowSummer": ("precip", ("r_rainshadow_summer",)),
    "rainShadowWinter": ("precip", ("r_rainshadow_winter",)), "oceanCurrentSummer": ("ocean", ("r_ocean_warmth_summer", "r_ocean_speed_summer")),
    "oceanCurrentWinter": ("ocean", ("r_ocean_warmth_winter", "r_ocean_speed_winter")), "pressureSummer": ("wind", ("r_pressure_summer",)),
    "pressureWinter": ("wind", ("r_pressure_winter",)), "windSpeedSummer": ("wind", ("r_wind_speed_summer",)), "windSpeedWinter": ("wind", ("r_wind_speed_winter",)),
}
_emu = None


@functools.lru_cache(maxsize=None)
def golden():
    return dict(np.load(GOLDEN / "map_layers_N2000_s1.npz"))


def emu():
    global _emu
    if _emu is None:
        subprocess.run(["make", "-s", "-C", str(EMU_DIR)], check=True)
        _emu = C.CDLL(str(EMU_DIR / "_build" / "libemu_map_layers.so"))
        _emu.emu_geometry_centered.restype = C.c_int32
    return _emu


def _f32(a):
    return None if a is None else np.ascontiguousarray(a, np.float32)


def emu_geometry(xyz, tri, he, center_lon):
    """-> (positions float32 [T, 3, 2], triRegions int32 [T], triSides int32 [T]) in the reference's order"""
    xyz, tri, he = _mesh_args(xyz, tri, he)
    pos, reg, side = np.empty(12 * tri.size, np.float32), np.empty(2 * tri.size, np.int32), np.empty(2 * tri.size, np.int32)
    n = emu().emu_geometry_centered(C.c_int32(xyz.size // 3), ptr(xyz), C.c_int32(tri.size), ptr(tri), ptr(he), C.c_double(center_lon), ptr(pos), ptr(reg), ptr(side))
    return pos[: 6 * n].reshape(n, 3, 2).copy(), reg[:n].copy(), side[:n].copy()


def emu_raster(xyz, tri, he, W, center_lon):
    """-> (regionMap int32 [H, W], covered, uncovered)"""
    xyz, tri, he = _mesh_args(xyz, tri, he)
    out, counts = np.empty((W // 2, W), np.int32), np.zeros(2, np.int64)
    emu().emu_raster_centered(C.c_int32(xyz.size // 3), ptr(xyz), C.c_int32(tri.size), ptr(tri), ptr(he), C.c_int32(W), C.c_double(center_lon), ptr(out), ptr(counts))
    return out, int(counts[0]), int(counts[1])


def emu_range(v):
    """-> float32 [2]: dbgMin, dbgMax"""
    v, out = _f32(v), np.empty(2, np.float32)
    emu().emu_range(C.c_int32(v.size), ptr(v), ptr(out))
    return out


def emu_layer_colors(layer, a, b=None, e=None, range=None):
    """one colour per element, float32 [3 n]; range None: the range of a"""
    a, b, e, range = _f32(a), _f32(b), _f32(e), _f32(range)
    out = np.empty(3 * a.size, np.float32)
    emu().emu_layer_colors(C.c_int32(LAYERS.index(layer)), C.c_int32(a.size), ptr(a), ptr(b), ptr(e), ptr(range), ptr(out))
    return out


def emu_layer_rgba(layer, a, b, e, region_map):
    """-> uint8 [H, W, 4]"""
    a, b, e = _f32(a), _f32(b), _f32(e)
    rm = np.ascontiguousarray(region_map, np.int32)
    out = np.empty(rm.size, np.uint32)
    emu().emu_layer_rgba(C.c_int32(LAYERS.index(layer)), C.c_int32(a.size), ptr(a), ptr(b), ptr(e), C.c_int64(rm.size), ptr(rm), ptr(out))
    return out.view(np.uint8).reshape(rm.shape + (4,))


def golden_layer_fields(name):
    """the golden's synthetic field(s) of a named layer: (a, b), b None but for the ocean currents (warmth, speed)"""
    g = golden()
    if name in OCEAN_CURRENT:
        season = "summer" if name.endswith("Summer") else "winter"
        return g[f"field_r_ocean_warmth_{season}"], g[f"field_r_ocean_speed_{season}"]
    return g[f"field_{name}"], None


# the golden's direct sweeps per colour function: name -> (a layer that goes through the function, a, b, e, recorded colours)
def sweeps():
    g = golden()
    out = {
        "precipitation": ("precipSummer", g["sweep_in_precipitation"], None, None, g["sweep_precipitation"]),
        "rainShadow": ("rainShadowWinter", g["sweep_in_rainShadow"], None, None, g["sweep_rainShadow"]),
        "continentality": ("continentality", g["sweep_in_continentality"], None, None, g["sweep_continentality"]),
        "temperature": ("tempWinter", g["sweep_in_temperature"], None, None, g["sweep_temperature"]),
        "debugSelf": ("debug", g["sweep_in_debugSelf"], None, None, g["sweep_debugSelf"]),
        "ocean": ("oceanCurrentSummer", g["sweep_ocean_warmth"], g["sweep_ocean_speed"], g["sweep_ocean_elevation"], g["sweep_ocean"]),
    }
    return out


def ulp_distance(a, b):
    """per element: 0 for equal bits or two NaNs, else the distance of the f32 bit patterns on the number line"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    def key(x):
        u = x.view(np.uint32).astype(np.int64)
        return np.where(u & 0x80000000, -(u & 0x7FFFFFFF), u)
    d = np.abs(key(a) - key(b))
    d[np.isnan(a) & np.isnan(b)] = 0
    d[np.isnan(a) != np.isnan(b)] = 1 << 40
    d[(a.view(np.uint32) != b.view(np.uint32)) & (d == 0) & ~np.isnan(a)] = 1        # +0 against -0
    return d
