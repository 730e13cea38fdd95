"""Shared pieces of the wind tests: the golden cases with their inputs, the host emulator of csrc/wind_ops.h (tests/emu_wind,
built on first use) and the comparison on the bar of DESIGN section 3.

The bar.  Bit for bit wherever no platform libm is involved in a way an f32 store can see: the integer and flag outputs,
r_lat / r_lon / r_sinLat, the six frame arrays, both continentalities and the three ITCZ arrays.  The eight season arrays
(pressure, wind east / north, speed) take assignElevation's bar: per cell |got - ref| <= 4 * 2^-23 * max(1, |ref|), with |ref|
replaced by 1013 for r_pressure_* (the magnitude at which the f32 store of the pressure is made, before 1013 is subtracted),
and at most max(8, N / 10^4) cells different at all.  The cap is a condition, not a measurement."""
from __future__ import annotations

import ctypes as C
import json
import subprocess
import zlib
from functools import lru_cache

import numpy as np

from conftest import GOLDEN, REPO

EMU_DIR = REPO / "tests" / "emu_wind"
GOLDEN_CASES = ("wind_config1_N10000_s1", "wind_import_N10000_s1", "wind_N2000_ocean_s1", "wind_N2000_land_s1", "wind_N250000_s4")
SEASON_FIELDS = tuple(f"r_{k}_{s}" for s in ("summer", "winter") for k in ("pressure", "wind_east", "wind_north", "wind_speed"))
ULP_BOUND = 4 * 2.0 ** -23
HOOK_K = 4                          # double ulps: twice the 2-ulp bound of ocml's double exp / sin / cos
_emu = {}


def result_fields():
    from planet_heightmap_generation_amd import wind as WD
    return WD.RESULT_FIELDS


def exact_fields():
    return tuple(k for k, _ in result_fields() if k not in SEASON_FIELDS)


def diff_cap(N):
    return max(8, N // 10 ** 4)


def crc(a) -> int:
    return zlib.crc32(np.ascontiguousarray(a).tobytes()) & 0xFFFFFFFF


def emu(libm_hook=False):
    if not _emu:
        subprocess.run(["make", "-s", "-C", str(EMU_DIR)], check=True)
        _emu[False] = C.CDLL(str(EMU_DIR / "_build" / "libemu_wind.so"))
        _emu[True] = C.CDLL(str(EMU_DIR / "_build" / "libemu_wind_libm.so"))
        _emu[False].emu_wind_percentile.restype = C.c_float
        _emu[True].emu_libm_calls.argtypes = [C.c_void_p]
    return _emu[bool(libm_hook)]


def ptr(a):
    assert a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(C.c_void_p)


@lru_cache(maxsize=None)
def golden_case(name):
    """dict(name, N, off, adj, xyz, e, plate, ocean, seed, ref, meta) of one fixture; ref[key] is the stored array (every
    meta['stride']-th cell unless the fixture keeps it whole)."""
    g = np.load(GOLDEN / f"{name}.npz")
    meta = json.loads(bytes(g["meta_json"]).decode())
    ref = {k[4:]: g[k] for k in g.files if k.startswith("ref_")}
    if name == "wind_config1_N10000_s1":
        s = np.load(GOLDEN / "elev_config1_N10000_s1.npz")
        off, adj, xyz, e, plate, ocean = s["adjOffset"], s["adjList"], s["xyz"], s["ref_final_elevation"], s["r_plate"], s["plateSeeds"][s["plateIsOcean"] == 1]
    elif name == "wind_import_N10000_s1":
        m, s = np.load(GOLDEN / "mesh_N10000_s1.npz"), np.load(GOLDEN / "import_N10000_s1.npz")
        off, adj, xyz, e, plate, ocean = m["ref_adjOffset"], m["ref_adjList"], m["xyz"], s["done_r_elevation"], s["done_r_plate"], s["done_plateIsOcean"]
    elif name.startswith("wind_N2000_"):
        m = np.load(GOLDEN / "mesh_N2000_s1.npz")
        off, adj, xyz, e, plate, ocean = m["ref_adjOffset"], m["ref_adjList"], m["xyz"], g["in_e"], g["in_plate"], g["in_ocean"]
    else:
        from plates_common import reference_mesh
        s = np.load(GOLDEN / "elev_N250000_s4_large.npz")           # keeps no mesh: rebuilt the way the reference harness did, checksums checked
        sm = json.loads(bytes(s["meta_json"]).decode())
        mesh, xyz = reference_mesh(sm["N"], 0.75, sm["seed"])
        assert crc(xyz) == sm["crc_xyz"] and crc(mesh.adjOffset) == sm["crc_adjOffset"] and crc(mesh.adjList) == sm["crc_adjList"]
        off, adj, e, plate, ocean = mesh.adjOffset, mesh.adjList, s["ref_elevation"], s["r_plate"], g["in_ocean"]
    c32 = lambda a, t: np.ascontiguousarray(a, t)  # noqa: E731
    return dict(name=name, N=int(meta["numRegions"]), off=c32(off, np.int32), adj=c32(adj, np.int32), xyz=c32(xyz, np.float32), e=c32(e, np.float32),
                plate=c32(plate, np.int32), ocean=c32(ocean, np.int32), seed=meta["seed"], ref=ref, meta=meta)


class Mesh:
    def __init__(self, off, adj):
        self.adjOffset, self.adjList, self.numRegions = off, adj, off.size - 1


def make_case(name, mesh, xyz, e, plate, ocean, seed=1):
    c32 = lambda a, t: np.ascontiguousarray(a, t)  # noqa: E731
    return dict(name=name, N=int(mesh.numRegions), off=c32(mesh.adjOffset, np.int32), adj=c32(mesh.adjList, np.int32), xyz=c32(xyz, np.float32).reshape(-1),
                e=c32(e, np.float32), plate=c32(plate, np.int32), ocean=c32(ocean, np.int32), seed=seed, ref=None, meta=None)


def emulate(case, order_seed=0, libm_hook=False, perturb=None):
    """The whole stage on the host; perturb = (seed, K) moves every exp / sin / cos of the bodies by up to K double ulps."""
    L = emu(libm_hook or perturb is not None)
    if perturb is not None:
        L.emu_set_libm_perturb(C.c_uint64(perturb[0]), C.c_int64(perturb[1]))
    N = case["N"]
    out = {k: np.zeros(360 if k.startswith("itcz") else N, ty) for k, ty in result_fields()}
    arr = (C.c_void_p * len(out))(*[ptr(a) for a in out.values()])
    levels = np.zeros(2, np.int32)
    L.emu_wind(C.c_int32(N), ptr(case["off"]), ptr(case["adj"]), ptr(case["xyz"]), ptr(case["e"]), ptr(case["plate"]), ptr(case["ocean"]),
               C.c_int32(case["ocean"].size), C.c_double(case["seed"]), C.c_uint64(order_seed), arr, ptr(levels))
    if perturb is not None:
        calls = np.zeros(7, np.uint64)
        L.emu_libm_calls(ptr(calls))
        out["_libm_calls"] = calls
        L.emu_set_libm_perturb(C.c_uint64(0), C.c_int64(0))
    out["_levels"] = (int(levels[0]), int(levels[1]))
    return out


def emulate_graph(case, order_seed=0):
    N = case["N"]
    label, coast, plate = np.empty(N, np.int32), np.empty(N, np.int32), np.empty(N, np.int32)
    main = np.zeros(1, np.int32)
    emu().emu_wind_graph(C.c_int32(N), ptr(case["off"]), ptr(case["adj"]), ptr(case["e"]), ptr(case["plate"]), ptr(case["ocean"]), C.c_int32(case["ocean"].size),
                         C.c_uint64(order_seed), ptr(label), ptr(main), ptr(coast), ptr(plate))
    return label, int(main[0]), coast, plate


def emu_percentile(v):
    v = np.ascontiguousarray(v, np.float32)
    return float(emu().emu_wind_percentile(ptr(v), C.c_int32(v.size)))


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def season_deviation(key, got, ref):
    """(cells that differ at all, largest |got - ref|, cells over the per-cell bound)"""
    g, r = got.astype(np.float64), ref.astype(np.float64)
    d = np.abs(g - r)
    d[np.isnan(g) & np.isnan(r)] = 0
    d[np.isnan(d)] = np.inf
    differ = got.view(np.uint32) != ref.view(np.uint32)
    scale = np.full(r.shape, 1013.0) if key.startswith("r_pressure_") else np.maximum(1.0, np.abs(r))
    over = d > ULP_BOUND * scale
    return int(differ.sum()), float(d[differ].max()) if differ.any() else 0.0, int(over.sum())


def compare(label, got, ref, N, stride=1, crcs=None):
    """got: full arrays; ref: arrays holding every stride-th cell (or whole ones: then they are compared whole).  crcs: CRC32 of
    the reference's whole arrays (sparse fixtures): the exact fields must reproduce them.  Prints every figure, then asserts."""
    figs, bad = {}, []
    for k in exact_fields():
        full = ref[k].size == got[k].size
        ok = same_bits(got[k] if full else got[k][::stride], ref[k])
        if ok and crcs is not None:
            ok = crc(got[k]) == crcs[k]
        figs[k] = "equal" if ok else "DIFFERS"
        if not ok:
            bad.append(k)
    cap = diff_cap(N)
    for k in SEASON_FIELDS:
        full = ref[k].size == got[k].size
        n, mx, over = season_deviation(k, got[k] if full else got[k][::stride], ref[k])
        figs[k] = (n, mx, over)
        if over or n > cap:
            bad.append(k)
    print(f"{label}: N {N}, cap {cap}; season arrays (cells differing, largest |d|, cells over the per-cell bound): "
          + ", ".join(f"{k} {figs[k]}" for k in SEASON_FIELDS) + "; exact fields: "
          + ("all equal" if not [k for k in exact_fields() if figs[k] != "equal"] else str({k: figs[k] for k in exact_fields() if figs[k] != "equal"})))
    assert not bad, f"{label}: off the bar in {bad}: {figs}"
    return figs


def compare_golden(label, got, case):
    m = case["meta"]
    return compare(label, got, case["ref"], case["N"], stride=m["stride"], crcs=m["crc"] if m["stride"] > 1 else None)


def ocean_plate_ids(ec):
    """The reference's plateIsOcean Set of an elev_inputs.ElevCase, as an id array."""
    return np.ascontiguousarray(np.asarray(ec.ids)[np.asarray(ec.isoc) == 1], np.int32)


def plate_mask_elevation(ec, seed, flip=0.03):
    """A cheap stand-in for a terrain on an ElevCase's plates: continental plates at +0.3, oceanic ones at -0.4, with a seeded
    `flip` share of the cells switched to the other side (lakes, inland seas, islands), so that the main-ocean choice, lakes and
    land the main ocean never reaches all occur."""
    rng = np.random.default_rng(seed)
    ids = np.asarray(ec.ids)
    order = np.argsort(ids)
    isoc = np.asarray(ec.isoc)[order][np.searchsorted(ids[order], ec.r_plate)] == 1
    isoc ^= rng.random(isoc.size) < flip
    return np.where(isoc, -0.4, 0.3).astype(np.float32) * rng.uniform(0.5, 1.5, isoc.size).astype(np.float32)


def case_from_elev(ec, e, seed=1):
    return make_case(ec.name, ec.mesh, ec.xyz, e, ec.r_plate, ocean_plate_ids(ec), seed)


def synthetic_case(N, seed=3, e=None, poles=48):
    """A planet of any size without a plate model: build_sphere(N, 0.75, 1), the bench's synthetic continents (fbm; from the
    C oracle unless `e` brings the device's, which is the same field bit for bit) and `poles` plates as the nearest of that many
    seeded poles, every third one oceanic.  Plate ids are not 0 .. P - 1."""
    from planet_heightmap_generation_amd import sphere_mesh as S
    mesh, xyz, _ = S.build_sphere(N, 0.75, 1)
    if e is None:
        from oracle import pyoracle as O
        e = O.synthetic_terrain(xyz, seed)
    rng = np.random.default_rng(poles)
    pole = rng.normal(size=(poles, 3))
    pole /= np.linalg.norm(pole, axis=1, keepdims=True)
    P = np.asarray(xyz, np.float32).reshape(-1, 3)
    plate = np.empty(P.shape[0], np.int32)
    for s in range(0, P.shape[0], 1 << 20):
        plate[s:s + (1 << 20)] = np.argmax(P[s:s + (1 << 20)] @ pole.T.astype(np.float32), axis=1)
    return make_case(f"synthetic_N{N}", mesh, xyz, e, plate * 1000 + 7, np.arange(0, poles, 3, dtype=np.int32) * 1000 + 7, seed=seed)
