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
GOLDEN_CASES = ("wind_config1_N10000_s1", "wind_import_N10000_s1", "wind_N2000_ocean_s1", "wind_N2000_land_s1", "wind_N250000_s4",
                "wind_N2000_edges_s1", "wind_N63_shape_s1", "wind_N255_shape_s1", "wind_N256_shape_s1", "wind_N4096_shape_s1")
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
        xyz = g["in_xyz"] if "in_xyz" in g.files else m["xyz"]      # the edge planet moves twelve cells of the mesh
        off, adj, e, plate, ocean = m["ref_adjOffset"], m["ref_adjList"], g["in_e"], g["in_plate"], g["in_ocean"]
    elif name.endswith("_shape_s1"):
        from plates_common import reference_mesh
        mesh, xyz = reference_mesh(meta["mesh_N"], 0.75, meta["seed"])      # keeps no mesh: rebuilt, checksums checked
        assert crc(np.asarray(xyz, np.float32)) == meta["crc_xyz"] and crc(mesh.adjOffset) == meta["crc_adjOffset"] and crc(mesh.adjList) == meta["crc_adjList"]
        off, adj, e, plate, ocean = mesh.adjOffset, mesh.adjList, g["in_e"], g["in_plate"], g["in_ocean"]
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


def host_coast_distance(case):
    """r_coastDistLand restated plainly (js/wind.js:485-541): the ocean components over non-land cells, the largest one (the
    first found among equals, scanning the cells in ascending order) is the main ocean, land cells that touch it are at distance 0,
    and a FIFO queue walks the land from them."""
    from collections import deque
    N, off, adj = case["N"], case["off"], case["adj"]
    land = case["e"] > 0
    label, best, main = np.full(N, -1, np.int64), 0, -1
    for r in range(N):
        if land[r] or label[r] >= 0:
            continue
        label[r], size, q = r, 0, deque([r])
        while q:
            c = q.popleft()
            size += 1
            for nb in adj[off[c]:off[c + 1]]:
                if not land[nb] and label[nb] < 0:
                    label[nb] = r
                    q.append(nb)
        if size > best:
            best, main = size, r
    dist, q = np.full(N, -1, np.int32), deque()
    for r in np.flatnonzero(land):
        if main >= 0 and any(not land[nb] and label[nb] == main for nb in adj[off[r]:off[r + 1]]):
            dist[r] = 0
            q.append(r)
    while q:
        c = q.popleft()
        for nb in adj[off[c]:off[c + 1]]:
            if land[nb] and dist[nb] < 0:
                dist[nb] = dist[c] + 1
                q.append(nb)
    return dist


def edge_cells(case):
    """The cells of the edge planet by what their f32 position is: dict of index arrays."""
    x, y, z = case["xyz"].reshape(-1, 3).T
    return dict(north=np.flatnonzero((y == 1) & (x == 0) & (z == 0)), south=np.flatnonzero(y == -1), near_pole=np.flatnonzero((y == 1) & (x != 0)),
                equator=np.flatnonzero(y == 0), date_line=np.flatnonzero((x == 0) & (z < 0)), quarter=np.flatnonzero((z == 0) & (x != 0)))


def check_edge_values(label, got, case):
    """What the outputs must be at the poles, on the date line and at lon = +-pi/2, from f64 numpy rounded to f32 and from the
    fallback of the tangent frame (js/wind.js:430-433); no reference output is read.  `got`: wind outputs (all of RESULT_FIELDS)."""
    c = edge_cells(case)
    x, y, z = case["xyz"].reshape(-1, 3).T
    assert [c[k].size for k in ("north", "south", "near_pole", "equator", "date_line", "quarter")] == [1, 1, 1, 4, 6, 3], {k: v.tolist() for k, v in c.items()}
    half_pi, pi = np.float32(np.pi / 2), np.float32(np.pi)
    lat, lon = got["r_lat"], got["r_lon"]
    poles = np.concatenate([c["north"], c["south"]])
    assert same_bits(lat[poles], np.array([half_pi, -half_pi], np.float32)), lat[poles]
    assert same_bits(lat[c["near_pole"]], np.array([half_pi], np.float32))
    assert same_bits(lat[c["equator"]], np.zeros(4, np.float32)), lat[c["equator"]]                    # +0, not -0: asin(+0)
    d = c["date_line"]
    assert np.signbit(x[d]).sum() == 3, "the date-line cells should have x = -0 and x = +0"
    assert same_bits(lon[d], np.where(np.signbit(x[d]), -pi, pi).astype(np.float32)), lon[d]
    q = c["quarter"]
    assert np.signbit(z[q]).any() and not np.signbit(z[q]).all(), "z = -0 and z = +0"
    assert same_bits(lon[q], np.where(x[q] > 0, half_pi, -half_pi).astype(np.float32)), lon[q]
    assert same_bits(lon[c["north"]], np.zeros(1, np.float32))
    everywhere = np.arctan2(x.astype(np.float64), z.astype(np.float64)).astype(np.float32), np.arcsin(y.astype(np.float64)).astype(np.float32)
    off = [int((np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64)) > 1).sum()) for a, b in zip((lon, lat), everywhere)]
    print(f"{label}: cells whose r_lon / r_lat is more than one f32 step from numpy's f64 atan2 / asin: {off}")
    assert off == [0, 0]
    for k, want in (("r_eastX", 1), ("r_eastY", 0), ("r_eastZ", 0)):
        assert same_bits(got[k][poles], np.full(2, want, np.float32)), (k, got[k][poles])
    for k, want in (("r_northX", np.zeros(2, np.float32)), ("r_northY", z[poles]), ("r_northZ", -y[poles])):     # north = p x (1, 0, 0) = (0, z, -y), of length 1 in f64
        assert np.array_equal(got[k][poles], want), (k, got[k][poles])
    n = c["near_pole"]                                                                                 # (1e-10, 1, 1e-10): the frame proper, east = (z, 0, -x) / |.|
    assert abs(float(got["r_eastX"][n[0]]) - np.sqrt(0.5)) < 1e-6 and abs(float(got["r_eastZ"][n[0]]) + np.sqrt(0.5)) < 1e-6
    for k, _ in result_fields():
        assert np.isfinite(got[k]).all(), f"{label}: {k} is not finite in {np.flatnonzero(~np.isfinite(got[k]))[:8]}"
    assert np.array_equal(got["r_coastDistLand"], host_coast_distance(case))


BOUNDARY_CELLS = (4096, 131072, 131073)     # one radix tile of 4 096 pairs exactly; one group of 32 tiles exactly; one group and a pair


@lru_cache(maxsize=None)
def boundary_case(cells):
    """synthetic_case with exactly `cells` cells (build_sphere adds the closing cell to the count it is given)."""
    case = synthetic_case(cells - 1)
    assert case["N"] == cells
    return case
