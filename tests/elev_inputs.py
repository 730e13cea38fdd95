"""assignElevation inputs at any size, built from committed fixtures or from seeds (no golden file of their own), the emulator
reference on them, and the per-cell comparison the device runs are held to.

Builders (each returns an ElevCase):
  golden_case(name) / large_golden_case()   the golden vectors' own inputs (5 k, 10 k and 250 k cells);
  realistic_case(N)     the coarse plates of plates_N10000_s1_P80 projected onto an N-cell build_sphere mesh and smoothed, with the
                        plate and super-plate tables of elev_config1_N10000_s1 (its plateSeeds are the plates fixture's, its
                        r_plate is r_plate_smoothed and plate -> super plate is a function there);
  many_plates_case(N, P)  P seeded graph-Voronoi plates (plate id = seed cell id, as in the reference), random poles / omegas /
                        densities, about half of them ocean, about P / 4 super plates grouping plates of one kind;
  hub_case(N) / relabelled_case(N)   realistic plates on a mesh with hubs of degree 9 .. 24 (WO_MAX_DEG), and on a relabelled
                        mesh with shuffled rows (tests/irregular_mesh.py).

The reference is the test-only emulator (tests/emu) with bfs_device = 0: the product's host stage, the reference's FIFO BFS and
the kernel bodies of csrc/elevation_ops.h with glibc's libm, equal to the reference JavaScript bit for bit on the goldens."""
import ctypes as C
import json
import subprocess
from dataclasses import dataclass
from functools import lru_cache

import numpy as np

from conftest import REPO, load_golden

EMU_DIR = REPO / "tests" / "emu"
LAYERS = ("base", "tectonic", "noise", "interior", "coastal", "ocean", "hotspot", "tecActivity", "margins", "backArc",
          "foldRidge", "orogenicPower")
BFS_FIELDS = ("coast", "rift", "ridge", "fracture", "backArc", "arc")
ULP_BOUND = 4 * 2.0 ** -23          # per cell, relative to max(1, |ref|): 4x the largest change a 2^20-ulp libm perturbation makes
HOOK_K = 4                          # double ulps: twice the 2-ulp bound of ocml's double tanh / exp / sin / cos / atan2 / pow / asin


def diff_cap(N):
    """The most cells of one output that may differ at all between the device and the emulator."""
    return max(8, N // 10 ** 4)


@dataclass
class Mesh:
    adjOffset: np.ndarray
    adjList: np.ndarray

    @property
    def numRegions(self):
        return self.adjOffset.size - 1


@dataclass
class ElevCase:
    name: str
    mesh: Mesh
    xyz: np.ndarray
    nd: np.ndarray
    r_plate: np.ndarray
    ids: np.ndarray             # plate ids (= plateSeeds), and per id: pole + omega (4 each), density, is-ocean
    vec4: np.ndarray
    dens: np.ndarray
    isoc: np.ndarray
    r_super: np.ndarray | None
    svec4: np.ndarray | None    # super plates 0 .. ns - 1
    sdens: np.ndarray | None
    sisoc: np.ndarray | None
    seed: int
    nMag: float
    spread: float

    @property
    def N(self):
        return self.mesh.numRegions


def _mesh(off, adj):
    return Mesh(np.ascontiguousarray(off, np.int32), np.ascontiguousarray(adj, np.int32))


def _case_from_golden(name, g, meta, mesh, xyz, nd):
    sup = meta["hasSuper"]
    return ElevCase(name, mesh, np.ascontiguousarray(xyz, np.float32), nd, np.ascontiguousarray(g["r_plate"], np.int32),
                    np.ascontiguousarray(g["plateSeeds"], np.int32), g["plateVec"], g["plateDensity"], g["plateIsOcean"],
                    np.ascontiguousarray(g["r_superPlate"], np.int32) if sup else None, g["superPlateVec"] if sup else None,
                    g["superPlateDensity"] if sup else None, g["superPlateIsOcean"] if sup else None,
                    int(meta["seed"]), float(meta["nMag"]), float(meta["spread"]))


def golden_case(name):
    g = load_golden(name)
    meta = json.loads(bytes(g["meta_json"]).decode())
    return _case_from_golden(name, g, meta, _mesh(g["adjOffset"], g["adjList"]), g["xyz"], g["neighborDist"])


def large_golden_case():
    from test_elevation_emulated import large_case
    g, meta, mesh, xyz, nd, _ = large_case()
    return _case_from_golden("elev_N250000_s4_large", g, meta, _mesh(mesh.adjOffset, mesh.adjList), xyz, nd)


# ---- realistic plates at any N ----

@lru_cache(maxsize=None)
def _config1_tables():
    g = load_golden("elev_config1_N10000_s1")
    rp, rs = g["r_plate"], g["r_superPlate"]
    to_super = np.full(int(g["plateSeeds"].max()) + 1, -1, np.int32)
    to_super[rp] = rs
    assert np.array_equal(to_super[rp], rs), "plate -> super plate is not a function in elev_config1_N10000_s1"
    return g, to_super


def _realistic_plates(mesh, xyz):
    from oracle import pyoracle as O
    from planet_heightmap_generation_amd import coarse_plates as CP
    from plates_common import plate_case
    c = plate_case("plates_N10000_s1_P80")
    g, _ = _config1_tables()
    assert np.array_equal(np.sort(g["plateSeeds"]), np.sort(c["seeds"])), "elev_config1 and plates_N10000_s1_P80 disagree on the plates"
    om, cm = O.Mesh(mesh.adjOffset, mesh.adjList), O.Mesh(c["cmesh"].adjOffset, c["cmesh"].adjList)
    rp = O.project_coarse_plates(om, xyz, cm, c["cxyz"], c["coarse_r_plate"], c["meta"]["seed"], c["meta"]["P"])
    CP.smooth_and_reconnect_plates(mesh, rp, c["seeds"], c["meta"]["passes"])
    return np.ascontiguousarray(rp, np.int32)


def _with_config1_tables(name, mesh, xyz, nd, rp):
    g, to_super = _config1_tables()
    assert (to_super[rp] >= 0).all(), "a projected plate has no super plate in elev_config1_N10000_s1"
    return ElevCase(name, mesh, np.ascontiguousarray(xyz, np.float32), nd, rp, np.ascontiguousarray(g["plateSeeds"], np.int32),
                    g["plateVec"], g["plateDensity"], g["plateIsOcean"], np.ascontiguousarray(to_super[rp], np.int32), g["superPlateVec"],
                    g["superPlateDensity"], g["superPlateIsOcean"], 1, 0.4, 5.0)


def realistic_case(N, seed=1):
    from planet_heightmap_generation_amd import sphere_mesh as S
    base, xyz, nd = S.build_sphere(N, 0.75, seed)
    mesh = _mesh(base.adjOffset, base.adjList)
    return _with_config1_tables(f"realistic_N{N}", mesh, xyz, nd, _realistic_plates(mesh, xyz))


# ---- many plates ----

def graph_voronoi(mesh, seeds):
    """Every cell takes the plate of its nearest seed in hops (ties: the smallest seed id); plate id = seed cell id."""
    off, adj = mesh.adjOffset.astype(np.int64), mesh.adjList
    deg = np.diff(off)
    label = np.full(mesh.numRegions, -1, np.int64)
    label[seeds] = seeds
    front = np.asarray(seeds, np.int64)
    while front.size:
        d = deg[front]
        idx = np.repeat(off[front] - np.cumsum(d) + d, d) + np.arange(int(d.sum()))
        src, dst = np.repeat(front, d), adj[idx].astype(np.int64)
        keep = label[dst] < 0
        src, dst = src[keep], dst[keep]
        order = np.lexsort((label[src], dst))
        dst, lab = dst[order], label[src][order]
        front, first = np.unique(dst, return_index=True)
        label[front] = lab[first]
    assert (label >= 0).all()
    return label.astype(np.int32)


def _random_poles(rng, n):
    p = rng.normal(size=(n, 3))
    return p / np.linalg.norm(p, axis=1, keepdims=True)


def many_plates_case(N, P, seed=7):
    from planet_heightmap_generation_amd import sphere_mesh as S
    rng = np.random.default_rng(seed)
    base, xyz, nd = S.build_sphere(N, 0.75, seed)
    mesh = _mesh(base.adjOffset, base.adjList)
    ids = np.sort(rng.choice(N, P, replace=False)).astype(np.int32)
    rp = graph_voronoi(mesh, ids)
    isoc = (rng.random(P) < 0.5).astype(np.uint8)
    vec4 = np.concatenate([_random_poles(rng, P), rng.uniform(-2, 2, (P, 1))], axis=1).reshape(-1)
    dens = np.where(isoc == 1, rng.uniform(3.0, 3.5, P), rng.uniform(2.4, 2.9, P))
    # super plates: the plates of one kind grouped around seeds of that kind (nearest seed by chord), like the fixtures'
    p3 = np.asarray(xyz, np.float64).reshape(-1, 3)[ids]
    to_super = np.empty(P, np.int64)
    sisoc, nsup = [], 0
    for kind in (1, 0):
        members = np.flatnonzero(isoc == kind)
        if members.size == 0:
            continue
        k = max(1, members.size // 4)
        centres = rng.choice(members, k, replace=False)
        to_super[members] = nsup + np.argmax(p3[members] @ p3[centres].T, axis=1)
        sisoc += [kind] * k
        nsup += k
    sdens = np.array([dens[to_super == s].mean() for s in range(nsup)])
    svec4 = np.concatenate([_random_poles(rng, nsup), rng.uniform(0.8, 1.8, (nsup, 1))], axis=1).reshape(-1)
    slot = np.full(N, -1, np.int64)
    slot[ids] = np.arange(P)
    r_super = to_super[slot[rp]].astype(np.int32)
    return ElevCase(f"many_plates_N{N}_P{P}", mesh, np.ascontiguousarray(xyz, np.float32), nd, rp, ids, vec4, dens, isoc, r_super,
                    svec4, sdens, np.array(sisoc, np.uint8), seed, 0.4, 5.0)


# ---- irregular meshes ----

def _boundary_cells(mesh, rp):
    rows = np.repeat(np.arange(mesh.numRegions), np.diff(mesh.adjOffset))
    b = np.zeros(mesh.numRegions, bool)
    np.logical_or.at(b, rows, rp[rows] != rp[mesh.adjList])
    return b


def hub_case(N, seed=3, max_degree=24):
    """Hubs of degree 9 .. max_degree (at least four of each), half of them on plate boundaries (where the BFS fields start)."""
    import irregular_mesh as IM
    from planet_heightmap_generation_amd import sphere_mesh as S
    base, xyz, _ = S.build_sphere(N, 0.75, seed)
    base = _mesh(base.adjOffset, base.adjList)
    rng = np.random.default_rng(seed)
    hd = IM.spread_degrees(max_degree, at_least=64)
    pools = [rng.permutation(np.flatnonzero(_boundary_cells(base, _realistic_plates(base, xyz)))).tolist(),
             rng.permutation(base.numRegions).tolist()]
    deg0 = IM.degrees(base)
    blocked, hubs = set(), []
    for i, d in enumerate(hd):
        pool = pools[i % 2]
        while pool[-1] in blocked or deg0[pool[-1]] > d:
            pool.pop()
        h = pool.pop()
        hubs.append(h)
        blocked |= IM.within_hops(base, h, IM.HUB_SEPARATION - 1)
    off, adj, nd = IM.add_hubs(base, xyz, list(zip(hubs, hd)), seed, cap=max_degree)
    mesh = _mesh(off, adj)
    assert int(IM.degrees(mesh).max()) == max_degree
    return _with_config1_tables(f"hub_N{N}_deg{max_degree}", mesh, xyz, nd, _realistic_plates(mesh, xyz))


def relabelled_case(N, seed=5):
    """build_sphere's mesh with its cells relabelled by a seeded permutation and the entries of every row shuffled."""
    import irregular_mesh as IM
    from planet_heightmap_generation_amd import sphere_mesh as S
    base, xyz, _ = S.build_sphere(N, 0.75, seed)
    perm = np.random.default_rng(seed).permutation(base.numRegions)
    m, p, _ = IM.permute_vertices(base, xyz, perm)
    m = IM.shuffle_rows(m, seed + 1)
    mesh = _mesh(m.adjOffset, m.adjList)
    return _with_config1_tables(f"relabelled_N{N}", mesh, p, S.compute_neighbor_dist(mesh, p), _realistic_plates(mesh, p))


# ---- the emulator reference ----

def _dense_table(ids, vec4, dens, isoc):
    n = int(np.max(ids)) + 1
    has = np.zeros(n, np.uint8); pole = np.zeros(3 * n); om = np.zeros(n); oc = np.zeros(n, np.uint8); de = np.full(n, np.nan)
    ids = np.asarray(ids)
    v = np.asarray(vec4, np.float64).reshape(-1, 4)
    has[ids] = 1; pole.reshape(-1, 3)[ids] = v[:, :3]; om[ids] = v[:, 3]; oc[ids] = isoc; de[ids] = dens
    return n, has, pole, om, oc, de


def _P(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def load_emulator(libm_hook=False):
    subprocess.run(["make", "-s", "-C", str(EMU_DIR)], check=True)
    L = C.CDLL(str(EMU_DIR / "_build" / ("libemu_libm.so" if libm_hook else "libemu.so")))
    p, i32, f64 = C.c_void_p, C.c_int32, C.c_double
    L.emu_assign_elevation.argtypes = [i32, p, p, p, p, i32, p, p, p, p, p, p, i32, p, i32, p, p, p, p, p, p, p, f64, f64, f64, p, p, p, p, p, p, p]
    L.emu_set_bfs_device.argtypes = [i32]
    L.emu_bfs_largest_frontiers.argtypes = [p]
    if libm_hook:
        L.emu_set_libm_perturb.argtypes = [C.c_uint64, C.c_int64]
        L.emu_libm_calls.argtypes = [p]
    return L


def libm_calls(L):
    """The hooked emulator's call counters since its last emu_set_libm_perturb: tanh, exp, sin, cos, atan2, pow, asin."""
    calls = np.zeros(7, np.uint64)
    L.emu_libm_calls(_P(calls))
    return calls


def emulate(L, case, bfs_device=0):
    """The emulator's outputs on `case`: elevation, stress, the 12 layers, the three Sets, and the largest frontier of every BFS field."""
    from oracle import pyoracle as O
    L.emu_set_bfs_device(bfs_device)
    N = case.N
    n, has, pole, om, oc, de = _dense_table(case.ids, case.vec4, case.dens, case.isoc)
    if case.r_super is not None:
        ns = len(case.sdens)
        sn, shas, spole, som, soc, sde = _dense_table(np.arange(ns), case.svec4, case.sdens, case.sisoc)
    else:
        sn, shas, spole, som, soc, sde = 0, None, None, None, None, None
    perm, pm12 = O.noise_tables(case.seed)
    e = np.zeros(N, np.float32); st = np.zeros(N, np.float32); dl = np.zeros(12 * N, np.float32)
    mo = np.zeros(N, np.int32); co = np.zeros(N, np.int32); oc_ = np.zeros(N, np.int32); cnt = np.zeros(3, np.int32)
    rc = L.emu_assign_elevation(N, _P(case.mesh.adjOffset), _P(case.mesh.adjList), _P(case.xyz), _P(case.r_plate), n, _P(has), _P(pole), _P(om),
                                _P(oc), _P(de), _P(case.ids), case.ids.size, _P(case.r_super), sn, _P(shas), _P(spole), _P(som), _P(soc), _P(sde),
                                _P(perm), _P(pm12), case.nMag, float(case.seed), float(case.spread), _P(e), _P(st), _P(dl), _P(mo), _P(co),
                                _P(oc_), _P(cnt))
    assert rc == 0
    fr = np.zeros(6, np.int32)
    L.emu_bfs_largest_frontiers(_P(fr))
    return {"r_elevation": e, "r_stress": st, "debugLayers": {name: dl[i * N:(i + 1) * N] for i, name in enumerate(LAYERS)},
            "mountain_r": mo[:cnt[0]].tolist(), "coastline_r": co[:cnt[1]].tolist(), "ocean_r": oc_[:cnt[2]].tolist(),
            "frontiers": dict(zip(BFS_FIELDS, fr.tolist()))}


# ---- the device ----

def device_args(case):
    """assign_elevation's argument objects (the reference's: keyed dicts, id lists) for `case`."""
    from planet_heightmap_generation_amd import elevation as EL
    ids = case.ids.tolist()
    v = np.asarray(case.vec4, np.float64).reshape(-1, 4)
    vec = {pid: {"pole": v[i, :3].tolist(), "omega": float(v[i, 3])} for i, pid in enumerate(ids)}
    dens = {pid: float(case.dens[i]) for i, pid in enumerate(ids)}
    is_ocean = [pid for i, pid in enumerate(ids) if case.isoc[i]]
    sup = None
    if case.r_super is not None:
        ns = len(case.sdens)
        sv = np.asarray(case.svec4, np.float64).reshape(-1, 4)
        sup = {"r_superPlate": case.r_super,
               "superPlateVec": {s: {"pole": sv[s, :3].tolist(), "omega": float(sv[s, 3])} for s in range(ns)},
               "superPlateIsOcean": [s for s in range(ns) if case.sisoc[s]],
               "superPlateDensity": {s: float(case.sdens[s]) for s in range(ns)}}
    return (is_ocean, case.r_plate, vec, ids, EL.SimplexNoise(case.seed), case.nMag, case.seed, case.spread, dens, sup)


def on_device(case, planet, debug=True):
    from planet_heightmap_generation_amd import elevation as EL
    is_ocean, rp, vec, ids, noise, nMag, seed, spread, dens, sup = device_args(case)
    return EL.assign_elevation(case.mesh, case.xyz, is_ocean, rp, vec, ids, noise, nMag, seed, spread, dens, sup, planet=planet, debug=debug)


# ---- the comparison ----

def deviation(out, ref):
    """(cells that differ at all, largest |out - ref|, cells past the per-cell bound) of one float output."""
    a, b = np.asarray(out, np.float64), np.asarray(ref, np.float64)
    d = np.abs(a - b)
    differ = out != ref
    over = ~(d <= ULP_BOUND * np.maximum(1.0, np.abs(b)))          # NaN on either side counts as past the bound
    return int(differ.sum()), float(d[differ].max()) if differ.any() else 0.0, int(over.sum())


def compare(label, got, ref, N, stress_exact=True, layers=LAYERS):
    """Sets bit for bit; stress bit for bit (stress_exact) or under the elevation rule; elevation and every layer: each cell within
    ULP_BOUND * max(1, |ref|) and at most diff_cap(N) cells different.  Prints every output's figures before asserting."""
    assert got["mountain_r"] == ref["mountain_r"], f"{label}: mountain Set differs"
    assert got["coastline_r"] == ref["coastline_r"], f"{label}: coastline Set differs"
    assert got["ocean_r"] == ref["ocean_r"], f"{label}: ocean Set differs"
    rows = [("r_elevation", got["r_elevation"], ref["r_elevation"]), ("r_stress", got["r_stress"], ref["r_stress"])]
    rows += [("dl_" + name, got["debugLayers"][name], ref["debugLayers"][name]) for name in layers]
    figs = {k: deviation(a, b) for k, a, b in rows}
    cap = diff_cap(N)
    print(f"{label} (N={N}, cap {cap}): " + "; ".join(f"{k} {n} differ, max {m:.3g}" + (f", {o} past bound" if o else "")
                                                        for k, (n, m, o) in figs.items()))
    bad = []
    for k, (n, m, o) in figs.items():
        if k == "r_stress" and stress_exact:
            if n:
                bad.append(f"{k}: {n} cells differ (must be bit for bit)")
        elif o or n > cap:
            bad.append(f"{k}: {n} cells differ (cap {cap}), {o} past the per-cell bound, largest deviation {m:.3g}")
    assert not bad, f"{label}: " + "; ".join(bad)
    return figs
