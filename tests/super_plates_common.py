"""buildSuperPlates (js/super-plates.js) for the tests: a Python emulator of the whole function, the committed cases, and the calls
into the library.

The emulator is written from the function's description, in the two halves the product has:
  tables(...)   what the device computes from the cells: area per plate (bincount) and, per ordered plate pair (a, b), the smallest
                adjList index at which a cell of a sees a cell of b (np.minimum.at);
  group(...)    the plate-level part: neighbours sorted by that index (the insertion order of the reference's Set), BFS components of
                one kind, farthest-point seeding, the two O(n^2) Dijkstras with strict <, area-weighted poles / kinds / densities.
Python floats are IEEE doubles and every sum is written left to right, so it can be — and is asserted to be — equal in every bit
to the reference's output on the two elevation goldens and on every case of super_plates_edits_N10000_s1.  That makes it the
reference for synthetic inputs.  Plates are "slots" (positions in plateSeeds) throughout."""
import ctypes as C
import json
import math
from dataclasses import dataclass
from functools import lru_cache

import numpy as np

from conftest import load_golden

NEVER = 0xFFFFFFFF
MAX_PLATES = 1024
FIXTURE = "super_plates_edits_N10000_s1"
ELEV_GOLDENS = ("elev_config1_N10000_s1", "elev_N10000_s2")


@dataclass
class SuperCase:
    name: str
    off: np.ndarray            # int32 CSR
    adj: np.ndarray
    r_plate: np.ndarray        # int32 plate id per cell
    seeds: np.ndarray          # int32 plateSeeds in the Set's order
    hasVec: np.ndarray         # uint8 per slot
    vec4: np.ndarray           # float64 (P, 4): pole, omega
    isoc: np.ndarray           # uint8 per slot
    dens: np.ndarray           # float64 per slot, NaN: undefined
    ref: dict | None = None    # the reference's r_superPlate, superPlateVec (ns, 4), superPlateDensity, superPlateIsOcean

    @property
    def P(self):
        return int(self.seeds.size)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


# ---- the emulator ----

def slot_table(seeds):
    slot = np.full(int(np.max(seeds)) + 1, -1, np.int64)
    slot[np.asarray(seeds)] = np.arange(len(seeds))
    return slot


def tables(off, adj, r_plate, seeds):
    """(area int32[P], firstSlot uint32[P * P])"""
    P = len(seeds)
    a = slot_table(seeds)[np.asarray(r_plate, np.int64)]
    assert (a >= 0).all()
    area = np.bincount(a, minlength=P).astype(np.int32)
    rows = np.repeat(np.arange(len(r_plate), dtype=np.int64), np.diff(np.asarray(off, np.int64)))
    sa, sb = a[rows], a[np.asarray(adj, np.int64)]
    keep = sa != sb
    first = np.full(P * P, NEVER, np.uint32)
    np.minimum.at(first, sa[keep] * P + sb[keep], np.flatnonzero(keep).astype(np.uint32))
    return area, first


def js_round(x):
    return int(math.floor(x + 0.5))


def group(P, hasVec, vec4, isoc, dens, area, first):
    """{plateToSuper int32[P], numSuper, vec4 (ns, 4), isOcean uint8[ns], density float64[ns]}"""
    first = np.asarray(first, np.uint32).reshape(P, P)
    area = [int(x) for x in area]
    vec4 = np.asarray(vec4, np.float64).reshape(-1, 4)
    nbrs = []
    for a in range(P):
        nb = [b for b in range(P) if b != a and first[a, b] != NEVER]
        nbrs.append(sorted(nb, key=lambda b: int(first[a, b])))
    seen, comps = [False] * P, []
    for a in range(P):
        if seen[a]:
            continue
        q, head = [a], 0
        seen[a] = True
        while head < len(q):
            for nb in nbrs[q[head]]:
                if not seen[nb] and bool(isoc[nb]) == bool(isoc[a]):
                    seen[nb] = True
                    q.append(nb)
            head += 1
        comps.append(q)
    target = max(2, min(20, js_round(P / 4)))
    to_super, nxt = [-1] * P, 0
    for comp in comps:
        k = max(1, js_round(target * len(comp) / P))
        if k <= 1:
            for a in comp:
                to_super[a] = nxt
            nxt += 1
            continue
        inside = set(comp)
        local = {a: [b for b in nbrs[a] if b in inside] for a in comp}
        w = {a: math.sqrt(area[a] or 1) for a in comp}

        def dijkstra(starts, carry=None):
            d = {a: math.inf for a in comp}
            done = set()
            for s in starts:
                d[s] = 0.0
            for _ in comp:
                cur, best = -1, math.inf
                for a in comp:
                    if a not in done and d[a] < best:
                        best, cur = d[a], a
                if cur == -1:
                    break
                done.add(cur)
                for nb in local[cur]:
                    nd = d[cur] + w[nb]
                    if nd < d[nb]:
                        d[nb] = nd
                        if carry is not None:
                            carry[nb] = carry[cur]
            return d

        seeds = [comp[0]]
        d = dijkstra(seeds)
        for _ in range(1, k):
            far, most = comp[0], -1
            for a in comp:
                if d[a] > most:
                    most, far = d[a], a
            seeds.append(far)
            d = dijkstra(seeds)
        carry = {a: -1 for a in comp}
        for si, s in enumerate(seeds):
            carry[s] = nxt + si
        dijkstra(seeds, carry)
        for a in comp:
            to_super[a] = carry[a]
        nxt += len(seeds)
    ns = nxt
    L = [[0.0, 0.0, 0.0] for _ in range(ns)]
    osum, asum, largest = [0.0] * ns, [0.0] * ns, [None] * ns
    for a in range(P):
        sp = to_super[a]
        if not hasVec[a]:
            continue
        ar, om = float(area[a]), float(vec4[a, 3])
        for j in range(3):
            L[sp][j] += ar * om * float(vec4[a, j])
        osum[sp] += ar * abs(om)
        asum[sp] += ar
        if largest[sp] is None or area[a] > area[largest[sp]]:
            largest[sp] = a
    out4 = np.zeros((ns, 4), np.float64)
    for sp in range(ns):
        lx, ly, lz = L[sp]
        ln = math.sqrt(lx * lx + ly * ly + lz * lz)
        if ln < 1e-8 or asum[sp] < 1:
            out4[sp] = vec4[largest[sp]] if largest[sp] is not None else (0.0, 1.0, 0.0, 0.0)
            continue
        out4[sp] = (lx / ln, ly / ln, lz / ln, osum[sp] / asum[sp])
    oc, tot, ds, da = [0.0] * ns, [0.0] * ns, [0.0] * ns, [0.0] * ns
    for a in range(P):
        sp, ar = to_super[a], float(area[a])
        tot[sp] += ar
        if isoc[a]:
            oc[sp] += ar
        if not math.isnan(dens[a]):
            ds[sp] += ar * float(dens[a])
            da[sp] += ar
    return {"plateToSuper": np.array(to_super, np.int32), "numSuper": ns, "vec4": out4,
            "isOcean": np.array([1 if oc[sp] > tot[sp] * 0.5 else 0 for sp in range(ns)], np.uint8),
            "density": np.array([ds[sp] / da[sp] if da[sp] > 0 else 2.7 for sp in range(ns)], np.float64)}


def emulate(case):
    """The four arrays of the reference's result (+ the tables they were made from) for a SuperCase."""
    area, first = tables(case.off, case.adj, case.r_plate, case.seeds)
    g = group(case.P, case.hasVec, case.vec4, case.isoc, case.dens, area, first)
    r_super = g["plateToSuper"][slot_table(case.seeds)[case.r_plate]].astype(np.int32)
    return {"r_superPlate": r_super, "superPlateVec": g["vec4"], "superPlateDensity": g["density"], "superPlateIsOcean": g["isOcean"],
            "area": area, "firstSlot": first, "plateToSuper": g["plateToSuper"]}


def assert_matches(label, got, ref):
    """r_superPlate exactly, the float64 tables bit for bit."""
    assert np.array_equal(got["r_superPlate"], ref["r_superPlate"]), f"{label}: r_superPlate differs in {(np.asarray(got['r_superPlate']) != ref['r_superPlate']).sum()} cells"
    assert same_bits(np.asarray(got["superPlateVec"]).reshape(-1), np.asarray(ref["superPlateVec"]).reshape(-1)), f"{label}: superPlateVec"
    assert same_bits(got["superPlateDensity"], ref["superPlateDensity"]), f"{label}: superPlateDensity"
    assert np.array_equal(np.asarray(got["superPlateIsOcean"], np.uint8), np.asarray(ref["superPlateIsOcean"], np.uint8)), f"{label}: superPlateIsOcean"


# ---- the committed cases ----

def _ref_of(g, prefix=""):
    return {"r_superPlate": np.ascontiguousarray(g[prefix + "r_superPlate"], np.int32), "superPlateVec": np.asarray(g[prefix + "superPlateVec"], np.float64).reshape(-1, 4),
            "superPlateDensity": np.asarray(g[prefix + "superPlateDensity"], np.float64), "superPlateIsOcean": np.asarray(g[prefix + "superPlateIsOcean"], np.uint8)}


@lru_cache(maxsize=None)
def elev_golden_case(name):
    g = load_golden(name)
    P = g["plateSeeds"].size
    return SuperCase(name, np.ascontiguousarray(g["adjOffset"], np.int32), np.ascontiguousarray(g["adjList"], np.int32), np.ascontiguousarray(g["r_plate"], np.int32),
                     np.ascontiguousarray(g["plateSeeds"], np.int32), np.ones(P, np.uint8), np.asarray(g["plateVec"], np.float64).reshape(P, 4),
                     np.asarray(g["plateIsOcean"], np.uint8), np.asarray(g["plateDensity"], np.float64), _ref_of(g))


@lru_cache(maxsize=None)
def fixture_names():
    return tuple(json.loads(bytes(load_golden(FIXTURE)["cases_json"]).decode()))


@lru_cache(maxsize=None)
def fixture_case(name):
    """A case of the fixture: config 1's mesh (and r_plate / plateSeeds / plateVec unless the case has its own) with the case's edits."""
    f, base = load_golden(FIXTURE), elev_golden_case("elev_config1_N10000_s1")
    k = name + "__"
    seeds = np.ascontiguousarray(f[k + "plateSeeds"], np.int32) if k + "plateSeeds" in f.files else base.seeds
    P = seeds.size
    r_plate = np.ascontiguousarray(f[k + "r_plate"], np.int32) if k + "r_plate" in f.files else base.r_plate
    has = np.asarray(f[k + "hasVec"], np.uint8) if k + "hasVec" in f.files else np.ones(P, np.uint8)
    return SuperCase(name, base.off, base.adj, r_plate, seeds, has, base.vec4[:P], np.asarray(f[k + "plateIsOcean"], np.uint8),
                     np.asarray(f[k + "plateDensity"], np.float64), _ref_of(f, k))


def from_elev_case(ec):
    """A tests/elev_inputs.py ElevCase as a SuperCase (its own super plates are not the function's: no reference)."""
    P = ec.ids.size
    return SuperCase(ec.name, ec.mesh.adjOffset, ec.mesh.adjList, np.ascontiguousarray(ec.r_plate, np.int32), np.ascontiguousarray(ec.ids, np.int32),
                     np.ones(P, np.uint8), np.asarray(ec.vec4, np.float64).reshape(P, 4), np.asarray(ec.isoc, np.uint8), np.asarray(ec.dens, np.float64))


# ---- the library ----

def dense_plate_table(case):
    """wo_plate_table (dense by plate id) of a SuperCase + the arrays that back it."""
    from planet_heightmap_generation_amd.elevation import PlateTable
    n = int(case.seeds.max()) + 1
    has = np.zeros(n, np.uint8); pole = np.zeros(3 * n); om = np.zeros(n); oc = np.zeros(n, np.uint8); de = np.full(n, np.nan)
    ids = case.seeds
    has[ids] = case.hasVec; pole.reshape(-1, 3)[ids] = case.vec4[:, :3]; om[ids] = case.vec4[:, 3]; oc[ids] = case.isoc; de[ids] = case.dens
    return PlateTable(n, has.ctypes.data, pole.ctypes.data, om.ctypes.data, oc.ctypes.data, de.ctypes.data), (has, pole, om, oc, de)


def lib_group(case, area, first):
    """wo_super_plates_group on a case and the two tables: (status, result dict in the emulator's shape)."""
    from planet_heightmap_generation_amd import capi
    P = case.P
    t, keep = dense_plate_table(case)
    to_super = np.full(P, -1, np.int32); ns = np.zeros(1, np.int32)
    pole = np.zeros(3 * P); om = np.zeros(P); oc = np.zeros(P, np.uint8); de = np.zeros(P)
    area, first = np.ascontiguousarray(area, np.int32), np.ascontiguousarray(first, np.uint32)
    rc = capi.lib().wo_super_plates_group(P, capi.ptr(case.seeds), C.byref(t), capi.ptr(area), capi.ptr(first), capi.ptr(to_super), capi.ptr(ns),
                                          capi.ptr(pole), capi.ptr(om), capi.ptr(oc), capi.ptr(de))
    if rc:
        return rc, None
    n = int(ns[0])
    return 0, {"plateToSuper": to_super, "numSuper": n, "r_superPlate": to_super[slot_table(case.seeds)[case.r_plate]].astype(np.int32) if case.r_plate is not None else None,
               "superPlateVec": np.concatenate([pole[:3 * n].reshape(n, 3), om[:n, None]], axis=1), "superPlateDensity": de[:n], "superPlateIsOcean": oc[:n]}


def reference_args(case):
    """build_super_plates' argument objects (the reference's: id lists, keyed dicts) for a SuperCase."""
    ids = case.seeds.tolist()
    vec = {pid: {"pole": case.vec4[i, :3].tolist(), "omega": float(case.vec4[i, 3])} for i, pid in enumerate(ids) if case.hasVec[i]}
    dens = {pid: float(case.dens[i]) for i, pid in enumerate(ids) if not math.isnan(case.dens[i])}
    return ids, vec, [pid for i, pid in enumerate(ids) if case.isoc[i]], dens


def result_arrays(res):
    """build_super_plates' dict in the emulator's shape."""
    n = res["numSuperPlates"]
    v = res["superPlateVec"]
    oc = np.zeros(n, np.uint8); oc[list(res["superPlateIsOcean"])] = 1
    return {"r_superPlate": res["r_superPlate"], "superPlateVec": np.array([list(v[s]["pole"]) + [v[s]["omega"]] for s in range(n)], np.float64).reshape(n, 4),
            "superPlateDensity": np.array([res["superPlateDensity"][s] for s in range(n)], np.float64), "superPlateIsOcean": oc}
