"""Shared pieces of the rivers tests: an independent serial statement of the contract of csrc/rivers_ops.h in Python (receivers by a row
loop, basins by following chains, spills by a literal Prim with heapq over the pass keys, W in pop order, discharge with Python
ints), the host emulator of the same header (tests/emu_rivers), the meshes and the field builders.  The oracle takes any CSR graph
(oracle_structure_graph, oracle_graph); oracle_structure and oracle are its kept forms on the meshes and fields named here."""
from __future__ import annotations

import ctypes as C
import functools
import heapq
import math
import struct
import subprocess

import numpy as np

import map_common as MC
import relief_common as RC
from conftest import REPO

EMU_DIR = REPO / "tests" / "emu_rivers"
FIELDS = ("r_river_receiver", "r_river_basin", "r_lake_level", "r_river_discharge", "r_river_flow")
QUIET_NAN = 0x7FC00000
NO_PASS = 0xFFFFFFFFFFFFFFFF
TINT = (41, 98, 168, 255)
MESHES = ("N256", "N2000", "N10000")
FIELD_KINDS = ("noise", "bowl", "plateau", "allLand", "allOcean", "cone")
SOURCES = ("precip", "uniform", "values")
BOWL_SEED = 5
_emu = None


# ---- meshes and fields -----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def mesh(which):
    """-> (mesh, xyz float32 [N, 3], off int32, adj int32)"""
    if which == "N256":
        from planet_heightmap_generation_amd import sphere_mesh as S
        m, xyz, _ = S.build_sphere(256, 0.75, 1)
    else:
        m, xyz = MC.golden_mesh("mesh_N2000_s1" if which == "N2000" else "mesh_N10000_s1")
    xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    return m, xyz, np.ascontiguousarray(m.adjOffset, np.int32), np.ascontiguousarray(m.adjList, np.int32)


def field(kind, xyz, seed=BOWL_SEED):
    """The elevation fields of the tests, float32 per cell"""
    p = xyz.astype(np.float64)
    n = p.shape[0]
    if kind == "noise":                                       # (a) both signs, a few NaN cells
        return RC.field(xyz, 11, nans=min(7, n // 40))
    if kind == "bowl":                                        # (b) white noise on a bowl around +z, its rim at z = -0.5, ocean below z = -0.8
        z = p[:, 2]
        bowl = np.where(z > -0.5, 0.15 + 0.5 * (1.0 - z) / 1.5, 0.65 - 1.5 * (-0.5 - z))
        e = bowl + np.random.default_rng(seed).normal(size=n) * 0.06
        return np.where(z < -0.8, -0.3, np.maximum(e, 0.01)).astype(np.float32)
    if kind == "plateau":                                     # (c) one value, one ocean cell: the keys are decided by the index alone
        e = np.full(n, 0.5, np.float32)
        e[n // 3] = -1.0
        return e
    if kind == "allLand":                                     # (d)
        return (np.abs(MC.fbm_like(xyz, 3)) + np.float32(0.05)).astype(np.float32)
    if kind == "allOcean":                                    # (e) with both zeros, which are no land
        e = (-np.abs(MC.fbm_like(xyz, 3))).astype(np.float32)
        e[1], e[2] = 0.0, -0.0
        return e
    if kind == "cone":                                        # (f) falls with z all the way to a small ocean cap: no pit
        z = p[:, 2]
        return np.where(z < -0.9, -0.2, 0.05 + (1.0 + z)).astype(np.float32)
    raise KeyError(kind)


def runoff_fields(xyz):
    """-> (summer, winter, values): two synthetic precipitation fields with negative values, values above the clamp and NaNs, and
    their f32 mean as the contract evaluates it"""
    s = (MC.fbm_like(xyz, 21) * np.float32(3.0) + np.float32(0.6)).astype(np.float32)
    w = (MC.fbm_like(xyz, 22) * np.float32(40.0) + np.float32(1.0)).astype(np.float32)
    s[5::97] = np.nan
    w[11::89] = np.nan
    return s, w, ((s + w) * np.float32(0.5)).astype(np.float32)


def runoff_of(source, xyz):
    """the per-cell runoff a source stands for, float32"""
    if source == "uniform":
        return np.ones(xyz.shape[0], np.float32)
    return runoff_fields(xyz)[2]


# ---- the oracle ------------------------------------------------------------------------------------------------------------------
def ordered_bits(x):
    u = struct.unpack("<I", struct.pack("<f", x))[0]
    return (~u & 0xFFFFFFFF) if u & 0x80000000 else (u | 0x80000000)


def quantise(runoff):
    """q per cell as Python ints (land is applied by the caller)"""
    out = []
    for x in np.asarray(runoff, np.float32).tolist():
        out.append(0 if x != x else int(math.floor(min(max(x, 0.0), 16.0) * 65536.0 + 0.5)))
    return out


def oracle_structure_graph(off, adj, e):
    """Steps 1 to 6 on any CSR graph and field -> dict(e, land, recv2 (step 2), receiver (final), basin, lake, pits, spilled, endorheic, drowned)"""
    e32 = np.ascontiguousarray(e, np.float32)
    e = e32.tolist()
    n = len(e)
    offl, adjl = np.asarray(off).tolist(), np.asarray(adj).tolist()
    land = [x > 0 for x in e]
    recv = [-1] * n
    for r in range(n):
        if not land[r]:
            continue
        best = (e[r], r)
        for k in range(offl[r], offl[r + 1]):
            v = adjl[k]
            if e[v] != e[v]:
                continue
            if (e[v], v) < best:
                best = (e[v], v)
        recv[r] = best[1] if best[1] != r else -1
    DRAINED, NOT_LAND = -1, -2
    basin = [NOT_LAND] * n
    for r in range(n):
        if not land[r]:
            continue
        chain, x = [], r
        while True:
            if basin[x] != NOT_LAND:
                c = basin[x]
                break
            chain.append(x)
            if recv[x] < 0:
                c = x
                break
            if not land[recv[x]]:
                c = DRAINED
                break
            x = recv[x]
        for y in chain:
            basin[y] = c
    # passes per class: (key, inner cell, outer cell)
    passes = {}
    for u in range(n):
        if not land[u]:
            continue
        for k in range(offl[u], offl[u + 1]):
            v = adjl[k]
            if v < u or not land[v] or basin[u] == basin[v]:
                continue
            key = (ordered_bits(max(e[u], e[v])) << 32) | k   # u < v: k is where v stands in the row of u
            passes.setdefault(basin[u], []).append((key, u, v))
            passes.setdefault(basin[v], []).append((key, v, u))
    resolved = {DRAINED}
    heap = [(key, outer, inner) for key, inner, outer in passes.get(DRAINED, [])]      # (key, u unresolved side, v resolved side)
    heapq.heapify(heap)
    spill_to, W = {}, {}
    drowned = 0
    while heap:
        key, u, v = heapq.heappop(heap)
        B = basin[u]
        if B in resolved:
            continue
        level = max(e[u], e[v])
        spill_to[B] = v
        P = basin[v]
        if P != DRAINED and e[v] < W[P]:
            W[B] = W[P]
            drowned += 1
        else:
            W[B] = level
        resolved.add(B)
        for k2, inner, outer in passes.get(B, []):
            if basin[outer] not in resolved:
                heapq.heappush(heap, (k2, outer, inner))
    final = list(recv)
    lake = np.full(n, np.nan, np.float32)
    lake.view(np.uint32)[:] = QUIET_NAN
    for r in range(n):
        B = basin[r]
        if B >= 0 and B in spill_to:
            if B == r:
                final[r] = spill_to[B]
            if e[r] < W[B]:
                lake[r] = np.float32(W[B])
    pits = sorted(b for b in set(basin) if b >= 0)
    return dict(e=e32, land=np.array(land), recv2=np.array(recv, np.int32), receiver=np.array(final, np.int32), basin=np.array(basin, np.int32), lake=lake, pits=len(pits),
                spilled=len(spill_to), endorheic=len(pits) - len(spill_to), drowned=drowned)


@functools.lru_cache(maxsize=None)
def oracle_structure(which, kind):
    """oracle_structure_graph on a mesh and a field of this file by their names, kept"""
    _, xyz, off, adj = mesh(which)
    return oracle_structure_graph(off, adj, field(kind, xyz))


def oracle(which, kind, runoff):
    """The five fields under their keys (+ the structure's entries) for per-cell runoff values"""
    return oracle_discharge(oracle_structure(which, kind), runoff)


def oracle_graph(off, adj, e, runoff):
    """oracle on any CSR graph: (off, adj, e, runoff) arrays"""
    return oracle_discharge(oracle_structure_graph(off, adj, e), runoff)


def oracle_discharge(S, runoff):
    """Step 7 on a structure"""
    n = S["e"].size
    q = quantise(runoff)
    D = [q[r] if S["land"][r] else 0 for r in range(n)]
    recv = S["receiver"].tolist()
    donors = [[] for _ in range(n)]
    for r in range(n):
        if recv[r] >= 0:
            donors[recv[r]].append(r)
    done = [False] * n
    for root in range(n):
        if recv[root] >= 0:
            continue
        stack = [(root, 0)]                                   # post-order: a cell's donors first
        while stack:
            r, i = stack.pop()
            if i < len(donors[r]):
                stack.append((r, i + 1))
                stack.append((donors[r][i], 0))
            else:
                done[r] = True
                if recv[r] >= 0:
                    D[recv[r]] += D[r]
    assert all(done), "the final receivers have a cycle"
    out = dict(S)
    out["q"] = q
    out["r_river_receiver"], out["r_river_basin"], out["r_lake_level"] = S["receiver"], S["basin"], S["lake"]
    out["r_river_discharge"] = np.array(D, np.uint64)
    out["r_river_flow"] = np.array([np.float32(d * 2.0 ** -16) for d in D], np.float32)
    return out


def oracle_river_cells(O, min_flow):
    """ascending cell ids of the river cells under min_flow"""
    m = max(0, int(math.ceil(min_flow * 65536.0)))
    D = O["r_river_discharge"]
    keep = O["land"] & (D >= np.uint64(min(m, 2 ** 64 - 1))) & (O["recv2"] >= 0) & np.isnan(O["r_lake_level"])
    return np.nonzero(keep)[0]


def oracle_lines(O, xyz, min_flow):
    """-> (segments float32 [count, 2, 3], flows float32 [count])"""
    cells = oracle_river_cells(O, min_flow)
    to = O["r_river_receiver"][cells]
    e = O["e"].astype(np.float64)
    with np.errstate(invalid="ignore"):
        d = 1.003 + np.where(e > 0, e * 0.04, e * 0.04 * 0.3)
    p = xyz.astype(np.float64)
    seg = np.stack([p[cells] * d[cells, None], p[to] * d[to, None]], axis=1).astype(np.float32)
    return seg, O["r_river_flow"][cells]


def oracle_tinted(O, min_flow):
    t = ~np.isnan(O["r_lake_level"])
    t[oracle_river_cells(O, min_flow)] = True
    return t


# ---- the emulator ----------------------------------------------------------------------------------------------------------------
def emu():
    global _emu
    if _emu is None:
        subprocess.run(["make", "-s", "-C", str(EMU_DIR)], check=True)
        _emu = C.CDLL(str(EMU_DIR / "_build" / "libemu_rivers.so"))
        _emu.emu_rivers_lines.restype = C.c_int32
    return _emu


def emu_compute(off, adj, e, source, a=None, b=None):
    """source: 0 precip (a, b), 1 uniform, 2 values (a) -> the five fields under their keys and info: landCells, pits, spilled,
    endorheic, lakeCells, rounds, drowned"""
    n = e.size
    e = np.ascontiguousarray(e, np.float32)
    a = None if a is None else np.ascontiguousarray(a, np.float32)
    b = None if b is None else np.ascontiguousarray(b, np.float32)
    out = dict(r_river_receiver=np.empty(n, np.int32), r_river_basin=np.empty(n, np.int32), r_lake_level=np.empty(n, np.float32), r_river_discharge=np.empty(n, np.uint64),
               r_river_flow=np.empty(n, np.float32))
    info = np.zeros(7, np.int32)
    emu().emu_rivers_compute(C.c_int32(n), MC.ptr(off), MC.ptr(adj), MC.ptr(e), C.c_int32(source), MC.ptr(a), MC.ptr(b), *(MC.ptr(out[k]) for k in FIELDS), MC.ptr(info))
    out["info"] = dict(zip(("landCells", "pits", "spilled", "endorheic", "lakeCells", "rounds", "drowned"), info.tolist()))
    return out


def emu_first_round(off, adj, e, basin):
    """The first contraction round's bodies (cell_offer, hook_of) on the basins of a structure, every pit a component of its own, the
    pit list in ascending cell order as the emulator builds it -> (pits, best uint64 [P + 1], to int32 [P], edges int32 [P, 4]: the
    pass root c recorded as u, v, pu, pv, -1 where it stayed a root)"""
    off, adj, e = np.ascontiguousarray(off, np.int32), np.ascontiguousarray(adj, np.int32), np.ascontiguousarray(e, np.float32)
    n = e.size
    pits = np.nonzero(basin == np.arange(n))[0].astype(np.int32)
    P = pits.size
    index = np.full(n, -1, np.int32)
    index[pits] = np.arange(P, dtype=np.int32)
    cellPit = np.where(basin >= 0, index[np.maximum(basin, 0)], np.where(basin == -1, P, -1)).astype(np.int32)
    comp = np.arange(P + 1, dtype=np.int32)
    best = np.empty(P + 1, np.uint64)
    emu().emu_rivers_offers(C.c_int32(n), MC.ptr(off), MC.ptr(adj), MC.ptr(e), MC.ptr(cellPit), MC.ptr(comp), C.c_int32(P), MC.ptr(best))
    to, edges = np.empty(P, np.int32), np.empty((P, 4), np.int32)
    emu().emu_rivers_hook.restype = C.c_int32
    for c in range(P):
        to[c] = emu().emu_rivers_hook(C.c_int32(n), MC.ptr(off), MC.ptr(adj), MC.ptr(e), MC.ptr(cellPit), MC.ptr(comp), MC.ptr(best), C.c_int32(c), MC.ptr(edges[c]))
    return pits, best, to, edges


def emu_by_source(off, adj, e, source, xyz):
    s, w, v = runoff_fields(xyz)
    if source == "precip":
        return emu_compute(off, adj, e, 0, s, w)
    return emu_compute(off, adj, e, 1) if source == "uniform" else emu_compute(off, adj, e, 2, v)


def emu_lines(xyz, e, R, min_flow):
    n = e.size
    seg, flows = np.empty((n, 2, 3), np.float32), np.empty(n, np.float32)
    k = emu().emu_rivers_lines(C.c_int32(n), MC.ptr(np.ascontiguousarray(xyz, np.float32)), MC.ptr(np.ascontiguousarray(e, np.float32)), MC.ptr(R["r_river_receiver"]),
                               MC.ptr(R["r_river_basin"]), MC.ptr(R["r_lake_level"]), MC.ptr(R["r_river_discharge"]), MC.ptr(R["r_river_flow"]), C.c_double(min_flow), MC.ptr(seg),
                               MC.ptr(flows))
    return seg[:k].copy(), flows[:k].copy()


def emu_tinted(e, R, min_flow):
    out = np.empty(e.size, np.uint8)
    emu().emu_rivers_tinted(C.c_int32(e.size), MC.ptr(np.ascontiguousarray(e, np.float32)), MC.ptr(R["r_river_receiver"]), MC.ptr(R["r_river_basin"]), MC.ptr(R["r_lake_level"]),
                            MC.ptr(R["r_river_discharge"]), C.c_double(min_flow), MC.ptr(out))
    return out.astype(bool)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def assert_fields_equal(tag, got, want):
    """all five fields in every bit (the lake level's NaN included)"""
    for k in FIELDS:
        g, w = bits(got[k]), bits(want[k])
        assert g.dtype == w.dtype and g.shape == w.shape, (tag, k, g.dtype, w.dtype)
        bad = int((g != w).sum())
        assert bad == 0, (tag, k, bad, np.nonzero(g != w)[0][:5].tolist())
