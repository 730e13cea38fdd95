"""Graphs and fields that put the rivers stage (csrc/rivers.hip, contract in csrc/rivers_ops.h) where its scheduling binds, none of which
a Fibonacci sphere with a smooth or white-noise field reaches: receiver chains as long as the graph (the launch count of the pointer
jumping, the single thread of the discharge climb), chains of hooks as long as the pit list (the relabel walk), mutual first choices,
log2 P contraction rounds, 23 donors that arrive at one cell together, rows of 24 entries, empty rows, relabelled cells and shuffled
rows, discharges of 2^32 and more.  Plain numpy, deterministic from a seed; the planet takes any simple symmetric CSR graph up to
degree 24, and the lines take any unit vectors for r_xyz.

shape(name) -> Graph, kept; reference(name, runoff) -> the oracle's result on it, kept and not to be written to; emulated(name,
runoff) -> the emulator's.  SHAPES lists the names with the runoffs each is run under, CPU and device alike."""
from __future__ import annotations

import functools
from dataclasses import dataclass

import numpy as np

import irregular_mesh as IM
import rivers_common as RV

SEED = 3
SAW_KINDS = ("asc", "desc", "random", "ruler", "pairs")
MAX_RUNOFF = 16.0                                             # the clamp of step 7: 2^20 per land cell


@dataclass(frozen=True, eq=False)
class Graph:
    off: np.ndarray
    adj: np.ndarray
    e: np.ndarray
    xyz: np.ndarray                                           # float32 [n, 3], unit vectors

    @property
    def n(self):
        return self.off.size - 1

    @property
    def mesh(self):
        return IM.CsrMesh(self.off, self.adj)


def unit_vectors(n, seed=SEED):
    v = np.random.default_rng(seed + 1000).normal(size=(n, 3))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


def path_csr(n):
    """cells 0 .. n - 1 in a row, each row in ascending order"""
    deg = np.full(n, 2, np.int32)
    deg[0] = deg[-1] = 1
    off = np.zeros(n + 1, np.int32)
    off[1:] = np.cumsum(deg)
    i = np.arange(1, n - 1, dtype=np.int32)
    adj = np.concatenate([[1], np.stack([i - 1, i + 1], axis=1).reshape(-1), [n - 2]]).astype(np.int32)
    return off, adj


def ramp(n, reversed=False):
    """A path with the ocean cell (e = -1) at one end and land of e = i / 1024 (exact in f32) rising away from it: one receiver chain
    over all n - 1 land cells, n - 2 hops on land and one into the ocean, no pit.  reversed: the ocean is the last cell, so the chain
    runs with the index instead of against it."""
    off, adj = path_csr(n)
    e = (np.arange(n, dtype=np.float64) / 1024.0).astype(np.float32)
    e[0] = -1.0
    if reversed:
        e = e[::-1].copy()
    return Graph(off, adj, e, unit_vectors(n))


def saw_ranks(P, kind, seed=SEED):
    """rank[k - 1] of pass k = 1 .. P among the pass levels, a permutation of 0 .. P - 1"""
    k = np.arange(1, P + 1, dtype=np.int64)
    if kind == "asc":
        key = k
    elif kind == "desc":
        key = -k
    elif kind == "random":
        key = np.random.default_rng(seed + 1).permutation(P)
    elif kind == "ruler":
        key = (k & -k) * P + k
    elif kind == "pairs":                                     # every odd pass below every even one, ascending within both
        key = np.where(k % 2 == 1, k, 2 * P + k)
    else:
        raise KeyError(kind)
    rank = np.empty(P, np.int64)
    rank[np.argsort(key, kind="stable")] = np.arange(P)
    return rank


def sawtooth(P, kind, seed=SEED):
    """A path of 2 P + 1 cells: the ocean cell 0, then pass cell k = 1 .. P at 2 k - 1 and pit cell k at 2 k.  P distinct pass levels in
    (1, 2] and pit floors in [0.5, 0.75), all multiples of 2^-23, from the seed; the kind orders the pass levels along the path.
    The basin graph is the path drained - B1 - .. - BP whose edge k has the level of pass k, so every basin spills and:
    asc: every basin's lowest pass is the one towards the ocean, one round, one chain of P hooks;  desc: every basin chooses the pass
    away from the ocean, the last two choose each other, the second round takes pass 1;  pairs: B(2j) and B(2j + 1) choose each
    other;  ruler: the lowest pass of a merged run is always at its end, about log2 P rounds;  random."""
    rng = np.random.default_rng(seed)
    levels = 1.0 + (np.sort(rng.choice(1 << 23, P, replace=False)) + 1) / float(1 << 23)
    floors = 0.5 + rng.integers(0, 1 << 21, P) / float(1 << 23)
    n = 2 * P + 1
    off, adj = path_csr(n)
    e = np.empty(n, np.float64)
    e[0] = -1.0
    e[1::2] = levels[saw_ranks(P, kind, seed)]
    e[2::2] = floors
    e32 = e.astype(np.float32)
    assert np.array_equal(e32.astype(np.float64), e)
    return Graph(off, adj, e32, unit_vectors(n))


def tree(k, depth):
    """The ocean cell 0, the land cell 1 on it, and below cell 1 a complete k-ary tree of `depth` levels numbered level by level;
    every child lies 0.01 above its parent.  Every interior cell has k donors whose chains are equally long, and a row of k + 1."""
    starts = [1]
    for level in range(depth + 1):
        starts.append(starts[-1] + k ** level)
    n = starts[-1]
    parent = np.zeros(n, np.int64)
    level_of = np.zeros(n, np.int64)
    for level in range(1, depth + 1):
        ids = np.arange(starts[level], starts[level + 1])
        parent[ids] = starts[level - 1] + (ids - starts[level]) // k
        level_of[ids] = level
    rows = [[] for _ in range(n)]
    rows[0].append(1)
    for c in range(1, n):                                     # the parent first, then the children in ascending order
        rows[c].insert(0, int(parent[c]))
        if c > 1:
            rows[int(parent[c])].append(c)
    m = IM._csr(rows)
    e = (0.01 * (level_of + 1)).astype(np.float32)
    e[0] = -1.0
    return Graph(m.adjOffset, m.adjList, e, unit_vectors(n))


def isolated(n=600):
    """A land cell with an empty row (a pit without a pass: endorheic) as cell 0, a ramp of n cells, an ocean cell with an empty row"""
    r = ramp(n)
    off = np.concatenate([[0], r.off, [r.off[-1]]]).astype(np.int32)
    adj = (r.adj + 1).astype(np.int32)
    e = np.concatenate([[0.5], r.e, [-0.5]]).astype(np.float32)
    return Graph(off, adj, e, unit_vectors(n + 2))


HUB_ARGS = (20000, 3, 24)


@functools.lru_cache(maxsize=None)
def hub(form):
    """-> (mesh, xyz [n, 3], e0) of irregular_mesh.hub_mesh(20000, 3, 24): as built, with the cells relabelled, with every row shuffled"""
    hp = IM.hub_mesh(*HUB_ARGS)
    xyz = np.ascontiguousarray(hp.xyz, np.float32).reshape(-1, 3)
    if form == "built":
        return hp.mesh, xyz, hp.e0
    if form == "permuted":
        perm = np.random.default_rng(SEED + 2).permutation(hp.mesh.numRegions)
        m, p, _ = IM.permute_vertices(hp.mesh, hp.xyz, perm)
        return m, np.ascontiguousarray(p, np.float32).reshape(-1, 3), np.ascontiguousarray(hp.e0[perm])
    if form == "shuffled":
        return IM.shuffle_rows(hp.mesh, SEED + 3), xyz, hp.e0
    raise KeyError(form)


def hub_graph(form, fieldKind):
    m, xyz, e0 = hub(form)
    e = e0 if fieldKind == "e0" else RV.field("bowl", xyz)
    return Graph(np.ascontiguousarray(m.adjOffset, np.int32), np.ascontiguousarray(m.adjList, np.int32), np.ascontiguousarray(e, np.float32), xyz)


# name -> (builder, the runoffs it is run under)
SHAPES = {}
for _n in (4096, 4097, 4098, 8193, 32769):
    for _rev in (False, True):
        SHAPES[f"ramp-{_n}{'-reversed' if _rev else ''}"] =(functools.partial(ramp, _n, _rev), ("max", "uniform") if _n == 32769 else ("max",))
for _kind in SAW_KINDS:
    SHAPES[f"saw-{_kind}-4096"] = (functools.partial(sawtooth, 4096, _kind), ("max",))
for _kind in ("asc", "ruler"):
    SHAPES[f"saw-{_kind}-16384"] = (functools.partial(sawtooth, 16384, _kind), ("max",))
SHAPES["tree-23-3"] = (functools.partial(tree, 23, 3), ("max", "values"))
SHAPES["isolated"] = (isolated, ("max",))
for _form in ("built", "permuted", "shuffled"):
    for _field in ("e0", "bowl"):
        SHAPES[f"hub-{_form}-{_field}"] = (functools.partial(hub_graph, _form, _field), ("uniform", "values"))
# the emulator follows every cell's chain to its end: seconds on the longest ramps, which are left to the oracle
EMULATED = tuple(k for k in SHAPES if not k.startswith("ramp-32769"))
CASES = tuple((name, runoff) for name, (_, runoffs) in SHAPES.items() for runoff in runoffs)


@functools.lru_cache(maxsize=None)
def shape(name):
    return SHAPES[name][0]()


def runoff_values(G, runoff):
    """float32 per cell: "max" 16 everywhere (the clamp), "uniform" 1, "values" rivers_common's field with negatives, NaNs and values
    above the clamp"""
    if runoff == "max":
        return np.full(G.n, MAX_RUNOFF, np.float32)
    if runoff == "uniform":
        return np.ones(G.n, np.float32)
    return RV.runoff_fields(G.xyz)[2]


@functools.lru_cache(maxsize=None)
def _structure(name):
    G = shape(name)
    return RV.oracle_structure_graph(G.off, G.adj, G.e)


@functools.lru_cache(maxsize=None)
def reference(name, runoff):
    return RV.oracle_discharge(_structure(name), runoff_values(shape(name), runoff))


@functools.lru_cache(maxsize=None)
def emulated(name, runoff):
    G = shape(name)
    return RV.emu_compute(G.off, G.adj, G.e, 1) if runoff == "uniform" else RV.emu_compute(G.off, G.adj, G.e, 2, runoff_values(G, runoff))


def thresholds_of(flows):
    """flows: of the segments at min_flow 0 -> (min_flow 0 and one threshold that keeps some of the segments and drops others, whether
    there is such a threshold).  The threshold is the median flow, or where that is the lowest flow (it would keep them all) the second
    lowest; segments of one flow only have none and get a threshold that drops them all.  The callers count what each keeps."""
    u = np.unique(flows)
    if u.size < 2:
        return (0.0, 2.0 * float(u[0]) if u.size else 1.0), False
    m = float(np.median(flows))
    return (0.0, m if m > float(u[0]) else float(u[1])), True


def thresholds(O):
    return thresholds_of(O["r_river_flow"][RV.oracle_river_cells(O, 0.0)])[0]


def splits(O):
    return thresholds_of(O["r_river_flow"][RV.oracle_river_cells(O, 0.0)])[1]


def check_kept(tag, kept, split):
    """kept: the segment counts under the two thresholds"""
    assert kept[0] > 0 and (0 < kept[1] < kept[0] if split else kept[1] == 0), (tag, kept)


def max_degree(G):
    return int(np.diff(G.off).max())
