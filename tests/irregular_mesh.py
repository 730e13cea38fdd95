"""Valid meshes the Fibonacci-sphere builder never makes, for the long-row and reordering tests: high-degree "hub" cells
(rows of 9 .. 24 entries, up to WO_MAX_DEG), relabelled cells and shuffled rows.  Everything is deterministic from a seed.

A hub gains symmetric edges to its nearest cells (chord distance) within 3 hops of the base mesh; each new entry goes in at a
seeded position of both rows.  Hubs are at least 4 hops apart, so a hub's row holds only its own new edges and a cell's row grows
by one entry per hub it is linked to."""
from dataclasses import dataclass
from functools import lru_cache

import numpy as np

HUB_HOPS = 3                                    # a hub links to cells at most this many hops away ...
HUB_SEPARATION = HUB_HOPS + 1                   # ... and hubs are at least this many hops apart
KINDS = ("relief", "polar", "interior", "coastal", "ocean")
THERMAL_CORNER = (0.8, 0.15)                    # talus / kThermal of the UI's thermal slider at 1
GLACIAL_STRENGTH = 0.8
ICE_FLOW_THRESHOLD = 0.1                        # a land cell whose ice flow exceeds this takes a carve turn (js/terrain-post.js:506-526)


@dataclass
class CsrMesh:
    adjOffset: np.ndarray
    adjList: np.ndarray

    @property
    def numRegions(self):
        return self.adjOffset.size - 1


def degrees(mesh):
    return np.diff(mesh.adjOffset)


def _rows(mesh):
    off, adj = mesh.adjOffset, mesh.adjList
    return [adj[off[i]:off[i + 1]].tolist() for i in range(off.size - 1)]


def _csr(rows):
    off = np.zeros(len(rows) + 1, np.int32)
    off[1:] = np.cumsum([len(r) for r in rows])
    adj = np.fromiter((c for r in rows for c in r), np.int32, count=int(off[-1]))
    return CsrMesh(off, adj)


def within_hops(mesh, cell, hops):
    """Cells at most `hops` edges from `cell` (itself included), as a set."""
    off, adj = mesh.adjOffset, mesh.adjList
    seen, frontier = {int(cell)}, [int(cell)]
    for _ in range(hops):
        nxt = []
        for c in frontier:
            for n in adj[off[c]:off[c + 1]].tolist():
                if n not in seen:
                    seen.add(n)
                    nxt.append(n)
        frontier = nxt
    return seen


def add_hubs(mesh, xyz, hubs_and_degrees, seed, cap=None):
    """Raise each hub's degree to the requested value with edges to its nearest cells within HUB_HOPS hops (nearest first, ties by
    index); a cell whose row already holds `cap` entries takes no new edge.  Returns (adjOffset, adjList, neighborDist)."""
    from planet_heightmap_generation_amd import sphere_mesh as S
    p = np.asarray(xyz, np.float64).reshape(-1, 3)
    rows = _rows(mesh)
    rng = np.random.default_rng(seed)
    hubs = [int(h) for h, _ in hubs_and_degrees]
    balls = {h: within_hops(mesh, h, HUB_HOPS) for h in hubs}
    for h in hubs:
        if any(o != h and o in balls[h] for o in hubs):
            raise ValueError(f"hub {h} is within {HUB_HOPS} hops of another hub")
    for h, want in hubs_and_degrees:
        h, want = int(h), int(want)
        if want < len(rows[h]):
            raise ValueError(f"hub {h} already has degree {len(rows[h])} > {want}")
        have = set(rows[h])
        cand = sorted((c for c in balls[h] if c != h and c not in have), key=lambda c: (float(((p[c] - p[h]) ** 2).sum()), c))
        for c in cand:
            if len(rows[h]) == want:
                break
            if cap is not None and len(rows[c]) >= cap:
                continue
            rows[h].insert(int(rng.integers(0, len(rows[h]) + 1)), c)
            rows[c].insert(int(rng.integers(0, len(rows[c]) + 1)), h)
        if len(rows[h]) != want:
            raise ValueError(f"hub {h}: only {len(rows[h])} of {want} neighbours within {HUB_HOPS} hops")
    m = _csr(rows)
    return m.adjOffset, m.adjList, S.compute_neighbor_dist(m, np.asarray(xyz, np.float32))


def carves_every_glacial_step(xyz, oc, strength=GLACIAL_STRENGTH):
    """Land cells whose glacial index clears the carve threshold on latitude alone (js/terrain-post.js:410-433): their ice flow is at
    least that index, so they take a carve turn in every glacial iteration, whatever the elevation does."""
    y = np.clip(np.asarray(xyz, np.float64).reshape(-1, 3)[:, 1], -1, 1)
    t = np.clip((np.abs(np.arcsin(y)) - (np.pi / 2 - strength * np.pi / 4.5)) / (strength * np.pi / 4.5), 0, 1)
    return (np.asarray(oc) == 0) & (t * t * (3 - 2 * t) * strength > 1.5 * ICE_FLOW_THRESHOLD)


def cell_kinds(mesh, e0, changed, xyz):
    """Masks of the cells hubs are drawn from: high-relief land that the oracle's thermal or glacial run changes (`changed`), polar
    land that carves in every glacial step, interior land (no ocean within 2 hops), coastal land (an ocean neighbour) and ocean."""
    off, adj = mesh.adjOffset, mesh.adjList
    N = off.size - 1
    rows = np.repeat(np.arange(N), np.diff(off))
    land = e0 > 0
    relief = np.zeros(N, np.float32)
    np.maximum.at(relief, rows, np.abs(e0[rows] - e0[adj]))
    near = ~land
    for _ in range(2):
        grown = near.copy()
        np.logical_or.at(grown, rows, near[adj])
        near = grown
    coastal = np.zeros(N, bool)
    np.logical_or.at(coastal, rows, ~land[adj])
    high = relief >= np.quantile(relief[land], 0.75) if land.any() else np.zeros(N, bool)
    return dict(relief=land & changed & high, polar=carves_every_glacial_step(xyz, ~land), interior=land & ~near,
                coastal=land & coastal, ocean=~land)


def pick_hubs(mesh, xyz, e0, changed, hub_degrees, seed):
    """One hub per entry of `hub_degrees`, the kinds of cell_kinds taken in turn (shifted by one kind per pass over the list, so that
    every kind gets high degrees), each at least HUB_SEPARATION hops from the others."""
    rng = np.random.default_rng(seed)
    pools = {k: rng.permutation(np.flatnonzero(m)).tolist() for k, m in cell_kinds(mesh, e0, changed, xyz).items()}
    base_deg = degrees(mesh)
    blocked, hubs = set(), []
    for i, d in enumerate(hub_degrees):
        kind = KINDS[(i + i // len(KINDS)) % len(KINDS)]
        pool = pools[kind]
        while pool and (pool[-1] in blocked or base_deg[pool[-1]] > d):
            pool.pop()
        if not pool:
            raise ValueError(f"no {kind} cell left for hub {i}")
        h = pool.pop()
        hubs.append(h)
        blocked |= within_hops(mesh, h, HUB_SEPARATION - 1)
    return np.array(hubs, np.int32)


def spread_degrees(max_degree, at_least=32):
    """Hub degrees 9 .. max_degree, highest first, repeated until there are `at_least` hubs."""
    one = list(range(max_degree, 8, -1))
    reps = max(2, -(-at_least // len(one)))
    return [d for _ in range(reps) for d in one]


@dataclass
class HubPlanet:
    mesh: CsrMesh
    xyz: np.ndarray
    nd: np.ndarray
    e0: np.ndarray              # oracle.synthetic_terrain of the points (the same field as on the base mesh)
    oc: np.ndarray
    hubs: np.ndarray
    hub_degrees: np.ndarray


@lru_cache(maxsize=None)
def hub_mesh(N, seed, max_degree):
    """A build_sphere(N, 0.75, seed) mesh with hubs of degree 9 .. max_degree (at least one at exactly max_degree); no other row is
    raised past max_degree, so the planet's largest degree is max_degree."""
    from oracle import pyoracle as O
    from planet_heightmap_generation_amd import sphere_mesh as S
    base, xyz, nd0 = S.build_sphere(N, 0.75, seed)
    e0 = O.synthetic_terrain(xyz, seed)
    oc = (e0 <= 0).astype(np.uint8)
    om = O.Mesh(base.adjOffset, base.adjList)
    talus, kth = THERMAL_CORNER
    changed = O.erode_composite(om, e0, xyz, oc, 0, 3e-4, 0.5, 1.0, 4, talus, kth, 0, 0.0, nd0) != e0
    changed |= O.erode_composite(om, e0, xyz, oc, 0, 3e-4, 0.5, 1.0, 0, talus, kth, 3, GLACIAL_STRENGTH, nd0) != e0
    hd = spread_degrees(max_degree)
    hubs = pick_hubs(base, xyz, e0, changed, hd, seed)
    off, adj, nd = add_hubs(base, xyz, list(zip(hubs.tolist(), hd)), seed, cap=max_degree)
    mesh = CsrMesh(off, adj)
    assert int(degrees(mesh).max()) == max_degree
    return HubPlanet(mesh, xyz, nd, e0, oc, hubs, np.array(hd, np.int32))


def permute_vertices(mesh, xyz, perm):
    """Relabel the cells: new cell k is old cell perm[k]; rows keep their order.  Returns (mesh, xyz, neighborDist)."""
    from planet_heightmap_generation_amd import sphere_mesh as S
    perm = np.asarray(perm, np.int64)
    inv = np.empty_like(perm)
    inv[perm] = np.arange(perm.size)
    deg = degrees(mesh)[perm]
    off = np.zeros(perm.size + 1, np.int32)
    off[1:] = np.cumsum(deg)
    src = np.arange(int(off[-1])) + np.repeat(mesh.adjOffset[perm] - off[:-1], deg)
    m = CsrMesh(off, inv[mesh.adjList[src]].astype(np.int32))
    p = np.ascontiguousarray(np.asarray(xyz, np.float32).reshape(-1, 3)[perm].reshape(-1))
    return m, p, S.compute_neighbor_dist(m, p)


def shuffle_rows(mesh, seed):
    """The same graph with the entries of every row in a seeded random order (compute neighborDist again for it)."""
    rng = np.random.default_rng(seed)
    off = mesh.adjOffset
    key = rng.random(mesh.adjList.size) + np.repeat(np.arange(off.size - 1), np.diff(off))
    return CsrMesh(off.copy(), mesh.adjList[np.argsort(key, kind="stable")].astype(np.int32))
