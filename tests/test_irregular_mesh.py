"""The irregular-mesh helper (tests/irregular_mesh.py) checks itself, and the kernel bodies of csrc/erode_ops.h, driven by the CPU
emulator (tests/emu), equal the oracle bit for bit on hub meshes whose rows reach WO_MAX_DEG = 24 entries: every row longer than
WO_ROW and WO_EAGER_ROW takes the plain-loop forms there.  The -m gpu tests (test_gpu_irregular_mesh.py) run the same meshes on gfx950."""
import numpy as np
import pytest

import irregular_mesh as IM
from test_emulated_kernels import P, emu  # noqa: F401  (the emulator fixture)


@pytest.fixture(scope="module")
def base():
    from planet_heightmap_generation_amd import sphere_mesh as S
    return S.build_sphere(20000, 0.75, 4)


def _pairs(mesh):
    rows = np.repeat(np.arange(mesh.numRegions), IM.degrees(mesh))
    return rows, mesh.adjList


def test_hub_helper_invariants(base):
    mesh, xyz, _ = base
    e0 = np.asarray(xyz, np.float32).reshape(-1, 3)[:, 1].copy() - np.float32(0.2)     # any field with land and ocean
    hd = IM.spread_degrees(24)
    hubs = IM.pick_hubs(mesh, xyz, e0, np.ones(mesh.numRegions, bool), hd, 7)
    want = list(zip(hubs.tolist(), hd))
    off, adj, nd = IM.add_hubs(mesh, xyz, want, 7, cap=24)
    m = IM.CsrMesh(off, adj)
    deg = IM.degrees(m)
    # degrees exactly as requested, the largest one present, nothing past the cap
    assert [int(deg[h]) for h in hubs] == hd and deg.max() == 24 and (deg[hubs] == 24).any()
    # hubs at least HUB_SEPARATION hops apart on the base mesh
    for h in hubs.tolist():
        assert not (IM.within_hops(mesh, h, IM.HUB_SEPARATION - 1) & (set(hubs.tolist()) - {h}))
    # symmetric, no repeated entries, no self loops
    r, c = _pairs(m)
    assert not (r == c).any()
    key = r.astype(np.int64) * m.numRegions + c
    assert np.unique(key).size == key.size
    assert np.array_equal(np.sort(key), np.sort(c.astype(np.int64) * m.numRegions + r))
    # the old graph is a subgraph; every new edge touches a hub and stays within HUB_HOPS hops of it
    r0, c0 = _pairs(mesh)
    old = set((r0.astype(np.int64) * m.numRegions + c0).tolist())
    new = [(int(a), int(b)) for a, b in zip(r, c) if int(a) * m.numRegions + int(b) not in old]
    assert old <= set(key.tolist())
    hubset = set(hubs.tolist())
    assert new and all((a in hubset) != (b in hubset) for a, b in new)
    assert all(b in IM.within_hops(mesh, a, IM.HUB_HOPS) for a, b in new if a in hubset)
    # rows without a new entry keep their order; rows with new entries hold the old ones in their old order
    touched = {a for a, _ in new}
    moved = 0
    for v in range(m.numRegions):
        row, row0 = adj[off[v]:off[v + 1]].tolist(), mesh.adjList[mesh.adjOffset[v]:mesh.adjOffset[v + 1]].tolist()
        if v not in touched:
            assert row == row0, v
        else:
            assert [x for x in row if x in set(row0)] == row0, v
            moved += row[:len(row0)] != row0          # new entries are not all appended
    assert moved > 0
    # neighborDist slot-aligned with the new list
    from planet_heightmap_generation_amd import sphere_mesh as S
    assert np.array_equal(nd, S.compute_neighbor_dist(m, xyz))
    # deterministic from the seed
    again = IM.add_hubs(mesh, xyz, want, 7, cap=24)
    assert all(np.array_equal(a, b) for a, b in zip((off, adj, nd), again))
    assert np.array_equal(hubs, IM.pick_hubs(mesh, xyz, e0, np.ones(mesh.numRegions, bool), hd, 7))
    other = IM.add_hubs(mesh, xyz, want, 8, cap=24)
    assert np.array_equal(other[0], off) and not np.array_equal(other[1], adj)      # same graph, other insertion points


def test_hub_mesh_degrees_and_determinism(oracle):
    hp = IM.hub_mesh(20000, 4, 24)
    deg = IM.degrees(hp.mesh)
    assert deg.max() == 24 and np.array_equal(deg[hp.hubs], hp.hub_degrees)
    assert set(hp.hub_degrees.tolist()) == set(range(9, 25))
    land = hp.e0 > 0
    assert land[hp.hubs].any() and (~land[hp.hubs]).any()
    again = IM.hub_mesh.__wrapped__(20000, 4, 24)
    assert np.array_equal(again.mesh.adjList, hp.mesh.adjList) and np.array_equal(again.hubs, hp.hubs)


def test_permute_and_shuffle(base):
    mesh, xyz, nd = base
    V = mesh.numRegions
    perm = np.random.default_rng(3).permutation(V)
    m, p, d = IM.permute_vertices(mesh, xyz, perm)
    inv = np.argsort(perm)
    for k in (0, 1, V // 2, V - 1, int(inv[V - 1])):
        old = perm[k]
        assert m.adjList[m.adjOffset[k]:m.adjOffset[k + 1]].tolist() == inv[mesh.adjList[mesh.adjOffset[old]:mesh.adjOffset[old + 1]]].tolist()
    assert np.array_equal(p.reshape(-1, 3), np.asarray(xyz).reshape(-1, 3)[perm])
    # distances follow their edges
    src = np.arange(m.adjList.size) + np.repeat(mesh.adjOffset[perm] - m.adjOffset[:-1], IM.degrees(m))
    assert np.array_equal(d, nd[src])
    s = IM.shuffle_rows(m, 5)
    assert np.array_equal(s.adjOffset, m.adjOffset) and not np.array_equal(s.adjList, m.adjList)
    for k in range(0, V, 997):
        a, b = s.adjList[s.adjOffset[k]:s.adjOffset[k + 1]], m.adjList[m.adjOffset[k]:m.adjOffset[k + 1]]
        assert sorted(a.tolist()) == sorted(b.tolist())
    assert np.array_equal(IM.shuffle_rows(m, 5).adjList, s.adjList)


EMU_ERODE = {"h": (12, 0, 0, 1.16, 0.015), "t_default": (0, 12, 0, 1.16, 0.015), "t_corner": (0, 12, 0, 0.8, 0.15),
             "g": (0, 0, 6, 1.16, 0.015), "hgt": (6, 6, 6, 1.16, 0.015)}


@pytest.fixture(scope="module")
def hub20k(oracle):
    return IM.hub_mesh(20000, 4, 24)


@pytest.mark.parametrize("case", list(EMU_ERODE))
def test_emulated_erode_on_hub_mesh(emu, oracle, hub20k, case):  # noqa: F811
    hp = hub20k
    h, t, g_, talus, kth = EMU_ERODE[case]
    m, V = hp.mesh, hp.mesh.numRegions
    om = oracle.Mesh(m.adjOffset, m.adjList)
    ref = oracle.erode_composite(om, hp.e0, hp.xyz, hp.oc, h, 3e-4, 0.5, 1.0, t, talus, kth, g_, IM.GLACIAL_STRENGTH, hp.nd)
    long_rows = IM.degrees(m) > 12
    assert (ref != hp.e0)[long_rows].any(), "no row longer than WO_EAGER_ROW changes: the case proves nothing"
    e = hp.e0.copy()
    stats = np.zeros(8)
    rc = emu.emu_erode_composite(V, P(m.adjOffset), P(m.adjList), P(e), P(hp.xyz), P(hp.oc), h, 3e-4, 0.5, 1.0, t, talus, kth, g_,
                                 IM.GLACIAL_STRENGTH, P(hp.nd), P(stats))
    assert rc == 0 and np.array_equal(e, ref), (case, int((e != ref).sum()))


def test_emulated_jacobi_flood_warp_on_hub_mesh(emu, oracle, hub20k):  # noqa: F811
    hp = hub20k
    m, V = hp.mesh, hp.mesh.numRegions
    om = oracle.Mesh(m.adjOffset, m.adjList)
    for kind, fn, args in ((0, oracle.smooth_elevation, (2, 0.3)), (1, oracle.sharpen_ridges, (3, 0.04)), (2, oracle.soil_creep, (3, 0.1125))):
        ref = fn(om, hp.e0, hp.oc, *args)
        e = hp.e0.copy()
        emu.emu_jacobi(kind, V, P(m.adjOffset), P(m.adjList), P(e), P(hp.oc), *args)
        assert np.array_equal(e, ref), (kind, int((e != ref).sum()))
    ref = oracle.priority_flood_carve(om, hp.e0, hp.oc, 0.5)
    e = hp.e0.copy()
    emu.emu_flood(V, P(m.adjOffset), P(m.adjList), P(e), P(hp.oc), 0.5)
    assert np.array_equal(e, ref), int((e != ref).sum())
    ref = oracle.warp_terrain(om, hp.e0, hp.xyz, 4, 0.75)
    e = hp.e0.copy()
    emu.emu_warp(V, P(m.adjOffset), P(m.adjList), P(e), P(hp.xyz), 4, 0.75, None)
    assert np.array_equal(e, ref), int((e != ref).sum())
