"""The kernel bodies of csrc/erode_ops.h, driven thread-by-thread on the CPU by the test-only emulator
(tests/emu), against the reference's golden vectors.  This checks the parallel re-formulations (dataflow
solve, pointer-doubling flow, rank-replayed thermal, 2-hop-ordered glacial carve) bit for bit without a GPU;
the -m gpu tests check the same bodies as launched on gfx950."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

from conftest import POST_TAGS, REPO, golden_cases, load_golden

EMU_DIR = REPO / "tests" / "emu"


@pytest.fixture(scope="module")
def emu():
    subprocess.run(["make", "-s", "-C", str(EMU_DIR)], check=True)
    L = C.CDLL(str(EMU_DIR / "_build" / "libemu.so"))
    p, i32, f64 = C.c_void_p, C.c_int32, C.c_double
    L.emu_erode_composite.argtypes = [i32, p, p, p, p, p, i32, f64, f64, f64, i32, f64, f64, i32, f64, p, p]
    L.emu_jacobi.argtypes = [i32, i32, p, p, p, p, i32, f64]
    L.emu_warp.argtypes = [i32, p, p, p, p, f64, f64, p]
    L.emu_flood.argtypes = [i32, p, p, p, p, f64]
    return L


def P(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


@pytest.mark.parametrize("tag", POST_TAGS)
def test_emulated_bodies_bit_exact(emu, tag):
    g = load_golden(f"post_{tag}")
    off, adj, e0, oc, xyz, nd = (g[k] for k in ("adjOffset", "adjList", "elevation0", "isOcean", "xyz", "neighborDist"))
    N = off.size - 1
    for name, c in golden_cases(g).items():
        a, fn, e = c["args"], c["fn"], e0.copy()
        if fn == "warpTerrain":
            emu.emu_warp(N, P(off), P(adj), P(e), P(xyz), a["seed"], a["strength"], P(g["hotspot"]) if "hot" in name else None)
        elif fn in ("smoothElevation", "sharpenRidges", "applySoilCreep"):
            kind = {"smoothElevation": 0, "sharpenRidges": 1, "applySoilCreep": 2}[fn]
            emu.emu_jacobi(kind, N, P(off), P(adj), P(e), P(oc), a["iterations"], a["strength"])
        elif fn == "priorityFloodCarve":
            emu.emu_flood(N, P(off), P(adj), P(e), P(oc), a["carveStrength"])
        else:
            stats = np.zeros(8)
            rc = emu.emu_erode_composite(N, P(off), P(adj), P(e), P(xyz), P(oc), a["hIters"], a["K"], a["m"], a["dt"], a["tIters"],
                                         a["talusSlope"], a["kThermal"], a["gIters"], a["glacialStrength"], P(nd), P(stats))
            assert rc == 0
        assert np.array_equal(e, g["ref_" + name]), f"{tag}/{name}: {(e != g['ref_' + name]).sum()} cells differ"


def test_emulated_ties_and_flats(emu, oracle):
    from planet_heightmap_generation_amd import sphere_mesh as S
    mesh, xyz, nd = S.build_sphere(20000, 0.75, 4)
    e0 = oracle.synthetic_terrain(xyz, 4)
    eq = (np.round(e0 * 64) / 64).astype(np.float32)        # thousands of exact ties, flats, pits
    oc = (eq <= 0).astype(np.uint8)
    om = oracle.Mesh(mesh.adjOffset, mesh.adjList)
    for (h, t, g_) in ((12, 12, 0), (6, 6, 6)):
        ref = oracle.erode_composite(om, eq, xyz, oc, h, 3e-4, 0.5, 1.0, t, 1.16, 0.015, g_, 0.8, nd)
        e = eq.copy()
        stats = np.zeros(8)
        rc = emu.emu_erode_composite(mesh.numRegions, P(mesh.adjOffset), P(mesh.adjList), P(e), P(xyz), P(oc), h, 3e-4, 0.5, 1.0, t,
                                     1.16, 0.015, g_, 0.8, P(nd), P(stats))
        assert rc == 0 and np.array_equal(e, ref), (h, t, g_, int((e != ref).sum()))


@pytest.mark.parametrize("land", [12000, 15000])
def test_flood_and_erosion_of_land_below_sea_level(emu, oracle, land):
    """A mask that is not `elevation <= 0`: land is the `land` highest of 20 001 cells, thousands of them below 0.  The carve's clamp
    at 0 (js/terrain-post.js:189) then LIFTS a height, above its flood surface; the chain form of pass 2 (flood_host.cc:
    tree_pass2_chains) ends its peak search on the strength of "no height exceeds its surface" and must leave such trees to the plain
    form.  Both pass-1 routes of the host flood and the whole emulated erodeComposite against the oracle (which equals the reference
    under Node on this planet), bit for bit."""
    from planet_heightmap_generation_amd import sphere_mesh as S
    mesh, xyz, nd = S.build_sphere(20000, 0.75, 4)
    eq = (np.round(oracle.synthetic_terrain(xyz, 4) * 64) / 64).astype(np.float32)
    oc = np.ones(eq.size, np.uint8)
    oc[np.argsort(-eq, kind="stable")[:land]] = 0
    assert int(((oc == 0) & (eq < 0)).sum()) > 5000
    om = oracle.Mesh(mesh.adjOffset, mesh.adjList)
    emu.emu_flood_host.argtypes = [C.c_int32] + [C.c_void_p] * 5 + [C.c_double, C.c_int32, C.c_int32, C.c_void_p]
    ref = oracle.priority_flood_carve(om, eq, oc, 0.5)
    assert (ref[oc == 0] != eq[oc == 0]).sum() > 1000
    for mode in (0, 1):
        e, stats = eq.copy(), np.zeros(11)
        emu.emu_flood_host(mesh.numRegions, P(mesh.adjOffset), P(mesh.adjList), P(xyz), P(e), P(oc), 0.5, mode, 1, P(stats))
        assert np.array_equal(e, ref), (mode, int((e != ref).sum()))
    for h, t in ((1, 0), (0, 3), (3, 3)):                      # the mid-loop flood runs without hydraulic iterations too
        ref = oracle.erode_composite(om, eq, xyz, oc, h, 3e-4, 0.5, 1.0, t, 1.16, 0.015, 0, 0.0, nd)
        e, stats = eq.copy(), np.zeros(8)
        rc = emu.emu_erode_composite(mesh.numRegions, P(mesh.adjOffset), P(mesh.adjList), P(e), P(xyz), P(oc), h, 3e-4, 0.5, 1.0, t, 1.16, 0.015, 0, 0.0, P(nd), P(stats))
        assert rc == 0 and np.array_equal(e, ref), (h, t, int((e != ref).sum()))


def test_flood_open_ocean_choice(emu, oracle):
    """The flood seeds only from the largest ocean component, the first one in cell order winning ties
    (js/terrain-post.js:66-94).  Masks with two equal oceans, with inland seas and with one ocean cell."""
    from planet_heightmap_generation_amd import sphere_mesh as S
    mesh, xyz, nd = S.build_sphere(6000, 0.75, 9)
    N = mesh.numRegions
    om = oracle.Mesh(mesh.adjOffset, mesh.adjList)
    base = oracle.synthetic_terrain(xyz, 9)
    land = np.abs(base).astype(np.float32) + np.float32(0.01)
    masks = []
    # two polar caps: mirror images need not be equal in cell count, so shave the larger one down to a tie
    y = xyz.reshape(-1, 3)[:, 1]
    cap_n = np.flatnonzero(y > 0.8)
    cap_s = np.flatnonzero(y < -0.8)
    k = min(cap_n.size, cap_s.size)
    order_n = cap_n[np.argsort(-y[cap_n], kind="stable")][:k]
    order_s = cap_s[np.argsort(y[cap_s], kind="stable")][:k]
    m = np.zeros(N, np.uint8); m[order_n] = 1; m[order_s] = 1
    masks.append(m)
    # a big ocean plus inland seas that touch land the main ocean never reaches
    m = (base <= -0.05).astype(np.uint8)
    masks.append(m)
    # a single ocean cell; and an ocean made of isolated single cells (all components tie at size 1)
    m = np.zeros(N, np.uint8); m[1234] = 1
    masks.append(m)
    m = np.zeros(N, np.uint8); m[[17, 2500, 5800]] = 1
    masks.append(m)
    for i, oc in enumerate(masks):
        e0 = np.where(oc == 1, np.float32(-0.2), land).astype(np.float32)
        ref = oracle.priority_flood_carve(om, e0, oc, 0.5)
        e = e0.copy()
        emu.emu_flood(N, P(mesh.adjOffset), P(mesh.adjList), P(e), P(oc), 0.5)
        assert np.array_equal(e, ref), (i, int((e != ref).sum()))


def test_solve_event_lists_equal_row_scans(emu, oracle, monkeypatch):
    """solve_setup / solve_final from the per-location event lists (flow_final_cell) and from the neighbour-row scans
    (WO_NO_EVENT_LISTS) are the same dataflow: both equal the oracle, on terrain with flats and cells that have more
    donors than a list holds."""
    from planet_heightmap_generation_amd import sphere_mesh as S
    mesh, xyz, nd = S.build_sphere(30000, 0.75, 9)
    e0 = oracle.synthetic_terrain(xyz, 9)
    eq = (np.round(e0 * 256) / 256).astype(np.float32)
    oc = (eq <= 0).astype(np.uint8)
    om = oracle.Mesh(mesh.adjOffset, mesh.adjList)
    ref = oracle.erode_composite(om, eq, xyz, oc, 9, 3e-4, 0.5, 1.0, 9, 1.16, 0.015, 0, 0.8, nd)
    for off in (False, True):
        if off:
            monkeypatch.setenv("WO_NO_EVENT_LISTS", "1")
        e = eq.copy()
        stats = np.zeros(8)
        rc = emu.emu_erode_composite(mesh.numRegions, P(mesh.adjOffset), P(mesh.adjList), P(e), P(xyz), P(oc), 9, 3e-4, 0.5, 1.0, 9,
                                     1.16, 0.015, 0, 0.8, P(nd), P(stats))
        assert rc == 0 and np.array_equal(e, ref), (off, int((e != ref).sum()))


def test_the_branch_free_solve_turn_equals_the_plain_one(emu):
    """erode_ops.h: solve_apply_flat (what a wave of the basin solve runs for whichever lanes are ready: every expression
    evaluated, the conditions select) against solve_apply (the serial loop's turn) on two million random tasks over all flag
    combinations and the awkward operands: not one output bit may differ."""
    import ctypes as C
    L = emu
    L.emu_solve_turn_forms_differ.restype = C.c_int64
    L.emu_solve_turn_forms_differ.argtypes = [C.c_int64, C.c_uint64]
    for seed in (1, 2, 3, 4):
        assert L.emu_solve_turn_forms_differ(500000, seed) == 0
