"""Rivers and lakes on the host: the emulator of csrc/rivers_ops.h (tests/emu_rivers: the bodies and the tree walk the device stage
runs, under serial Boruvka rounds) against the independent serial oracle of tests/rivers_common.py (a literal Prim over the pass
keys) in every bit of all five fields, on three meshes, six fields and the three runoff sources; and the properties of the result
that need neither: the final receivers are a forest, the lakes are exactly the cells below their basin's level, the discharge is
conserved, the lines are ordered and honour the threshold.  Then the same equality on the explicit graphs of tests/rivers_graphs.py
(ramps, sawtooth paths, the 23-ary tree, empty rows, the hub meshes), and the properties each of those graphs is there for."""
import numpy as np
import pytest

import rivers_common as RV
import rivers_graphs as RG


@pytest.mark.parametrize("kind", RV.FIELD_KINDS)
@pytest.mark.parametrize("which", RV.MESHES)
def test_emulator_equals_oracle(which, kind):
    _, xyz, off, adj = RV.mesh(which)
    e = RV.field(kind, xyz)
    for source in RV.SOURCES:
        got = RV.emu_by_source(off, adj, e, source, xyz)
        want = RV.oracle(which, kind, RV.runoff_of(source, xyz))
        RV.assert_fields_equal((which, kind, source), got, want)
        I = got["info"]
        assert (I["pits"], I["spilled"], I["endorheic"], I["drowned"]) == (want["pits"], want["spilled"], want["endorheic"], want["drowned"]), (which, kind, I)
        assert I["landCells"] == int(want["land"].sum()) and I["lakeCells"] == int((~np.isnan(want["r_lake_level"])).sum())
        for min_flow in (0.0, 2.5, 1e9):
            seg, flows = RV.emu_lines(xyz, e, got, min_flow)
            wseg, wflows = RV.oracle_lines(want, xyz, min_flow)
            assert np.array_equal(RV.bits(seg), RV.bits(wseg)) and np.array_equal(RV.bits(flows), RV.bits(wflows)), (which, kind, source, min_flow)
            assert np.array_equal(RV.emu_tinted(e, got, min_flow), RV.oracle_tinted(want, min_flow))


@pytest.mark.parametrize("which", RV.MESHES)
def test_the_bowl_needs_three_rounds_and_drowns_a_basin(which):
    """what field (b) is for: contraction rounds beyond the first two, and a basin whose water level is its parent's"""
    _, xyz, off, adj = RV.mesh(which)
    I = RV.emu_compute(off, adj, RV.field("bowl", xyz), 1)["info"]
    print(which, I)
    assert I["rounds"] >= 3 and I["drowned"] >= 1 and I["spilled"] >= 8, I


@pytest.mark.parametrize("which", RV.MESHES)
def test_special_fields(which):
    _, xyz, off, adj = RV.mesh(which)
    n = xyz.shape[0]
    # (c) the plateau: every cell but one is land, all of it reaches the one ocean cell, which holds the whole discharge
    R = RV.emu_compute(off, adj, RV.field("plateau", xyz), 1)
    assert R["info"]["landCells"] == n - 1 and R["info"]["endorheic"] == 0
    assert int(R["r_river_discharge"][n // 3]) == (n - 1) << 16
    # (d) all land: nothing drains, nothing spills, no lake
    R = RV.emu_compute(off, adj, RV.field("allLand", xyz), 1)
    assert R["info"]["spilled"] == 0 and R["info"]["endorheic"] == R["info"]["pits"] >= 1 and R["info"]["lakeCells"] == 0 and R["info"]["rounds"] >= 1
    assert (R["r_river_basin"] >= 0).all()
    # (e) all ocean: every array holds its "nothing" value and there is no segment
    e = RV.field("allOcean", xyz)
    R = RV.emu_compute(off, adj, e, 1)
    assert (R["r_river_receiver"] == -1).all() and (R["r_river_basin"] == -2).all() and (RV.bits(R["r_lake_level"]) == RV.QUIET_NAN).all()
    assert (R["r_river_discharge"] == 0).all() and (RV.bits(R["r_river_flow"]) == 0).all()
    assert RV.emu_lines(xyz, e, R, 0.0)[0].shape[0] == 0 and not RV.emu_tinted(e, R, 0.0).any()
    # (f) the cone has no pit; with uniform runoff the discharge counts the cells upstream: a plain accumulation from the top down
    e = RV.field("cone", xyz)
    R = RV.emu_compute(off, adj, e, 1)
    assert R["info"]["pits"] == 0 and R["info"]["rounds"] == 0
    size = (e > 0).astype(np.int64)
    recv = R["r_river_receiver"]
    for r in np.argsort(-e, kind="stable"):
        if recv[r] >= 0:
            size[recv[r]] += size[r]
    assert np.array_equal(R["r_river_discharge"], (size << 16).astype(np.uint64))
    assert np.array_equal(R["r_river_flow"], size.astype(np.float32))


@pytest.mark.parametrize("kind", ["noise", "bowl", "plateau", "allLand"])
@pytest.mark.parametrize("which", RV.MESHES)
def test_properties(which, kind):
    _, xyz, off, adj = RV.mesh(which)
    e = RV.field(kind, xyz)
    n = e.size
    s, w, v = RV.runoff_fields(xyz)
    R = RV.emu_compute(off, adj, e, 2, v)
    recv, basin, lake, D = R["r_river_receiver"], R["r_river_basin"], R["r_lake_level"], R["r_river_discharge"]
    land = e > 0
    # every chain of final receivers ends within n steps
    x = np.arange(n)
    for _ in range(n):
        nxt = np.where(recv[x] >= 0, recv[x], x)
        if np.array_equal(nxt, x):
            break
        x = nxt
    assert (recv[x] < 0).all()
    assert (recv[~land] == -1).all() and (basin[~land] == -2).all() and (basin[land] >= -1).all()
    # lakes: inside spilled basins, one level per basin, exactly the cells below it
    has = ~np.isnan(lake)
    assert (basin[has] >= 0).all()
    for b in np.unique(basin[basin >= 0]):
        cells = np.nonzero(basin == b)[0]
        levels = np.unique(RV.bits(lake[cells][has[cells]]))
        if recv[b] < 0:
            assert levels.size == 0, "an endorheic basin has no lake"
            continue
        assert levels.size <= 1
        if levels.size:
            W = levels.view(np.float32)[0]
            assert np.array_equal(has[cells], e[cells] < W)
    # what falls on the land arrives at the roots
    q = np.array(RV.quantise(v), dtype=object) * land
    roots = recv < 0
    assert int(sum(q)) == int(sum(int(d) for d in D[roots]))
    # the lines: ascending cells, the threshold honoured, none in a lake
    for min_flow in (0.0, 1.0, 40.0):
        seg, flows = RV.emu_lines(xyz, e, R, min_flow)
        keep = land & (D >= np.uint64(int(np.ceil(min_flow * 65536)))) & (recv >= 0) & (basin != np.arange(n)) & ~has
        cells = np.nonzero(keep)[0]
        assert seg.shape[0] == cells.size and np.array_equal(RV.bits(flows), RV.bits(R["r_river_flow"][cells]))
        assert (flows >= np.float32(min_flow)).all()
        # a segment starts at its own cell: the directions agree with the cells in ascending order
        p0 = seg[:, 0, :].astype(np.float64)
        p0 /= np.linalg.norm(p0, axis=1, keepdims=True) if cells.size else 1.0
        assert np.allclose(p0, xyz[cells].astype(np.float64), atol=1e-6)


# ---- the explicit graphs of rivers_graphs.py -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,runoff", [c for c in RG.CASES if c[0] in RG.EMULATED])
def test_shapes_emulator_equals_oracle(name, runoff):
    """every shape the device is held to (tests/test_gpu_rivers_shapes.py) but the 32 769-cell ramps, on which the emulator, which
    follows every cell's chain to its end, takes seconds: those are the oracle's alone"""
    G = RG.shape(name)
    got, want = RG.emulated(name, runoff), RG.reference(name, runoff)
    RV.assert_fields_equal((name, runoff), got, want)
    I = got["info"]
    assert (I["pits"], I["spilled"], I["endorheic"], I["drowned"]) == (want["pits"], want["spilled"], want["endorheic"], want["drowned"]), (name, I)
    assert I["landCells"] == int(want["land"].sum()) and I["lakeCells"] == int((~np.isnan(want["r_lake_level"])).sum())
    kept = []
    for min_flow in RG.thresholds(want):
        seg, flows = RV.emu_lines(G.xyz, G.e, got, min_flow)
        wseg, wflows = RV.oracle_lines(want, G.xyz, min_flow)
        assert np.array_equal(RV.bits(seg), RV.bits(wseg)) and np.array_equal(RV.bits(flows), RV.bits(wflows)), (name, runoff, min_flow)
        assert np.array_equal(RV.emu_tinted(G.e, got, min_flow), RV.oracle_tinted(want, min_flow))
        kept.append(seg.shape[0])
    assert kept[0] > 0 and (0 < kept[1] < kept[0] if RG.splits(want) else kept[1] == 0), (name, runoff, kept)


@pytest.mark.parametrize("n", [4096, 4097, 4098, 8193, 32769])
@pytest.mark.parametrize("reversed", [False, True])
def test_ramp_is_one_chain_and_carries_into_the_high_word(n, reversed):
    """One receiver chain over all n - 1 land cells and no pit; the ocean cell holds exactly land * q.  With runoff 16, q = 2^20: the
    ocean cell of the 4 097-cell ramp holds 2^32 exactly, that of 8 193 cells 2^33, and the 4 096-cell ramp, with 4 095 land cells,
    ends 2^20 short of 2^32, so the three sizes stand on both sides of the carry as they do on both sides of 2^12 hops."""
    name = f"ramp-{n}{'-reversed' if reversed else ''}"
    G = RG.shape(name)
    ocean, step = (n - 1, 1) if reversed else (0, -1)
    assert G.n == n and RG.max_degree(G) == 2 and G.e[ocean] == -1.0 and int((G.e > 0).sum()) == n - 1
    for runoff in RG.SHAPES[name][1]:
        O = RG.reference(name, runoff)
        land = np.arange(n) != ocean
        assert O["pits"] == 0 and np.array_equal(O["r_river_receiver"][land], np.arange(n)[land] + step) and O["r_river_receiver"][ocean] == -1
        assert (O["r_river_basin"][land] == -1).all()
        q = (16 if runoff == "max" else 1) << 16
        D = O["r_river_discharge"]
        assert int(D[ocean]) == (n - 1) * q == int(D.max())
        hops = np.abs(np.arange(n) - ocean)                   # a land cell holds what falls on it and on the cells above it
        assert np.array_equal(D[land], ((n - hops[land]) * q).astype(np.uint64))
        if runoff == "max":
            assert int(D[ocean]) >= 2 ** 32 if n >= 4097 else int(D[ocean]) == 2 ** 32 - 2 ** 20
        if n == 8193 and runoff == "max":
            assert int(D[ocean]) == 2 ** 33


@pytest.mark.parametrize("P", [4096, 16384])
def test_sawtooth_rounds_and_spills(P):
    """what each order of the pass levels is for: the emulator's round count, every basin spilled, some drowned"""
    want_rounds = dict(asc=lambda r: r == 1, desc=lambda r: r == 2, pairs=lambda r: r == 2, ruler=lambda r: r >= 10, random=lambda r: r >= 5)
    for kind in (RG.SAW_KINDS if P == 4096 else ("asc", "ruler")):
        name = f"saw-{kind}-{P}"
        G, O, I = RG.shape(name), RG.reference(name, "max"), RG.emulated(name, "max")["info"]
        print(name, I, "max D 2^%.2f" % np.log2(float(O["r_river_discharge"].max())))
        assert G.n == 2 * P + 1
        passes, floors = G.e[1::2], G.e[2::2]
        assert (passes > 1).all() and (passes <= 2).all() and (floors >= 0.5).all() and (floors < 0.75).all() and np.unique(passes).size == P
        assert O["pits"] == O["spilled"] == P and O["endorheic"] == 0 and O["drowned"] > 0, (name, O["pits"], O["spilled"], O["drowned"])
        assert want_rounds[kind](I["rounds"]), (name, I)
        assert int(O["r_river_discharge"].max()) == (2 * P) << 20 >= 2 ** 32      # all of it reaches the ocean cell
    # asc is one chain of P hooks: basin k spills into basin k - 1, the first over pass 1 to the drained pass cell
    O = RG.reference(f"saw-asc-{P}", "max")
    pits = np.arange(2, 2 * P + 1, 2)
    assert np.array_equal(O["r_river_receiver"][pits], pits - 1 - (O["r_river_basin"][pits - 1] == pits))
    # pairs: basins 2 j and 2 j + 1 share the low pass 2 j + 1 and chose each other in the first round
    if P == 4096:
        e = RG.shape("saw-pairs-4096").e[1::2]
        assert e[0::2].max() < e[1::2].min()


def test_mutual_choice_keeps_the_lower_component_as_root():
    """On the pairs sawtooth basins 2 j and 2 j + 1 (pit-list indices 2 j - 1 and 2 j) choose the pass between them in the first round.
    rivers_ops.h: the lower id stays a root, the higher hooks to it and records the pass with u on its own side.  The five fields
    cannot hold this rule (either root gives the same tree), so hook_of is called directly."""
    P = 64
    G = RG.sawtooth(P, "pairs")
    S = RV.oracle_structure_graph(G.off, G.adj, G.e)
    pits, best, to, edges = RV.emu_first_round(G.off, G.adj, G.e, S["basin"])
    assert np.array_equal(pits, np.arange(2, 2 * P + 1, 2)) and best[P] == np.uint64(RV.NO_PASS) and (best[:P] != np.uint64(RV.NO_PASS)).all()
    # basin 1 (index 0) hooks to the drained class over pass 1, from its own cell 2 or 1 to the drained cell
    assert to[0] == P and edges[0, 2] == 0 and edges[0, 3] == P and S["basin"][edges[0, 0]] == 2 and S["basin"][edges[0, 1]] == -1
    for lo in range(1, P - 1, 2):
        hi = lo + 1
        assert best[lo] == best[hi], (lo, hi)
        assert to[lo] == lo and (edges[lo] == -1).all(), (lo, to[lo], edges[lo])
        assert to[hi] == lo and edges[hi, 2] == hi and edges[hi, 3] == lo, (hi, to[hi], edges[hi])
        u, v = edges[hi, 0], edges[hi, 1]
        assert S["basin"][u] == pits[hi] and S["basin"][v] == pits[lo] and abs(int(u) - int(v)) == 1 and max(G.e[u], G.e[v]) == G.e[2 * hi + 1]
    assert to[P - 1] == P - 2 and best[P - 1] != best[P - 2]  # the last basin has one pass only, which its neighbour did not choose


def test_tree_rows_and_donors():
    G = RG.shape("tree-23-3")
    assert G.n == 12721 and RG.max_degree(G) == 24
    O = RG.reference("tree-23-3", "max")
    donors = np.bincount(O["r_river_receiver"][O["r_river_receiver"] >= 0], minlength=G.n)
    assert O["pits"] == 0 and int((donors == 23).sum()) == 1 + 23 + 529 and donors[0] == 1
    D = O["r_river_discharge"]
    assert int(D[0]) == 12720 << 20 == int(D.max()) and int(D[0]) >= 2 ** 33
    assert int(D[1]) == 12720 << 20 and (D[2:25] == np.uint64(553 << 20)).all()


def test_isolated_cells_have_empty_rows():
    G = RG.shape("isolated")
    O = RG.reference("isolated", "max")
    deg = np.diff(G.off)
    assert G.n == 602 and np.array_equal(np.nonzero(deg == 0)[0], [0, 601]) and G.e[0] > 0 and G.e[601] < 0
    assert (O["pits"], O["spilled"], O["endorheic"]) == (1, 0, 1) and O["r_river_basin"][0] == 0 and O["r_river_basin"][601] == -2
    assert int(O["r_river_discharge"][0]) == 16 << 16 and int(O["r_river_discharge"][601]) == 0


def test_hub_forms_are_three_orders_of_one_graph():
    built, permuted, shuffled = (RG.shape(f"hub-{f}-e0") for f in ("built", "permuted", "shuffled"))
    for G in (built, permuted, shuffled):
        assert RG.max_degree(G) == 24
    assert np.array_equal(built.off, shuffled.off) and not np.array_equal(built.adj, shuffled.adj)
    rows = lambda G, r: sorted(G.adj[G.off[r]:G.off[r + 1]].tolist())
    assert all(rows(built, r) == rows(shuffled, r) for r in range(0, built.n, 37))
    assert not np.array_equal(built.off, permuted.off) and np.array_equal(np.sort(built.e), np.sort(permuted.e))
    for form in ("built", "permuted", "shuffled"):            # relabelling and row order move ties and slots, not the count of land
        assert RG.reference(f"hub-{form}-bowl", "uniform")["pits"] > 2000 and RG.emulated(f"hub-{form}-bowl", "uniform")["info"]["rounds"] >= 3
        assert int(RG.reference(f"hub-{form}-bowl", "values")["r_river_discharge"].max()) >= 2 ** 32
