"""Rivers and lakes on the host: the emulator of csrc/rivers_ops.h (tests/emu_rivers: the bodies and the tree walk the device stage
runs, under serial Boruvka rounds) against the independent serial oracle of tests/rivers_common.py (a literal Prim over the pass
keys) in every bit of all five fields, on three meshes, six fields and the three runoff sources; and the properties of the result
that need neither: the final receivers are a forest, the lakes are exactly the cells below their basin's level, the discharge is
conserved, the lines are ordered and honour the threshold."""
import numpy as np
import pytest

import rivers_common as RV


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
