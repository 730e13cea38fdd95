"""Rivers and lakes on the device (csrc/rivers.hip) where its scheduling binds, on the graphs of tests/rivers_graphs.py and at a size the
chip cannot hold at once.  Every case is compared in every bit of all five fields, the counters of wo_rivers_info and the segments
and flows of wo_river_lines under two thresholds; no tolerance anywhere.  The reference is the serial oracle of
tests/rivers_common.py, at 600 000 cells the emulator (tests/emu_rivers), which tests/test_rivers.py holds to the oracle.

ramps of 4 096, 4 097, 4 098 cells   the chain of receivers crosses 2^12 hops: the launch count of the pointer jumping; D crosses 2^32
ramps of 8 193 and 32 769 cells      33 and 129 workgroups on one chain; one thread of the climb walks all of it; the call is timed
sawtooth, P = 4 096 and 16 384       asc: one chain of P hooks under the relabel;  pairs, desc: mutual choices;  ruler: 12 and 14 rounds
tree of 23 children, depth 3         rows of 24 entries; 23 donors arrive at a cell together; three runs must agree in every bit
isolated                             empty rows, a pit without a pass
hub meshes                           rows of up to 24 entries as built, with the cells relabelled, with the rows shuffled
600 000 cells                        2 344 workgroups: more than are resident at once (256 CUs x 8 workgroups of 256 threads)"""
import functools
import time

import numpy as np
import pytest

import rivers_common as RV
import rivers_graphs as RG

pytestmark = pytest.mark.gpu


def _check_lines(tag, pl, e, want_lines, thresholds, split):
    """wo_river_lines against want_lines(min_flow) -> (segments, flows) in every bit, under both thresholds"""
    from planet_heightmap_generation_amd import rivers as RI
    kept = []
    for min_flow in thresholds:
        L = RI.river_lines(pl, min_flow, e)
        wseg, wflows = want_lines(min_flow)
        assert L["segments"].shape == wseg.shape, (tag, min_flow, L["segments"].shape, wseg.shape)
        assert np.array_equal(RV.bits(L["segments"]), RV.bits(wseg)) and np.array_equal(RV.bits(L["flows"]), RV.bits(wflows)), (tag, min_flow)
        kept.append(wseg.shape[0])
    RG.check_kept(tag, kept, split)


def _check_counters(tag, got, want):
    """want: the oracle's result"""
    assert (got["landCells"], got["pits"], got["spilledBasins"], got["endorheicBasins"]) == (int(want["land"].sum()), want["pits"], want["spilled"], want["endorheic"]), (tag, got)
    assert got["lakeCells"] == int((~np.isnan(want["r_lake_level"])).sum()), (tag, got)


def _runoff_arg(G, runoff):
    return "uniform" if runoff == "uniform" else RG.runoff_values(G, runoff)


@pytest.mark.parametrize("name,runoff", RG.CASES)
def test_device_equals_oracle_on_shape(name, runoff):
    from planet_heightmap_generation_amd import rivers as RI, terrain_post as TP
    G = RG.shape(name)
    want = RG.reference(name, runoff)
    tag = (name, runoff)
    pl = TP.Planet(G.mesh, G.xyz)
    try:
        t0 = time.perf_counter()
        got = RI.compute_rivers(pl, G.e, _runoff_arg(G, runoff), download=True)
        first = time.perf_counter() - t0
        RV.assert_fields_equal(tag, got, want)
        _check_counters(tag, got, want)
        if name in RG.EMULATED:
            assert got["rounds"] == RG.emulated(name, runoff)["info"]["rounds"], (tag, got)
        else:                                                 # the longest ramps: no pit, so no round
            assert want["pits"] == 0 and got["rounds"] == 0, (tag, got)
        print(f"{name} {runoff}: {G.n} cells, {got['pits']} pits, {got['lakeCells']} lake cells, {got['rounds']} rounds, {got['launches']} launches, "
              f"max D 2^{np.log2(float(want['r_river_discharge'].max())):.2f}, first call with downloads {first * 1e3:.2f} ms")
        _check_lines(tag, pl, G.e, lambda m: RV.oracle_lines(want, G.xyz, m), RG.thresholds(want), RG.splits(want))
        if name.startswith("ramp-32769"):
            # what a hop of the single-thread climb costs: the same call again, a host clock around it (it ends in a stream synchronise)
            times = []
            for _ in range(3):
                t0 = time.perf_counter()
                RI.compute_rivers(pl, G.e, _runoff_arg(G, runoff))
                times.append(time.perf_counter() - t0)
            print(f"{name} {runoff}: wo_compute_rivers on a chain of {G.n - 2} hops: {sorted(times)[1] * 1e3:.2f} ms median of 3 [{min(times) * 1e3:.2f} - {max(times) * 1e3:.2f}]")
            again = {k: RI.download(pl, k) for k in RV.FIELDS}
            RV.assert_fields_equal(tag + ("again",), again, want)
    finally:
        pl.close()


@pytest.mark.parametrize("runoff", ["max", "values"])
def test_tree_runs_agree_in_every_bit(runoff):
    """23 donors whose chains are equally long hand over to one cell at the same time, at every interior cell: a race in the last
    arriver's hand-off shows as a difference between runs before it shows against the oracle"""
    from planet_heightmap_generation_amd import rivers as RI, terrain_post as TP
    G = RG.shape("tree-23-3")
    want = RG.reference("tree-23-3", runoff)
    if runoff == "max":
        assert int(want["r_river_discharge"].max()) == 12720 << 20 >= 2 ** 33
    pl = TP.Planet(G.mesh, G.xyz)
    try:
        runs = [RI.compute_rivers(pl, G.e, _runoff_arg(G, runoff), download=True) for _ in range(3)]
        for i in (1, 2):
            RV.assert_fields_equal(("tree", runoff, "run", i, "against run 0"), runs[i], runs[0])
        for i, got in enumerate(runs):
            RV.assert_fields_equal(("tree", runoff, "run", i), got, want)
            _check_counters(("tree", runoff, i), got, want)
    finally:
        pl.close()


# ---- scale ---------------------------------------------------------------------------------------------------------------------------
SCALE_N = 600_000
SCALE_FIELDS = ("noise", "bowl", "eroded")


@functools.lru_cache(maxsize=None)
def _scale_mesh():
    from planet_heightmap_generation_amd import sphere_mesh as S
    m, xyz, nd = S.build_sphere(SCALE_N, 0.75, 3)
    return m, np.ascontiguousarray(xyz, np.float32).reshape(-1, 3), nd, np.ascontiguousarray(m.adjOffset, np.int32), np.ascontiguousarray(m.adjList, np.int32)


@pytest.mark.parametrize("kind", SCALE_FIELDS)
def test_device_equals_emulator_at_scale(kind):
    """600 000 cells are 2 344 workgroups of 256 threads, more than the chip holds at once, so the climb's late workgroups start after
    early ones have handed over, and the line compaction scans 3 counts per thread.  Runoff 16 everywhere.  eroded: synthetic terrain,
    warped and carved by erodeComposite on the device as tests/test_gpu_parity.py sets it up, read back and handed over by pointer:
    flats and exact ties decided by the index."""
    from planet_heightmap_generation_amd import rivers as RI, terrain_post as TP
    m, xyz, nd, off, adj = _scale_mesh()
    n = xyz.shape[0]
    pl = TP.Planet(m, xyz, nd)
    try:
        if kind == "eroded":
            pl.synthetic_terrain(3)
            pl.warp_terrain_resident(3, 0.75)
            pl.ocean_from_elevation()
            pl.erode_composite_resident(6, 3e-4, 0.5, 1.0, 6, 1.16, 0.015, 2, 0.5)
            e = pl.download()
        else:
            e = RV.field(kind, xyz)
        runoff = np.full(n, RG.MAX_RUNOFF, np.float32)
        t0 = time.perf_counter()
        want = RV.emu_compute(off, adj, e, 2, runoff)
        t_emu = time.perf_counter() - t0
        got = RI.compute_rivers(pl, e, runoff, download=True)
        RV.assert_fields_equal((kind, n), got, want)
        I = want["info"]
        assert (got["landCells"], got["pits"], got["spilledBasins"], got["endorheicBasins"], got["lakeCells"], got["rounds"]) == (
            I["landCells"], I["pits"], I["spilled"], I["endorheic"], I["lakeCells"], I["rounds"]), (kind, got, I)
        assert I["pits"] > 0 and I["landCells"] > n // 8, I
        times = []
        for _ in range(3):
            t0 = time.perf_counter()
            RI.compute_rivers(pl, e, runoff)
            times.append(time.perf_counter() - t0)
        print(f"{kind}: {n} cells, {I}, max D 2^{np.log2(float(want['r_river_discharge'].max())):.2f}, {got['launches']} launches; wo_compute_rivers by pointer "
              f"{sorted(times)[1] * 1e3:.2f} ms median of 3 [{min(times) * 1e3:.2f} - {max(times) * 1e3:.2f}], the emulator {t_emu * 1e3:.0f} ms")
        thresholds, split = RG.thresholds_of(RV.emu_lines(xyz, e, want, 0.0)[1])
        _check_lines((kind, n), pl, e, lambda mf: RV.emu_lines(xyz, e, want, mf), thresholds, split)
        assert split
    finally:
        pl.close()
