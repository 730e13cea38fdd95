"""HIP path (through the C ABI) against the reference's golden vectors and against the CPU oracle.

Bars: integer / index work and every pass whose arithmetic is +,-,*,/,sqrt in double is BIT-EXACT.  The
glacial passes call pow()/asin() on the device (ocml) where the reference calls V8's, and so does the solve with
m != 0.5; a last-ulp double difference can flip one float32 rounding, so those cases are held per cell
(erode_common.check_cells): every cell within ERODE_ULP_BOUND * max(1, |ref|), at most max(8, N / 10^4) cells
different at all, and RMS < 1e-5 (north_star's bound) on top.  tests/test_erode_libm.py derives the bound; the
figures are printed before they are asserted (expected: 0 cells differ on these fixtures).
"""
import numpy as np
import pytest

from conftest import POST_TAGS, golden_cases, load_golden
from erode_common import check_cells
from hooks import del_hook, set_hook

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def TP():
    from planet_heightmap_generation_amd import terrain_post
    return terrain_post


class _Mesh:
    def __init__(self, off, adj):
        self.adjOffset, self.adjList, self.numRegions = off, adj, off.size - 1


def rms(a, b):
    d = a.astype(np.float64) - b.astype(np.float64)
    return float(np.sqrt((d * d).mean()))


NOISE_KINDS = {"noise3D": (0, 5, 2 / 3, 0.5, 1.0), "fbm5": (1, 5, 2 / 3, 0.5, 1.0), "fbm4h": (1, 4, 0.5, 0.5, 1.0),
               "fbm2": (1, 2, 2 / 3, 0.5, 1.0), "ridged6": (2, 6, 2.0, 0.5, 1.0), "ridged3h": (2, 3, 0.5, 0.5, 1.0),
               "ridged4": (2, 4, 2.0, 0.5, 1.0)}


@pytest.mark.parametrize("seed", [1, 10000, 78, 420])
def test_noise_bit_exact(TP, seed):
    g = load_golden(f"noise_seed{seed}")
    for key, (kind, octv, p0, p1, p2) in NOISE_KINDS.items():
        got = TP.noise_eval(seed, kind, g["points"], octv, p0, p1, p2)
        assert np.array_equal(got, g["ref_" + key]), key


def run_case(pl, g, name, case):
    e = g["elevation0"].copy()
    oc, a, fn = g["isOcean"], case["args"], case["fn"]
    if fn == "warpTerrain":
        pl.warp_terrain(e, a["seed"], a["strength"], g["hotspot"] if "hot" in name else None)
    elif fn == "smoothElevation":
        pl.smooth_elevation(e, oc, a["iterations"], a["strength"])
    elif fn == "sharpenRidges":
        pl.sharpen_ridges(e, oc, a["iterations"], a["strength"])
    elif fn == "applySoilCreep":
        pl.apply_soil_creep(e, oc, a["iterations"], a["strength"])
    elif fn == "erodeComposite":
        pl.erode_composite(e, oc, a["hIters"], a["K"], a["m"], a["dt"], a["tIters"], a["talusSlope"], a["kThermal"],
                           a["gIters"], a["glacialStrength"])
    else:
        return None
    return e


@pytest.mark.parametrize("tag", POST_TAGS)
def test_golden_cases(TP, tag):
    g = load_golden(f"post_{tag}")
    pl = TP.Planet(_Mesh(g["adjOffset"], g["adjList"]), g["xyz"], g["neighborDist"])
    pl.synthetic_terrain(float(g["seed"]))
    assert np.array_equal(pl.download(), g["elevation0"])           # device noise == reference noise, bit for bit
    assert np.array_equal(pl.download_ocean(), g["isOcean"])
    report = []
    for name, case in golden_cases(g).items():
        got = run_case(pl, g, name, case)
        if got is None:
            continue                                            # priorityFloodCarve alone is not an export
        ref = g["ref_" + name]
        nbad = int((got != ref).sum())
        report.append((name, nbad, rms(got, ref)))
        uses_libm = case["fn"] == "erodeComposite" and (case["args"]["gIters"] > 0 or case["args"]["m"] != 0.5)
        if uses_libm:
            check_cells(f"{tag} {name}", got, ref, ref.size)
        else:
            assert nbad == 0, (tag, name, nbad, float(np.abs(got - ref).max()))
    print("\n".join(f"{tag} {n:24s} non-identical cells {b:5d}  rms {r:.2e}" for n, b, r in report))
    pl.close()


@pytest.mark.parametrize("N,seed,h,t,g", [(200000, 3, 20, 20, 10), (1000000, 1, 3, 3, 2)])
def test_against_oracle_large(TP, oracle, N, seed, h, t, g):
    """Sizes the oracle finishes in seconds; same seeded inputs on both sides."""
    from planet_heightmap_generation_amd import sphere_mesh as S
    mesh, xyz, nd = S.build_sphere(N, 0.75, seed)
    pl = TP.Planet(mesh, xyz, nd)
    pl.synthetic_terrain(seed)
    e0, oc = pl.download(), pl.download_ocean()
    assert np.array_equal(e0, oracle.synthetic_terrain(xyz, seed))
    om = oracle.Mesh(mesh.adjOffset, mesh.adjList)
    ref = oracle.erode_composite(om, e0, xyz, oc, h, 3e-4, 0.5, 1.0, t, 1.16, 0.015, g, 0.5, nd)
    got = e0.copy()
    pl.erode_composite(got, oc, h, 3e-4, 0.5, 1.0, t, 1.16, 0.015, g, 0.5)
    nbad = int((got != ref).sum())
    print(f"N={N}: non-identical cells {nbad}, rms {rms(got, ref):.2e}, stats {pl.last_erode_stats()}")
    check_cells(f"N={N} ({h}, {t}, {g})", got, ref, ref.size)
    # hydraulic + thermal only: no libm on the path -> bit-exact
    ref2 = oracle.erode_composite(om, e0, xyz, oc, h, 3e-4, 0.5, 1.0, t, 1.16, 0.015, 0, 0.0, nd)
    got2 = e0.copy()
    pl.erode_composite(got2, oc, h, 3e-4, 0.5, 1.0, t, 1.16, 0.015, 0, 0.0)
    assert np.array_equal(got2, ref2)
    # the flood ran one heap per landmass and vouched for the single heap's result (no serial redo on ordinary terrain)
    st = pl.last_erode_stats()
    assert st["flood_host_calls"] == 2 and st["flood_host_serial_pass1"] == 0 and st["flood_host_unresolved"] == 0, st
    # the other exports at this size
    for fn, ofn, args in (("warp_terrain", "warp_terrain", None), ("smooth_elevation", "smooth_elevation", (2, 0.3)),
                          ("sharpen_ridges", "sharpen_ridges", (3, 0.04)), ("apply_soil_creep", "soil_creep", (3, 0.1125))):
        a = e0.copy()
        if args is None:
            pl.warp_terrain(a, seed, 0.75)
            b = oracle.warp_terrain(om, e0, xyz, seed, 0.75)
        else:
            getattr(pl, fn)(a, oc, *args)
            b = getattr(oracle, ofn)(om, e0, oc, *args)
        assert np.array_equal(a, b), fn
    pl.close()


def test_pipeline_matches_oracle_composition(TP, oracle):
    """runPostProcessing (js/planet-worker.js:40-102) with the UI defaults, resident on the device."""
    g = load_golden("post_N10000_s1")
    mesh = _Mesh(g["adjOffset"], g["adjList"])
    pl = TP.Planet(mesh, g["xyz"], g["neighborDist"])
    params = dict(terrainWarp=0.75, smoothing=0.10, glacialErosion=0.5, hydraulicErosion=0.5, thermalErosion=0.1, ridgeSharpening=0.5)
    e = g["elevation0"].copy()
    oc, delta = TP.run_post_processing(pl, e, params, 1.0, g["hotspot"])
    om = oracle.Mesh(g["adjOffset"], g["adjList"])
    r = oracle.warp_terrain(om, g["elevation0"], g["xyz"], 1.0, 0.75, g["hotspot"])
    roc = (r <= 0).astype(np.uint8)
    pre = r.copy()
    r = oracle.smooth_elevation(om, r, roc, 1, 0.2 + 0.10 * 0.5)
    r = oracle.erode_composite(om, r, g["xyz"], roc, 10, 0.0006 * 0.5, 0.5, 1.0, 1, 1.2 - 0.1 * 0.4, 0.1 * 0.15, 5, 0.5, g["neighborDist"])
    r = oracle.sharpen_ridges(om, r, roc, 3, 0.5 * 0.08)
    r = oracle.soil_creep(om, r, roc, 3, 0.1125)
    assert np.array_equal(oc, roc)
    check_cells("pipeline, UI defaults", e, r, r.size)
    assert np.array_equal(delta, (e.astype(np.float64) - pre.astype(np.float64)).astype(np.float32))      # dl_erosionDelta = final - preErosion of the SAME run
    check_cells("pipeline, UI defaults, delta", delta, (r.astype(np.float64) - pre.astype(np.float64)).astype(np.float32), r.size)
    pl.close()


def test_edge_cases(TP, oracle):
    from planet_heightmap_generation_amd import capi, sphere_mesh as S
    mesh, xyz, nd = S.build_sphere(30, 0.75, 2)          # tiny mesh
    om = oracle.Mesh(mesh.adjOffset, mesh.adjList)
    pl = TP.Planet(mesh, xyz, None)                       # neighborDist computed by the library
    V = mesh.numRegions
    rng = np.random.default_rng(0)
    e0 = rng.uniform(-0.5, 1.0, V).astype(np.float32)
    for oc in (np.ones(V, np.uint8), np.zeros(V, np.uint8), (e0 <= 0).astype(np.uint8)):
        for (h, t, g_) in ((5, 5, 5), (0, 3, 0), (0, 0, 0), (4, 0, 0), (0, 0, 4), (1, 0, 0)):
            a = e0.copy()
            pl.erode_composite(a, oc, h, 3e-4, 0.5, 1.0, t, 1.16, 0.015, g_, 0.7)
            b = oracle.erode_composite(om, e0, xyz, oc, h, 3e-4, 0.5, 1.0, t, 1.16, 0.015, g_, 0.7, nd)
            if g_ > 0:
                check_cells(f"30 cells, {int(oc.sum())} ocean, ({h}, {t}, {g_})", a, b, V)
            else:
                assert np.array_equal(a, b), (oc.sum(), h, t, g_)
    # flats and exact ties: quantised heights exercise the stable-sort / least-ascent / late-edge rules
    eq = (np.round(e0 * 4) / 4).astype(np.float32)
    oc = (eq <= 0).astype(np.uint8)
    a = eq.copy()
    pl.erode_composite(a, oc, 6, 3e-4, 0.5, 1.0, 6, 0.2, 0.05, 0, 0.0)
    assert np.array_equal(a, oracle.erode_composite(om, eq, xyz, oc, 6, 3e-4, 0.5, 1.0, 6, 0.2, 0.05, 0, 0.0, nd))
    # no-ops of the reference: strength <= 0 (js/terrain-post.js:234), zero iterations
    a = e0.copy(); pl.warp_terrain(a, 1, 0.0); assert np.array_equal(a, e0)
    a = e0.copy(); pl.smooth_elevation(a, oc, 0, 0.5); assert np.array_equal(a, e0)
    # errors surface as exceptions
    with pytest.raises((TypeError, ValueError)):
        pl.smooth_elevation(e0.astype(np.float64), oc, 1, 0.5)
    with pytest.raises(ValueError):
        pl.smooth_elevation(e0[:-1].copy(), oc, 1, 0.5)
    with pytest.raises(capi.WorogenError):
        pl.warp_terrain_resident(1, 0.5, use_hotspot=True)      # no hotspot uploaded
    pl.close()
    # malformed meshes are refused at creation: a repeated neighbour, a self loop, an index out of range
    for pos, val, msg in ((mesh.adjOffset[5], mesh.adjList[mesh.adjOffset[5] + 1], "twice"), (mesh.adjOffset[7], 7, "itself"), (3, V + 5, "out of range")):
        bad = mesh.adjList.copy()
        bad[pos] = val
        with pytest.raises(capi.WorogenError, match=msg):
            TP.Planet(oracle.Mesh(mesh.adjOffset, bad), xyz, None)


def test_ties_on_larger_mesh(TP, oracle):
    """Heavily quantised terrain at 20k cells: thousands of equal-elevation pairs, flats and pits."""
    from planet_heightmap_generation_amd import sphere_mesh as S
    mesh, xyz, nd = S.build_sphere(20000, 0.75, 4)
    om = oracle.Mesh(mesh.adjOffset, mesh.adjList)
    e0 = oracle.synthetic_terrain(xyz, 4)
    eq = (np.round(e0 * 64) / 64).astype(np.float32)
    oc = (eq <= 0).astype(np.uint8)
    pl = TP.Planet(mesh, xyz, nd)
    a = eq.copy()
    pl.erode_composite(a, oc, 12, 3e-4, 0.5, 1.0, 12, 1.16, 0.015, 0, 0.0)
    b = oracle.erode_composite(om, eq, xyz, oc, 12, 3e-4, 0.5, 1.0, 12, 1.16, 0.015, 0, 0.0, nd)
    assert np.array_equal(a, b), int((a != b).sum())
    pl.close()


def test_full_size_properties(TP):
    """Config 2 size (1M cells): properties that need no oracle — determinism, ocean untouched, land stays
    >= 0 after hydraulic steps, finite values, every land cell drains (no interior pit deeper than EPS after the flood)."""
    from planet_heightmap_generation_amd import sphere_mesh as S
    mesh, xyz, nd = S.build_sphere(1000000, 0.75, 1)
    pl = TP.Planet(mesh, xyz, nd)
    pl.synthetic_terrain(1)
    pl.save_state()
    e0, oc = pl.download(), pl.download_ocean()
    outs = []
    for _ in range(2):
        pl.restore_state()
        pl.erode_composite_resident(8, 3e-4, 0.5, 1.0, 8, 1.16, 0.015, 4, 0.5)
        pl.apply_soil_creep_resident(3, 0.1125)
        outs.append(pl.download())
    assert np.array_equal(outs[0], outs[1])                       # bit-deterministic run to run
    out = outs[0]
    assert np.isfinite(out).all()
    assert np.array_equal(out[oc == 1], e0[oc == 1])               # ocean cells are never written
    assert (out[oc == 0] >= 0).all()
    assert (out != e0).sum() > 0.5 * (oc == 0).sum()
    st = pl.last_stage_timing()
    assert "solve" in st and "thermal" in st and "priority_flood" in st
    pl.close()


@pytest.mark.isolated
def test_headline_size_properties(TP):
    """BASELINE config 3 size (10 M cells, the bench workload): size-independent properties — bit-deterministic run
    to run (two different schedules of the same dataflow: the launch-count prediction differs between the runs),
    ocean cells never written, land stays >= 0 and finite, zero iterations leave the field alone."""
    import os
    from planet_heightmap_generation_amd import sphere_mesh as S
    mesh, xyz, nd = S.build_sphere(10_000_000, 0.75, 1)
    pl = TP.Planet(mesh, xyz, nd)
    pl.synthetic_terrain(1)
    pl.warp_terrain_resident(1, 0.75)
    pl.ocean_from_elevation()
    pl.save_state()
    e0, oc = pl.download(), pl.download_ocean()
    pl.erode_composite_resident(0, 3e-4, 0.5, 1.0, 0, 1.16, 0.015, 0, 0.5)
    assert np.array_equal(pl.download(), e0)
    outs = []
    for _ in range(2):
        pl.restore_state()
        pl.erode_composite_resident(6, 3e-4, 0.5, 1.0, 6, 1.16, 0.015, 2, 0.5)
        pl.apply_soil_creep_resident(3, 0.1125)
        outs.append(pl.download())
    assert np.array_equal(outs[0], outs[1])
    out = outs[0]
    assert np.isfinite(out).all()
    assert np.array_equal(out[oc == 1], e0[oc == 1])
    assert (out[oc == 0] >= 0).all()
    st = pl.last_erode_stats()
    assert st["solve_patch_launches_total"] > 0 and st["land_cells"] == float((oc == 0).sum())
    pl.close()


@pytest.mark.isolated
def test_headline_size_against_oracle(TP, oracle):
    """BASELINE config 3 size (10 M cells) head to head with the CPU oracle on a bounded number of iterations (the
    oracle needs ~7 s per composite iteration here): warp + erodeComposite(3, 3, 1) + creep, bit for bit where no
    libm call is involved, the per-cell bar of erode_common.check_cells for the glacial pass."""
    from planet_heightmap_generation_amd import sphere_mesh as S
    mesh, xyz, nd = S.build_sphere(10_000_000, 0.75, 1)
    om = oracle.Mesh(mesh.adjOffset, mesh.adjList)
    e0 = oracle.synthetic_terrain(xyz, 1)
    pl = TP.Planet(mesh, xyz, nd)
    pl.synthetic_terrain(1)
    assert np.array_equal(pl.download(), e0)
    ref = oracle.warp_terrain(om, e0, xyz, 1, 0.75)
    got = e0.copy()
    pl.warp_terrain(got, 1, 0.75)
    assert np.array_equal(got, ref)
    oc = (ref <= 0).astype(np.uint8)
    ref2 = oracle.erode_composite(om, ref, xyz, oc, 3, 3e-4, 0.5, 1.0, 3, 1.16, 0.015, 0, 0.0, nd)
    got2 = ref.copy()
    pl.erode_composite(got2, oc, 3, 3e-4, 0.5, 1.0, 3, 1.16, 0.015, 0, 0.0)
    assert np.array_equal(got2, ref2), int((got2 != ref2).sum())            # hydraulic + thermal: no libm on the path
    ref3 = oracle.erode_composite(om, ref, xyz, oc, 2, 3e-4, 0.5, 1.0, 2, 1.16, 0.015, 1, 0.5, nd)
    got3 = ref.copy()
    pl.erode_composite(got3, oc, 2, 3e-4, 0.5, 1.0, 2, 1.16, 0.015, 1, 0.5)
    nbad = int((got3 != ref3).sum())
    print(f"10M cells, glacial pass: non-identical cells {nbad}, rms {rms(got3, ref3):.2e}")
    check_cells("10M cells, glacial pass", got3, ref3, ref3.size)
    ref4 = oracle.soil_creep(om, ref2, oc, 3, 0.1125)
    pl.apply_soil_creep(got2, oc, 3, 0.1125)
    assert np.array_equal(got2, ref4)
    pl.close()


def test_planets_in_flight_match_sequential(TP):
    """Four planets in flight on one GPU (own context / stream / host thread each) give bit for bit what the same
    seeds give one after the other: the library shares no mutable state between planets."""
    from planet_heightmap_generation_amd import sphere_mesh as S
    from planet_heightmap_generation_amd.ensemble import EnsembleRunner
    mesh, xyz, nd = S.build_sphere(60000, 0.75, 5)

    def job(pl, seed):
        pl.synthetic_terrain(seed)
        pl.warp_terrain_resident(seed, 0.75)
        pl.ocean_from_elevation()
        pl.erode_composite_resident(8, 3e-4, 0.5, 1.0, 8, 1.16, 0.015, 3, 0.5)
        pl.apply_soil_creep_resident(3, 0.1125)
        return pl.download()
    seeds = [1, 2, 3, 4, 5, 6, 7, 8]
    seq = EnsembleRunner(mesh, xyz, nd, in_flight=1).map(job, seeds)
    par = EnsembleRunner(mesh, xyz, nd, in_flight=4).map(job, seeds)
    for a, b in zip(seq, par):
        assert np.array_equal(a, b)
    assert not np.array_equal(seq[0], seq[1])
    with pytest.raises(ZeroDivisionError):
        EnsembleRunner(mesh, xyz, nd, in_flight=2).map(lambda pl, s: 1 // 0, [1, 2, 3])


def test_mirror_layout_is_invisible(TP, oracle, monkeypatch):
    """erodeComposite runs on a patch-major renaming of the cells (csrc/mirror.hip, MirrorScope; WO_LAYOUT=index switches it
    off).  Names enter the reference only through the initial landCells order (js/terrain-post.js:384-390) and cellNoise(r) in
    the flood (:98-105), both kept: with glacial iterations, both floods and quantised (tie-heavy) terrain the field must be
    the index-order run's bit for bit, and the oracle's without the libm passes."""
    from planet_heightmap_generation_amd import sphere_mesh as S
    mesh, xyz, nd = S.build_sphere(300000, 0.75, 5)
    pl = TP.Planet(mesh, xyz, nd)
    pl.synthetic_terrain(5)
    e0, oc = pl.download(), pl.download_ocean()
    eq = (np.round(e0 * 64) / 64).astype(np.float32)          # long runs of equal heights: stable-sort history, flats, pits
    om = oracle.Mesh(mesh.adjOffset, mesh.adjList)
    for field, args in ((e0, (12, 3e-4, 0.5, 1.0, 12, 1.16, 0.015, 4, 0.5)), (eq, (8, 3e-4, 0.5, 1.0, 8, 1.16, 0.015, 0, 0.0)),
                        (e0, (0, 3e-4, 0.5, 1.0, 5, 1.16, 0.015, 0, 0.0))):
        res = {}
        for layout in ("mirror", "index"):
            if layout == "index":
                monkeypatch.setenv("WO_LAYOUT", "index")
            else:
                monkeypatch.delenv("WO_LAYOUT", raising=False)
            got = field.copy()
            ocm = (field <= 0).astype(np.uint8)
            pl.erode_composite(got, ocm, *args)
            assert pl.last_erode_stats()["mirror_layout"] == (1.0 if layout == "mirror" else 0.0)
            res[layout] = got
        monkeypatch.delenv("WO_LAYOUT", raising=False)
        assert np.array_equal(res["mirror"], res["index"]), args
        if args[7] == 0:
            ref = oracle.erode_composite(om, field, xyz, (field <= 0).astype(np.uint8), *args, nd)
            assert np.array_equal(res["mirror"], ref), args
    # the call leaves the planet in its own order: a Jacobi pass after it sees the same field either way
    a = e0.copy(); pl.erode_composite(a, oc, 3, 3e-4, 0.5, 1.0, 3, 1.16, 0.015, 0, 0.0); pl.apply_soil_creep(a, oc, 2, 0.1)
    b = oracle.soil_creep(om, oracle.erode_composite(om, e0, xyz, oc, 3, 3e-4, 0.5, 1.0, 3, 1.16, 0.015, 0, 0.0, nd), oc, 2, 0.1)
    assert np.array_equal(a, b)
    pl.close()


def test_flow_accumulation_routes_agree(TP, oracle, monkeypatch):
    """Flow accumulation (js/terrain-post.js:604-611) has two forms: under the land-first mirror (default) two levels — the last-arriver climb
    inside every tile of 1 024 cells on LDS atomics, a climb over the tiles' local roots, and the tile sums again with the inflows (k_flow_tiles) —
    and on the planet's own cell order (WO_LAYOUT=index) one launch over all cells in which the thread that completes a receiver carries on
    with it (k_flow_climb).  Integer sums: both must give the oracle's field bit for bit, on ordinary and on quantised (flat-heavy: long
    unbranched chains) terrain."""
    from planet_heightmap_generation_amd import sphere_mesh as S
    mesh, xyz, nd = S.build_sphere(250000, 0.75, 9)
    pl = TP.Planet(mesh, xyz, nd)
    pl.synthetic_terrain(9)
    e0 = pl.download()
    eq = (np.round(e0 * 32) / 32).astype(np.float32)
    om = oracle.Mesh(mesh.adjOffset, mesh.adjList)
    args = (10, 3e-4, 0.5, 1.0, 4, 1.16, 0.015, 0, 0.0)
    for field in (e0, eq):
        oc = (field <= 0).astype(np.uint8)
        ref = oracle.erode_composite(om, field, xyz, oc, *args, nd)
        for route in (None, "index"):
            if route:
                monkeypatch.setenv("WO_LAYOUT", route)
            else:
                monkeypatch.delenv("WO_LAYOUT", raising=False)
            got = field.copy()
            pl.erode_composite(got, oc, *args)
            st = pl.last_erode_stats()
            assert np.array_equal(got, ref), (route, int((got != ref).sum()))
            assert st["flow_two_level"] == (1.0 if route is None else 0.0), (route, st["flow_two_level"])
    monkeypatch.delenv("WO_LAYOUT", raising=False)
    pl.close()


def test_flood_routes_agree(TP, oracle, monkeypatch):
    """The host flood's three routes — one heap per landmass pipelined with passes 2/3 (default), the same in two phases,
    and the single serial heap walk (WO_FLOOD_HOST) — are read once per process, so each runs in its own interpreter;
    all must give the oracle's field (reference: js/terrain-post.js:59-215)."""
    import os, subprocess, sys, textwrap
    from conftest import REPO
    code = textwrap.dedent("""
        import sys, numpy as np
        sys.path.insert(0, %r)
        from oracle import pyoracle as O
        from planet_heightmap_generation_amd import sphere_mesh as S, terrain_post as TP
        mesh, xyz, nd = S.build_sphere(150000, 0.75, 11)
        pl = TP.Planet(mesh, xyz, nd)
        pl.synthetic_terrain(11)
        e0, oc = pl.download(), pl.download_ocean()
        om = O.Mesh(mesh.adjOffset, mesh.adjList)
        ref = O.erode_composite(om, e0, xyz, oc, 8, 3e-4, 0.5, 1.0, 8, 1.16, 0.015, 0, 0.0, nd)
        got = e0.copy()
        pl.erode_composite(got, oc, 8, 3e-4, 0.5, 1.0, 8, 1.16, 0.015, 0, 0.0)
        st = pl.last_erode_stats()
        print("ROUTE", int(np.array_equal(got, ref)), int(st["flood_host_serial_pass1"]), int(st["flood_host_calls"]))
    """) % str(REPO)
    for route, serial_calls in ((None, 0), ("two-phase", 0), ("serial", 2)):
        env = dict(os.environ)
        env.pop("WO_FLOOD_HOST", None)
        if route:
            env["WO_FLOOD_HOST"] = route
        out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
        line = [l for l in out.stdout.splitlines() if l.startswith("ROUTE")]
        assert line, (route, out.stdout[-500:], out.stderr[-1500:])
        same, serial, calls = (int(v) for v in line[0].split()[1:])
        assert same == 1 and calls == 2 and serial == serial_calls, (route, line)


def test_device_flood_is_order_equivalent(TP, oracle, monkeypatch):
    """priorityFloodCarve pass 1 on the device (WO_FLOOD=device: label-correcting fixed point, csrc/flood_ops.h) against
    the reference: every erodeComposite golden with hydraulic iterations, then 200 k / 1 M cells against the oracle.
    Bit for bit; `flood_pass1_on_host` must be 0 (the device result was used) unless an equal-key decision was counted."""
    from planet_heightmap_generation_amd import sphere_mesh as S
    monkeypatch.setenv("WO_FLOOD", "device")
    used = 0
    for tag in POST_TAGS:
        g = load_golden(f"post_{tag}")
        pl = TP.Planet(_Mesh(g["adjOffset"], g["adjList"]), g["xyz"], g["neighborDist"])
        for name, case in golden_cases(g).items():
            a = case["args"]
            if case["fn"] != "erodeComposite" or a["hIters"] <= 0 or a["gIters"] > 0 or a["m"] != 0.5:
                continue
            got = run_case(pl, g, name, case)
            st = pl.last_erode_stats()
            assert np.array_equal(got, g["ref_" + name]), (tag, name, st)
            assert st["flood_device_rounds"] > 0
            if st["flood_equal_key_decisions"] == 0:
                assert st["flood_pass1_on_host"] == 0, st
                used += 1
        pl.close()
    assert used > 0
    for N, seed, iters in ((200000, 3, 24), (1000000, 1, 8)):
        mesh, xyz, nd = S.build_sphere(N, 0.75, seed)
        om = oracle.Mesh(mesh.adjOffset, mesh.adjList)
        e0 = oracle.warp_terrain(om, oracle.synthetic_terrain(xyz, seed), xyz, seed, 0.75)
        oc = (e0 <= 0).astype(np.uint8)
        ref = oracle.erode_composite(om, e0, xyz, oc, iters, 3e-4, 0.5, 1.0, iters, 1.16, 0.015, 0, 0.0, nd)   # two floods: start and 75 %
        pl = TP.Planet(mesh, xyz, nd)
        got = e0.copy()
        pl.erode_composite(got, oc, iters, 3e-4, 0.5, 1.0, iters, 1.16, 0.015, 0, 0.0)
        st = pl.last_erode_stats()
        print(f"device flood N={N}: {({k: v for k, v in st.items() if 'flood' in k})}")
        assert np.array_equal(got, ref), (N, int((got != ref).sum()), st)
        assert st["flood_device_rounds"] > 0 and (st["flood_equal_key_decisions"] > 0 or st["flood_pass1_on_host"] == 0)
        pl.close()


def test_config2_verbatim_against_oracle(TP, oracle):
    """BASELINE config 2 at its own parameters: 1 M cells, erodeComposite(200, 3e-4, 0.5, 1, 200, 1.16, 0.015, 0, 0) then
    applySoilCreep(3, 0.1125), head to head with the oracle (about 70 s of oracle time): bit for bit (no libm on this path)."""
    from planet_heightmap_generation_amd import sphere_mesh as S
    mesh, xyz, nd = S.build_sphere(1_000_000, 0.75, 1)
    om = oracle.Mesh(mesh.adjOffset, mesh.adjList)
    e0 = oracle.synthetic_terrain(xyz, 1)
    oc = (e0 <= 0).astype(np.uint8)
    ref = oracle.erode_composite(om, e0, xyz, oc, 200, 3e-4, 0.5, 1.0, 200, 1.16, 0.015, 0, 0.0, nd)
    ref = oracle.soil_creep(om, ref, oc, 3, 0.1125)
    pl = TP.Planet(mesh, xyz, nd)
    got = e0.copy()
    pl.erode_composite(got, oc, 200, 3e-4, 0.5, 1.0, 200, 1.16, 0.015, 0, 0.0)
    pl.apply_soil_creep(got, oc, 3, 0.1125)
    nbad = int((got != ref).sum())
    print(f"config 2 (1M x 200 iterations): non-identical cells {nbad}, rms {rms(got, ref):.2e}")
    assert nbad == 0
    pl.close()


@pytest.mark.isolated
def test_config3_checksum_of_the_benched_field(TP):
    """The field bench.py times (BASELINE config 3: 10 M cells, warp + erodeComposite(200,200,10) + creep) has the CRC of
    the ORACLE's result for the same inputs (tests/golden/crc_config3.json, made by oracle/ref_harness/make_crc_config3.py).
    The glacial passes call libm on the device, so bit equality is not guaranteed by construction; it holds on gfx950."""
    import json
    import zlib
    from conftest import GOLDEN
    from planet_heightmap_generation_amd import sphere_mesh as S
    gold = json.loads((GOLDEN / "crc_config3.json").read_text())["10000000"]
    mesh, xyz, nd = S.build_sphere(10_000_000, 0.75, 1)
    assert int(zlib.crc32(mesh.adjList.tobytes())) == gold["crc32_mesh"]
    pl = TP.Planet(mesh, xyz, nd)
    pl.synthetic_terrain(1)
    assert int(zlib.crc32(pl.download().tobytes())) == gold["crc32_input"]
    pl.warp_terrain_resident(1, 0.75)
    pl.ocean_from_elevation()
    pl.erode_composite_resident(200, 3e-4, 0.5, 1.0, 200, 1.16, 0.015, 10, 0.5)
    stats = pl.last_erode_stats()
    pl.apply_soil_creep_resident(3, 0.1125)
    out = pl.download()
    assert abs(float(out.astype(np.float64).sum()) - gold["sum"]) < 1e-5 * out.size      # RMS-scale guard before the exact check
    assert int(zlib.crc32(out.tobytes())) == gold["crc32"], "field differs from the oracle's"
    assert stats["calls_run_again_with_checks"] == 0 and stats["flow_two_level"] == 1.0, stats
    pl.close()


def _checksum_case(TP, key, cells, seed, iters, g):
    """warp 0.75 -> isOcean -> erodeComposite(iters, ..., iters, ..., g, 0.5) -> creep x3 on a fixed-seed sphere, resident on the
    device; the CRC of the result against the oracle's (tests/golden/crc_config3.json, oracle/ref_harness/make_crc_config3.py)."""
    import json
    import zlib
    from conftest import GOLDEN
    from planet_heightmap_generation_amd import sphere_mesh as S
    gold = json.loads((GOLDEN / "crc_config3.json").read_text())[key]
    assert (gold["cells"], gold["seed"], gold["iterations"], gold["gIters"]) == (cells, seed, iters, g)
    mesh, xyz, nd = S.build_sphere(cells, 0.75, seed)
    assert int(zlib.crc32(mesh.adjList.tobytes())) == gold["crc32_mesh"]
    pl = TP.Planet(mesh, xyz, nd)
    pl.synthetic_terrain(seed)
    assert int(zlib.crc32(pl.download().tobytes())) == gold["crc32_input"]
    pl.warp_terrain_resident(seed, 0.75)
    pl.ocean_from_elevation()
    pl.erode_composite_resident(iters, 3e-4, 0.5, 1.0, iters, 1.16, 0.015, g, 0.5)
    stats = pl.last_erode_stats()
    pl.apply_soil_creep_resident(3, 0.1125)
    out = pl.download()
    pl.close()
    assert abs(float(out.astype(np.float64).sum()) - gold["sum"]) < 1e-5 * out.size      # RMS-scale guard before the exact check
    assert int(zlib.crc32(out.tobytes())) == gold["crc32"], "field differs from the oracle's"
    assert stats["calls_run_again_with_checks"] == 0, "a basin-solve launch left tasks pending (the layout split a drainage component?)"
    return stats


@pytest.mark.isolated
def test_config4_size_checksum_on_one_gpu(TP):
    """BASELINE config 4's planet (40 M cells, seed 1) on one GPU, 20 composite iterations (1 glacial): CRC == the oracle's.
    At this size both flood calls meet equal keys whose order matters (13 contested cells per step in round 2, which sent the
    call to the serial heap walk): they are decided by the replay of the single heap (flood_host.cc), never the serial walk."""
    stats = _checksum_case(TP, "40000000", 40_000_000, 1, 20, 1)
    print({k: v for k, v in stats.items() if k.startswith("flood_host")})
    assert stats["flood_host_serial_pass1"] == 0
    assert stats["solve_basin_passes_with_leftovers"] == 0


@pytest.mark.isolated
def test_config4_full_length_checksum_on_one_gpu(TP):
    """BASELINE config 4's planet at its OWN iteration count: 40 M cells, 200 composite iterations (10 glacial), one GPU.  The oracle's
    CRC (53 minutes of one core, oracle/ref_harness/make_crc_config3.py 40000000 1 200) is the one bench.py's one-planet leg checks
    its timed steps against."""
    stats = _checksum_case(TP, "40000000_iters200", 40_000_000, 1, 200, 10)
    print({k: v for k, v in stats.items() if k.startswith("flood_host") or k == "flood_stage_ms"})
    assert stats["flood_host_serial_pass1"] == 0 and stats["solve_basin_passes_with_leftovers"] == 0


@pytest.mark.isolated
def test_config4_decomposed_8_shares_checksum(TP):
    """BASELINE config 4 as its 8-rank plan: the 40 M-cell planet dealt to 8 landmass shares (one host thread, context and
    planet per share on this GPU), 20 composite iterations, the flood exchange between the shares.  Both flood calls meet
    equal keys that matter at this size, so a share that replayed a heap of its own landmasses only would not end on the
    oracle's field (round 3: CRC 1594252700); with the shares pooling their heights the merged field's CRC == the oracle's."""
    import json
    import zlib
    from conftest import GOLDEN
    from planet_heightmap_generation_amd import decomposed as D
    from planet_heightmap_generation_amd import sphere_mesh as S
    gold = json.loads((GOLDEN / "crc_config3.json").read_text())["40000000"]
    cells, seed, iters, g = 40_000_000, 1, 20, 1
    assert (gold["cells"], gold["seed"], gold["iterations"], gold["gIters"]) == (cells, seed, iters, g)
    mesh, xyz, nd = S.build_sphere(cells, 0.75, seed)
    pl = TP.Planet(mesh, xyz, nd)
    pl.synthetic_terrain(seed)
    pl.warp_terrain_resident(seed, 0.75)
    pl.ocean_from_elevation()
    warped, oc = pl.download(), pl.download_ocean()
    pl.close()
    merged, stats, secs, plan = D.erode_shares_concurrently(TP, mesh, xyz, nd, warped, oc, 8, (iters, 3e-4, 0.5, 1.0, iters, 1.16, 0.015, g, 0.5), (3, 0.1125))
    print("share seconds", [round(v, 2) for v in secs], "whole-planet floods per share", [st["flood_exchange_whole_planet_floods"] for st in stats],
          "gathers", stats[0]["flood_exchange_gathers"])
    assert sum(st["flood_exchange_whole_planet_floods"] for st in stats) >= 1            # the exchange was needed (else the test has no power)
    # ONE share floods the whole planet per undecided call and hands the land heights back to the others
    assert sum(st["flood_exchange_whole_planet_floods"] for st in stats) == stats[0]["flood_exchange_gathers"]
    assert all(st["flood_host_serial_pass1"] == 0 for st in stats)
    assert int(zlib.crc32(merged.tobytes())) == gold["crc32"], "merged field differs from the oracle's"


@pytest.mark.isolated
def test_config4_two_processes_over_gloo(TP, tmp_path):
    """BASELINE config 4's planet (40 M cells, 20 iterations) as two PROCESSES sharing this GPU, the flood exchange and the merge over
    torch.distributed (gloo): the multi-process path at a size where flood calls ARE undecided (the thread form of the same plan:
    test_config4_decomposed_8_shares_checksum).  Every rank must end on the oracle's field.  The RCCL form of the exchange
    (csrc/comm.hip: flood_link_exchange) still has never had a peer: RCCL refuses two ranks on one device, and this pool has one."""
    import json
    import os
    import subprocess
    import sys
    from conftest import GOLDEN, REPO
    gold = json.loads((GOLDEN / "crc_config3.json").read_text())["40000000"]
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY="0", WO_FLOOD_THREADS="12", WO_HOST_THREADS="32")
    subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1", "--master-port", "29741",
                    str(REPO / "tests" / "config4_worker.py"), str(tmp_path), str(gold["cells"]), str(gold["seed"]), str(gold["iterations"]), str(gold["gIters"])],
                   check=True, env=env, timeout=1500)
    res = json.loads((tmp_path / "result.json").read_text())
    print(res)
    assert len(res) == 2 and sum(r["land_cells"] for r in res) == gold["land_cells"]
    assert sum(r["whole_planet_floods"] for r in res) >= 1 and res[0]["gathers"] >= 1          # the exchange was needed: the test has power
    assert sum(r["whole_planet_floods"] for r in res) == res[0]["gathers"]                      # one rank floods per undecided call, the others receive
    assert all(r["serial_pass1"] == 0 for r in res)
    assert all(r["crc32"] == gold["crc32"] for r in res), [r["crc32"] for r in res]


def test_decomposed_shares_with_flood_exchange_small(TP, oracle):
    """The same machinery where the oracle can check every cell: 300 k cells quantised so that equal keys matter, 5 shares as
    threads with the flood exchange, glacial + both floods: merged == oracle bit for bit (and the exchange did run)."""
    from planet_heightmap_generation_amd import decomposed as D
    from planet_heightmap_generation_amd import sphere_mesh as S
    mesh, xyz, nd = S.build_sphere(300000, 0.75, 6)
    om = oracle.Mesh(mesh.adjOffset, mesh.adjList)
    e0 = oracle.synthetic_terrain(xyz, 6)
    e0 = (np.round(e0 * 4096) / 4096).astype(np.float32)
    oc = (e0 <= 0).astype(np.uint8)
    args = (8, 3e-4, 0.5, 1.0, 8, 1.16, 0.015, 2, 0.5)
    ref = oracle.soil_creep(om, oracle.erode_composite(om, e0, xyz, oc, *args, nd), oc, 3, 0.1125)
    merged, stats, secs, plan = D.erode_shares_concurrently(TP, mesh, xyz, nd, e0, oc, 5, args, (3, 0.1125))
    print("gathers", stats[0]["flood_exchange_gathers"], "whole-planet floods", [st["flood_exchange_whole_planet_floods"] for st in stats])
    assert np.array_equal(merged, ref), int((merged != ref).sum())
    assert stats[0]["flood_exchange_calls"] == 2


@pytest.mark.isolated
@pytest.mark.parametrize("seed", list(range(2, 17)))
def test_config5_seeds_checksum(TP, seed):
    """BASELINE config 5 runs config 3's stack on other seeds: 10 M cells, seeds 2 .. 16, 20 composite iterations (1 glacial),
    CRC == the oracle's (seed 1 at the full 200 iterations: test_config3_checksum_of_the_benched_field; seeds 2 and 3 at the full
    200 iterations: test_config5_seeds_full_length_checksum)."""
    stats = _checksum_case(TP, f"10000000_seed{seed}_iters20", 10_000_000, seed, 20, 1)
    assert stats["flood_host_serial_pass1"] == 0


@pytest.mark.isolated
@pytest.mark.parametrize("seed", list(range(2, 16)))
def test_config5_seeds_full_length_checksum(TP, seed):
    """Fourteen more planets of BASELINE config 5 at the full 200 iterations (10 glacial): CRC == the oracle's (10-30 minutes of one core each,
    oracle/ref_harness/make_crc_config3.py 10000000 <seed> 200)."""
    stats = _checksum_case(TP, f"10000000_seed{seed}_iters200", 10_000_000, seed, 200, 10)
    assert stats["flood_host_serial_pass1"] == 0


@pytest.mark.isolated
@pytest.mark.parametrize("seed", [16, 24, 32, 40, 48, 56, 64])
def test_config5_every_eighth_of_the_64_seeds_full_length_checksum(TP, seed):
    """BASELINE config 5 names 64 seeds; tests/golden/crc_config3.json pins ALL of them at the full 200 iterations (round 6: seeds 16-64 added,
    12-30 minutes of one core each) and `bench.py --gpus N` checks every planet it erodes against that file.  Here: every eighth of the new ones."""
    import json
    from conftest import GOLDEN
    key = f"10000000_seed{seed}_iters200"
    if key not in json.loads((GOLDEN / "crc_config3.json").read_text()):
        pytest.skip(f"{key} is not in tests/golden/crc_config3.json")
    stats = _checksum_case(TP, key, 10_000_000, seed, 200, 10)
    assert stats["flood_host_serial_pass1"] == 0


@pytest.mark.parametrize("world,cells,iters,engine", [(3, 200000, (8, 8, 3), "planet"), (2, 1000000, (6, 6, 2), "planet"), (3, 200000, (8, 8, 3), "planet-device")])
def test_landmass_decomposition_on_the_device(TP, oracle, tmp_path, world, cells, iters, engine):
    """One planet eroded by `world` ranks (processes sharing this box's GPU, gloo for the merge): every rank runs the HIP
    stack with the other ranks' landmasses masked as ocean, the land elevations are merged through the C ABI's pack /
    unpack kernels.  Partitioned == unpartitioned, bit for bit, on every rank.  Engine "planet-device": the exchange takes the
    device-tensor branch of a RCCL run (pack / unpack through device pointers), with the collective stood in for by gloo."""
    import os
    import subprocess
    import sys
    from conftest import REPO
    from planet_heightmap_generation_amd import sphere_mesh as S
    mesh, xyz, nd = S.build_sphere(cells, 0.75, 2)
    om = oracle.Mesh(mesh.adjOffset, mesh.adjList)
    e = oracle.warp_terrain(om, oracle.synthetic_terrain(xyz, 2), xyz, 2, 0.75)
    oc = (e <= 0).astype(np.uint8)
    np.savez(tmp_path / "case.npz", adjOffset=mesh.adjOffset, adjList=mesh.adjList, xyz=xyz, neighborDist=nd, elevation=e, isOcean=oc, iters=np.array(iters))
    h, t, g = iters
    pl = TP.Planet(mesh, xyz, nd)
    pl.upload(e, oc)
    pl.erode_composite_resident(h, 3e-4, 0.5, 1.0, t, 1.16, 0.015, g, 0.5)
    pl.apply_soil_creep_resident(3, 0.1125)
    ref = pl.download()
    pl.close()
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(29700 + world), HSA_ENABLE_IPC_MODE_LEGACY="0")
    subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}", "--master-addr", "127.0.0.1",
                    "--master-port", str(29700 + world), str(REPO / "tests" / "decomposed_worker.py"), str(tmp_path), engine],
                   check=True, env=env, timeout=1200)
    for r in range(world):
        out = np.load(tmp_path / f"result_{r}.npy")
        assert np.array_equal(out, ref), (r, int((out != ref).sum()))


def test_flood_exchange_protocol_handshake_and_mask_check(TP):
    """include/worogen.h, wo_planet_set_flood_exchange: (i) a callback that does not acknowledge the protocol (phase -1) — e.g. one written for
    the two-phase protocol of round 4 that answers every phase != 0 with its all-gather and returns 0 — is refused when it is set, not at the
    first undecided flood; (ii) a resident mask with land where the planet's true mask has ocean fails the erodeComposite call instead of reading
    unset positions."""
    import ctypes as C
    from planet_heightmap_generation_amd import capi
    from planet_heightmap_generation_amd import sphere_mesh as S
    mesh, xyz, nd = S.build_sphere(20000, 0.75, 1)
    pl = TP.Planet(mesh, xyz, nd)
    pl.synthetic_terrain(1)
    e, oc = pl.download(), pl.download_ocean()
    seen = []

    def old_style(_user, phase, buf, n):          # knows phases 0 and "the other one"
        seen.append(int(phase))
        return 0
    cb = capi.FLOOD_EXCHANGE_FN(old_style)
    rc = capi.lib().wo_planet_set_flood_exchange(pl.handle, capi.ptr(oc), cb, None)
    assert rc != 0 and seen == [-1]
    assert "protocol" in capi.lib().wo_last_error().decode()

    class Alone:                                   # a one-rank exchange: nothing to pool
        def allreduce_max(self, v): return v
        def allgather(self, field): pass
        def broadcast(self, land, sender): pass
    true_oc = oc.copy()
    true_oc[np.flatnonzero(oc == 0)[:7]] = 1       # seven cells the resident mask calls land, the "true" mask ocean
    pl.set_flood_exchange(true_oc, Alone())
    with pytest.raises(Exception, match="true mask"):
        pl.erode_composite_resident(2, 3e-4, 0.5, 1.0, 2, 1.16, 0.015, 0, 0.0)
    pl.set_flood_exchange(None)
    pl.upload(e, oc)
    pl.set_flood_exchange(oc, Alone())
    pl.erode_composite_resident(4, 3e-4, 0.5, 1.0, 4, 1.16, 0.015, 0, 0.0)
    assert pl.last_erode_stats()["flood_exchange_calls"] == 2          # both floods (before iteration 0 and at iteration 3) asked the exchange
    pl.close()


def test_exchange_behind_the_c_abi_single_rank(TP):
    """wo_comm_* / wo_planet_exchange_*: the RCCL communicator and both exchange shapes on a real device.  RCCL refuses two
    ranks on one GPU, so a one-GPU box can only run the one-rank communicator: the all-gather then returns the rank's own
    contribution (nothing to unpack) and the chain has no neighbours — what is checked is that the communicator comes up
    from the 128-byte id, that ncclAllGather / the send-recv group run on the planet's stream, and that the field is
    untouched.  The N-rank logic (which cells go where) is covered by the gloo tests (tests/test_decomposed.py,
    tests/test_banded.py) that drive the same pack / unpack lists."""
    from planet_heightmap_generation_amd import sphere_mesh as S
    mesh, xyz, nd = S.build_sphere(20000, 0.75, 1)
    pl = TP.Planet(mesh, xyz, nd)
    pl.synthetic_terrain(1)
    before = pl.download()
    uid = TP.Comm.unique_id()
    assert len(uid) == 128 and any(uid)
    comm = TP.Comm(pl.ctx, uid, 1, 0)
    send = np.arange(0, 5000, 3, dtype=np.int32)
    pl.set_halo(send, np.empty(0, np.int32))
    pl.exchange_allgather(comm, [send.size])
    with pytest.raises(Exception):
        pl.exchange_allgather(comm, [send.size + 1])          # counts must match the planet's lists
    with pytest.raises(Exception):
        pl.exchange_neighbors(comm, 0, 0)                     # a one-rank chain has nobody to send these to
    pl.set_halo(np.empty(0, np.int32), np.empty(0, np.int32))
    pl.exchange_neighbors(comm, 0, 0)
    assert np.array_equal(pl.download(), before)
    comm.close()
    pl.close()


def test_basin_leftovers_are_finished_by_patch_launches(TP, oracle, monkeypatch):
    """The basin-local solve never leaves a task pending on real layouts (`solve_basin_passes_with_leftovers` is 0 in every run),
    so the path that finishes pending tasks — blocker hints made from the records, then k_solve_patch launches over the same
    store order — is exercised with a layout that is wrong on purpose (test hook basin_scramble: every third cell in its neighbour's
    group).  The solve is a single-assignment dataflow: the result must be the oracle's bit for bit all the same."""
    from planet_heightmap_generation_amd import sphere_mesh as S
    mesh, xyz, nd = S.build_sphere(200000, 0.75, 4)
    pl = TP.Planet(mesh, xyz, nd)
    pl.synthetic_terrain(4)
    e0 = pl.download()
    oc = (e0 <= 0).astype(np.uint8)
    om = oracle.Mesh(mesh.adjOffset, mesh.adjList)
    args = (12, 3e-4, 0.5, 1.0, 12, 1.16, 0.015, 0, 0.0)
    ref = oracle.erode_composite(om, e0, xyz, oc, *args, nd)
    set_hook(monkeypatch, "basin_scramble", 1)
    got = e0.copy()
    pl.erode_composite(got, oc, *args)
    st = pl.last_erode_stats()
    del_hook(monkeypatch, "basin_scramble")
    assert st["solve_basin_passes_with_leftovers"] > 0, st
    # the pending count is not looked at after every pass any more: the call notices at its next host synchronisation that a launch
    # left tasks behind, restores the field and runs again with the check (and the k_solve_patch finisher) after every pass
    assert st["solve_check_every_pass"] == 1 and st["calls_run_again_with_checks"] >= 1, st
    assert np.array_equal(got, ref), int((got != ref).sum())
    got = e0.copy()
    pl.erode_composite(got, oc, *args)
    assert pl.last_erode_stats()["solve_basin_passes_with_leftovers"] == 0
    assert pl.last_erode_stats()["solve_check_every_pass"] == 0
    assert np.array_equal(got, ref)
    pl.close()


def test_glacial_step_one_launch_and_its_finisher(TP, oracle, monkeypatch):
    """The glacial step's two dependency walks run as ONE launch each: the ice accumulation by last-arriver climb (k_ice_climb),
    the carve turns by agent-scope hand-offs between the tasks' own threads (k_carve_granules: heights as self-validating granules).
    Both must give the oracle's field bit for bit, and so must (i) the mixed case in which the one-launch carve gives up at once (test hook
    carve_budget_ms=0: every lane that finds a dependency open leaves its task) and the synchronous rounds (k_carve_round_static) finish from
    whatever state it left, and (ii) a launch of two workgroups for thousands of tasks (hook carve_blocks)."""
    from planet_heightmap_generation_amd import sphere_mesh as S
    mesh, xyz, nd = S.build_sphere(300000, 0.75, 6)
    pl = TP.Planet(mesh, xyz, nd)
    pl.synthetic_terrain(6)
    e0 = pl.download()
    oc = (e0 <= 0).astype(np.uint8)
    om = oracle.Mesh(mesh.adjOffset, mesh.adjList)
    args = (6, 3e-4, 0.5, 1.0, 6, 1.16, 0.015, 4, 0.8)
    ref = oracle.erode_composite(om, e0, xyz, oc, *args, nd)
    got = e0.copy(); pl.erode_composite(got, oc, *args)
    st = pl.last_erode_stats()
    assert st["carve_active_total"] > 1000, st                 # the case does carve
    assert st["carve_flow_launches_with_leftovers"] == 0, st
    assert st["carve_rounds_total"] == 4 and st["ice_rounds_total"] == 4, st      # one launch per glacial step
    assert np.array_equal(got, ref), int((got != ref).sum())
    set_hook(monkeypatch, "carve_budget_ms", 0)
    got = e0.copy(); pl.erode_composite(got, oc, *args)
    st = pl.last_erode_stats()
    assert st["carve_flow_launches_with_leftovers"] > 0 and st["carve_rounds_total"] > 4, st
    assert np.array_equal(got, ref), int((got != ref).sum())
    del_hook(monkeypatch, "carve_budget_ms")
    # two workgroups for thousands of tasks: every thread takes many positions of the (rank-ordered) activation list in turn, which is
    # how a planet with more active tasks than resident threads runs (40 M cells); the launch must still finish everything itself
    set_hook(monkeypatch, "carve_blocks", 2)
    got = e0.copy(); pl.erode_composite(got, oc, *args)
    st = pl.last_erode_stats()
    assert st["carve_flow_launches_with_leftovers"] == 0 and st["carve_rounds_total"] == 4, st
    assert np.array_equal(got, ref), int((got != ref).sum())
    del_hook(monkeypatch, "carve_blocks")
    pl.close()


def test_sorts_are_stable_under_ties(TP, oracle):
    """Both sorts of an iteration (landCells by elevation; the basin-local solve's group-major store order) run on the in-tree
    stable radix sort (csrc/radix.hip: count + scatter launch per 8-bit digit, the last pass writes rank[] / slotOf[]).  On a
    heavily quantised field — thousands of equal keys, whose order is the previous iteration's, as V8's stable sort keeps it —
    it must give the oracle's field bit for bit.  300 k cells: 21 tiles
    of 4096 pairs, so the prefix over earlier tiles (group totals + tile counts) and a partly filled last tile are exercised."""
    from planet_heightmap_generation_amd import sphere_mesh as S
    mesh, xyz, nd = S.build_sphere(300000, 0.75, 9)
    om = oracle.Mesh(mesh.adjOffset, mesh.adjList)
    e0 = oracle.synthetic_terrain(xyz, 9)
    eq = (np.round(e0 * 256) / 256).astype(np.float32)
    oc = (eq <= 0).astype(np.uint8)
    args = (8, 3e-4, 0.5, 1.0, 8, 1.16, 0.015, 2, 0.6)
    ref = oracle.erode_composite(om, eq, xyz, oc, *args, nd)
    pl = TP.Planet(mesh, xyz, nd)
    got = eq.copy(); pl.erode_composite(got, oc, *args)
    assert np.array_equal(got, ref), int((got != ref).sum())
    # so few distinct heights that a single key holds a fifth of the land
    e4 = (np.round(e0 * 4) / 4).astype(np.float32)
    oc4 = (e4 <= 0).astype(np.uint8)
    args4 = (4, 3e-4, 0.5, 1.0, 4, 1.16, 0.015, 0, 0.0)
    ref4 = oracle.erode_composite(om, e4, xyz, oc4, *args4, nd)
    got = e4.copy(); pl.erode_composite(got, oc4, *args4)
    assert np.array_equal(got, ref4), int((got != ref4).sum())
    pl.close()


def test_tile_staging_route_agrees(TP, oracle, monkeypatch):
    """WO_TILE_LDS=1 (north_star's "neighbour cells staged into LDS": the neighbour window of a workgroup's tile copied into LDS for the
    receivers and thermal passes; measured no faster, off by default).  Same dataflow, same operations: the route must give the oracle's
    field bit for bit, ties included."""
    from planet_heightmap_generation_amd import sphere_mesh as S
    mesh, xyz, nd = S.build_sphere(300000, 0.75, 11)
    pl = TP.Planet(mesh, xyz, nd)
    pl.synthetic_terrain(11)
    e0 = pl.download()
    eq = (np.round(e0 * 64) / 64).astype(np.float32)
    om = oracle.Mesh(mesh.adjOffset, mesh.adjList)
    args = (10, 3e-4, 0.5, 1.0, 10, 1.16, 0.015, 2, 0.5)
    for field in (e0, eq):
        oc = (field <= 0).astype(np.uint8)
        ref = oracle.erode_composite(om, field, xyz, oc, *args, nd)
        for env in ({}, {"WO_TILE_LDS": "1"}):
            for k, v in env.items():
                monkeypatch.setenv(k, v)
            got = field.copy()
            pl.erode_composite(got, oc, *args)
            st = pl.last_erode_stats()
            for k in env:
                monkeypatch.delenv(k)
            assert np.array_equal(got, ref), (env, int((got != ref).sum()))
            assert st["solve_basin_passes"] == 10 and st["solve_basin_passes_with_leftovers"] == 0, (env, st)
    pl.close()


def test_relaxed_mode_runs_and_is_not_the_parity_path(TP, oracle, monkeypatch):
    """WO_RELAXED=full (SURVEY 7.3's roofline mode: one sort per flood, affine pointer-jumping solve with deferred deposition, Jacobi glacial
    carve) is a MEASUREMENT mode: it must run, say so in the stats, stay in the neighbourhood of the exact field — and differ from it (the
    default path is the exact one and equals the oracle; nothing relaxed is ever reported as parity)."""
    from planet_heightmap_generation_amd import sphere_mesh as S
    mesh, xyz, nd = S.build_sphere(200000, 0.75, 4)
    pl = TP.Planet(mesh, xyz, nd)
    pl.synthetic_terrain(4)
    e0, oc = pl.download(), pl.download_ocean()
    om = oracle.Mesh(mesh.adjOffset, mesh.adjList)
    args = (12, 3e-4, 0.5, 1.0, 12, 1.16, 0.015, 3, 0.5)
    ref = oracle.erode_composite(om, e0, xyz, oc, *args, nd)
    exact = e0.copy(); pl.erode_composite(exact, oc, *args)
    assert pl.last_erode_stats()["relaxed_full"] == 0.0
    check_cells("exact path beside the relaxed mode", exact, ref, ref.size)
    monkeypatch.setenv("WO_RELAXED", "full")
    relaxed = e0.copy(); pl.erode_composite(relaxed, oc, *args)
    st = pl.last_erode_stats()
    monkeypatch.delenv("WO_RELAXED")
    assert st["relaxed_full"] == 1.0 and st["sorts"] <= 3
    assert np.isfinite(relaxed).all() and np.array_equal(relaxed[oc != 0], e0[oc != 0])          # ocean cells untouched
    d = rms(relaxed, exact)
    print(f"relaxed vs exact: rms {d:.2e}, cells differing {int((relaxed != exact).sum())}")
    assert 0 < d < 0.05
    again = e0.copy(); pl.erode_composite(again, oc, *args)                                          # and the exact path is what it was
    assert np.array_equal(again, exact)
    pl.close()


def test_land_count_shrinks_and_grows_on_one_planet(TP, oracle):
    """Masks of very different land counts on ONE planet (what a rank of the landmass decomposition sees when plans change): a
    large land mass, then a few cells of land, then the large one again.  The in-tree radix sort keeps per-planet scratch whose
    two group-total buffers swap roles every pass (csrc/radix.hip); every call must still give the oracle's field."""
    from planet_heightmap_generation_amd import decomposed as D
    from planet_heightmap_generation_amd import sphere_mesh as S
    mesh, xyz, nd = S.build_sphere(120000, 0.75, 13)
    om = oracle.Mesh(mesh.adjOffset, mesh.adjList)
    e0 = oracle.synthetic_terrain(xyz, 13)
    oc = (e0 <= 0).astype(np.uint8)
    lab = D.land_components(mesh, oc)
    ids, cnt = np.unique(lab[lab >= 0], return_counts=True)
    small = ids[np.flatnonzero((cnt >= 3) & (cnt <= 200))[:1]]
    assert small.size == 1
    tiny = np.where(lab == small[0], 0, 1).astype(np.uint8)          # one small island is all the land there is
    args = (6, 3e-4, 0.5, 1.0, 6, 1.16, 0.015, 0, 0.0)
    pl = TP.Planet(mesh, xyz, nd)
    for mask in (oc, tiny, oc, tiny, oc):
        ref = oracle.erode_composite(om, e0, xyz, mask, *args, nd)
        got = e0.copy()
        pl.erode_composite(got, mask, *args)
        assert np.array_equal(got, ref), (int((mask == 0).sum()), int((got != ref).sum()))
    pl.close()


@pytest.mark.parametrize("cells,counts", [(20000, (2049, 4097, 2048, 4096)), (200000, (131072, 131073, 131072, 131073))])
def test_sorts_at_tile_and_group_boundaries(TP, oracle, cells, counts):
    """The land count L is the pair count of both sorts of an iteration.  L exactly one tile of select_active_by_rank (2 048) and of
    the radix sort (4 096: csrc/radix.hip), exactly one group of 32 radix tiles (131 072), and one pair more than each; the
    field is quantised to 1/64, so runs of equal keys cross the tile seams.  All counts of a mesh run on one planet, up, down and
    up again, which also crosses the rule that a sort starts on the group totals its predecessor cleared.  Bit for bit the C
    oracle without the glacial passes; with them (L = 4 097) on the per-cell bar of this file.  At 200 k cells the 131 072 highest
    cells reach below sea level (56 181 lie above it): the mask is not `elevation <= 0` there, and the flood's clamp at 0 lifts
    heights; this case found the chain form of the flood's pass 2 wrong on such land (46 014 cells off the oracle, fixed in
    flood_host.cc: tree_pass2_chains; without a GPU: test_emulated_kernels.py)."""
    from planet_heightmap_generation_amd import sphere_mesh as S
    mesh, xyz, nd = S.build_sphere(cells, 0.75, 4)
    om = oracle.Mesh(mesh.adjOffset, mesh.adjList)
    eq = (np.round(oracle.synthetic_terrain(xyz, 4) * 64) / 64).astype(np.float32)
    highest = np.argsort(-eq, kind="stable")
    assert np.unique(eq).size < 200, "thousands of equal keys"
    args = (3, 3e-4, 0.5, 1.0, 3, 1.16, 0.015, 0, 0.0)
    refs = {}
    pl = TP.Planet(mesh, xyz, nd)
    try:
        for L in counts:
            oc = np.ones(eq.size, np.uint8)
            oc[highest[:L]] = 0                                   # land is exactly the L highest cells
            assert int((oc == 0).sum()) == L
            if L not in refs:
                refs[L] = oracle.erode_composite(om, eq, xyz, oc, *args, nd)
                assert not np.array_equal(refs[L], eq)
            got = eq.copy()
            pl.erode_composite(got, oc, *args)
            print(f"{eq.size} cells, L = {L}: cells that differ from the oracle {int((got != refs[L]).sum())}")
            assert np.array_equal(got, refs[L]), (L, int((got != refs[L]).sum()))
        if 4097 in counts:
            glacial = args[:7] + (2, 0.5)
            oc = np.ones(eq.size, np.uint8)
            oc[highest[:4097]] = 0
            ref = oracle.erode_composite(om, eq, xyz, oc, *glacial, nd)
            got = eq.copy()
            pl.erode_composite(got, oc, *glacial)
            print(f"{eq.size} cells, L = 4097, two glacial passes: rms {rms(got, ref):.3e}, cells that differ {int((got != ref).sum())}")
            check_cells(f"{eq.size} cells, L = 4097, two glacial passes", got, ref, eq.size)
    finally:
        pl.close()


def test_decomposed_shares_when_some_shares_have_no_land(TP, oracle):
    """More shares than landmasses: the land-less shares' erodeComposite calls do nothing but answer the flood exchange (the same
    number of calls as everybody else).  Merged == oracle."""
    from planet_heightmap_generation_amd import decomposed as D
    from planet_heightmap_generation_amd import sphere_mesh as S
    mesh, xyz, nd = S.build_sphere(60000, 0.75, 8)
    om = oracle.Mesh(mesh.adjOffset, mesh.adjList)
    base = (np.round(oracle.synthetic_terrain(xyz, 8) * 512) / 512).astype(np.float32)            # quantised: equal keys matter
    lab = D.land_components(mesh, (base <= 0).astype(np.uint8))
    ids, cnt = np.unique(lab[lab >= 0], return_counts=True)
    keep = ids[np.argsort(-cnt)[:4]]                                                                 # only the four largest landmasses stay land
    e0 = np.where(np.isin(lab, keep), base, np.float32(-0.1)).astype(np.float32)
    oc = (e0 <= 0).astype(np.uint8)
    n_land = D.plan_landmasses(mesh, oc, 1).num_landmasses
    shares = 7
    assert 0 < n_land < shares
    args = (6, 3e-4, 0.5, 1.0, 6, 1.16, 0.015, 0, 0.0)
    ref = oracle.soil_creep(om, oracle.erode_composite(om, e0, xyz, oc, *args, nd), oc, 3, 0.1125)
    merged, stats, secs, plan = D.erode_shares_concurrently(TP, mesh, xyz, nd, e0, oc, shares, args, (3, 0.1125))
    assert any(c.size == 0 for c in plan.cells)
    assert np.array_equal(merged, ref), int((merged != ref).sum())



@pytest.mark.gpu
def test_flood_stage_inside_the_mirror_copies_the_land_only(TP, oracle, monkeypatch, capfd):
    """Inside the land-first mirror the flood stage copies the first L floats of the mirrored field — the land heights, in the host flood's
    own land order — instead of the whole field in the planet's order (flood.hip: flood_stage_land).  The first flood of a call after the
    mask changed takes the full route (it rebuilds the host tables), the second one and every flood of the calls that follow the land-only
    route (WO_FLOOD_TIMING names it on stderr); the field after 12 composite iterations must be the oracle's bit for bit, call after call."""
    from planet_heightmap_generation_amd import sphere_mesh as S
    mesh, xyz, nd = S.build_sphere(600_000, 0.75, 3)
    om = oracle.Mesh(mesh.adjOffset, mesh.adjList)
    e0 = oracle.warp_terrain(om, oracle.synthetic_terrain(xyz, 3), xyz, 3, 0.75)
    oc = (e0 <= 0).astype(np.uint8)
    ref = oracle.erode_composite(om, e0, xyz, oc, 12, 3e-4, 0.5, 1.0, 12, 1.16, 0.015, 0, 0.0, nd)
    monkeypatch.setenv("WO_FLOOD_TIMING", "1")
    pl = TP.Planet(mesh, xyz, nd)
    seen_land_only = 0
    for call in range(3):
        got = e0.copy()
        capfd.readouterr()
        pl.erode_composite(got, oc, 12, 3e-4, 0.5, 1.0, 12, 1.16, 0.015, 0, 0.0)
        log = capfd.readouterr().err
        assert int((got != ref).sum()) == 0, call
        seen_land_only += log.count("D2H (land)")
    assert seen_land_only >= 3, seen_land_only
    pl.close()


@pytest.mark.soak
@pytest.mark.isolated
@pytest.mark.timeout(1800)
def test_soak_hundred_planets_in_one_process(TP):
    """100 create / warp / erode / creep / download / destroy cycles of 10 M-cell planets in ONE process (round 5's GPU suite died with SIGABRT
    in its 61st test, ~50 planets into one interpreter, under the download's hipStreamSynchronize): 50 different terrains, each twice, 50 cycles
    apart — the second run of a seed must give the first run's bits (nothing of a destroyed planet leaks into a later one), the fields are finite,
    and the process does not grow (host RSS after cycle 100 within 1 GB of cycle 20)."""
    import zlib
    import psutil
    from planet_heightmap_generation_amd import sphere_mesh as S
    mesh, xyz, nd = S.build_sphere(10_000_000, 0.75, 1)
    me = psutil.Process()
    crcs, rss = [], []
    for k in range(100):
        seed = 100 + k % 50
        pl = TP.Planet(mesh, xyz, nd)
        pl.synthetic_terrain(seed)
        pl.warp_terrain_resident(seed, 0.75)
        pl.ocean_from_elevation()
        pl.erode_composite_resident(6, 3e-4, 0.5, 1.0, 6, 1.16, 0.015, 2, 0.5)      # both floods (iteration 0 and round(0.75 x 6)), 2 glacial steps
        pl.apply_soil_creep_resident(3, 0.1125)
        out = pl.download()
        pl.close()
        assert np.isfinite(out).all(), k
        crcs.append(int(zlib.crc32(out.tobytes())))
        rss.append(me.memory_info().rss)
        if k >= 50:
            assert crcs[k] == crcs[k - 50], (k, seed)
    assert len(set(crcs[:50])) == 50
    print(f"soak: 100 planets, rss after cycle 20 / 100: {rss[19] / 2**30:.2f} / {rss[99] / 2**30:.2f} GiB")
    assert rss[99] - rss[19] < (1 << 30)
