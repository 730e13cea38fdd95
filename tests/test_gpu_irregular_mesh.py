"""The HIP path on valid meshes the Fibonacci-sphere builder never makes (tests/irregular_mesh.py): hub cells of degree 9 .. 24, relabelled
cells and shuffled rows, against the CPU oracle on the same mesh.

The planet's largest degree picks the thermal apply kernel (csrc/erode.hip: k_thermal_apply_reg<12> up to 12, k_thermal_apply_reg<16>
for 13-16, the dynamic-LDS k_thermal_apply for 17-24, whose request passes 64 KiB from degree 22 on); rows longer than WO_EAGER_ROW = 12
take the long-row glacial carve (carve_granule_turn_long_row) and rows longer than WO_ROW = 8 the plain-loop forms.  Bars as in
test_gpu_parity.py: bit for bit where the device calls no libm; with glacial iterations or m != 0.5 (pow / asin on the device) the
per-cell bar of erode_common.check_cells: every cell within ERODE_ULP_BOUND * max(1, |ref|), at most max(8, N / 10^4) cells
different, RMS < 1e-5 (tests/test_erode_libm.py derives the bound)."""
import numpy as np
import pytest

import erode_common as EC
import irregular_mesh as IM
from erode_common import ERODE, PLANETS, erode_args
from hooks import del_hook, set_hook

pytestmark = pytest.mark.gpu

# PLANETS (largest degree -> cells, seed) and ERODE (the cases; h_m06 is the stream-power step with m = 0.6, K = 6e-4: pow(flow, m) on
# rows longer than WO_ROW) are erode_common's, shared with the CPU sensitivity test
ROUTES = {"default": {}, "index": {"WO_LAYOUT": "index"}, "tile_lds": {"WO_TILE_LDS": "1"}, "device_flood": {"WO_FLOOD": "device"}}


@pytest.fixture(scope="module")
def TP():
    from planet_heightmap_generation_amd import terrain_post
    return terrain_post


def rms(a, b):
    d = a.astype(np.float64) - b.astype(np.float64)
    return float(np.sqrt((d * d).mean()))


def set_route(monkeypatch, env):
    for k in ("WO_LAYOUT", "WO_TILE_LDS", "WO_FLOOD"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def check(got, ref, libm, what):
    """The bar of test_golden_cases: per cell (erode_common.check_cells, which prints its figures) where the device calls libm, else
    bit for bit; returns the report line still to be printed."""
    if libm:
        EC.check_cells(what, got, ref, got.size)
        return None
    nbad, r = int((got != ref).sum()), rms(got, ref)
    assert nbad == 0, (what, nbad, float(np.abs(got.astype(np.float64) - ref).max()))
    return f"{what}: non-identical cells {nbad}, rms {r:.2e}"


def touched(mesh, ref, e0, c):
    nb = mesh.adjList[mesh.adjOffset[c]:mesh.adjOffset[c + 1]]
    return bool(ref[c] != e0[c] or (ref[nb] != e0[nb]).any())


def planet(max_degree):
    N, seed = PLANETS[max_degree]
    return IM.hub_mesh(N, seed, max_degree)


@pytest.mark.timeout(300)
@pytest.mark.parametrize("max_degree", list(PLANETS))
def test_hub_planet_erode_matches_oracle(TP, oracle, monkeypatch, max_degree):
    hp = planet(max_degree)
    assert int(IM.degrees(hp.mesh).max()) == max_degree
    om = oracle.Mesh(hp.mesh.adjOffset, hp.mesh.adjList)
    long_hubs = hp.hubs[hp.hub_degrees > 12]
    carving = long_hubs[IM.carves_every_glacial_step(hp.xyz, hp.oc)[long_hubs]]
    pl = TP.Planet(hp.mesh, hp.xyz, hp.nd)
    report = []
    for case in ERODE:
        args = erode_args(case)
        ref = oracle.erode_composite(om, hp.e0, hp.xyz, hp.oc, *args, hp.nd)
        # the case must reach the long rows: a hub of degree > 12 changes under thermal; one that carves in every glacial step changes
        # (or a neighbour does) under glacial
        if case == "t_corner":
            assert (ref[long_hubs] != hp.e0[long_hubs]).any(), "no hub of degree > 12 changes in the thermal case"
        if case == "h_m06":
            assert (ref[hp.hubs] != hp.e0[hp.hubs]).any(), "no hub (rows longer than WO_ROW) changes in the m = 0.6 case"
        if case == "g":
            assert any(touched(hp.mesh, ref, hp.e0, int(c)) for c in carving), "no carving hub of degree > 12 in the glacial case"
        for route, env in ROUTES.items():
            set_route(monkeypatch, env)
            got = hp.e0.copy()
            pl.erode_composite(got, hp.oc, *args)
            st = pl.last_erode_stats()
            report.append(check(got, ref, EC.uses_libm(args), f"deg {max_degree} {case} {route}"))
            if route == "index":
                assert st["mirror_layout"] == 0.0, st
            if route == "device_flood" and args[0] > 0:
                assert st["flood_device_rounds"] > 0, st
            if args[7] > 0:
                assert st["carve_active_total"] > 0 and st["carve_flow_launches_with_leftovers"] == 0, (route, st)
    set_route(monkeypatch, {})
    print("\n".join(line for line in report if line))
    pl.close()


@pytest.mark.timeout(300)
def test_hub_planet_glacial_finisher(TP, oracle, monkeypatch):
    """test_glacial_step_one_launch_and_its_finisher on the degree-24 planet: the one-launch carve with its long-row turns, the synchronous
    rounds finishing from whatever state a launch that gives up at once left (carve_budget_ms=0), and a launch of two workgroups
    (carve_blocks=2).  All three give the same field."""
    hp = planet(24)
    om = oracle.Mesh(hp.mesh.adjOffset, hp.mesh.adjList)
    args = erode_args("g")
    ref = oracle.erode_composite(om, hp.e0, hp.xyz, hp.oc, *args, hp.nd)
    pl = TP.Planet(hp.mesh, hp.xyz, hp.nd)
    got = hp.e0.copy(); pl.erode_composite(got, hp.oc, *args)
    st = pl.last_erode_stats()
    assert st["carve_active_total"] > 0, st
    assert st["carve_flow_launches_with_leftovers"] == 0 and st["carve_rounds_total"] == args[7], st
    check(got, ref, True, "deg 24 glacial, one launch")
    set_hook(monkeypatch, "carve_budget_ms", 0)
    a = hp.e0.copy(); pl.erode_composite(a, hp.oc, *args)
    st = pl.last_erode_stats()
    del_hook(monkeypatch, "carve_budget_ms")
    assert st["carve_flow_launches_with_leftovers"] > 0 and st["carve_rounds_total"] > args[7], st
    assert np.array_equal(a, got), int((a != got).sum())
    set_hook(monkeypatch, "carve_blocks", 2)
    b = hp.e0.copy(); pl.erode_composite(b, hp.oc, *args)
    st = pl.last_erode_stats()
    del_hook(monkeypatch, "carve_blocks")
    assert st["carve_flow_launches_with_leftovers"] == 0 and st["carve_rounds_total"] == args[7], st
    assert np.array_equal(b, got), int((b != got).sum())
    pl.close()


@pytest.mark.timeout(300)
@pytest.mark.parametrize("max_degree", list(PLANETS))
def test_hub_planet_other_passes(TP, oracle, max_degree):
    from climate_common import sweep_inputs
    from planet_heightmap_generation_amd import climate_util as CU
    from test_climate_util import _run_sweeps
    hp = planet(max_degree)
    N, seed = PLANETS[max_degree]
    m = hp.mesh
    om = oracle.Mesh(m.adjOffset, m.adjList)
    pl = TP.Planet(m, hp.xyz, hp.nd)
    a = hp.e0.copy()
    pl.warp_terrain(a, seed, 0.75)
    assert np.array_equal(a, oracle.warp_terrain(om, hp.e0, hp.xyz, seed, 0.75)), "warp_terrain"
    for fn, ofn, args in (("smooth_elevation", "smooth_elevation", (2, 0.3)), ("sharpen_ridges", "sharpen_ridges", (3, 0.04)),
                          ("apply_soil_creep", "soil_creep", (3, 0.1125))):
        a = hp.e0.copy()
        getattr(pl, fn)(a, hp.oc, *args)
        b = getattr(oracle, ofn)(om, hp.e0, hp.oc, *args)
        assert np.array_equal(a, b), (fn, int((a != b).sum()))
    f = hp.e0.copy()
    CU.smooth_field(m, f, 3, planet=pl)
    assert np.array_equal(f, oracle.smooth_field(om, hp.e0, 3)), "smooth_field"
    inputs = sweep_inputs(m.adjOffset, m.adjList, hp.xyz, hp.e0)
    got = _run_sweeps(dict(diffuse=CU.diffuse_ocean_warmth, conv=CU.compute_wind_convergence, advect=CU.advect_moisture), m, hp.xyz, inputs,
                      dict(planet=pl))
    ref = _run_sweeps(dict(diffuse=oracle.diffuse_ocean_warmth, conv=oracle.wind_convergence, advect=oracle.advect_moisture), om, hp.xyz,
                      inputs, {})
    for k in ref:
        assert np.array_equal(got[k], ref[k]), (k, int((got[k] != ref[k]).sum()))
    pl.close()


@pytest.mark.timeout(300)
def test_degree_limit(TP):
    """WO_MAX_DEG = 24: a planet whose largest row has 24 entries is accepted, one with 25 is refused at creation."""
    from planet_heightmap_generation_amd import capi, sphere_mesh as S
    mesh, xyz, _ = S.build_sphere(5000, 0.75, 2)
    hub = 2500
    for deg in (24, 25):
        off, adj, nd = IM.add_hubs(mesh, xyz, [(hub, deg)], 1)
        m = IM.CsrMesh(off, adj)
        assert int(IM.degrees(m).max()) == deg
        if deg == 24:
            TP.Planet(m, xyz, nd).close()
        else:
            with pytest.raises(capi.WorogenError, match="exceeds the supported maximum"):
                TP.Planet(m, xyz, nd)


@pytest.mark.timeout(300)
@pytest.mark.parametrize("order", ["permuted", "permuted_rows_shuffled"])
def test_reordered_mesh_matches_oracle(TP, oracle, monkeypatch, order):
    """Cell ids in random order (the pole anywhere), and rows in random order as well: the mirror layout, the XCD tiling and the LDS window
    staging assume locality only for speed.  Against the oracle on the same mesh (the reference breaks ties by index, so not against
    the unpermuted run)."""
    from planet_heightmap_generation_amd import sphere_mesh as S
    mesh, xyz, _ = S.build_sphere(200000, 0.75, 8)
    m, p, nd = IM.permute_vertices(mesh, xyz, np.random.default_rng(8).permutation(mesh.numRegions))
    if order == "permuted_rows_shuffled":
        m = IM.shuffle_rows(m, 9)
        nd = S.compute_neighbor_dist(m, p)
    e0 = oracle.synthetic_terrain(p, 8)
    oc = (e0 <= 0).astype(np.uint8)
    om = oracle.Mesh(m.adjOffset, m.adjList)
    pl = TP.Planet(m, p, nd)
    report = []
    for case in ("ht", "hgt"):
        args = erode_args(case)
        ref = oracle.erode_composite(om, e0, p, oc, *args, nd)
        for route in ("default", "index", "tile_lds"):
            set_route(monkeypatch, ROUTES[route])
            got = e0.copy()
            pl.erode_composite(got, oc, *args)
            report.append(check(got, ref, EC.uses_libm(args), f"{order} {case} {route}"))
    set_route(monkeypatch, {})
    print("\n".join(line for line in report if line))
    pl.close()


SLIDERS = ("terrainWarp", "smoothing", "glacialErosion", "hydraulicErosion", "thermalErosion", "ridgeSharpening")
SLIDER_CORNERS = [{s: 1.0} for s in SLIDERS] + [{s: 1.0 for s in SLIDERS}, {}]


def js_round(x):
    return int(np.floor(x + 0.5))


def oracle_post(oracle, om, e0, xyz, nd, params, seed, hotspot):
    """runPostProcessing (js/planet-worker.js:40-102) composed from the oracle's passes, with the UI's slider mapping."""
    g = lambda k: float(params.get(k, 0.0))  # noqa: E731
    warp, smoothing, glac, hyd, therm, ridge = (g(k) for k in SLIDERS)
    r = oracle.warp_terrain(om, e0, xyz, seed, warp, hotspot) if warp > 0 else e0.copy()
    roc = (r <= 0).astype(np.uint8)
    pre = r.copy()
    if smoothing > 0:
        r = oracle.smooth_elevation(om, r, roc, js_round(1 + smoothing * 4), 0.2 + smoothing * 0.5)
    if glac > 0 or hyd > 0 or therm > 0:
        r = oracle.erode_composite(om, r, xyz, roc, js_round(hyd * 20), 0.0006 * hyd, 0.5, 1.0, js_round(therm * 10), 1.2 - therm * 0.4,
                                   therm * 0.15, js_round(glac * 10), glac, nd)
    if ridge > 0:
        r = oracle.sharpen_ridges(om, r, roc, js_round(1 + ridge * 3), ridge * 0.08)
    r = oracle.soil_creep(om, r, roc, 3, 0.1125)
    return roc, pre, r


@pytest.mark.timeout(300)
@pytest.mark.parametrize("where", ["post_N10000_s1", "hub_planet_deg22"])
def test_slider_corners_match_oracle_composition(TP, oracle, where):
    """test_pipeline_matches_oracle_composition at the sliders' corners: each slider alone at 1, all at 1, all at 0.  Thermal at 1 is
    talus 0.8 with kThermal 0.15, ten times the kThermal of the other GPU tests."""
    from conftest import load_golden
    if where.startswith("post_"):
        g = load_golden(where)
        m, xyz, nd, e0, hot = IM.CsrMesh(g["adjOffset"], g["adjList"]), g["xyz"], g["neighborDist"], g["elevation0"], g["hotspot"]
    else:
        hp = planet(22)
        m, xyz, nd, e0, hot = hp.mesh, hp.xyz, hp.nd, hp.e0, None
    om = oracle.Mesh(m.adjOffset, m.adjList)
    pl = TP.Planet(m, xyz, nd)
    report = []
    for params in SLIDER_CORNERS:
        e = e0.copy()
        oc, delta = TP.run_post_processing(pl, e, params, 1.0, hot)
        roc, pre, r = oracle_post(oracle, om, e0, xyz, nd, params, 1.0, hot)
        what = f"{where} {params or 'all at 0'}"
        assert np.array_equal(oc, roc), what
        glacial = params.get("glacialErosion", 0.0) > 0
        report.append(check(e, r, glacial, what))
        assert np.array_equal(delta, (e.astype(np.float64) - pre.astype(np.float64)).astype(np.float32)), what
        check(delta, (r.astype(np.float64) - pre.astype(np.float64)).astype(np.float32), glacial, what + " delta")
    print("\n".join(line for line in report if line))
    pl.close()
