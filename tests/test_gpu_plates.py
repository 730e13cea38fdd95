"""k_plate_project (csrc/plates_ops.h, launched by wo_project_coarse_plates) per coarse cell on the MI355X.

With identity plates (plates_common.identity_plates) the call returns the coarse region each cell's walk ended on, so every
wrong walk shows, not only those across a plate border.  The device starts each walk from its 64 x 128 bucket grid; the reference
(oracle/plates_oracle.c, js/coarse-plates.js:51-117) walks serially, warm-started, gives up after ceil(sqrt(NC)) steps and scans.
Both must name the same region, cell for cell: at the fan of the closing pole vertex, on the grid's longitude seam, at z = +-1,
on coarse meshes of 21 to 80 001 regions, for every numPlates corner, at planet sizes around a block and at 500 003 cells, between
other calls that rewrite the planet's noise tables, and after refused calls.  All comparisons are exact (int32)."""
import ctypes as C
import gc
import re

import numpy as np
import pytest

import plates_common as PC
import wind_common as WC

pytestmark = pytest.mark.gpu


def device_project(pl, cmesh, cxyz, coarse_r_plate, seed, num_plates=None):
    from planet_heightmap_generation_amd import coarse_plates as CP
    return CP.project_coarse_plates(None, None, cmesh, cxyz, coarse_r_plate, seed, num_plates, planet=pl)


def check(got, want, what, where=None):
    assert got.dtype == np.int32
    bad = PC.mismatch(got, want, where)
    if bad:
        pytest.fail(f"{what}: {bad}", pytrace=False)


def in_use():
    """(device bytes, pinned bytes) the library holds in this process"""
    from planet_heightmap_generation_amd import capi
    d, h, n = C.c_int64(0), C.c_int64(0), C.c_int64(0)
    assert capi.lib().wo_memory_in_use(C.byref(d), C.byref(h), C.byref(n)) == 0
    return d.value, h.value


@pytest.mark.parametrize("seed", (7, 9, 1))
def test_identity_plates_match_reference_walk(seed):
    """Two coarse meshes no golden uses and the one of plates_N10000_s1_P80; Fibonacci cells, +z cap, -z cap and seam in one planet."""
    cmesh, cxyz = PC.coarse_mesh(20000, seed)
    xyz, where = PC.query_points(seed)
    ref, emu = PC.walk_answers(20000, seed, None)
    pl = PC.points_planet(xyz)
    try:
        got = device_project(pl, cmesh, cxyz, PC.identity_plates(cmesh.numRegions), seed, None)
    finally:
        pl.close()
    check(got, emu, "device against the emulator", where)
    check(got, ref, "device against the reference's walk", where)
    assert (got[where["cap+z"]] == cmesh.numRegions - 1).any(), "no cell of the +z cap ended on the pole vertex"


def test_num_plates_corners():
    """perturbAmp = coarseEdgeRad * (1.5 + lowPlateT), lowPlateT = clamp((80 - numPlates) / 60, 0, 1), 0 for null."""
    seed = 8
    cmesh, cxyz = PC.coarse_mesh(20000, seed)
    xyz, where = PC.query_points(seed)
    ident = PC.identity_plates(cmesh.numRegions)
    pl = PC.points_planet(xyz)
    try:
        got = {p: device_project(pl, cmesh, cxyz, ident, seed, p) for p in (None, 0, 20, 50, 80, 200)}
    finally:
        pl.close()
    for p in (None, 0, 50, 200):
        check(got[p], PC.walk_answers(20000, seed, p)[0], f"numPlates {p} against the reference's walk", where)
    check(got[20], got[0], "numPlates 20 against 0 (lowPlateT clamps at 1)", where)
    check(got[80], got[200], "numPlates 80 against 200 (lowPlateT 0)", where)
    check(got[200], got[None], "numPlates 200 against null", where)
    assert PC.mismatch(got[0], got[50]) and PC.mismatch(got[50], got[None]), "the amplitude did not change the answer: the corners test nothing"


@pytest.mark.parametrize("N", (3, 255, 256, 257, 4095, 4097))
def test_block_boundary_sizes(N):
    """Planets around one block of 256 threads and around 16 of them; the four query sets interleaved, so the pole fan and the
    seam are in the smallest one too."""
    seed = 10
    cmesh, cxyz = PC.coarse_mesh(20000, seed)
    q = PC.query_sets(seed)
    pool = np.stack([q[k][:1025] for k in ("cap+z", "seam", "fibonacci", "cap-z")], 1).reshape(-1, 3)        # interleaved
    xyz = np.ascontiguousarray(pool[:N]).reshape(-1)
    ident = PC.identity_plates(cmesh.numRegions)
    pl = PC.points_planet(xyz)
    try:
        got = device_project(pl, cmesh, cxyz, ident, seed, 12)
    finally:
        pl.close()
    assert got.shape == (N,)
    check(got, PC.emu_project_plates(xyz, cmesh, cxyz, ident, seed, 12), f"{N} cells against the emulator")


@pytest.mark.parametrize("n, seed, num_plates", ((20, 2, None), (80000, 6, 12)))
def test_coarse_sizes(n, seed, num_plates):
    """21 regions under 8192 start buckets; 80 001 regions, where the reference's walk stops after 283 steps and scans."""
    cmesh, cxyz = PC.coarse_mesh(n, seed)
    xyz, where = PC.query_points(seed)
    pl = PC.points_planet(xyz)
    try:
        got = device_project(pl, cmesh, cxyz, PC.identity_plates(cmesh.numRegions), seed, num_plates)
    finally:
        pl.close()
    check(got, PC.walk_answers(n, seed, num_plates)[0], f"{cmesh.numRegions} coarse regions against the reference's walk", where)


def test_scale_500k(oracle):
    """500 003 cells in index order: 1954 blocks of 256 threads, more than the device holds at once, the last one partly filled."""
    seed, N = 9, 500003
    cmesh, cxyz = PC.coarse_mesh(20000, seed)
    xyz = np.ascontiguousarray(PC.fib_points(N, 21)).reshape(-1)
    ident = PC.identity_plates(cmesh.numRegions)
    pl = PC.points_planet(xyz)
    try:
        got = device_project(pl, cmesh, cxyz, ident, 21, None)
    finally:
        pl.close()
    assert got.shape == (N,)
    check(got, PC.emu_project_plates(xyz, cmesh, cxyz, ident, 21, None), "500 003 cells against the emulator")
    check(got, PC.oracle_project_plates(oracle, xyz, cmesh, cxyz, ident, 21, None), "500 003 cells against the reference's walk")
    assert np.unique(got).size > 0.99 * cmesh.numRegions


def test_shared_tables_and_repeat_calls():
    """The projection, warpTerrain and computeWind each upload their own noise tables into the planet's one table buffer: a
    projection after either of them, and a warp after a projection, must equal what a fresh planet gives."""
    from planet_heightmap_generation_amd import wind as WD
    from planet_heightmap_generation_amd.terrain_post import Planet
    wc = WC.synthetic_case(20000)
    mesh = WC.Mesh(wc["off"], wc["adj"])
    cmesh, cxyz = PC.coarse_mesh(20000, 7)
    ident = PC.identity_plates(cmesh.numRegions)

    def project(pl):
        return device_project(pl, cmesh, cxyz, ident, 5, 50)

    def warp(pl):
        e = wc["e"].copy()
        pl.warp_terrain(e, 1, 0.75)
        return e

    fresh = Planet(mesh, wc["xyz"])
    try:
        want = project(fresh)
    finally:
        fresh.close()
    fresh = Planet(mesh, wc["xyz"])
    try:
        want_warp = warp(fresh)
    finally:
        fresh.close()
    assert PC.mismatch(want_warp, wc["e"]), "the warp changed nothing"
    check(want, PC.emu_project_plates(wc["xyz"], cmesh, cxyz, ident, 5, 50), "fresh planet against the emulator")
    pl = Planet(mesh, wc["xyz"])
    try:
        first = project(pl)
        warped = warp(pl)
        second = project(pl)
        WD.compute_wind(pl, wc["xyz"], wc["e"], set(int(i) for i in wc["ocean"]), wc["plate"], 3, fields=("r_pressure_summer",))
        third = project(pl)
    finally:
        pl.close()
    check(first, want, "first projection against a fresh planet's")
    assert WC.same_bits(warped, want_warp), f"warp after a projection: {int((warped != want_warp).sum())} cells differ from a fresh planet's warp"
    check(second, want, "projection after warpTerrain against a fresh planet's")
    check(third, want, "projection after computeWind against a fresh planet's")


def _broken_csr(cmesh, how):
    off, adj, NC = cmesh.adjOffset.copy(), cmesh.adjList.copy(), cmesh.numRegions
    if how == "offset0":
        off[0] = 1
    elif how == "monotone":
        off[10] = off[11] + 3
    elif how == "adjNC":
        adj[adj.size // 2] = NC
    elif how == "adjNeg":
        adj[-1] = -1
    m = WC.Mesh(off, adj)
    m.numRegions = NC
    return m


def test_refusals_leave_the_planet_usable():
    """The coarse CSR is validated on the host before anything is allocated: each refusal names its reason, leaves the library's
    memory where it was and the planet serving the next valid call."""
    from planet_heightmap_generation_amd import capi
    seed = 7
    cmesh, cxyz = PC.coarse_mesh(20000, seed)
    xyz, where = PC.query_points(seed)
    ident = PC.identity_plates(cmesh.numRegions)
    want = PC.walk_answers(20000, seed, None)[0]
    refusals = (("offset0", "wo_project_coarse_plates: coarseAdjOffset[0] != 0"), ("monotone", "wo_project_coarse_plates: coarseAdjOffset is not monotone"),
                ("adjNC", "wo_project_coarse_plates: coarseAdjList entry out of range"), ("adjNeg", "wo_project_coarse_plates: coarseAdjList entry out of range"))
    pl = PC.points_planet(xyz)
    try:
        gc.collect()
        for how, message in (("zero", "wo_project_coarse_plates: bad arguments"),) + refusals:
            before = in_use()
            with pytest.raises(capi.WorogenError, match=re.escape(message)):
                if how == "zero":                                   # coarseRegions = 0, every pointer valid
                    out = np.empty(pl.numRegions, np.int32)
                    capi.check(capi.lib().wo_project_coarse_plates(pl.handle, 0, capi.ptr(cmesh.adjOffset), capi.ptr(cmesh.adjList), capi.ptr(cxyz), capi.ptr(ident),
                                                                   float(seed), -1, capi.ptr(out)), "wo_project_coarse_plates")
                else:
                    device_project(pl, _broken_csr(cmesh, how), cxyz, ident, seed, None)
            after = in_use()
            print(f"refusal {how}: live (device, pinned) bytes {before} -> {after}")
            assert after == before, (how, before, after)
            check(device_project(pl, cmesh, cxyz, ident, seed, None), want, f"valid call after refusal {how}", where)
    finally:
        pl.close()


@pytest.mark.parametrize("name", PC.PLATE_CASES)
def test_golden_pipeline_through_identity(name):
    """coarse_r_plate[region the device finds] is the reference's recorded r_plate: ties the per-region answer to the goldens."""
    from planet_heightmap_generation_amd.terrain_post import Planet
    c = PC.plate_case(name)
    pl = Planet(c["mesh"], c["xyz"])
    try:
        idx = device_project(pl, c["cmesh"], c["cxyz"], PC.identity_plates(c["cmesh"].numRegions), c["meta"]["seed"], c["meta"]["P"])
    finally:
        pl.close()
    assert idx.min() >= 0 and idx.max() < c["cmesh"].numRegions
    check(np.ascontiguousarray(c["coarse_r_plate"], np.int32)[idx], np.ascontiguousarray(c["projected"], np.int32), f"{name}: coarse_r_plate[device region] against the golden")
