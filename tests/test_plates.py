"""Plate projection step: projectCoarsePlates (js/coarse-plates.js:51-117) and
smoothAndReconnectPlates (js/plates.js:241-348) against the reference's own outputs.  Plate ids are integers: exact."""
import ctypes as C

import numpy as np
import pytest

import plates_common as PC
from plates_common import PLATE_CASES, plate_case


def P(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


@pytest.mark.parametrize("name", PLATE_CASES)
def test_host_smooth_and_reconnect_matches_reference(name):
    """The native host stage needs no GPU: run it here through the C ABI's Python mirror."""
    from planet_heightmap_generation_amd import coarse_plates as CP
    c = plate_case(name)
    rp = c["projected"].copy()
    CP.smooth_and_reconnect_plates(c["mesh"], rp, c["seeds"], c["meta"]["passes"])
    assert np.array_equal(rp, c["smoothed"]), int((rp != c["smoothed"]).sum())


def test_host_smooth_edge_cases(oracle):
    """Fragmented plates, ties in component size, seed protection that applies (plate id == cell id) — vs the oracle."""
    from planet_heightmap_generation_amd import coarse_plates as CP
    from planet_heightmap_generation_amd import sphere_mesh as S
    mesh, xyz, _ = S.build_sphere(3000, 0.75, 11)
    N = mesh.numRegions
    om = oracle.Mesh(mesh.adjOffset, mesh.adjList)
    rng = np.random.default_rng(5)
    seeds = rng.choice(N, 12, replace=False).astype(np.int32)
    P3 = xyz.reshape(-1, 3).astype(np.float64)
    nearest = seeds[np.argmax(P3 @ P3[seeds].T, axis=1)].astype(np.int32)          # Voronoi plates: plate id = seed cell id
    for trial in range(4):
        rp = nearest.copy()
        flip = rng.random(N) < (0.05 + 0.1 * trial)                                 # salt-and-pepper fragments
        rp[flip] = seeds[rng.integers(0, seeds.size, flip.sum())]
        rp[seeds] = seeds                                                           # protected seeds
        for passes in (0, 1, 3):
            ref = oracle.smooth_reconnect_plates(om, rp, seeds, passes)
            mine = rp.copy()
            CP.smooth_and_reconnect_plates(mesh, mine, seeds, passes)
            assert np.array_equal(mine, ref), (trial, passes, int((mine != ref).sum()))


@pytest.mark.parametrize("name", PLATE_CASES[:2])
def test_emulated_projection_matches_reference(name):
    """The projection kernel body (csrc/plates_ops.h), driven cell by cell on the CPU."""
    c = plate_case(name)
    out = PC.emu_project_plates(c["xyz"], c["cmesh"], c["cxyz"], c["coarse_r_plate"], c["meta"]["seed"], c["meta"]["P"])
    assert np.array_equal(out, c["projected"]), int((out != c["projected"]).sum())


# ---- the start cell does not matter: oracle (warm start, sqrt(NC) cap, brute-force fallback) against the emulator (bucket
# grid start, NC cap) with identity plates, where every wrong walk shows.  Exact equality.
@pytest.mark.parametrize("num_plates", (None, 0, 50, 200))
@pytest.mark.parametrize("seed", PC.FRESH_SEEDS)
def test_identity_walk_is_start_independent_seeds(seed, num_plates):
    """Coarse meshes no golden uses; Fibonacci cells in index order, a 4 degree cap on the closing pole's fan (+z), a -z cap, the
    start grid's longitude seam.  perturbAmp is 2.5 coarse cells at numPlates 0, 2.0 at 50 and 1.5 at 200 and None."""
    ref, emu = PC.walk_answers(20000, seed, num_plates)
    _, where = PC.query_points(seed)
    assert ref.size == sum(n for _, n in PC.QUERY_SIZES) and max(n for _, n in PC.QUERY_SIZES) <= 50000
    assert not PC.mismatch(emu, ref, where), PC.mismatch(emu, ref, where)


@pytest.mark.parametrize("n, seed, num_plates", ((20, 2, None), (200, 2, 12), (2000, 4, None), (80000, 6, 12)))
def test_identity_walk_is_start_independent_sizes(n, seed, num_plates):
    """20 requested cells: 8192 start buckets over 21 regions; 80000: the reference gives up its walk after 283 steps."""
    ref, emu = PC.walk_answers(n, seed, num_plates)
    _, where = PC.query_points(seed)
    assert not PC.mismatch(emu, ref, where), PC.mismatch(emu, ref, where)
    assert np.unique(ref).size > (n + 1) * (0.9 if n <= 2000 else 0.05), "the query sets reach too few coarse regions to say anything"


@pytest.mark.parametrize("num_plates", (None, 0, 50, 200))
@pytest.mark.parametrize("seed", PC.FRESH_SEEDS)
def test_pole_cap_reaches_the_pole_vertex(seed, num_plates):
    """The +z cap is there for the fan of the closing pole vertex, region NC - 1: some of its cells must end on it, in the
    reference's answer and in the emulator's, or the cap tests nothing."""
    ref, emu = PC.walk_answers(20000, seed, num_plates)
    cap = PC.query_points(seed)[1]["cap+z"]
    NC = PC.coarse_mesh(20000, seed)[0].numRegions
    print(f"seed {seed}, numPlates {num_plates}: cells of the +z cap on the pole vertex {int((ref[cap] == NC - 1).sum())}, on its fan's regions in all {np.unique(ref[cap]).size}")
    assert (ref[cap] == NC - 1).any() and (emu[cap] == NC - 1).any()


@pytest.mark.gpu
@pytest.mark.parametrize("name", PLATE_CASES)
def test_gpu_projection_and_pipeline(name):
    """projectCoarsePlates on the device, then the host smoothing: both equal the reference's arrays."""
    from planet_heightmap_generation_amd import coarse_plates as CP
    from planet_heightmap_generation_amd.terrain_post import Planet
    c = plate_case(name)
    pl = Planet(c["mesh"], c["xyz"])
    rp = CP.project_coarse_plates(c["mesh"], c["xyz"], c["cmesh"], c["cxyz"], c["coarse_r_plate"], c["meta"]["seed"], c["meta"]["P"], planet=pl)
    assert np.array_equal(rp, c["projected"]), int((rp != c["projected"]).sum())
    CP.smooth_and_reconnect_plates(c["mesh"], rp, c["seeds"], c["meta"]["passes"])
    assert np.array_equal(rp, c["smoothed"])
    pl.close()


@pytest.mark.gpu
def test_gpu_projection_null_plate_count(oracle):
    """numPlates == null (lowPlateT = 0) and a start grid that must not matter: compare with the oracle's warm-started walk."""
    from planet_heightmap_generation_amd import coarse_plates as CP
    c = plate_case(PLATE_CASES[2])
    om, oc = oracle.Mesh(c["mesh"].adjOffset, c["mesh"].adjList), oracle.Mesh(c["cmesh"].adjOffset, c["cmesh"].adjList)
    ref = oracle.project_coarse_plates(om, c["xyz"], oc, c["cxyz"], c["coarse_r_plate"], 77, None)
    rp = CP.project_coarse_plates(c["mesh"], c["xyz"], c["cmesh"], c["cxyz"], c["coarse_r_plate"], 77, None)
    assert np.array_equal(rp, ref), int((rp != ref).sum())
