"""Python mirror of the reference's plate projection step over the C ABI:

``project_coarse_plates(mesh, r_xyz, coarseMesh, coarse_xyz, coarse_r_plate, seed, numPlates)``
(js/coarse-plates.js:51-117) — HIP kernel, one thread per hi-res cell;
``smooth_and_reconnect_plates(mesh, r_plate, plateSeeds, numPasses)`` (js/plates.js:241-348) — native host stage
(order-defined in-place passes), mutates ``r_plate`` like the reference.

``generate_plates(mesh, r_xyz, numPlates, seed)`` (js/plates.js:6-232), ``assign_ocean_land(...)`` (js/ocean-land.js:7-238)
and ``generate_coarse_plates(seed, numPlates, numContinents, ...)`` (js/coarse-plates.js:19-38) — native host stages on the
fixed 20 000-cell mesh (RNG-ordered serial logic, no device part), bit for bit the reference's on the same mesh.
"""
from __future__ import annotations

import numpy as np

from . import capi
from .terrain_post import Planet, _planet_for

N_COARSE = 20000            # js/coarse-plates.js:11-12
COARSE_JITTER = 0.75
PLATES_GEN_STATS = ("governor_halved", "seeds_trimmed", "continent_at_target", "sea_absorbed", "sea_refused", "sea_two_continents",
                    "orphans")          # include/worogen.h: WO_PGS_*


def project_coarse_plates(mesh, r_xyz, coarseMesh, coarse_xyz, coarse_r_plate, seed, numPlates=None, planet: Planet | None = None) -> np.ndarray:
    pl = planet or _planet_for(mesh, r_xyz)
    c_off = np.ascontiguousarray(coarseMesh.adjOffset, np.int32)
    c_adj = np.ascontiguousarray(coarseMesh.adjList, np.int32)
    c_xyz = np.ascontiguousarray(coarse_xyz, np.float32)
    c_plate = np.ascontiguousarray(coarse_r_plate, np.int32)
    NC = int(coarseMesh.numRegions)
    if c_off.size != NC + 1 or c_xyz.size != 3 * NC or c_plate.size != NC:
        raise ValueError("coarse mesh / coarse_xyz / coarse_r_plate size mismatch")
    r_plate = np.empty(pl.numRegions, np.int32)
    capi.check(capi.lib().wo_project_coarse_plates(pl.handle, NC, capi.ptr(c_off), capi.ptr(c_adj), capi.ptr(c_xyz), capi.ptr(c_plate),
                                                   float(seed), -1 if numPlates is None else int(numPlates), capi.ptr(r_plate)),
               "wo_project_coarse_plates")
    return r_plate


def smooth_and_reconnect_plates(mesh, r_plate: np.ndarray, plateSeeds, numPasses: int) -> None:
    if not (isinstance(r_plate, np.ndarray) and r_plate.dtype == np.int32 and r_plate.flags.c_contiguous):
        raise TypeError("r_plate must be a contiguous int32 array (it is rewritten in place)")
    off = np.ascontiguousarray(mesh.adjOffset, np.int32)
    adj = np.ascontiguousarray(mesh.adjList, np.int32)
    if r_plate.size != off.size - 1:
        raise ValueError("r_plate length must equal mesh.numRegions")
    seeds = np.ascontiguousarray(list(plateSeeds), np.int32)
    capi.check(capi.lib().wo_smooth_reconnect_plates(int(mesh.numRegions), capi.ptr(off), capi.ptr(adj), capi.ptr(r_plate), capi.ptr(seeds),
                                                     int(seeds.size), int(numPasses)), "wo_smooth_reconnect_plates")


def _csr(mesh, what):
    off = np.ascontiguousarray(mesh.adjOffset, np.int32)
    adj = np.ascontiguousarray(mesh.adjList, np.int32)
    N = int(mesh.numRegions)
    if N < 1 or off.size != N + 1 or int(off[-1]) != adj.size:
        raise ValueError(f"{what}: mesh.adjOffset / adjList do not describe mesh.numRegions cells")
    return N, off, adj


def generate_plates(mesh, r_xyz, numPlates, seed, stats: dict | None = None):
    """generatePlates(mesh, r_xyz, numPlates, seed) -> (r_plate int32, plateSeeds list in Set order, plateVec {id: {pole, omega}}).
    `stats` (a dict) receives the branch counters of the call."""
    N, off, adj = _csr(mesh, "generate_plates")
    xyz = np.ascontiguousarray(r_xyz, np.float32).reshape(-1)
    if xyz.size != 3 * N:
        raise ValueError("generate_plates: r_xyz must hold 3 * mesh.numRegions floats")
    numPlates = int(numPlates)
    if numPlates < 1:
        raise ValueError("generate_plates: numPlates must be at least 1")
    cap = min(numPlates, N)
    r_plate = np.empty(N, np.int32)
    seeds = np.empty(cap, np.int32)
    pole = np.empty(3 * cap, np.float64)
    omega = np.empty(cap, np.float64)
    n = np.zeros(1, np.int32)
    st = np.zeros(len(PLATES_GEN_STATS), np.int64)
    capi.check(capi.lib().wo_generate_plates(N, capi.ptr(off), capi.ptr(adj), capi.ptr(xyz), numPlates, float(seed), capi.ptr(r_plate),
                                             capi.ptr(seeds), capi.ptr(n), capi.ptr(pole), capi.ptr(omega), capi.ptr(st)), "wo_generate_plates")
    P = int(n[0])
    if stats is not None:
        stats.update(zip(PLATES_GEN_STATS, st.tolist()))
    ids = seeds[:P].tolist()
    vec = {pid: {"pole": pole[3 * i:3 * i + 3].tolist(), "omega": float(omega[i])} for i, pid in enumerate(ids)}
    return r_plate, ids, vec


def assign_ocean_land(mesh, r_plate, plateSeeds, r_xyz, seed, numContinents, continentSizeVariety=0, landCoverage=0.3,
                      stats: dict | None = None) -> list:
    """assignOceanLand(...) -> the oceanic plate ids, in plateSeeds order (the reference's Set)."""
    N, off, adj = _csr(mesh, "assign_ocean_land")
    xyz = np.ascontiguousarray(r_xyz, np.float32).reshape(-1)
    rp = np.ascontiguousarray(r_plate, np.int32).reshape(-1)
    seeds = np.ascontiguousarray(list(plateSeeds), np.int32)
    if xyz.size != 3 * N or rp.size != N:
        raise ValueError("assign_ocean_land: r_xyz / r_plate do not match mesh.numRegions")
    if seeds.size < 1:
        raise ValueError("assign_ocean_land: plateSeeds is empty")
    flags = np.zeros(seeds.size, np.uint8)
    st = np.zeros(len(PLATES_GEN_STATS), np.int64)
    capi.check(capi.lib().wo_assign_ocean_land(N, capi.ptr(off), capi.ptr(adj), capi.ptr(rp), capi.ptr(seeds), int(seeds.size), capi.ptr(xyz),
                                               float(seed), int(numContinents), float(continentSizeVariety), float(landCoverage),
                                               capi.ptr(flags), capi.ptr(st)), "wo_assign_ocean_land")
    if stats is not None:
        stats.update(zip(PLATES_GEN_STATS, st.tolist()))
    return [int(p) for p, f in zip(seeds.tolist(), flags.tolist()) if f]


def generate_coarse_plates(seed, numPlates, numContinents, continentSizeVariety=0, landCoverage=0.3, stats: dict | None = None) -> dict:
    """generateCoarsePlates(seed, numPlates, numContinents, continentSizeVariety, landCoverage) -> the reference's six keys.
    The coarse mesh is build_sphere(20000, 0.75, seed + 137) with the pole fan numbered as the reference numbers it: the growth
    pushes neighbours in CSR row order, so the rows around the pole have to start where the reference's do."""
    from .sphere_mesh import build_sphere
    cmesh, cxyz, _ = build_sphere(N_COARSE, COARSE_JITTER, seed + 137, reference_closure=True)
    st1, st2 = {}, {}
    r_plate, seeds, vec = generate_plates(cmesh, cxyz, numPlates, seed, st1)
    ocean = assign_ocean_land(cmesh, r_plate, seeds, cxyz, seed, numContinents, continentSizeVariety, landCoverage, st2)
    if stats is not None:
        stats.update({k: st1[k] + st2[k] for k in PLATES_GEN_STATS})
    return {"coarseMesh": cmesh, "coarse_xyz": cxyz, "coarse_r_plate": r_plate, "coarsePlateSeeds": seeds, "coarsePlateVec": vec,
            "coarsePlateIsOcean": ocean}
