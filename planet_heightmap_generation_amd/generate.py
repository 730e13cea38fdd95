"""handleGenerate (js/planet-worker.js:136-339) without the message layer and without climate: a seed becomes a planet.

``generate_planet(ctx, N, P, jitter, nMag, numContinents, sliders, seed, ...)`` runs the reference's chain on one resident
``Planet``: native mesh (pole fan numbered as the reference numbers it), neighbour distances, triangle centres,
``generate_coarse_plates`` (host), ``project_coarse_plates`` (device), ``smooth_and_reconnect_plates(…, 3)`` (host), the toggled
plates, the three density tables, ``build_super_plates`` when P >= 8, ``assign_elevation``, ``run_post_processing_resident`` with
the call's hotspot layer, triangle elevations.  From assign_elevation on the field stays in HBM; the pre-erosion field is the
planet's saved state (W.prePostElev), so a reapply works on the returned planet.  Climate is the caller's next step
(``skipClimate`` is reported as True and the climate fields are absent), as for the worker's other commands.

The new logic of this chain (plate generation, ocean / land) is serial host code of a few milliseconds; the chain has no kernel of
its own.
"""
from __future__ import annotations

import math
import random
import time

import numpy as np

from . import coarse_plates as CP
from . import elevation as EL
from . import sphere_mesh as SM
from . import super_plates as SP
from . import terrain_post as TP
from .heightmap_import import triangle_centers

_SLIDERS = ("smoothing", "hydraulicErosion", "thermalErosion", "ridgeSharpening", "glacialErosion", "terrainWarp")


def _park_miller(seed: float):
    """makeRng(seed) (js/rng.js:3-6)."""
    s = math.fmod(abs(math.floor(seed * 9301 + 49297)), 2147483646) + 1

    def draw():
        nonlocal s
        s = (s * 16807) % 2147483647
        return (s - 1) / 2147483646
    return draw


def plate_densities(plateSeeds, plateIsOcean):
    """The three density tables of handleGenerate (:193-201): per plate makeRng(id + 777), first draw oceanic, second continental."""
    ocean = set(plateIsOcean)
    dens, land, oc = {}, {}, {}
    for r in plateSeeds:
        draw = _park_miller(r + 777)
        oc[r] = 3.0 + draw() * 0.5
        land[r] = 2.4 + draw() * 0.5
        dens[r] = oc[r] if r in ocean else land[r]
    return dens, land, oc


def generate_planet(ctx, N, P, jitter, nMag, numContinents, sliders: dict, seed=None, continent_size_variety=0, land_coverage=0.3,
                    toggled_indices=(), device_mesh=False, device_points=False):
    """Returns (planet, result): the resident Planet (caller closes it) and the fields of the reference's `done` message.
    device_mesh: the mesh and the neighbour distances come from the device builder (the same arrays) instead of the host's.
    device_points: the points come from the device as well, in the same call (the same floats); implies device_mesh."""
    N, P = int(N), int(P)
    if N < 1 or P < 1:
        raise ValueError("generate_planet: N and P must be positive integers")
    seed = random.randrange(16777216) if seed is None else seed
    spread = 5
    timing = []

    def lap(stage, t0):
        timing.append(dict(stage=stage, ms=(time.perf_counter() - t0) * 1e3))

    t_total = time.perf_counter()
    t0 = time.perf_counter()
    device_mesh = bool(device_mesh or device_points)
    if device_points:
        mesh, xyz, nd = SM.device_sphere_from_seed(N, float(jitter), float(seed), True, ctx if ctx is not None else TP.default_context())
    else:
        xyz = SM.fibonacci_sphere(N, float(jitter), float(seed))
        if device_mesh:
            mesh, nd = SM.device_sphere_mesh(xyz, True, ctx if ctx is not None else TP.default_context())
        else:
            mesh = SM.sphere_mesh_from_points(xyz, reference_closure=True)
    lap("Sphere mesh (Fibonacci + Delaunay + pole)", t0)
    t0 = time.perf_counter()
    if not device_mesh:
        nd = SM.compute_neighbor_dist(mesh, xyz)
    lap("Neighbor distances", t0)
    t0 = time.perf_counter()
    t_xyz = triangle_centers(mesh, xyz)
    lap("Triangle centers", t0)

    t0 = time.perf_counter()
    co = CP.generate_coarse_plates(seed, P, numContinents, continent_size_variety, land_coverage)
    lap(f"Coarse plates ({P} plates, {numContinents} continents)", t0)

    planet = TP.Planet(mesh, xyz, nd, ctx=ctx)
    try:
        t0 = time.perf_counter()
        r_plate = CP.project_coarse_plates(mesh, xyz, co["coarseMesh"], co["coarse_xyz"], co["coarse_r_plate"], seed, P, planet=planet)
        lap("Project coarse → hi-res", t0)
        t0 = time.perf_counter()
        plateSeeds = list(co["coarsePlateSeeds"])
        CP.smooth_and_reconnect_plates(mesh, r_plate, plateSeeds, 3)
        lap("Smooth projected plates", t0)

        plateVec = co["coarsePlateVec"]
        original = list(co["coarsePlateIsOcean"])
        is_ocean = list(original)                       # a Set in insertion order: delete removes, add appends
        for i in toggled_indices or ():
            if i < len(plateSeeds):
                r = plateSeeds[i]
                if r in is_ocean:
                    is_ocean.remove(r)
                else:
                    is_ocean.append(r)
        dens, dens_land, dens_ocean = plate_densities(plateSeeds, is_ocean)
        noise = EL.SimplexNoise(seed)

        sup = None
        if P >= 8:
            t0 = time.perf_counter()
            sup = SP.build_super_plates(mesh, r_plate, plateSeeds, plateVec, is_ocean, dens, planet=planet)
            lap(f"Super plates ({sup['numSuperPlates']} groups from {P} plates)", t0)

        t0 = time.perf_counter()
        el = EL.assign_elevation(mesh, xyz, is_ocean, r_plate, plateVec, plateSeeds, noise, nMag, seed, spread, dens, sup, planet=planet)
        lap("Elevation (collisions + stress + distance fields + assignment)", t0)
        pre = el["r_elevation"]

        t0 = time.perf_counter()
        planet.save_state()                              # W.prePostElev, device copy: assign_elevation left the field resident
        planet.upload_hotspot(el["debugLayers"]["hotspot"])
        params = {k: sliders.get(k, 0) for k in _SLIDERS}
        r_elevation, delta, post_timing = TP.run_post_processing_resident(planet, params, seed, True)
        lap("Terrain post-processing (total)", t0)
        debug = dict(el["debugLayers"])
        debug["erosionDelta"] = delta

        t0 = time.perf_counter()
        t_elevation = SM.triangle_elevations(mesh, r_elevation)
        lap("Triangle elevations", t0)
        lap("Clone state for retention", time.perf_counter())

        result = dict(type="done", triangles=mesh.triangles, halfedges=mesh.halfedges, numRegions=mesh.numRegions, r_xyz=xyz, t_xyz=t_xyz,
                      r_plate=r_plate, plateSeeds=plateSeeds, plateVec=plateVec, plateIsOcean=is_ocean, originalPlateIsOcean=original,
                      plateDensity=dens, plateDensityLand=dens_land, plateDensityOcean=dens_ocean, prePostElev=pre, r_elevation=r_elevation,
                      t_elevation=t_elevation, mountain_r=el["mountain_r"], coastline_r=el["coastline_r"], ocean_r=el["ocean_r"],
                      r_stress=el["r_stress"], skipClimate=True, seed=seed, nMag=nMag, debugLayers=debug, _timing=el["_timing"],
                      _pipelineTiming=timing, _postTiming=post_timing, _workerTotal=(time.perf_counter() - t_total) * 1e3,
                      _params=dict(N=N, P=P, jitter=jitter, nMag=nMag, numContinents=numContinents, smoothing=params["smoothing"],
                                   terrainWarp=params["terrainWarp"], hydraulicErosion=params["hydraulicErosion"],
                                   thermalErosion=params["thermalErosion"], ridgeSharpening=params["ridgeSharpening"],
                                   glacialErosion=params["glacialErosion"], continentSizeVariety=continent_size_variety, temperatureOffset=0,
                                   precipitationOffset=0, landCoverage=land_coverage, seed=seed),
                      mesh=mesh, neighborDist=nd)
        return planet, result
    except BaseException:
        planet.close()
        raise
