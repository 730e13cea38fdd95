"""Heightmap import (js/planet-worker.js:682-940) over the C ABI: the reference's names, snake-cased, on a device-resident planet.

``sample_heightmap`` / ``derive_synthetic_plates`` / ``classify_regions`` are the reference's ``sampleHeightmap`` /
``deriveSyntheticPlates`` / the region classification of handleImportHeightmap (:811-831); all three run in HIP kernels
(csrc/heightmap.hip) and are bit-identical to the reference (csrc/import_ops.h).  ``import_heightmap`` is the worker's
``importHeightmap`` handler without the message layer: it returns the fields of the reference's ``done`` message.  Climate
is not run (``skipClimate`` is always true), as for ``reapply``.
"""
from __future__ import annotations

import random
import time

import numpy as np

from . import capi
from . import sphere_mesh as SM
from . import terrain_post as TP


def check_image(gray, W, H) -> np.ndarray:
    """The grayscale image as a C-contiguous uint8 array of W*H pixels; refused before any device work otherwise."""
    W, H = int(W), int(H)
    if W <= 0 or H <= 0:
        raise ValueError(f"image size {W}x{H}: width and height must be positive")
    if W * H > 2**31 - 1:
        raise ValueError(f"image size {W}x{H}: more than 2^31 - 1 pixels")
    if not isinstance(gray, np.ndarray) or gray.dtype != np.uint8:
        raise TypeError("the grayscale image must be a uint8 array (Uint8Array / Uint8ClampedArray in the reference)")
    g = np.ascontiguousarray(gray).reshape(-1)
    if g.size != W * H:
        raise ValueError(f"the grayscale image has {g.size} pixels, expected {W}x{H} = {W * H}")
    return g


def sample_heightmap(planet: TP.Planet, gray, W, H, download: bool = True) -> np.ndarray | None:
    """sampleHeightmap(mesh, r_xyz, imageData, imgW, imgH) on the planet's r_xyz.  The result becomes the resident r_elevation
    (and r_isOcean = r_elevation <= 0); returned as float32 [numRegions] unless download is False."""
    g = check_image(gray, W, H)
    out = np.empty(planet.numRegions, np.float32) if download else None
    capi.check(capi.lib().wo_sample_heightmap(planet.handle, capi.ptr(g), int(W), int(H), capi.ptr(out)), "sampleHeightmap")
    return out


def derive_synthetic_plates(planet: TP.Planet) -> dict:
    """deriveSyntheticPlates(mesh, r_elevation) on the resident field: {r_plate, plateSeeds, plateIsOcean, plateVec}; the two
    Sets as int32 arrays in insertion order (ascending id), plateVec[seed] = [0, 0, 0]."""
    n = planet.numRegions
    r_plate, seeds, is_ocean = np.empty(n, np.int32), np.empty(n, np.int32), np.empty(n, np.uint8)
    count = np.zeros(1, np.int32)
    capi.check(capi.lib().wo_synthetic_plates(planet.handle, capi.ptr(r_plate), capi.ptr(seeds), capi.ptr(is_ocean), capi.ptr(count)),
               "deriveSyntheticPlates")
    k = int(count[0])
    seeds = seeds[:k].copy()
    return dict(r_plate=r_plate, plateSeeds=seeds, plateIsOcean=seeds[is_ocean[:k] != 0], plateVec={int(s): [0, 0, 0] for s in seeds})


def classify_regions(planet: TP.Planet) -> dict:
    """mountain_r / coastline_r / ocean_r of the resident field (js/planet-worker.js:811-831), int32 arrays in ascending id."""
    n = planet.numRegions
    lists = [np.empty(n, np.int32) for _ in range(3)]
    counts = np.zeros(3, np.int32)
    capi.check(capi.lib().wo_classify_regions(planet.handle, *(capi.ptr(a) for a in lists), capi.ptr(counts)), "classifyRegions")
    return {k: a[: int(c)].copy() for k, a, c in zip(("mountain_r", "coastline_r", "ocean_r"), lists, counts)}


def triangle_centers(mesh, r_xyz) -> np.ndarray:
    """generateTriangleCenters(mesh, r_xyz) (js/sphere-mesh.js:206-219): float32 [3*numTriangles]."""
    out = np.empty(3 * mesh.numTriangles, np.float32)
    xyz = np.ascontiguousarray(r_xyz, np.float32)
    capi.check(capi.lib().wo_triangle_centers(mesh.numTriangles, capi.ptr(mesh.triangles), capi.ptr(xyz), capi.ptr(out)), "generateTriangleCenters")
    return out


_SLIDERS = ("smoothing", "hydraulicErosion", "thermalErosion", "ridgeSharpening", "glacialErosion", "terrainWarp")


def import_heightmap(N, jitter, gray, W, H, params: dict, seed=None, planet_out: list | None = None, device_mesh=False,
                     device_points=False) -> dict:
    """handleImportHeightmap (js/planet-worker.js:771-940) without the message layer and without climate: the fields of the
    reference's `done` message.  The planet stays resident (W.prePostElev is its saved state) and is appended to planet_out
    when a list is given, so that a following reapply works on it; otherwise it is closed.  device_mesh: the mesh and the
    neighbour distances come from the device builder (the same arrays) instead of the host's.  device_points: the points come from
    the device as well, in the same call (the same floats); implies device_mesh."""
    g = check_image(gray, W, H)
    seed = random.randrange(16777216) if seed is None else seed
    timing = []

    def lap(stage, t0):
        timing.append(dict(stage=stage, ms=(time.perf_counter() - t0) * 1e3))

    t_total = time.perf_counter()
    t0 = time.perf_counter()
    device_mesh = bool(device_mesh or device_points)
    if device_points:
        mesh, xyz, nd = SM.device_sphere_from_seed(int(N), float(jitter), float(seed), False, TP.default_context())
    else:
        xyz = SM.fibonacci_sphere(int(N), float(jitter), float(seed))
        if device_mesh:
            mesh, nd = SM.device_sphere_mesh(xyz, False, TP.default_context())
        else:
            mesh = SM.sphere_mesh_from_points(xyz)
    lap("Sphere mesh", t0)
    t0 = time.perf_counter()
    if not device_mesh:
        nd = SM.compute_neighbor_dist(mesh, xyz)
    lap("Neighbor distances", t0)
    t0 = time.perf_counter()
    t_xyz = triangle_centers(mesh, xyz)
    lap("Triangle centers", t0)
    planet = TP.Planet(mesh, xyz, nd)
    try:
        t0 = time.perf_counter()
        pre = sample_heightmap(planet, g, W, H)
        planet.save_state()                                   # W.prePostElev, device copy
        lap("Sample heightmap", t0)
        t0 = time.perf_counter()
        r_elevation, delta, post_timing = TP.run_post_processing_resident(planet, params, seed)
        lap("Terrain post-processing", t0)
        t0 = time.perf_counter()
        plates = derive_synthetic_plates(planet)
        lap("Synthetic plates", t0)
        regions = classify_regions(planet)
        t0 = time.perf_counter()
        t_elevation = SM.triangle_elevations(mesh, r_elevation)
        lap("Triangle elevations", t0)
        lap("Clone state for retention", time.perf_counter())
        p = {k: params.get(k, 0) for k in _SLIDERS}
        return dict(type="done", triangles=mesh.triangles, halfedges=mesh.halfedges, numRegions=mesh.numRegions, r_xyz=xyz, t_xyz=t_xyz,
                    r_plate=plates["r_plate"], plateSeeds=plates["plateSeeds"], plateVec=plates["plateVec"], plateIsOcean=plates["plateIsOcean"],
                    originalPlateIsOcean=plates["plateIsOcean"].copy(), plateDensity={}, plateDensityLand={}, plateDensityOcean={},
                    prePostElev=pre, r_elevation=r_elevation, t_elevation=t_elevation, **regions,
                    r_stress=np.zeros(mesh.numRegions, np.float32), skipClimate=True, seed=seed, nMag=0,
                    debugLayers=dict(erosionDelta=delta), _timing=[], _pipelineTiming=timing, _postTiming=post_timing,
                    _workerTotal=(time.perf_counter() - t_total) * 1e3,
                    _params=dict(N=N, P=0, jitter=jitter, nMag=0, numContinents=0, smoothing=p["smoothing"], terrainWarp=p["terrainWarp"],
                                 hydraulicErosion=p["hydraulicErosion"], thermalErosion=p["thermalErosion"],
                                 ridgeSharpening=p["ridgeSharpening"], glacialErosion=p["glacialErosion"], seed=seed),
                    )
    finally:
        if planet_out is not None:
            planet_out.append(planet)
        else:
            planet.close()
