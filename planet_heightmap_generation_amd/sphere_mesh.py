"""Python mirror of the reference's mesh producer (js/sphere-mesh.js) over the C ABI.

``build_sphere(N, jitter, seed)`` is the counterpart of ``buildSphere(N, jitter, makeRng(seed))``
(js/sphere-mesh.js:174-186) plus ``computeNeighborDist`` (js/sphere-mesh.js:191-203); the returned
``SphereMesh`` exposes the three members the hot path reads: ``numRegions``, ``adjOffset``, ``adjList``
(js/sphere-mesh.js:144-145).
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from . import capi


@dataclass
class SphereMesh:
    numRegions: int
    triangles: np.ndarray    # int32 [numSides]
    halfedges: np.ndarray    # int32 [numSides]
    adjOffset: np.ndarray    # int32 [numRegions + 1]
    adjList: np.ndarray      # int32 [E]
    adjTriList: np.ndarray   # int32 [E]

    @property
    def numSides(self) -> int:
        return int(self.triangles.shape[0])

    @property
    def numTriangles(self) -> int:
        return self.numSides // 3


def fibonacci_sphere(N: int, jitter: float, seed: float, ctx=None) -> np.ndarray:
    """generateFibonacciSphere + appended pole: float32 [3*(N+1)] (js/sphere-mesh.js:9-37,179-181).  ctx: a terrain_post.Context
    makes the points on the device (wo_fib_sphere_points_device), one thread per point; None: the host loop."""
    xyz = np.empty(3 * (max(int(N), 0) + 1), dtype=np.float32)
    if ctx is not None:
        capi.check(capi.lib().wo_fib_sphere_points_device(ctx.handle, N, float(jitter), float(seed), capi.ptr(xyz)), "wo_fib_sphere_points_device")
        return xyz
    capi.check(capi.lib().wo_fib_sphere_points(N, float(jitter), float(seed), capi.ptr(xyz)), "wo_fib_sphere_points")
    return xyz


def device_sphere_from_seed(N: int, jitter: float, seed: float, reference_closure: bool, ctx):
    """Points and mesh in one device call (wo_sphere_mesh_seed_device): (SphereMesh, r_xyz, neighborDist).  The points are generated
    where the mesh stage reads them; the arrays are device_sphere_mesh's on those points."""
    V = int(N) + 1
    ns = max(3 * (2 * V - 4), 0)
    xyz = np.empty(3 * V, dtype=np.float32)
    tri, he = np.empty(ns, dtype=np.int32), np.empty(ns, dtype=np.int32)
    off = np.empty(V + 1, dtype=np.int32)
    adj, adjt, nd = np.empty(ns, dtype=np.int32), np.empty(ns, dtype=np.int32), np.empty(ns, dtype=np.float32)
    capi.check(capi.lib().wo_sphere_mesh_seed_device(ctx.handle, int(N), float(jitter), float(seed), 1 if reference_closure else 0, capi.ptr(xyz),
                                                     capi.ptr(tri), capi.ptr(he), capi.ptr(off), capi.ptr(adj), capi.ptr(adjt), capi.ptr(nd)),
               "wo_sphere_mesh_seed_device")
    E = int(off[-1])
    return SphereMesh(V, tri, he, off, adj[:E].copy(), adjt[:E].copy()), xyz, nd[:E].copy()


def device_sphere_mesh(r_xyz: np.ndarray, reference_closure: bool, ctx):
    """The whole mesh product in one device call (wo_sphere_mesh_device): (SphereMesh, neighborDist), every array equal to the host
    route's.  ctx: a terrain_post.Context."""
    r_xyz = np.ascontiguousarray(r_xyz, dtype=np.float32).reshape(-1)
    V = r_xyz.size // 3
    ns = max(3 * (2 * V - 4), 0)
    tri, he = np.empty(ns, dtype=np.int32), np.empty(ns, dtype=np.int32)
    off = np.empty(V + 1, dtype=np.int32)
    adj, adjt, nd = np.empty(ns, dtype=np.int32), np.empty(ns, dtype=np.int32), np.empty(ns, dtype=np.float32)
    capi.check(capi.lib().wo_sphere_mesh_device(ctx.handle, V, capi.ptr(r_xyz), 1 if reference_closure else 0, capi.ptr(tri), capi.ptr(he),
                                                capi.ptr(off), capi.ptr(adj), capi.ptr(adjt), capi.ptr(nd)), "wo_sphere_mesh_device")
    E = int(off[-1])
    return SphereMesh(V, tri, he, off, adj[:E].copy(), adjt[:E].copy()), nd[:E].copy()


def sphere_mesh_from_points(r_xyz: np.ndarray, reference_closure: bool = False, ctx=None) -> SphereMesh:
    """reference_closure: number the closing pole fan the way the reference's addPoleToMesh does (js/sphere-mesh.js:55-88).
    ctx: a terrain_post.Context sends the work to the device builder (the same arrays); None: the host builder.
    Raises capi.WorogenError (status 2) for points whose hull does not hold the sphere's centre strictly inside, e.g. points inside
    a hemisphere: they have no triangulation of the sphere."""
    if ctx is not None:
        return device_sphere_mesh(r_xyz, reference_closure, ctx)[0]
    r_xyz = np.ascontiguousarray(r_xyz, dtype=np.float32).reshape(-1)
    V = r_xyz.size // 3
    ns = 3 * (2 * V - 4)
    tri = np.empty(ns, dtype=np.int32)
    he = np.empty(ns, dtype=np.int32)
    L = capi.lib()
    capi.check(L.wo_sphere_delaunay(V, capi.ptr(r_xyz), capi.ptr(tri), capi.ptr(he)), "wo_sphere_delaunay")
    if reference_closure:
        capi.check(L.wo_sphere_reference_closure(V, capi.ptr(tri), capi.ptr(he)), "wo_sphere_reference_closure")
    return sphere_mesh_from_triangles(tri, he, V)


def sphere_mesh_from_triangles(tri: np.ndarray, he: np.ndarray, numRegions: int) -> SphereMesh:
    """new SphereMesh(triangles, halfedges, numRegions) (js/sphere-mesh.js:94-146)."""
    tri = np.ascontiguousarray(tri, dtype=np.int32)
    he = np.ascontiguousarray(he, dtype=np.int32)
    ns = tri.size
    off = np.empty(numRegions + 1, dtype=np.int32)
    adj = np.empty(ns, dtype=np.int32)
    adjt = np.empty(ns, dtype=np.int32)
    capi.check(capi.lib().wo_mesh_csr(numRegions, ns, capi.ptr(tri), capi.ptr(he), capi.ptr(off), capi.ptr(adj), capi.ptr(adjt)),
               "wo_mesh_csr")
    E = int(off[-1])
    return SphereMesh(numRegions, tri, he, off, adj[:E].copy(), adjt[:E].copy())


def compute_neighbor_dist(mesh: SphereMesh, r_xyz: np.ndarray) -> np.ndarray:
    out = np.empty(mesh.adjList.size, dtype=np.float32)
    r_xyz = np.ascontiguousarray(r_xyz, dtype=np.float32)
    capi.check(capi.lib().wo_neighbor_dist(mesh.numRegions, capi.ptr(mesh.adjOffset), capi.ptr(mesh.adjList),
                                           capi.ptr(r_xyz), capi.ptr(out)), "wo_neighbor_dist")
    return out


def build_sphere(N: int, jitter: float, seed: float, reference_closure: bool = False, ctx=None, device_points: bool = False):
    """Returns (mesh, r_xyz, neighborDist) for N requested cells (numRegions = N + 1).  ctx: as for sphere_mesh_from_points.
    device_points (needs ctx): the points are generated on the device too, in the same call (device_sphere_from_seed)."""
    if device_points:
        if ctx is None:
            raise ValueError("build_sphere: device_points needs a context")
        return device_sphere_from_seed(N, jitter, seed, reference_closure, ctx)
    xyz = fibonacci_sphere(N, jitter, seed)
    if ctx is not None:
        mesh, nd = device_sphere_mesh(xyz, reference_closure, ctx)
        return mesh, xyz, nd
    mesh = sphere_mesh_from_points(xyz, reference_closure)
    return mesh, xyz, compute_neighbor_dist(mesh, xyz)


def triangle_elevations(mesh: SphereMesh, r_elevation: np.ndarray) -> np.ndarray:
    out = np.empty(mesh.numTriangles, dtype=np.float32)
    r_elevation = np.ascontiguousarray(r_elevation, dtype=np.float32)
    capi.check(capi.lib().wo_triangle_elevations(mesh.numTriangles, capi.ptr(mesh.triangles), capi.ptr(r_elevation),
                                                 capi.ptr(out)), "wo_triangle_elevations")
    return out
