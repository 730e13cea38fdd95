"""Shared by the plate-projection tests: rebuilds the meshes of a plates_* golden case with the build's mesh producer
(checked against the checksums the reference harness recorded) and returns everything a call needs.

The second half serves the per-coarse-cell tests (test_plates.py, test_gpu_plates.py): with identity_plates every coarse region
is its own plate, so the projection returns the coarse region each walk ended on and any wrong walk shows.  The query sets put
cells where the coarse mesh and the start grid are not generic: the fan of the closing pole vertex at +z, the -z band, and the
start grid's longitude seam atan2(y, x) = +-pi on the -x meridian."""
import ctypes as C
import json
import subprocess
import zlib
from functools import lru_cache

import numpy as np

from conftest import REPO, load_golden

PLATE_CASES = ("plates_N10000_s1_P80", "plates_N5000_s3_P24", "plates_N200000_s5_P12")
FRESH_SEEDS = (7, 8, 9, 10)          # coarse meshes reference_mesh(20000, 0.75, s + 137) that no golden uses (those: 1, 3, 5)
CAP_DEGREES = 4.0
_emu = None


def _crc(a):
    return zlib.crc32(np.ascontiguousarray(a).tobytes())


def reference_mesh(N, jitter, seed):
    """The mesh the reference's buildSphere makes when its Delaunay provider returns the build's triangulation: the
    planar part of our closed triangulation (pole fan removed, hull half-edges -1) closed again the reference's way
    (js/sphere-mesh.js:55-88 addPoleToMesh numbers the pole triangles along the hull walk), then our CSR builder."""
    from planet_heightmap_generation_amd import sphere_mesh as S
    xyz = S.fibonacci_sphere(N, jitter, seed)
    m0 = S.sphere_mesh_from_points(xyz)
    tri = m0.triangles.reshape(-1, 3)
    keep = ~(tri == N).any(axis=1)
    new_id = np.full(tri.shape[0], -1, np.int64)
    new_id[keep] = np.arange(keep.sum())
    t2 = tri[keep].reshape(-1).astype(np.int32)
    old_sides = (np.nonzero(keep)[0][:, None] * 3 + np.arange(3)[None, :]).reshape(-1)
    h_old = m0.halfedges[old_sides]
    h2 = np.where(new_id[h_old // 3] >= 0, new_id[h_old // 3] * 3 + h_old % 3, -1).astype(np.int32)
    num_sides = t2.size
    unpaired = np.flatnonzero(h2 == -1)
    point_to_side = {int(t2[s]): int(s) for s in unpaired}          # later sides overwrite earlier ones, as in the reference
    nu = unpaired.size
    nt = np.concatenate([t2, np.zeros(3 * nu, np.int32)])
    nh = np.concatenate([h2, np.zeros(3 * nu, np.int32)])
    nxt = lambda s: s - 2 if s % 3 == 2 else s + 1
    s = int(unpaired[-1])
    for i in range(nu):
        ns = num_sides + 3 * i
        nh[s] = ns; nh[ns] = s
        nt[ns] = nt[nxt(s)]; nt[ns + 1] = nt[s]; nt[ns + 2] = N
        k = num_sides + (3 * i + 4) % (3 * nu)
        nh[ns + 2] = k; nh[k] = ns + 2
        s = point_to_side[int(nt[nxt(s)])]
    return S.sphere_mesh_from_triangles(nt, nh, N + 1), xyz


@lru_cache(maxsize=None)
def plate_case(name):
    g = load_golden(name)
    meta = json.loads(bytes(g["meta_json"]).decode())
    mesh, xyz = reference_mesh(meta["N"], 0.75, meta["seed"])
    cmesh, cxyz = reference_mesh(20000, 0.75, meta["seed"] + 137)              # js/coarse-plates.js:20-21
    for key, arr in (("xyz", xyz), ("adjOffset", mesh.adjOffset), ("adjList", mesh.adjList), ("coarse_xyz", cxyz),
                     ("coarse_adjOffset", cmesh.adjOffset), ("coarse_adjList", cmesh.adjList)):
        assert _crc(arr) == meta["crc_" + key], f"{name}: rebuilt {key} differs from what the reference saw"
    return dict(meta=meta, mesh=mesh, xyz=xyz, cmesh=cmesh, cxyz=cxyz, coarse_r_plate=g["coarse_r_plate"], seeds=g["plateSeeds"],
                projected=g["r_plate_projected"], smoothed=g["r_plate_smoothed"])


# ---------------------------------------------------------------- per coarse cell: identity plates, edge query sets ----
class PointsMesh:
    """A mesh over arbitrary positions: the ring of import_common.ring_csr (the projection reads positions only)."""

    def __init__(self, n):
        from import_common import ring_csr
        self.adjOffset, self.adjList = ring_csr(n)
        self.numRegions = n


@lru_cache(maxsize=None)
def coarse_mesh(n, seed):
    """(coarse mesh, coarse_xyz) the way js/coarse-plates.js:20-21 builds them for generation seed `seed`, with n requested cells
    (the reference always asks for 20000); numRegions = n + 1, the last region is the closing pole vertex at (0, 0, 1)."""
    return reference_mesh(n, 0.75, seed + 137)


def identity_plates(NC):
    return np.arange(NC, dtype=np.int32)


def fib_points(n, seed):
    """n jittered Fibonacci points in index order, float32 [n, 3] (the last one is the pole the mesh builder appends)."""
    from planet_heightmap_generation_amd import sphere_mesh as S
    return S.fibonacci_sphere(n - 1, 0.75, seed).reshape(-1, 3)


def cap_points(rng, n, axis, degrees):
    """n float32 unit vectors uniform in the spherical cap of `degrees` around `axis` ('+x', '-x', '+y', '-y', '+z', '-z')."""
    c = rng.uniform(np.cos(np.radians(degrees)), 1.0, n)
    s, phi = np.sqrt(1.0 - c * c), rng.uniform(0.0, 2.0 * np.pi, n)
    local = np.stack([s * np.cos(phi), s * np.sin(phi), c], 1)                    # cap around +z
    k = "xyz".index(axis[1])
    out = np.empty_like(local)
    out[:, k], out[:, (k + 1) % 3], out[:, (k + 2) % 3] = local[:, 2], local[:, 0], local[:, 1]
    if axis[0] == "-":
        out = -out
    return np.ascontiguousarray(out, np.float32)


def seam_points(n):
    """n float32 points on and next to the -x meridian, where atan2(y, x) jumps from +pi to -pi: x < 0, z spread over (-1, 1),
    |y| cycling through 0, the smallest subnormal, the smallest normal and 1, 2, 4 float32 steps of x's magnitude; the sign of y
    alternates, so both +0.0 and -0.0 occur."""
    i = np.arange(n)
    z = (-1.0 + 2.0 * (i + 0.5) / n).astype(np.float32)
    x = -np.sqrt(1.0 - z.astype(np.float64) ** 2).astype(np.float32)
    step = np.spacing(np.abs(x)).astype(np.float32)
    mag = np.stack([np.zeros(n, np.float32), np.full(n, 1e-45, np.float32), np.full(n, np.finfo(np.float32).tiny, np.float32),
                    step, 2 * step, 4 * step], 0)[i % 6, i]
    y = np.where((i // 6) % 2 == 0, mag, -mag).astype(np.float32)
    assert (x < 0).all() and (np.signbit(y) & (y == 0)).any() and (~np.signbit(y) & (y == 0)).any()
    return np.ascontiguousarray(np.stack([x, y, z], 1), np.float32)


QUERY_SIZES = (("fibonacci", 30000), ("cap+z", 50000), ("cap-z", 20000), ("seam", 4098))


@lru_cache(maxsize=None)
def query_sets(seed):
    """The four query sets of a seed, in the order they are concatenated: dict name -> float32 [n, 3].  Not to be written to."""
    rng = np.random.default_rng(1000 + seed)
    n = dict(QUERY_SIZES)
    q = {"fibonacci": fib_points(n["fibonacci"], seed), "cap+z": cap_points(rng, n["cap+z"], "+z", CAP_DEGREES),
         "cap-z": cap_points(rng, n["cap-z"], "-z", CAP_DEGREES), "seam": seam_points(n["seam"])}
    for a in q.values():
        a.setflags(write=False)
    return q


@lru_cache(maxsize=None)
def query_points(seed):
    """(float32 [3 * n] of the concatenated query sets, dict name -> slice of cells)"""
    q = query_sets(seed)
    xyz = np.ascontiguousarray(np.concatenate(list(q.values())).reshape(-1))
    xyz.setflags(write=False)
    where, at = {}, 0
    for k, a in q.items():
        where[k] = slice(at, at + a.shape[0])
        at += a.shape[0]
    return xyz, where


def points_planet(xyz):
    """A device planet whose cells sit at `xyz` (any count), joined in a ring."""
    from planet_heightmap_generation_amd.terrain_post import Planet
    xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1)
    return Planet(PointsMesh(xyz.size // 3), xyz)


def emu_lib():
    """tests/emu/libemu.so: the kernel bodies of csrc/plates_ops.h compiled for the host, built on first use."""
    global _emu
    if _emu is None:
        d = REPO / "tests" / "emu"
        subprocess.run(["make", "-s", "-C", str(d)], check=True)
        _emu = C.CDLL(str(d / "_build" / "libemu.so"))
        _emu.emu_project_plates.argtypes = [C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_int32, C.c_void_p]
        _emu.emu_project_plates.restype = None
    return _emu


def emu_project_plates(xyz, cmesh, cxyz, coarse_r_plate, seed, numPlates=None):
    """The device's projection (bucket grid, walk from the bucket's start cell) cell by cell on the host."""
    c32 = lambda a, t: np.ascontiguousarray(a, t).reshape(-1)  # noqa: E731
    xyz, off, adj, cxyz, plate = c32(xyz, np.float32), c32(cmesh.adjOffset, np.int32), c32(cmesh.adjList, np.int32), c32(cxyz, np.float32), c32(coarse_r_plate, np.int32)
    NC = int(cmesh.numRegions)
    assert off.size == NC + 1 and cxyz.size == 3 * NC and plate.size == NC
    out = np.empty(xyz.size // 3, np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    emu_lib().emu_project_plates(out.size, p(xyz), NC, p(off), p(adj), p(cxyz), p(plate), float(seed), -1 if numPlates is None else int(numPlates), p(out))
    return out


def oracle_project_plates(oracle, xyz, cmesh, cxyz, coarse_r_plate, seed, numPlates=None):
    """The reference's serial, warm-started walk with its brute-force fallback (oracle/plates_oracle.c) over the cells in order."""
    xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1)
    return oracle.project_coarse_plates(PointsMesh(xyz.size // 3), xyz, oracle.Mesh(cmesh.adjOffset, cmesh.adjList), cxyz, coarse_r_plate, seed, numPlates)


def mismatch(got, want, where=None):
    """'' when the arrays are equal, else the count, the first differing cell with both answers and, with `where`
    (name -> slice), the count per query set."""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape:
        return f"shape {got.shape} against {want.shape}"
    bad = np.flatnonzero(got != want)
    if bad.size == 0:
        return ""
    per = "" if where is None else "; per set " + str({k: int((got[s] != want[s]).sum()) for k, s in where.items()})
    return f"{bad.size} of {got.size} cells differ, first cell {int(bad[0])}: got {int(got[bad[0]])}, want {int(want[bad[0]])}{per}"


@lru_cache(maxsize=None)
def walk_answers(n, seed, numPlates):
    """(oracle, emulator) answers with identity plates on coarse_mesh(n, seed) over query_points(seed), noise seed `seed`: computed
    once, shared by the CPU and the GPU tests, not to be written to."""
    from oracle import pyoracle
    cmesh, cxyz = coarse_mesh(n, seed)
    xyz, _ = query_points(seed)
    ident = identity_plates(cmesh.numRegions)
    ref = oracle_project_plates(pyoracle, xyz, cmesh, cxyz, ident, seed, numPlates)
    emu = emu_project_plates(xyz, cmesh, cxyz, ident, seed, numPlates)
    ref.setflags(write=False)
    emu.setflags(write=False)
    return ref, emu
