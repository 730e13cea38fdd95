"""An independent verifier of a spherical Delaunay triangulation: check(xyz, triangles, halfedges).

It reads the three arrays and nothing else of the builders: no star, no grid, no predicate of csrc/mesh_ops.h.  The arithmetic is
numpy float64, and Python fractions where float64 cannot decide.

What it establishes, and why that is the Delaunay property:
  1. the points are the builders' own: the f32 position in f64 divided by sqrt(x*x + y*y + z*z), the operations in mesh::normalise's
     order, so the bits are the same;
  2. structure: 3 (2V - 4) sides, halfedges an involution that pairs the sides (u -> v) and (v -> u), every vertex used: a closed
     oriented surface of the sphere's Euler characteristic;
  3. every triangle has the centre strictly behind it (det[p0, p1 - p0, p2 - p0] > 0), and the signed spherical areas sum to 4 pi
     times ONE: the surface covers the sphere once (0: the hull of a set inside a hemisphere; 2: a double wrap);
  4. at every side the vertex opposite in the twin's triangle lies strictly below the triangle's plane (det[b - a, c - a, d - a] < 0):
     the surface is locally convex at every edge.
A closed surface that covers the sphere once around a centre strictly inside, and is locally convex at every edge, is the boundary
of a convex body: the convex hull of its vertices.  The hull of points on a sphere is their spherical Delaunay triangulation.  So 2 to
4 together are the GLOBAL empty-circumcap property, not just a local one, and no point is tested against every triangle.

The float64 determinant of step 4 is trusted when |det| > (7 + 56 eps) eps * permanent, eps = 2^-53 (Shewchuk's bound for this
expression on rounded differences).  The other sides are evaluated exactly in rationals on the f64 coordinates.  An exact value > 0
is a violation only if it exceeds the same bound; a smaller one is a tie, which the builders' own float predicate (evaluated on
another ordering of the same four points) may legitimately have settled either way.  Ties are counted.  More than MAX_UNDECIDED
undecided sides fail the check: they are never skipped."""
from fractions import Fraction

import numpy as np

EPS = 2.0 ** -53
ERR_BOUND = (7 + 56 * EPS) * EPS
MAX_UNDECIDED = 20000
CHUNK = 1 << 20


class CheckFailed(AssertionError):
    pass


def unit_points(xyz):
    """mesh::normalise in numpy: (V, 3) float64"""
    p = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3).astype(np.float64)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    l = np.sqrt(x * x + y * y + z * z)
    return np.stack([x / l, y / l, z / l], axis=1)


def next_side(s):
    return np.where(s % 3 == 2, s - 2, s + 1)


def halfedges_of(triangles):
    """the twin of every side of a closed oriented triangle list, -1 where there is none (for meshes made by hand in the tests)"""
    tri = np.asarray(triangles, np.int64)
    u, v = tri, tri[next_side(np.arange(tri.size))]
    n = int(tri.max()) + 1
    fwd, bwd = u * n + v, v * n + u
    order = np.argsort(fwd, kind="stable")
    at = np.searchsorted(fwd[order], bwd)
    at = np.minimum(at, tri.size - 1)
    he = order[at]
    return np.where(fwd[he] == bwd, he, -1).astype(np.int32)


def det_and_permanent(A, B, C, D):
    """det[B - A, C - A, D - A] row by row in float64, and the same expression on absolute values"""
    b, c, d = B - A, C - A, D - A
    bx, by, bz = b[:, 0], b[:, 1], b[:, 2]
    cx, cy, cz = c[:, 0], c[:, 1], c[:, 2]
    dx, dy, dz = d[:, 0], d[:, 1], d[:, 2]
    det = bx * (cy * dz - cz * dy) - by * (cx * dz - cz * dx) + bz * (cx * dy - cy * dx)
    perm = (np.abs(bx) * (np.abs(cy * dz) + np.abs(cz * dy)) + np.abs(by) * (np.abs(cx * dz) + np.abs(cz * dx))
            + np.abs(bz) * (np.abs(cx * dy) + np.abs(cy * dx)))
    return det, perm


def exact_det(a, b, c, d):
    """det[b - a, c - a, d - a] of four float64 points, as a Fraction"""
    a, b, c, d = ([Fraction(float(v)) for v in p] for p in (a, b, c, d))
    (bx, by, bz), (cx, cy, cz), (dx, dy, dz) = ([q[i] - a[i] for i in range(3)] for q in (b, c, d))
    return bx * (cy * dz - cz * dy) - by * (cx * dz - cz * dx) + bz * (cx * dy - cy * dx)


def classify(P, a, b, c, d):
    """The sides (a, b, c | d) given as index arrays into P.  Returns (violations, undecided, ties): boolean masks over the sides.
    A violation is a d that is not strictly below the plane of (a, b, c), decided in float64 or exactly."""
    det, perm = det_and_permanent(P[a], P[b], P[c], P[d])
    bound = ERR_BOUND * perm
    undecided = ~(np.abs(det) > bound)
    violations = ~undecided & (det > 0)
    ties = np.zeros(det.size, bool)
    idx = np.flatnonzero(undecided)
    if idx.size > MAX_UNDECIDED:
        raise CheckFailed(f"{idx.size} sides are undecided in float64, more than {MAX_UNDECIDED}")
    for i in idx:
        e = exact_det(P[a[i]], P[b[i]], P[c[i]], P[d[i]])
        if e > 0 and e > Fraction(float(bound[i])):
            violations[i] = True
        elif e >= 0:
            ties[i] = True
    return violations, undecided, ties


def check(xyz, triangles, halfedges):
    """The figures of a triangulation (see the module's text).  Keys: V, sides, structure (a list of what is wrong with the arrays: with
    sizes or indices wrong nothing else is looked at, and the sides only when it is empty), inward (triangles whose volume against the
    centre is not > 0), min_volume, cover (the signed spherical areas over 4 pi), violations (the sides that are not locally Delaunay),
    undecided, ties."""
    P = unit_points(xyz)
    V = P.shape[0]
    tri = np.asarray(triangles, np.int64).reshape(-1)
    he = np.asarray(halfedges, np.int64).reshape(-1)
    fig = dict(V=V, sides=int(tri.size), structure=[], inward=None, min_volume=None, cover=None, violations=None, undecided=None, ties=None)
    bad = fig["structure"]
    if tri.size != 3 * (2 * V - 4):
        bad.append(f"{tri.size} sides, 3 (2V - 4) is {3 * (2 * V - 4)}")
    if he.size != tri.size:
        bad.append(f"{he.size} half-edges for {tri.size} sides")
    if tri.size and (tri.min() < 0 or tri.max() >= V):
        bad.append("a triangle corner is out of range")
    if he.size and (he.min() < 0 or he.max() >= he.size):
        bad.append("a half-edge is out of range")
    if bad:
        return fig
    s = np.arange(tri.size)
    if not np.array_equal(he[he], s):
        bad.append("halfedges is no involution")
    if not (np.array_equal(tri[he], tri[next_side(s)]) and np.array_equal(tri[next_side(he)], tri)):
        bad.append("a side's twin does not run the other way between the same two vertices")
    if (np.bincount(tri, minlength=V) == 0).any():
        bad.append("a vertex occurs in no triangle")
    closed = not bad                                        # the corners are in range either way: orientation and cover are still figures

    T = tri.reshape(-1, 3)
    A, B, C = P[T[:, 0]], P[T[:, 1]], P[T[:, 2]]
    vol = np.einsum("ij,ij->i", A, np.cross(B - A, C - A))
    fig["inward"] = int((~(vol > 0)).sum())
    fig["min_volume"] = float(vol.min())
    triple = np.einsum("ij,ij->i", A, np.cross(B, C))
    dots = 1.0 + np.einsum("ij,ij->i", A, B) + np.einsum("ij,ij->i", B, C) + np.einsum("ij,ij->i", C, A)
    fig["cover"] = float((2.0 * np.arctan2(triple, dots)).sum() / (4.0 * np.pi))

    if not closed:
        return fig
    viol, und, tie = [], 0, 0
    for lo in range(0, tri.size, CHUNK):
        ss = s[lo:lo + CHUNK]
        t3 = 3 * (ss // 3)
        a, b, c = tri[t3], tri[t3 + 1], tri[t3 + 2]
        d = tri[next_side(next_side(he[ss]))]              # the corner of the twin's triangle that is not on the shared edge
        v, u, t = classify(P, a, b, c, d)
        viol.append(ss[v])
        und += int(u.sum())
        tie += int(t.sum())
        if und > MAX_UNDECIDED:
            raise CheckFailed(f"more than {MAX_UNDECIDED} sides are undecided in float64")
    fig["violations"] = np.concatenate(viol) if viol else np.zeros(0, np.int64)
    fig["undecided"], fig["ties"] = und, tie
    return fig


def describe(name, fig):
    nv = None if fig["violations"] is None else int(fig["violations"].size)
    return (f"{name}: V {fig['V']}, sides {fig['sides']}, structure {fig['structure'] or 'ok'}, inward {fig['inward']}, smallest volume "
            f"{fig['min_volume']}, cover {fig['cover']}, violations {nv}, undecided {fig['undecided']}, ties {fig['ties']}")


def assert_delaunay(name, xyz, triangles, halfedges):
    """prints the figures, then asserts all of 2 to 4; returns the figures"""
    fig = check(xyz, triangles, halfedges)
    print(describe(name, fig))
    assert not fig["structure"], f"{name}: {fig['structure']}"
    assert fig["inward"] == 0, f"{name}: {fig['inward']} triangles do not have the centre behind them, smallest volume {fig['min_volume']}"
    assert round(fig["cover"]) == 1 and abs(fig["cover"] - 1) < 1e-6, f"{name}: the surface covers the sphere {fig['cover']} times"
    assert fig["violations"].size == 0, f"{name}: not locally Delaunay at sides {fig['violations'][:10].tolist()} ({fig['violations'].size} in all)"
    return fig
