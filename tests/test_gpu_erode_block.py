"""The erosion block of a planet (csrc/erode_block.h: wo_erode_block): erodeComposite's device state, built group by group at
first use.  A planet that never erodes holds none of it; the groups may be built in any order; the alternate routes (index
layout, relaxed mode, the patch finisher behind a scrambled basin layout) build theirs after the default route's and leave
the default route's results as they were; a repeated sequence allocates nothing and close() returns everything.

The planet is test_gpu_memory's: 5 000 cells, land and ocean mixed; the erosion call is its ERODE (glacial strength 1.0, so
that the carve runs).  A reference result is computed once per call on a planet of its own.  Every test prints its figures
before it asserts.  (The failure path of the block's one build helper needs an allocation that fails: it is driven on a
machine without a device by tools/sanitize/erode_block_main.cc.)"""
from functools import lru_cache

import numpy as np
import pytest

from test_gpu_memory import ERODE, _case, _planet, baseline, in_use

pytestmark = pytest.mark.gpu

THERMAL = (0, 3e-4, 0.5, 1.0, 3, 1.16, 0.015, 0, 0.0)
HYDRAULIC = (3, 3e-4, 0.5, 1.0, 0, 1.16, 0.015, 0, 0.0)
CALLS = {"thermal": THERMAL, "hydraulic": HYDRAULIC, "full": ERODE}


def _erode(pl, wc, ocean, args):
    """the same field and mask, one erosion call; (result, stats)"""
    pl.upload(wc["e"], ocean)
    pl.erode_composite_resident(*args)
    return pl.download(), pl.last_erode_stats()


@lru_cache(maxsize=None)
def _fresh(name):
    """the call on a planet that has run nothing else"""
    ec, wc, ocean = _case()
    pl = _planet(ec)
    try:
        got, stats = _erode(pl, wc, ocean, CALLS[name])
    finally:
        pl.close()
    got.setflags(write=False)
    return got, stats


def test_planet_that_never_erodes_has_no_erosion_memory():
    """One pass each of smoothElevation, sharpenRidges and soil creep on a new planet allocates nothing: the reading equals the one
    taken right after creation (the parent commit reads the same: created [411078 20068 13], after the passes [411078 20068 13]).
    Two or more passes of one call run on the patch-major mirror, which the planet then builds (on the parent commit too:
    [821132 20068 23]); it is the planet's and not the erosion's, and the growth is held to its ten buffers, to the byte."""
    ec, wc, ocean = _case()
    base = baseline()
    pl = _planet(ec)
    try:
        created = in_use() - base
        pl.upload(wc["e"], ocean)
        pl.smooth_elevation_resident(1, 0.25)
        pl.sharpen_ridges_resident(1, 0.04)
        pl.apply_soil_creep_resident(1, 0.1125)
        after = in_use() - base
        pl.smooth_elevation_resident(2, 0.25)
        pl.sharpen_ridges_resident(2, 0.04)
        pl.apply_soil_creep_resident(3, 0.1125)
        mirrored = in_use() - base
    finally:
        pl.close()
    left = in_use() - base
    print(f"created (device, pinned, allocations) {created}; after one pass of each {after}; after 2, 2 and 3 passes {mirrored}; after close() {left}")
    assert np.array_equal(after, created), (created, after)
    # the mirror (csrc/mirror.hip): perm, inv, off, adj and dist (rows padded by 8), xyz, e, e2 — 4-byte words — and ocean, coast
    N, E = ec.N, int(ec.mesh.adjOffset[ec.N])
    mirror = 4 * (N + N + (N + 1) + 2 * (E + 8) + 3 * N + N + N) + 2 * N
    assert np.array_equal(mirrored - created, [mirror, 0, 10]), (created, mirrored, mirror)
    assert left[0] == 0 and left[1] == 0, left


@pytest.mark.parametrize("order", [("thermal", "hydraulic", "full"), ("full", "hydraulic", "thermal")], ids=["thermal_first", "full_first"])
def test_groups_are_built_in_any_order(order):
    ec, wc, ocean = _case()
    pl = _planet(ec)
    try:
        seen = [(name, *_erode(pl, wc, ocean, CALLS[name])) for name in order]
    finally:
        pl.close()
    for name, got, stats in seen:
        print(f"{name}: {stats}")
    for name, got, stats in seen:
        assert np.array_equal(got, _fresh(name)[0]), f"{name} after {order[:order.index(name)]} differs from the call on a fresh planet"
        if name == "hydraulic":
            assert stats["solve_basin_passes"] > 0
        if name == "full":
            assert stats["carve_active_total"] > 0 and stats["flow_two_level"] == 1


ROUTES = (("default", {}), ("index", {"WO_LAYOUT": "index"}), ("relaxed", {"WO_RELAXED": "full"}),
          ("scramble", {"WO_TEST_HOOKS": "basin_scramble=1"}), ("default_again", {}))


def _routes(pl, wc, ocean, monkeypatch):
    out = {}
    for name, env in ROUTES:
        with monkeypatch.context() as m:
            for k, v in env.items():
                m.setenv(k, v)
            out[name] = _erode(pl, wc, ocean, ERODE)
    return out


def test_alternate_routes_after_the_default_one_and_back(monkeypatch):
    ec, wc, ocean = _case()
    for var in ("WO_LAYOUT", "WO_RELAXED", "WO_TEST_HOOKS", "WO_RELAXED_SORT_EVERY", "WO_FLOOD"):
        monkeypatch.delenv(var, raising=False)
    base = baseline()
    pl = _planet(ec)
    try:
        first = _routes(pl, wc, ocean, monkeypatch)
        once = in_use() - base
        second = _routes(pl, wc, ocean, monkeypatch)
        twice = in_use() - base
    finally:
        pl.close()
    left = in_use() - base
    for name, (got, stats) in first.items():
        print(f"{name}: mirror {stats['mirror_layout']}, two-level flow {stats['flow_two_level']}, relaxed {stats['relaxed_full']}, basin passes {stats['solve_basin_passes']}, "
              f"with leftovers {stats['solve_basin_passes_with_leftovers']}, run again with checks {stats['calls_run_again_with_checks']}, carve tasks {stats['carve_active_total']}")
    print(f"after the sequence (device, pinned, allocations) {once}; after its repeat {twice}; after close() {left}")
    ref = first["default"][0]
    assert np.array_equal(ref, _fresh("full")[0])
    assert first["index"][1]["mirror_layout"] == 0 and first["relaxed"][1]["relaxed_full"] == 1
    assert np.array_equal(first["index"][0], ref)                       # an exact route (csrc/device.h: Options)
    assert np.isfinite(first["relaxed"][0]).all()                       # (not a parity route)
    s = first["scramble"][1]
    assert s["solve_basin_passes_with_leftovers"] > 0 or s["calls_run_again_with_checks"] == first["relaxed"][1]["calls_run_again_with_checks"] + 1
    assert np.array_equal(first["scramble"][0], ref)                    # the patch finisher is an exact route
    assert np.array_equal(first["default_again"][0], ref)
    for name, _ in ROUTES:
        if name != "relaxed":
            assert np.array_equal(second[name][0], ref), name
    assert np.array_equal(once, twice), (once, twice)                   # live bytes AND the allocation count
    assert left[0] == 0 and left[1] == 0, left
