"""The C-ABI library loads here (no GPU) and exports every symbol include/worogen.h declares; device entry
points fail loudly instead of falling back to a CPU path."""
import re

import pytest

from conftest import REPO


def declared_symbols():
    text = (REPO / "include" / "worogen.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(wo_[a-z0-9_]+)\s*\(", text)))


def test_library_exports_every_declared_symbol():
    from planet_heightmap_generation_amd import capi
    L = capi.lib()
    syms = declared_symbols()
    assert len(syms) >= 35
    for s in syms:
        assert hasattr(L, s), f"libworogen.so does not export {s}"
    assert capi.MISSING == []
    assert set(capi.SIGNATURES) == set(syms), set(capi.SIGNATURES) ^ set(syms)
    assert L.wo_abi_version() == 1


def test_no_cpu_fallback_without_device():
    from planet_heightmap_generation_amd import capi, terrain_post
    if capi.lib().wo_device_count() > 0:
        pytest.skip("a HIP device is present")
    with pytest.raises(capi.WorogenError, match="no usable HIP device"):
        terrain_post.Context(0)


def test_rccl_is_not_a_load_time_dependency():
    """Single-GPU hosts never map librccl: the collectives are bound by name at the first multi-GPU entry point (csrc/comm.hip)."""
    import subprocess
    from planet_heightmap_generation_amd import capi
    needed = subprocess.run(["readelf", "-d", str(capi.LIB_PATH)], capture_output=True, text=True, check=True).stdout
    assert "libamdhip64" in needed and "rccl" not in needed, needed


def test_product_does_not_reference_the_oracle():
    pkg = REPO / "planet_heightmap_generation_amd"
    for f in list(pkg.rglob("*.py")) + list(pkg.rglob("*.cc")) + list(pkg.rglob("*.hip")) + list(pkg.rglob("*.h")) + list(pkg.rglob("*.js")) + list(pkg.rglob("*.mjs")):
        txt = f.read_text(errors="ignore")
        assert "pyoracle" not in txt and "liboracle" not in txt and "wo_or_" not in txt, f


def test_device_memory_has_one_owner():
    """Only csrc/device_mem.h (DeviceArena) calls the HIP allocator; the hand-written allocate / free helpers are gone."""
    csrc = REPO / "planet_heightmap_generation_amd" / "csrc"
    call = re.compile(r"hip(Host)?(Malloc|Free)\s*\(")
    gone = re.compile(r"\b(dalloc|dfree|walloc|wfree|DevBufs)\b")
    files = sorted(list(csrc.glob("*.hip")) + list(csrc.glob("*.h")) + list(csrc.glob("*.cc")))
    assert (csrc / "device_mem.h") in files and call.search((csrc / "device_mem.h").read_text())
    for f in files:
        txt = f.read_text(errors="ignore")
        if f.name != "device_mem.h":
            assert not call.search(txt), f"{f.name} calls the HIP allocator itself: {call.search(txt).group(0)}"
        assert not gone.search(txt), f"{f.name} still has {gone.search(txt).group(0)}"


def test_host_entry_points_reject_bad_arguments():
    """Status 1 + a message instead of a crash: null pointers, sizes that cannot be right, malformed meshes."""
    import numpy as np
    from planet_heightmap_generation_amd import capi
    L = capi.lib()
    i32 = np.zeros(8, np.int32)
    f32 = np.zeros(24, np.float32)
    assert L.wo_fib_sphere_points(0, 0.75, 1.0, capi.ptr(f32)) != 0 and "wo_fib_sphere_points" in capi.last_error()
    assert L.wo_fib_sphere_points(4, 0.75, 1.0, None) != 0
    assert L.wo_sphere_delaunay(8, None, capi.ptr(i32), capi.ptr(i32)) != 0 and "wo_sphere_delaunay" in capi.last_error()
    assert L.wo_neighbor_dist(4, None, None, None, None) != 0
    assert L.wo_smooth_reconnect_plates(0, capi.ptr(i32), capi.ptr(i32), capi.ptr(i32), None, 0, 3) != 0
    assert L.wo_smooth_reconnect_plates(4, capi.ptr(i32), capi.ptr(i32), None, None, 0, 3) != 0 and "wo_smooth_reconnect_plates" in capi.last_error()
    assert L.wo_smooth_reconnect_plates(4, capi.ptr(i32), capi.ptr(i32), capi.ptr(i32), None, 2, 3) != 0
    # device entry points with a NULL planet / context never dereference it
    assert L.wo_planet_num_regions(None) == 0
    assert L.wo_smooth_field(None, capi.ptr(f32), 1) != 0
    assert L.wo_project_coarse_plates(None, 4, capi.ptr(i32), capi.ptr(i32), capi.ptr(f32), capi.ptr(i32), 1.0, 8, capi.ptr(i32)) != 0
    assert L.wo_erode_composite_resident(None, 1, 3e-4, 0.5, 1.0, 1, 1.16, 0.015, 0, 0.0) != 0
    assert not L.wo_planet_create(None, 4, capi.ptr(i32), capi.ptr(i32), capi.ptr(f32), None)


def test_ensemble_runner_argument_checks():
    from planet_heightmap_generation_amd.ensemble import EnsembleRunner
    with pytest.raises(ValueError):
        EnsembleRunner(None, None, in_flight=0)
    assert EnsembleRunner(None, None, in_flight=2).map(lambda pl, s: s, []) == []        # nothing to do: no device touched
