"""The one transfer path of the four climate blocks (csrc/stage_block.h: block_download, block_upload, block_require) through
ctypes, for every block and every result key: what a planet that ran no stage refuses, what a block filled by one upload serves
and refuses, the size and pointer checks with their exact texts, and that everything a planet took goes back on close(), a
block left empty by a refused upload included.

The planets are two shape goldens: temp_N63_shape_s1, the smallest (64 cells: 256 bytes per float field, 64 for r_isLand), and
temp_N256_shape_s1 (257 cells: 1 028 and 257 bytes, an odd count, which is all a copy path can be sensitive to); the ITCZ arrays
are 360 floats whatever N is.  Each key gets a fresh planet of the shape, so that "this field alone" holds.  Every refusal is an
argument check on the host that returns before any device work."""
import ctypes as C
import gc
from functools import lru_cache

import numpy as np
import pytest

import temperature_common as TC
import wind_common as WC

pytestmark = pytest.mark.gpu

# block -> (module, C prefix, noun of the messages, compute entry point)
BLOCKS = {
    "wind": ("wind", "wo_wind", "wind", "wo_compute_wind"),
    "ocean": ("ocean", "wo_ocean", "ocean", "wo_compute_ocean_currents"),
    "precip": ("precipitation", "wo_precip", "precipitation", "wo_compute_precipitation"),
    "temp": ("temperature", "wo_temperature", "temperature", "wo_compute_temperature"),
}


SHAPES = {"temp_N63_shape_s1": 64, "temp_N256_shape_s1": 257}


@lru_cache(maxsize=None)
def _case(shape):
    case = TC.golden_case(shape)
    assert case["N"] == SHAPES[shape]
    return case


def _planet(shape):
    from planet_heightmap_generation_amd import terrain_post as TP
    case = _case(shape)
    return TP.Planet(WC.Mesh(case["off"], case["adj"]), case["xyz"])


def _in_use():
    """(device bytes, pinned bytes) the process holds"""
    from planet_heightmap_generation_amd import capi
    d, h, n = C.c_int64(0), C.c_int64(0), C.c_int64(0)
    assert capi.lib().wo_memory_in_use(C.byref(d), C.byref(h), C.byref(n)) == 0
    return d.value, h.value


def _refused(rc, want):
    from planet_heightmap_generation_amd import capi
    got = capi.last_error()
    print(f"    status {rc}: {got}")
    assert rc == 1 and got == want, (rc, got, want)


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("name", list(BLOCKS))
def test_every_key(name, shape):
    import importlib

    from planet_heightmap_generation_amd import capi
    module, prefix, noun, compute = BLOCKS[name]
    M = importlib.import_module(f"planet_heightmap_generation_amd.{module}")
    L = capi.lib()
    down, up = getattr(L, f"{prefix}_download"), getattr(L, f"{prefix}_upload")
    dfn, ufn = f"{prefix}_download", f"{prefix}_upload"
    no_result = f"{dfn}: no {noun} result on this planet (call {compute} first)"
    fields = M.RESULT_FIELDS
    N = SHAPES[shape]
    rng = np.random.default_rng(7)
    gc.collect()
    for i, (key, ty) in enumerate(fields):
        count = 360 if key.startswith("itcz") else N
        nbytes = count * np.dtype(ty).itemsize
        other = fields[(i + 1) % len(fields)][0]
        print(f"{name}.{key}: {count} x {np.dtype(ty).name}, {nbytes} bytes")
        base = _in_use()
        pl = _planet(shape)
        try:
            out = np.zeros(count + 1, ty)
            _refused(down(pl.handle, key.encode(), capi.ptr(out), out.nbytes), no_result)
            for size in (count - 1, count + 1):
                data = np.zeros(size, ty)
                _refused(up(pl.handle, key.encode(), capi.ptr(data), data.nbytes), f"{ufn}: {key} takes {nbytes} bytes, data has {data.nbytes}")
            _refused(down(pl.handle, key.encode(), capi.ptr(out), out.nbytes), no_result)      # the block a refused upload built is empty
            _refused(up(pl.handle, key.encode(), None, nbytes), f"{ufn}: null pointer")
            _refused(down(pl.handle, key.encode(), None, nbytes), f"{dfn}: null pointer")
            _refused(up(pl.handle, b"nope", capi.ptr(out), nbytes), f"{ufn}: unknown field 'nope'")
            # this field alone
            sent = np.frombuffer(rng.bytes(nbytes), dtype=ty).copy()          # any bits: NaN payloads must come back as they went
            M.upload(pl, key, sent)
            got = M.download(pl, key)
            assert got.dtype == ty and got.size == count and got.tobytes() == sent.tobytes(), f"{key}: the download differs from what was uploaded"
            _refused(down(pl.handle, other.encode(), capi.ptr(out), out.nbytes), f"{dfn}: no {noun} result on this planet: {other} was never set (call {compute} first)")
            _refused(down(pl.handle, b"nope", capi.ptr(out), out.nbytes), f"{dfn}: unknown field 'nope'")
            short = np.zeros(nbytes - 1, np.uint8)
            _refused(down(pl.handle, key.encode(), capi.ptr(short), short.nbytes), f"{dfn}: {key} needs {nbytes} bytes, out has {nbytes - 1}")
            assert _in_use()[0] > base[0]
        finally:
            pl.close()
        left = _in_use()
        assert left == base, (key, base, left)
