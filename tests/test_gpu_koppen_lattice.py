"""classifyKoppen on the device (k_koppen of csrc/temp.hip, the body koppen_cell of csrc/temp_ops.h) on the synthetic lattice
tests/golden/koppen_lattice.npz against the classes the reference recorded for it, not the emulator's: every threshold of the
classifier with its two f32 neighbours, all 31 classes (the D?d ones no planet reaches) and 30 rows with one input NaN, +inf or
-inf.  Class equality in every cell.  The stage reads no adjacency and no positions: the planet is a ring with dummy positions."""
import numpy as np
import pytest

import elev_inputs as EI
import temperature_common as TC

pytestmark = pytest.mark.gpu

COLUMNS = ("elevation", "tSummer", "tWinter", "pSummer", "pWinter")


def ring_planet(n):
    """A planet of n cells on a ring with dummy positions and unit neighbour distances (as planet_of in tests/test_gpu_super_plates.py)"""
    from planet_heightmap_generation_amd import terrain_post as TP
    r = np.arange(n, dtype=np.int32)
    off = (2 * np.arange(n + 1)).astype(np.int32)
    adj = np.stack([(r - 1) % n, (r + 1) % n], axis=1).reshape(-1).astype(np.int32)
    xyz = np.zeros(3 * n, np.float32); xyz[0::3] = 1.0
    return TP.Planet(EI.Mesh(off, adj), xyz, np.ones(adj.size, np.float32))


def rows(sel=slice(None)):
    e, temp, precip, ref = TC.lattice()
    take = lambda d: {k: np.ascontiguousarray(v[sel]) for k, v in d.items()}  # noqa: E731
    return np.ascontiguousarray(e[sel]), take(temp), take(precip), np.ascontiguousarray(ref[sel])


def classify(pl, e, temp, precip):
    from planet_heightmap_generation_amd import koppen
    return koppen.classify_koppen(pl, e, temp_result=temp, precip_result=precip)


def differing(label, got, e, temp, precip, ref):
    """Prints the count and the first differing rows with their five inputs; returns the count."""
    bad = np.flatnonzero(got != ref)
    print(f"{label}: {bad.size} of {ref.size} cells differ from the reference's recorded classes")
    cols = (e, temp["r_temperature_summer"], temp["r_temperature_winter"], precip["r_precip_summer"], precip["r_precip_winter"])
    for r in bad[:8]:
        print(f"    row {int(r)}: device {int(got[r])}, reference {int(ref[r])}; " + ", ".join(f"{k} {float(c[r])!r}" for k, c in zip(COLUMNS, cols)))
    return int(bad.size)


@pytest.fixture(scope="module")
def full():
    e, temp, precip, ref = rows()
    pl = ring_planet(e.size)
    yield pl, e, temp, precip, ref
    pl.close()


def test_lattice_has_the_reference_s_classes(full):
    pl, e, temp, precip, ref = full
    # 3 871 = 15 x 256 + 31 rows, 3 841 = 15 x 256 + 1 of them finite: the last block of k_koppen is a partial one
    assert e.size == 3871 and e.size % 256 != 0 and TC.LATTICE_FINITE == 3841 and pl.numRegions == e.size
    got = classify(pl, e, temp, precip)
    assert got.dtype == np.uint8 and got.shape == ref.shape
    bad = differing("lattice", got, e, temp, precip, ref)
    classes = np.bincount(got, minlength=31)
    print(f"lattice: cells per class on the device {classes.tolist()}")
    assert bad == 0
    assert classes.size == 31 and (classes > 0).all(), f"classes not reached: {np.flatnonzero(classes == 0).tolist()}"
    tail = got[TC.LATTICE_FINITE:]
    print(f"non-finite rows: device classes {tail.tolist()}")
    assert np.array_equal(tail, ref[TC.LATTICE_FINITE:]) and not np.isfinite(e[TC.LATTICE_FINITE:]).all()


def test_reversed_rows_give_reversed_classes(full):
    """A cell's class does not depend on its index, and a second call on the planet replaces the whole Koppen block."""
    from planet_heightmap_generation_amd import koppen
    pl, e, temp, precip, ref = full
    assert differing("forward", classify(pl, e, temp, precip), e, temp, precip, ref) == 0
    er, tr, pr, rr = rows(slice(None, None, -1))
    assert np.array_equal(rr, ref[::-1]) and not np.array_equal(rr, ref)
    got = classify(pl, er, tr, pr)
    assert differing("reversed", got, er, tr, pr, rr) == 0
    assert np.array_equal(koppen.download(pl), rr)


def test_resident_elevation_gives_the_same_classes(full):
    pl, e, temp, precip, ref = full
    passed = classify(pl, e, temp, precip)
    pl.upload(e)
    resident = classify(pl, None, temp, precip)
    assert differing("resident elevation", resident, e, temp, precip, ref) == 0
    assert np.array_equal(resident, passed)


@pytest.mark.parametrize("n", [255, 256, 257])
def test_prefixes_at_the_block_edge(n):
    """One block less a thread, exactly one block, one block and one live thread of the next"""
    e, temp, precip, ref = rows(slice(0, n))
    assert n < TC.LATTICE_FINITE and np.array_equal(ref, TC.lattice()[3][:n])
    pl = ring_planet(n)
    try:
        got = classify(pl, e, temp, precip)
    finally:
        pl.close()
    assert got.size == n and differing(f"first {n} rows", got, e, temp, precip, ref) == 0
