"""The bookkeeping of csrc/radix.hip restated on the host and run at the pair counts where it can go wrong: the tail guard of a
partly filled last tile, a count that is exactly one tile (4 096 pairs) or one group of 32 tiles (131 072) and one pair more, and
the two group-total buffers that swap roles every pass while sorts of different sizes follow each other on one scratch.

This is a model of the launch structure (what each tile counts, what the prefix over earlier tiles and groups reads, what a pass
clears for the next), not of the wave-level ranking inside a tile, which only the device can run: test_gpu_parity.py
(test_sorts_at_tile_and_group_boundaries), test_gpu_wind.py and test_gpu_ocean.py hold the kernels to the same counts."""
import numpy as np
import pytest

TILE, GROUP, DIGITS = 4096, 32, 256


def tiles_of(n):
    return (n + TILE - 1) // TILE


def groups_of(n):
    return (tiles_of(n) + GROUP - 1) // GROUP


class RadixModel:
    """radix_scratch + radix_sort_pairs: scratch all zero before the first sort, `flip` the parity of the passes run so far."""

    def __init__(self, n_max):
        self.n_max = n_max
        self.group_tot = np.zeros((2, groups_of(n_max), DIGITS), np.int64)
        self.counts = np.zeros((tiles_of(n_max), DIGITS), np.int64)
        self.flip = 0

    def sort(self, keys, vals, begin_bit, end_bit):
        passes = (end_bit - begin_bit + 7) // 8
        n = keys.size
        assert passes % 2 == 0 and 0 < n <= self.n_max
        tiles, groups = tiles_of(n), groups_of(n)
        pos = np.full(int(vals.max()) + 1, -1, np.int64)
        for q in range(passes):
            shift = begin_bit + 8 * q
            gt, other = self.group_tot[self.flip & 1], self.group_tot[(self.flip + 1) & 1]
            # k_rs_count: a tile counts the digits of its pairs with index < n and adds them to its group's totals
            for t in range(tiles):
                i = np.arange(t * TILE, (t + 1) * TILE)
                i = i[i < n]                                                      # the tail guard
                c = np.bincount((keys[i] >> shift) & 255, minlength=DIGITS)
                self.counts[t] = c
                gt[t // GROUP] += c
            # k_rs_scatter: base of the digit + its pairs in earlier groups and in the earlier tiles of this group + place in the tile
            hist = gt[:groups].sum(axis=0)
            hbase = np.cumsum(hist) - hist
            out_k, out_v = np.full(n, -1, np.int64), np.full(n, -1, np.int64)
            for t in range(tiles):
                g = t // GROUP
                excl = gt[:g].sum(axis=0) + self.counts[g * GROUP:t].sum(axis=0)
                have = min(TILE, n - t * TILE)
                k, v = keys[t * TILE:t * TILE + have], vals[t * TILE:t * TILE + have]
                d = (k >> shift) & 255
                order = np.argsort(d, kind="stable")                              # the tile in destination order (s_keys / s_vals)
                start = np.cumsum(self.counts[t]) - self.counts[t]
                ds = d[order]
                dst = (hbase + excl - start)[ds] + np.arange(have)
                out_k[dst], out_v[dst] = k[order], v[order]
                if q == passes - 1:
                    pos[v[order]] = dst
                if t < groups:
                    other[t] = 0                                                  # the other buffer, for the next pass
            assert (out_v >= 0).all(), "a destination was written twice or never"
            keys, vals = out_k, out_v
            self.flip += 1
        return keys, vals, pos


SIZES = (64, 4095, 4096, 4097, 8192, 131072, 131073, 4097, 1, 131073, 2049, 131072)


@pytest.mark.parametrize("bits", [16, 32])
def test_model_sorts_stably_at_every_boundary_on_one_scratch(bits):
    """Sorts of very different sizes one after another on one scratch (up, down and up again across the tile and the group
    boundary): each is the stable order of its keys, and its rank array is the inverse of its value array."""
    rng = np.random.default_rng(bits)
    model = RadixModel(max(SIZES))
    for n in SIZES:
        keys = rng.integers(0, 2592 if bits == 16 else 1 << 32, n, dtype=np.int64)
        if bits == 32:
            keys &= 0xFFF000FF                                                    # runs of equal keys, and digits that are all zero
        vals = rng.permutation(n).astype(np.int64)
        k, v, pos = model.sort(keys, vals, 0, bits)
        want = np.argsort(keys, kind="stable")
        assert np.array_equal(k, keys[want]) and np.array_equal(v, vals[want]), n
        assert np.array_equal(pos[v], np.arange(n)), n
    assert model.flip == len(SIZES) * bits // 8


def test_model_scratch_rule():
    """After a sort of G groups the buffer the next sort starts on is clear; the other one still holds the last pass's totals up to
    G, which the next sort clears as far as its own group count and reads no further (csrc/radix.hip: radix_sort_pairs)."""
    model = RadixModel(131073 * 2)
    for n in (131073 * 2, 4097, 131073 * 2):
        model.sort(np.arange(n, dtype=np.int64) % 2592, np.arange(n, dtype=np.int64), 0, 16)
        assert not model.group_tot[model.flip & 1].any()
        assert model.group_tot[(model.flip + 1) & 1][:groups_of(n)].sum() == n
