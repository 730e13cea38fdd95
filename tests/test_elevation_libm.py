"""How far assignElevation's outputs move when libm moves: the emulator built with the libm perturbation hook (tests/emu:
_build/libemu_libm.so, every tanh / exp / sin / cos / atan2 / pow / asin call of namespace wo returns glibc's result moved by k
double ulps) against the plain emulator (libemu.so).  On the device only those calls differ from the emulator (ocml instead of
glibc), so this is what bounds the device tests of test_gpu_elevation_scale.py and test_gpu_elevation.py:
  - K = 0 reproduces libemu.so bit for bit (the hook itself changes nothing) and the call counters are non-zero;
  - K = 2^20 (about 2^-32 relative, far beyond any libm error) changes some cells of every case (the hook is live), every change within the
    per-cell bound ULP_BOUND * max(1, |ref|) of the device tests;
  - K = 4 (twice the 2-ulp bound taken for ocml's doubles), all +K, all -K and two hashed seeds: stress and the Sets never change,
    and no output changes in more than a tenth of the device tests' cap max(8, N / 10^4) cells.

Measured (changed cells / largest change):
  K = 4, all cases, all four seeds: 0 cells in every output.
  K = 2^20, +K / -K: 5 k golden: elevation 4 / 5 cells (1.2e-7 / 3.0e-8), foldRidge 21 / 15; config 1 10 k: elevation 15 / 8
    (6.0e-8), foldRidge 49 / 37; 10 k s2: elevation 13 / 13 (6.0e-8), foldRidge 43 / 42; stress and Sets 0 everywhere.
  See DESIGN.md section 3 for the 250 k, 1 M and hub-mesh rows."""
import numpy as np
import pytest

import elev_inputs as EI

HOOK_LIVE_K = 2 ** 20
SEEDS_K4 = (1, 2, 3, 4)                 # all +K, all -K, two hashed


@pytest.fixture(scope="module")
def libs():
    return EI.load_emulator(False), EI.load_emulator(True)


CASE_BUILDERS = {
    "elev_N5000_s3_nosuper": lambda: EI.golden_case("elev_N5000_s3_nosuper"),
    "elev_config1_N10000_s1": lambda: EI.golden_case("elev_config1_N10000_s1"),
    "elev_N10000_s2": lambda: EI.golden_case("elev_N10000_s2"),
    "elev_N250000_s4_large": EI.large_golden_case,
    "realistic_N1000000": lambda: EI.realistic_case(1_000_000),
    "hub_N200000_deg24": lambda: EI.hub_case(200_000),
}


def _outputs(r):
    return [("r_elevation", r["r_elevation"]), ("r_stress", r["r_stress"])] + [("dl_" + k, r["debugLayers"][k]) for k in EI.LAYERS]


def _same(a, b):
    return all(np.array_equal(x, y) for (_, x), (_, y) in zip(_outputs(a), _outputs(b))) and \
        all(a[k] == b[k] for k in ("mountain_r", "coastline_r", "ocean_r"))


@pytest.mark.parametrize("name", list(CASE_BUILDERS))
def test_libm_sensitivity(libs, name):
    plain, hooked = libs
    case = CASE_BUILDERS[name]()
    N = case.N
    ref = EI.emulate(plain, case)
    hooked.emu_set_libm_perturb(0, 0)
    assert _same(EI.emulate(hooked, case), ref), f"{name}: the hook at K = 0 changed an output"
    calls = EI.libm_calls(hooked)
    print(f"{name}: libm calls (tanh, exp, sin, cos, atan2, pow, asin) {calls.tolist()}")
    assert calls[:6].min() > 0, "the hook is not reached by every wrapped function the kernel bodies call"
    changed = 0
    for seed in (1, 2):
        hooked.emu_set_libm_perturb(seed, HOOK_LIVE_K)
        got = EI.emulate(hooked, case)
        figs = {k: EI.deviation(x, y) for (k, x), (_, y) in zip(_outputs(got), _outputs(ref))}
        print(f"{name}: K = 2^20, seed {seed}: " + "; ".join(f"{k} {n} ({m:.3g})" for k, (n, m, _) in figs.items() if n))
        over = {k: o for k, (_, _, o) in figs.items() if o}
        assert not over, f"{name}: K = 2^20 moved cells past the per-cell bound: {over}"
        changed += sum(n for n, _, _ in figs.values())
    assert changed > 0, f"{name}: K = 2^20 changed no cell: the hook is not live"
    cap = EI.diff_cap(N)
    for seed in SEEDS_K4:
        hooked.emu_set_libm_perturb(seed, EI.HOOK_K)
        got = EI.emulate(hooked, case)
        figs = {k: EI.deviation(x, y) for (k, x), (_, y) in zip(_outputs(got), _outputs(ref))}
        print(f"{name}: K = {EI.HOOK_K}, seed {seed}: " + ("; ".join(f"{k} {n} ({m:.3g})" for k, (n, m, _) in figs.items() if n) or "no change"))
        assert got["mountain_r"] == ref["mountain_r"] and got["coastline_r"] == ref["coastline_r"] and got["ocean_r"] == ref["ocean_r"], name
        assert figs["r_stress"][0] == 0, f"{name}: K = {EI.HOOK_K} changed stress (the device tests hold it bit for bit)"
        for k, (n, _, o) in figs.items():
            assert o == 0, f"{name}: K = {EI.HOOK_K}, seed {seed}: {k} has {o} cells past the per-cell bound"
            assert 10 * n <= cap, f"{name}: K = {EI.HOOK_K}, seed {seed}: {k} changed {n} cells, more than a tenth of the cap {cap}"

