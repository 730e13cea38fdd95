"""How far computeTemperature's outputs move when libm moves: the emulator built with the libm perturbation hook of tests/emu
(_build/libemu_temperature_libm.so: every pow of namespace wo returns glibc's result moved by k double ulps) against the plain
emulator.  On the device only those calls differ from the emulator (ocml's pow instead of glibc's), and in the reference only
those differ as well (V8's), so this is what bounds the golden and the device tests:
  - K = 0 reproduces the plain build bit for bit and the pow counter is 6 per cell (three curves per season);
  - K = 4 double ulps (twice the 2-ulp bound taken for ocml's double pow), all +K, all -K and two hashed seeds, changes no cell;
  - K = 2^20 (about 2^-32 relative, far beyond any libm error) changes cells (the hook is live), every change within the per-cell
    bound; TEMP_ULP_BOUND is the next power of two at or above 4 x the largest relative change, in units of 2^-23.

Measured (changed cells summer / winter, largest change relative to max(1, |ref|) in units of 2^-23):
  K = 4, every golden, all four seeds: 0 cells.
  K = 2^20, +K / -K: config 1 7 / 2 and 5 / 2 cells (0.5); import 1 / 12 and 1 / 6 (0.5); wet 4 / 2 and 6 / 3 (0.5); cold 4 / 10
    and 5 / 9 (0.5); warm 4 / 0 and 1 / 3 (0.5); all-ocean 0 / 1 (0.25); all-land 2 / 0 and 1 / 2 (0.5); edges 0 / 1 and 0 / 3
    (0.5); 64 and 256 cells 0; 257 cells 0 and 1 / 0 (0.5); 4 097 cells 2 / 5 and 2 / 0 (0.5); 250 001 cells 99 / 111 and
    102 / 153 (0.5).
The largest relative change is 0.5 x 2^-23 (one f32 ulp of a normalised temperature in [0.5, 1)); 4 x 0.5 = 2, so
TEMP_ULP_BOUND = 2.  The emulator alone (glibc against Node 12's Math.pow) differs from the goldens in 0 cells of every case
(tests/test_temperature.py prints the count per case)."""
import pytest

import temperature_common as TC

HOOK_LIVE_K = 2 ** 20
SEEDS_K4 = (1, 2, 3, 4)                 # all +K, all -K, two hashed
_by_2_20 = {}


@pytest.fixture(scope="module")
def libs():
    return TC.emu(False), TC.emu(True)


def _moved_by_2_20(hooked, name, case, ref):
    if name not in _by_2_20:
        rows = []
        for seed in (1, 2):
            hooked.emu_set_libm_perturb(seed, HOOK_LIVE_K)
            got = TC.emulate(case, offset=case["offset"], lib=hooked)
            rows.append([TC.deviation(got[k], ref[k]) for k in TC.RESULT_KEYS])
        hooked.emu_set_libm_perturb(0, 0)
        _by_2_20[name] = rows
    return _by_2_20[name]


@pytest.mark.parametrize("name", TC.GOLDEN_CASES)
def test_libm_sensitivity(libs, name):
    plain, hooked = libs
    case = TC.golden_case(name)
    N = case["N"]
    ref = TC.emulate(case, offset=case["offset"], lib=plain)
    hooked.emu_set_libm_perturb(0, 0)
    zero = TC.emulate(case, offset=case["offset"], lib=hooked)
    assert all(TC.same_bits(zero[k], ref[k]) for k in TC.RESULT_KEYS), f"{name}: the hook at K = 0 changed an output"
    calls = TC.libm_calls(hooked)
    print(f"{name}: N = {N}, pow calls {calls}")
    assert calls == 6 * N, "the hook is not reached by every pow of the per-cell loop"
    bound = TC.TEMP_ULP_BOUND * 2.0 ** -23
    for seed, figs in zip((1, 2), _moved_by_2_20(hooked, name, case, ref)):
        print(f"{name}: K = 2^20, seed {seed}: " + "; ".join(f"{k}: {n} cells changed, largest {m:.3g} ({rel / 2.0 ** -23:.2f} x 2^-23)" for k, (n, m, _, rel) in zip(TC.RESULT_KEYS, figs)))
        for n, m, over, rel in figs:
            assert over == 0, f"{name}: K = 2^20, seed {seed} moved {over} cells past the per-cell bound (largest change {m:.3g})"
            assert 4 * rel <= bound, f"{name}: K = 2^20, seed {seed}: 4 x {rel:.3g} exceeds the bound {bound:.3g}"
    for seed in SEEDS_K4:
        hooked.emu_set_libm_perturb(seed, TC.HOOK_K)
        got = TC.emulate(case, offset=case["offset"], lib=hooked)
        changed = {k: TC.deviation(got[k], ref[k])[0] for k in TC.RESULT_KEYS}
        print(f"{name}: K = {TC.HOOK_K}, seed {seed}: cells changed {changed}")
        assert not any(changed.values()), f"{name}: K = {TC.HOOK_K}, seed {seed} changed cells: {changed}"
    hooked.emu_set_libm_perturb(0, 0)


def test_libm_hook_is_live_and_the_bound_follows_the_rule(libs):
    """At least one case moved under K = 2^20 (else the sensitivity tests prove nothing), and TEMP_ULP_BOUND x 2^-23 is the next
    power of two times 2^-23 at or above 4 x the largest relative change of all cases, no looser than computeWind's 4 x 2^-23."""
    import wind_common as WC
    plain, hooked = libs
    for name in TC.GOLDEN_CASES:
        if name not in _by_2_20:                        # (run on its own: measure here what test_libm_sensitivity would have)
            case = TC.golden_case(name)
            _moved_by_2_20(hooked, name, case, TC.emulate(case, offset=case["offset"], lib=plain))
    rows = [f for name in TC.GOLDEN_CASES for seed in _by_2_20[name] for f in seed]
    assert sum(r[0] for r in rows) > 0, "K = 2^20 changed no cell of any case: the hook is not live"
    worst = max(r[3] for r in rows)
    want = 2.0 ** -23
    while want < 4 * worst:
        want *= 2
    print(f"largest relative change {worst:.3g} ({worst / 2.0 ** -23:.2f} x 2^-23): the rule gives {want / 2.0 ** -23:.0f} x 2^-23")
    assert TC.TEMP_ULP_BOUND * 2.0 ** -23 == want, (TC.TEMP_ULP_BOUND, want / 2.0 ** -23)
    assert TC.TEMP_ULP_BOUND * 2.0 ** -23 <= WC.ULP_BOUND
