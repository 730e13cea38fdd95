"""How far erodeComposite's field moves when libm moves: the emulator built with the libm perturbation hook (tests/emu:
_build/libemu_libm.so, every unqualified pow / asin call of csrc/erode_ops.h returns glibc's result moved by k double ulps) against
the plain emulator (libemu.so).  On the device only those calls differ from the emulator (ocml instead of glibc), so this is what
bounds the device tests that run glacial passes or m != 0.5 (erode_common.check_cells in test_gpu_parity.py,
test_gpu_irregular_mesh.py and test_gpu_elevation.py):
  - K = 0 reproduces libemu.so bit for bit (the hook itself changes nothing) and the pow counter is non-zero: the hook reaches the
    glacial turn, the deposit / fjord terms and the pow(flow, m) of the stream-power step;
  - K = 2^20 (about 2^-32 relative, far beyond any libm error), all +K and all -K: every change within the per-cell bound
    ERODE_ULP_BOUND * max(1, |ref|) of the device tests, and at least one case changes (the hook is live);
  - K = 4 (twice the 2-ulp bound taken for ocml's double pow / asin), all +K, all -K and two hashed seeds: no cell past the bound
    and no more than a tenth of the device tests' cap max(8, N / 10^4) cells changed.

ERODE_ULP_BOUND = 4 x the largest relative change of the K = 2^20 runs, rounded up to the next power of two times 2^-23.

Measured (largest relative change: the largest |change| / max(1, |ref|) of both seeds):
  case                              N        pow calls   K = 2^20: changed (+K, -K)   largest relative change
  sphere_N20000_s4_g                20 001       2 284     0, 0                         0
  sphere_N20000_s4_hgt              20 001       2 284     0, 0                         0
  sphere_N20000_s4_h_m04            20 001      46 712     0, 1                         3.7e-9  (0.03 x 2^-23)
  hub13_N50000_g                    50 001      12 576     14, 0                        2.6e-8  (0.22 x 2^-23)
  hub13_N50000_hgt                  50 001      12 916     21, 1                        1.1e-8  (0.09 x 2^-23)
  hub13_N50000_h_m04                50 001     112 456     2, 2                         1.5e-8  (0.12 x 2^-23)
  hub13_N50000_h_m06                50 001      70 285     4, 3                         1.5e-8  (0.12 x 2^-23)
  quantised_N20000_L4097_glacial    20 001         116     0, 0                         0
  quantised_N20000_hgt              20 001       2 123     0, 0                         0
  hub24_N200000_hgt                200 001      61 791     55, 31                       3.0e-8  (0.25 x 2^-23)
  hub24_N200000_long               200 001     160 039     78, 42                       4.5e-8  (0.38 x 2^-23)
  hub24_N200000_h_m06              200 001     262 065     41, 50                       3.0e-8  (0.25 x 2^-23)
  sphere_N200000_s3_hgt            200 001      14 682     8, 9                         3.7e-9  (0.03 x 2^-23)
  sphere_N200000_s3_h_m06          200 001     289 165     41, 20                       3.0e-8  (0.25 x 2^-23)
  post_N10000_s1_glacial            10 001       1 550     0, 0                         0
  post_N10000_s1_m06                10 001      14 000     0, 0                         0
  post_N10000_s1_glacial_corner     10 001       6 474     2, 1                         1.5e-8  (0.12 x 2^-23)
  hub22_N150000_glacial_corner     150 001     115 466     17, 76                       3.7e-8  (0.31 x 2^-23)
  K = 4, all four seeds: 0 cells changed in every case.
The largest relative change is 0.38 x 2^-23 (hub24_N200000_long, +K); 4 x 0.38 = 1.5, so ERODE_ULP_BOUND = 2 x 2^-23.
"""
import numpy as np
import pytest

import erode_common as EC

HOOK_LIVE_K = 2 ** 20
SEEDS_K4 = (1, 2, 3, 4)                 # all +K, all -K, two hashed
_by_2_20 = {}


@pytest.fixture(scope="module")
def libs():
    return EC.load_emulator(False), EC.load_emulator(True)


def _relative(got, ref):
    d = np.abs(got.astype(np.float64) - ref.astype(np.float64)) / np.maximum(1.0, np.abs(ref.astype(np.float64)))
    return float(d.max()) if d.size else 0.0


def _moved_by_2_20(hooked, name, case, ref):
    """Per seed (+K, -K) of the K = 2^20 runs of one case: (cells changed, largest change, cells past the bound, largest relative
    change).  Kept per case name, so that the test of the rule reads what the sensitivity tests measured."""
    if name not in _by_2_20:
        rows = []
        for seed in (1, 2):
            hooked.emu_set_libm_perturb(seed, HOOK_LIVE_K)
            got = EC.emulate(hooked, case)
            rows.append(EC.deviation(got, ref) + (_relative(got, ref),))
        hooked.emu_set_libm_perturb(0, 0)
        _by_2_20[name] = rows
    return _by_2_20[name]


@pytest.mark.parametrize("name", list(EC.CASE_BUILDERS))
def test_libm_sensitivity(libs, name):
    plain, hooked = libs
    case = EC.CASE_BUILDERS[name]()
    N = case.N
    ref = EC.emulate(plain, case)
    assert not np.array_equal(ref, case.e0), f"{name}: the case changes nothing"
    hooked.emu_set_libm_perturb(0, 0)
    assert np.array_equal(EC.emulate(hooked, case), ref), f"{name}: the hook at K = 0 changed the field"
    npow, nasin = EC.libm_calls(hooked)
    print(f"{name}: N = {N}, libm calls: pow {npow}, asin {nasin}")
    assert npow > 0, "the hook is not reached by the pow calls of the kernel bodies"
    assert nasin > 0 or not (case.args[7] > 0 and case.args[8] > 0), "the hook is not reached by the glacial index's asin"
    for seed, (n, m, over, rel) in zip((1, 2), _moved_by_2_20(hooked, name, case, ref)):
        print(f"{name}: K = 2^20, seed {seed}: {n} cells changed, largest change {m:.3g} ({rel:.3g} relative to max(1, |ref|), {rel / 2.0 ** -23:.2f} x 2^-23)")
        assert over == 0, f"{name}: K = 2^20, seed {seed} moved {over} cells past the per-cell bound (largest change {m:.3g})"
        # the 4x rule: the bound is at least four times whatever this perturbation does
        assert 4 * rel <= EC.ERODE_ULP_BOUND, f"{name}: K = 2^20, seed {seed}: 4 x {rel:.3g} exceeds ERODE_ULP_BOUND {EC.ERODE_ULP_BOUND:.3g}"
    cap = EC.diff_cap(N)
    for seed in SEEDS_K4:
        hooked.emu_set_libm_perturb(seed, EC.HOOK_K)
        got = EC.emulate(hooked, case)
        n, m, over = EC.deviation(got, ref)
        print(f"{name}: K = {EC.HOOK_K}, seed {seed}: " + (f"{n} cells changed, largest change {m:.3g}" if n else "no change"))
        assert over == 0, f"{name}: K = {EC.HOOK_K}, seed {seed}: {over} cells past the per-cell bound"
        assert 10 * n <= cap, f"{name}: K = {EC.HOOK_K}, seed {seed}: {n} cells changed, more than a tenth of the cap {cap}"
    hooked.emu_set_libm_perturb(0, 0)


def test_libm_hook_is_live_and_the_bound_follows_the_rule(libs):
    """At least one case moved under K = 2^20 (else the sensitivity tests prove nothing), and ERODE_ULP_BOUND is the next power of two
    times 2^-23 at or above 4 x the largest relative change of all cases, no looser than assignElevation's 4 x 2^-23."""
    import elev_inputs as EI
    plain, hooked = libs
    for name, build in EC.CASE_BUILDERS.items():
        if name not in _by_2_20:                        # (run on its own: measure here what test_libm_sensitivity would have)
            case = build()
            _moved_by_2_20(hooked, name, case, EC.emulate(plain, case))
    rows = [r for name in EC.CASE_BUILDERS for r in _by_2_20[name]]
    assert sum(r[0] for r in rows) > 0, "K = 2^20 changed no cell of any case: the hook is not live"
    worst = max(r[3] for r in rows)
    want = 2.0 ** -23
    while want < 4 * worst:
        want *= 2
    print(f"largest relative change {worst:.3g} ({worst / 2.0 ** -23:.2f} x 2^-23): the rule gives {want / 2.0 ** -23:.0f} x 2^-23")
    assert EC.ERODE_ULP_BOUND == want, (EC.ERODE_ULP_BOUND, want)
    assert EC.ERODE_ULP_BOUND <= EI.ULP_BOUND


def test_the_bar_sees_one_cell_and_one_row():
    """The defects the RMS bar let through, on arrays alone: one cell of 50 000 off by 1e-4, and a hub with its row (40 cells) off
    by 1e-5, both pass rms < 1e-5 and both fail check_cells; the unchanged field and three cells moved by one float32 ulp pass."""
    rng = np.random.default_rng(1)
    N = 50000
    ref = rng.uniform(-0.5, 1.5, N).astype(np.float32)
    assert EC.check_cells("unchanged", ref.copy(), ref, N)
    one = ref.copy()
    one[12345] += np.float32(1e-4)
    assert EC.rms(one, ref) < EC.RMS_TOL
    with pytest.raises(AssertionError, match="past"):
        EC.check_cells("one cell off by 1e-4", one, ref, N)
    row = ref.copy()
    cells = rng.choice(N, 40, replace=False)
    row[cells] += np.float32(1e-5)
    assert EC.rms(row, ref) < EC.RMS_TOL
    assert EC.deviation(row, ref)[0] == 40
    with pytest.raises(AssertionError, match="past"):
        EC.check_cells("a hub and its row off by 1e-5", row, ref, N)
    ulp = ref.copy()
    three = rng.choice(N, 3, replace=False)
    ulp[three] = np.nextafter(ulp[three], np.float32(np.inf))
    assert EC.deviation(ulp, ref)[0] == 3
    assert EC.check_cells("three cells one ulp up", ulp, ref, N)
    # more cells than the cap, each within the bound: the cap alone refuses it; a NaN is past the bound
    many = ref.copy()
    many[:EC.diff_cap(N) + 1] = np.nextafter(many[:EC.diff_cap(N) + 1], np.float32(np.inf))
    with pytest.raises(AssertionError, match="cap"):
        EC.check_cells("one cell past the cap", many, ref, N)
    nan = ref.copy()
    nan[7] = np.nan
    with pytest.raises(AssertionError, match="past"):
        EC.check_cells("a NaN", nan, ref, N)
