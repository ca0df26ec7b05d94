"""CPU tests of tests/ddvar_ref.py: the exact variance and the bound B on hand-worked cases, and the
emulation of dd_var (csrc/dcor_device.h) on the inputs tests/test_gpu_variance_edges.py gives the
device -- constants, whose exact variance is 0 and whose one-pass numerator is rounding residue of
either sign, and nearly constant data."""
import math
from fractions import Fraction

import numpy as np
import pytest

import ddvar_ref as V

CONSTANTS = [0.3, 0.7, 1.1, 1.7, 2.0 / 3.0]


def test_exact_var_hand_worked():
    assert V.exact_var([1.0, 2.0, 3.0, 4.0]) == Fraction(5, 3)
    assert V.exact_var([2.0, 4.0, 4.0, 4.0, 5.0, 5.0, 7.0, 9.0]) == Fraction(32, 7)
    assert V.exact_var([-1.5, 1.5]) == Fraction(9, 2)
    # the doubles themselves, not the decimals they print as: 0.1 + 2^-55 = 3602879701896397 / 2^55
    a = Fraction(0.1)
    assert a == Fraction(3602879701896397, 2 ** 55)
    assert V.exact_var([0.1, 0.3]) == (Fraction(0.3) - a) ** 2 / 2
    with pytest.raises(ValueError):
        V.exact_var([1.0])


@pytest.mark.parametrize("c", CONSTANTS + [-1.7, 1e300, 5e-324])
def test_exact_var_of_a_constant_is_zero(c):
    assert V.exact_var([c] * 1000) == 0


def test_bound_hand_worked():
    # sum x^2 = 30, n - 1 = 3: B = 4 * 2^-53 * 10 = 40 * 2^-53
    assert V.var_bound([1.0, 2.0, 3.0, 4.0]) == Fraction(40, 2 ** 53)
    assert V.var_bound([2.0] * 5) == Fraction(4 * 20, 4 * 2 ** 53)
    sb = V.sd_bound([1.0, 2.0, 3.0, 4.0])
    assert Fraction(sb) ** 2 >= V.var_bound([1.0, 2.0, 3.0, 4.0])
    assert sb == pytest.approx(math.sqrt(40.0) * 2.0 ** -26.5, rel=1e-15)


def test_emulation_exact_on_small_integers():
    """Every square and sum is exact: the one-pass value is the correctly rounded variance."""
    for xs in ([1.0, 2.0, 3.0, 4.0], [2.0, 4.0, 4.0, 4.0, 5.0, 5.0, 7.0, 9.0], [3.0] * 17, [0.0] * 9):
        want = float(V.exact_var(xs))
        for paired in (False, True):
            assert V.emulate_dd_var(xs, paired=paired) == want
            assert V.emulate_dd_var(xs, paired=paired, clamp=False, constant=False) == want
    assert math.isnan(V.emulate_dd_var([1.0]))


@pytest.mark.parametrize("paired", [False, True])
def test_constant_input_residue_has_either_sign_and_the_clamp_removes_the_negative(paired):
    """n copies of c, without the recognition of a constant: S2 - S1^2 / n = n (fl(c^2) - c^2) up to
    O(n 2^-106), so the value has the sign of the square's rounding error -- negative for some of
    the constants, positive for others -- and lies within B of the exact 0.  Clamped, it is never
    negative, but a positive residue stays."""
    signs = set()
    for c in CONSTANTS:
        xs = [c] * 1000
        raw = V.emulate_dd_var(xs, paired=paired, clamp=False, constant=False)
        err = Fraction(c * c) - Fraction(c) ** 2
        assert (raw > 0) == (err > 0) and (raw < 0) == (err < 0), (c, raw)
        assert abs(Fraction(raw)) <= V.var_bound(xs), (c, raw)
        got = V.emulate_dd_var(xs, paired=paired, constant=False)
        assert got == (raw if raw > 0 else 0.0) and not math.copysign(1.0, got) < 0, (c, got)
        signs.add(raw > 0)
    assert signs == {True, False}
    # a NaN stays a NaN
    assert math.isnan(V.emulate_dd_var([1.0, math.nan, 2.0], paired=paired))


@pytest.mark.parametrize("paired", [False, True])
@pytest.mark.parametrize("n", [2, 3, 125, 1000, 1001])
def test_constant_sample_is_recognised_exactly(n, paired):
    """The sums of n copies of c are n c and n fl(c c) without rounding (odd n, paired: the last pair
    is (c, 0)), so dd_var returns exactly 0 for every constant, whatever the sign of its residue."""
    for c in CONSTANTS + [-1.7, 8 * 0.3 * 0.3, 1e-160, 3e150]:
        assert V.emulate_dd_var([c] * n, paired=paired) == 0.0, c


def test_recognition_fires_on_nothing_but_a_constants_sums():
    """One value moved by one ulp, or by a part in 1e9, is not a constant: the value is what the
    one-pass arithmetic gives (within B), not 0 -- unless the clamp applies."""
    for c in CONSTANTS:
        for d in (math.nextafter(c, math.inf), c * (1.0 + 1e-9), -c):
            xs = [c] * 999 + [d]
            a = V.emulate_dd_var(xs)
            assert a == V.emulate_dd_var(xs, constant=False), (c, d)
            assert abs(Fraction(a) - V.exact_var(xs)) <= V.var_bound(xs)
    xs = [1.3 * (1.0 + 1e-7 * math.sin(i)) for i in range(2000)]
    assert V.emulate_dd_var(xs) == V.emulate_dd_var(xs, constant=False) != 0.0


@pytest.mark.parametrize("cv", [1e-3, 1e-5, 1e-7])
def test_nearly_constant_input_stays_within_the_bound(cv):
    """mean 1.3, n = 2,000: the relative error of the variance grows as the spread shrinks (of the
    order of 1e-12, 1e-8 and 1e-4 on this draw) and stays under B."""
    g = np.random.default_rng(20261021)
    xs = list(1.3 * (1.0 + cv * g.standard_normal(2000)))
    exact = V.exact_var(xs)
    for paired in (False, True):
        got = Fraction(V.emulate_dd_var(xs, paired=paired))
        assert abs(got - exact) <= V.var_bound(xs), (cv, float(got - exact))
        print(f"cv={cv} paired={paired}: relative error {float(abs(got - exact) / exact):.2e}, "
              f"B / var {float(V.var_bound(xs) / exact):.2e}")
    assert float(V.var_bound(xs) / exact) > 1e-10 * (1e-3 / cv) ** 2   # the bound is not slack by orders


def test_cancelling_sum():
    """+v, -v alternating: S1 = 0 exactly, the variance is n v^2 / (n - 1) to rounding."""
    v = 1.7
    xs = [v, -v] * 500
    want = float(V.exact_var(xs))
    for paired in (False, True):
        assert V.emulate_dd_var(xs, paired=paired) == pytest.approx(want, rel=4e-16)
