"""References for the engine's one-pass sample variance (dd_var, csrc/dcor_device.h): the exact
two-pass variance in rationals, the error bound the kernel's arithmetic is entitled to, and an
emulation of dd_var's own operations (doubles, with every fma rounded once from exact rationals).

The bound.  The kernels add x and fl(x^2) (or fl(fl(x0^2) + fl(x1^2)) for a pair of samples) into
compensated sums and dd_var forms (S2 - S1^2 / n) / (n - 1).  Each square is rounded once
(relative 2^-53) and once more in the paired form, so S2 is off by at most 2 * 2^-53 * sum x^2; the
compensated sums and the double-double products add O(n 2^-106).  With a factor 2 over that for the
division and the final hi + lo rounding:

    |var_kernel - var_exact| <= B = 4 * 2^-53 * sum x^2 / (n - 1),

and, since |sqrt a - sqrt b| <= sqrt |a - b|,  |sd_kernel - sd_exact| <= sqrt B.  B is derived, not
measured.  dd_var returns 0 when the two sums are exactly those of a constant sample, and for a
negative value; both stay inside B (a sample with a constant's sums has a variance below the
rounding of its squares)."""
import math
from fractions import Fraction

U = Fraction(1, 2 ** 53)


def exact_var(xs):
    """The two-pass sample variance (n - 1) of a list of doubles, as an exact rational."""
    fx = [Fraction(float(x)) for x in xs]
    n = len(fx)
    if n < 2:
        raise ValueError("exact_var needs two values")
    mean = sum(fx) / n
    return sum((x - mean) ** 2 for x in fx) / (n - 1)


def var_bound(xs):
    """B = 4 * 2^-53 * sum x^2 / (n - 1), as an exact rational."""
    fx = [Fraction(float(x)) for x in xs]
    return 4 * U * sum(x * x for x in fx) / (len(fx) - 1)


def sd_bound(xs):
    """sqrt B as a double, rounded up."""
    return math.nextafter(math.sqrt(float(var_bound(xs))), math.inf)


# ---------------------------------------------------------------- dd_var's operations, emulated
def _fma(a, b, c):
    if not (math.isfinite(a) and math.isfinite(b) and math.isfinite(c)):
        return a * b + c   # NaN and infinities propagate as in the device's fma
    return float(Fraction(a) * Fraction(b) + Fraction(c))   # float(Fraction) rounds to nearest even


def _two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def _two_prod(a, b):
    p = a * b
    return p, _fma(a, b, -p)


def _ks_acc(acc, x):
    hi, lo = acc
    s = hi + x
    bb = s - hi
    return s, lo + ((hi - (s - bb)) + (x - bb))


def _dd_add(a, b):
    s, se = _two_sum(a[0], b[0])
    t, te = _two_sum(a[1], b[1])
    r, re = _two_sum(s, se + t)
    return _two_sum(r, re + te)


def _dd_mul(a, b):
    p, pl = _two_prod(a[0], b[0])
    pl = _fma(a[0], b[1], pl)
    pl = _fma(a[1], b[0], pl)
    return _two_sum(p, pl)


def _dd_div_d(a, b):
    q1 = a[0] / b
    p = _two_prod(q1, b)
    r = _dd_add(a, (-p[0], -p[1]))
    return _two_sum(q1, r[0] / b)


def emulate_dd_var(xs, paired=False, clamp=True, constant=True):
    """dd_var on the sums one thread would form over xs in index order: x into S1 and fl(x * x) into
    S2 (paired: x0 + x1 and fl(x0 * x0) + fl(x1 * x1), two samples at a time, as the INT loops do).
    constant = False: without the recognition of a constant sample's sums (S1 == n q and
    S2 == n fl(q q) exactly, q = fl(S1 / n): the variance is 0); clamp = False: the sign of the
    value is kept.  Both False: dd_var as it was before either."""
    xs = [float(x) for x in xs]
    n = float(len(xs))
    if not n >= 2:
        return math.nan
    s1, s2 = (0.0, 0.0), (0.0, 0.0)
    if paired:
        if len(xs) % 2:
            xs = xs + [0.0]
        for a, b in zip(xs[0::2], xs[1::2]):
            s1 = _ks_acc(s1, a + b)
            s2 = _ks_acc(s2, a * a + b * b)
    else:
        for x in xs:
            s1 = _ks_acc(s1, x)
            s2 = _ks_acc(s2, x * x)
    mean = _dd_div_d(s1, n)
    if constant:
        q = mean[0] + mean[1]
        if (_two_sum(*s1), _two_sum(*s2)) == (_two_prod(n, q), _two_prod(n, q * q)):
            return 0.0
    m = _dd_mul(s1, mean)
    c = _dd_add(s2, (-m[0], -m[1]))
    v = _dd_div_d(c, n - 1.0)
    var = v[0] + v[1]
    return 0.0 if clamp and var < 0.0 else var
