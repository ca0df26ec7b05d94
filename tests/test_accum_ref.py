"""CPU tests of the accumulators' exact reference (tests/accum_ref.py) and of the host helpers
dcor_accum_merge / dcor_accum_finalize against it ("Accumulators against an exact
reference"): the reference against values written out by hand, dcor.sim.r_cover and detail_frame
against the truth table, a restatement of the device's double-double steps showing that the error
bound of accum_ref.assert_accum is reachable and that a plain float64 sum misses it, and the two
host helpers on every builder."""
import math
from fractions import Fraction as F

import numpy as np
import pytest

import accum_ref as R

NAN = float("nan")
INF = float("inf")
RHOS = (0.0, 0.5, -1.0, 1.0)
COUNT = 4097     # three accumulate blocks of 1,366 records


def _records(name, rho=0.5):
    return R.BUILDERS[name](COUNT, rho) if name in R.BUILDERS else R.na_classes(rho, 7)


ALL = tuple(R.BUILDERS) + ("na_classes",)


# ------------------------------------------------------- the reference itself
def test_cover_truth_table_by_hand():
    T, Fa, NA = R.TRUE, R.FALSE, R.NA
    hand = [
        ((0.5, NAN, 0.25), Fa),     # NA & FALSE = FALSE: hi < rho decides alone
        ((0.5, NAN, 0.75), NA),     # NA & TRUE = NA
        ((0.5, NAN, 0.5), NA),      # rho on hi: TRUE, so still NA
        ((0.5, 0.75, NAN), Fa),     # FALSE & NA = FALSE
        ((0.5, 0.25, NAN), NA),
        ((0.5, NAN, NAN), NA),
        ((0.5, 0.5, 0.75), T),      # rho on lo
        ((0.5, 0.25, 0.5), T),      # rho on hi
        ((0.5, 0.5, 0.5), T),
        ((0.5, 0.75, 1.0), Fa),
        ((0.5, 0.0, 0.25), Fa),
        ((0.0, -0.0, 0.0), T),      # signed zeros compare equal
        ((-1.0, -1.0, -0.5), T),
        ((0.5, -INF, INF), T),
        ((0.5, INF, NAN), Fa),
    ]
    for (rho, lo, hi), want in hand:
        assert R.cover3(rho, lo, hi) == want, (rho, lo, hi)
        rec = np.array([[0.0, lo, hi, 0.0, hi, lo]])
        c = R.exact_counts(rec, rho, 0)
        assert (c["n_cover"], c["n_cover_na"]) == (int(want == T), int(want == NA)), (rho, lo, hi)
    assert len(R.AND3) == 9 and all(R.AND3[(a, b)] == R.AND3[(b, a)] for a, b in R.AND3)


def test_exact_accum_and_summary_by_hand():
    rho = 0.5
    est = np.array([0.25, 0.5, 0.75])
    rec = np.stack([est, est - 0.25, est + 0.25, -est, est, est], axis=1)   # INT: lo = hi
    ex = R.exact_accum(rec, rho, 0)
    assert ex == {"n": 3, "n_cover": 3, "n_cover_na": 0, "n_na_est": 0, "n_na_ci": 0, "est": F(3, 2),
                  "est2": F(7, 8), "se2": F(1, 8), "len": F(3, 2), "lo": F(3, 4), "hi": F(9, 4)}
    assert R.sum_abs(rec, rho, 1)["est"] == F(3, 2) and R.exact_accum(rec, rho, 1)["est"] == F(-3, 2)
    s = R.exact_summary(ex, rho)
    assert s == {"mse": F(1, 24), "bias": F(0), "var": F(1, 16), "coverage": F(1), "ci_length": F(1, 2)}
    # INT: estimates -0.25, -0.5, -0.75 against rho 0.5; lo = hi = est covers only at est = rho
    si = R.exact_summary(R.exact_accum(rec, rho, 1), rho)
    assert si["bias"] == F(-1) and si["coverage"] == F(1, 3) and si["ci_length"] == 0
    assert si["mse"] == (F(9, 16) + 1 + F(25, 16)) / 3
    # an NA estimate beside a finite CI: mse, bias, var NA; coverage and ci_length stay
    rec2 = np.vstack([rec, [NAN, 0.0, 1.0, 0.0, 0.0, 0.0]])
    s2 = R.exact_summary(R.exact_accum(rec2, rho, 0), rho)
    assert (s2["mse"], s2["bias"], s2["var"]) == (None, None, None)
    assert s2["coverage"] == F(1) and s2["ci_length"] == F(5, 8)
    # one NA endpoint with the other deciding FALSE: ci_length NA, coverage not
    rec3 = np.vstack([rec, [0.5, NAN, 0.25, 0.0, 0.0, 0.0]])
    s3 = R.exact_summary(R.exact_accum(rec3, rho, 0), rho)
    assert s3["ci_length"] is None and s3["coverage"] == F(3, 4) and s3["mse"] == F(1, 32)
    rec4 = np.vstack([rec, [0.5, NAN, 0.75, 0.0, 0.0, 0.0]])
    assert R.exact_summary(R.exact_accum(rec4, rho, 0), rho)["coverage"] is None
    # n = 1: var NA, the rest defined; n = 0: everything NA
    s1 = R.exact_summary(R.exact_accum(rec[:1], rho, 0), rho)
    assert s1["var"] is None and s1["mse"] == F(1, 16) and s1["bias"] == F(-1, 4)
    assert R.exact_summary(R.exact_accum(rec[:0], rho, 0), rho) == dict.fromkeys(R.SUMMARY)


def test_terms_are_the_float64_terms():
    """se2 is fl(fl(est - rho)^2) and est2 is fl(est * est): rounded where float64 rounds, zero
    where the product underflows."""
    rec = np.array([[1.0 + 2.0 ** -52, 0.0, 0.0, 2.0 ** -600, 0.0, 0.0]])
    t = R.terms(rec, 1.0 / 3.0, 0)
    assert t["est2"][0] == 1.0 + 2.0 ** -51 and F(float(t["est2"][0])) != F(1 + F(1, 2 ** 52)) ** 2
    d = (1.0 + 2.0 ** -52) - 1.0 / 3.0
    assert t["se2"][0] == d * d
    assert R.terms(rec, 0.0, 1)["est2"][0] == 0.0


@pytest.mark.parametrize("name", ALL)
def test_exact_sums_equal_fraction_sums(name):
    rec = _records(name)[:700]
    for meth in (0, 1):
        ex, sabs = R.exact_accum_abs(rec, 0.5, meth)
        for k, t in R.terms(rec, 0.5, meth).items():
            assert ex[k] == sum(map(F, t.tolist()), F(0)), (name, meth, k)
            assert sabs[k] == sum((abs(F(x)) for x in t.tolist()), F(0)), (name, meth, k)


def test_partition_and_builders():
    assert [R.acc_nblocks(c) for c in (0, 1, 2048, 2049, 4097, 1 << 20, (1 << 20) + 1, 1 << 22)] == \
        [1, 1, 1, 2, 3, 512, 512, 512]
    assert [R.acc_per(c) for c in (1, 2048, 2049, 4097, 1 << 20, (1 << 20) + 1)] == [1, 2048, 1025, 1366, 2048, 2049]
    assert R.boundary_indices(4097) == [0, 63, 64, 255, 256, 1365, 1366, 4096]
    assert R.boundary_indices(2) == [0, 1] and R.boundary_indices(0) == []
    assert R.giant_indices(4097) == (1365, 1366) and R.giant_indices(2048) == (0, 64)
    for name, b in R.BUILDERS.items():
        rec = b(COUNT, 0.5)
        assert rec.shape == (COUNT, 6) and np.array_equal(rec, b(COUNT, 0.5), equal_nan=True)
        assert not np.array_equal(rec[:, :3], rec[:, 3:], equal_nan=True), name   # a wrong method offset shows
        for i in R.boundary_indices(COUNT):
            if name != "giant" or i not in R.giant_indices(COUNT):
                assert np.isnan(rec[i]).any() or (rec[i] == 0.5).any(), (name, i)
        for c in (0, 1, 2):
            assert b(c, 0.5).shape == (c, 6)
    g = R.giant(COUNT, 0.5)
    assert g[1365, 0] == 2.0 ** 60 and g[1366, 0] == -(2.0 ** 60)
    t = R.terms(R.tiny(COUNT, 0.0), 0.0, 0)
    assert np.all(t["est2"] == 0.0) and np.any(t["est"] != 0.0)
    c = R.cancelling(COUNT, 0.5)
    ex, sabs = R.exact_accum_abs(c, 0.5, 0)
    assert abs(ex["est"]) * 2000 < sabs["est"]


@pytest.mark.parametrize("rho", RHOS)
def test_na_classes_counts_r_cover_and_detail_frame(rho):
    """The 40 classes' counters by class arithmetic, by the truth table over the records, and by
    dcor.sim.r_cover / detail_frame: all the same."""
    from dcor.sim import detail_frame, r_cover
    for r in (3, 7):
        rec = R.na_classes(rho, r)
        assert rec.shape == (40 * r, 6)
        d = detail_frame(rec, rho)
        for meth, m in enumerate(("ni", "int")):
            want = R.na_class_counts(rho, r, meth)
            assert R.exact_counts(rec, rho, meth) == want
            assert len(set(want.values())) == 5, want       # no two counters coincide
            lo, hi = rec[:, 3 * meth + 1], rec[:, 3 * meth + 2]
            ref = np.array([R.cover3(rho, a, b) for a, b in zip(lo.tolist(), hi.tolist())])
            for cov in (r_cover(rho, lo, hi), d[f"{m}_cover"]):
                assert np.array_equal(np.isnan(cov), ref == R.NA)
                assert np.array_equal(cov == 1.0, ref == R.TRUE) and np.array_equal(cov == 0.0, ref == R.FALSE)
            t = R.terms(rec, rho, meth)
            assert np.array_equal(d[f"{m}_se2"][~np.isnan(rec[:, 3 * meth])], t["se2"])
            assert np.array_equal(d[f"{m}_ci_len"][~(np.isnan(lo) | np.isnan(hi))], t["len"])
    assert sorted(R.na_class_runs(3)) == [1] * 8 + [2] * 8 + [3] * 8 + [4] * 8 + [5] * 8


# ------------------------------------------- the bound is reachable and has teeth
def two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def ks_acc(acc, x):             # dcor_device.h: TwoSum into hi, the errors added plainly into lo
    s = acc[0] + x
    bb = s - acc[0]
    return s, acc[1] + ((acc[0] - (s - bb)) + (x - bb))


def dd_fold_step(a, b):         # unnormalised fold of two partials
    s, e = two_sum(a[0], b[0])
    return s, (a[1] + b[1]) + e


def dd_add(a, b):
    s, se = two_sum(a[0], b[0])
    t, te = two_sum(a[1], b[1])
    r, re = two_sum(s, se + t)
    return two_sum(r, re + te)


def dd_model(t, count):
    """The double-double steps of the accumulate path over one term array in a thread-strided
    order: per block of acc_per(count) records 256 compensated per-thread sums, a pairwise
    dd_fold_step tree over the threads closed by two_sum, then dd_add over the blocks.  The term
    array lists the records that passed the NaN test, so a thread's records here are not always
    the kernel's: this checks the inputs and the bound, not the kernel's exact order."""
    per, tot = max(R.acc_per(count), 1), (0.0, 0.0)
    for b0 in range(0, max(len(t), 1), per):
        blk = t[b0:b0 + per]
        th = []
        for i in range(256):
            a = (0.0, 0.0)
            for x in blk[i::256]:
                a = ks_acc(a, x)
            th.append(a)
        while len(th) > 1:
            th = [dd_fold_step(th[i], th[i + 1]) for i in range(0, len(th), 2)]
        tot = dd_add(tot, two_sum(*th[0]))
    return tot


@pytest.mark.parametrize("name", ALL)
def test_double_double_restatement_meets_the_bound(name, capsys):
    rho = 0.5
    rec = _records(name, rho)
    count = rec.shape[0]
    worst = 0.0
    for meth in (0, 1):
        ex, sabs = R.exact_accum_abs(rec, rho, meth)
        for k, t in R.terms(rec, rho, meth).items():
            hi, lo = dd_model(t.tolist(), count)
            bound = max(count, 1024) * R.TWO100 * sabs[k]
            err = abs(F(hi) + F(lo) - ex[k])
            assert err <= bound, (name, meth, k, float(err), float(bound))
            assert abs(F(lo)) * 2 ** 53 <= abs(F(hi))
            worst = max(worst, float(err / bound) if bound else 0.0)
    with capsys.disabled():
        print(f"\n  dd restatement, {name}: worst error / bound = {worst:.3e}")


@pytest.mark.parametrize("name,which", [("cancelling", ("est", "lo", "hi")), ("giant", ("est", "lo", "hi"))])
def test_plain_float64_sum_misses_the_bound(name, which):
    """A float64 running sum of the same terms -- what an accumulator without its low words is --
    misses the bound by at least 2^20 on the sums that cancel: est, lo and hi of `cancelling`
    (terms of 2^27 whose sum is of order 2^27) and of `giant` (a +2^60 and a -2^60 among terms of
    order 1)."""
    rho = 0.5
    rec = _records(name, rho)
    for meth in (0, 1):
        ex, sabs = R.exact_accum_abs(rec, rho, meth)
        t = R.terms(rec, rho, meth)
        for k in which:
            s = 0.0
            for x in t[k].tolist():
                s += x
            bound = max(COUNT, 1024) * R.TWO100 * sabs[k]
            assert abs(F(s) - ex[k]) >= 2 ** 20 * bound, (name, meth, k, float(abs(F(s) - ex[k]) / bound))


# --------------------------------------------------------------- host helpers
def dd_pair(x):
    """A Fraction as a correctly rounded (hi, lo) pair."""
    hi = float(x)
    return hi, float(x - F(hi))


def accum_of(rec, rho, meth):
    """A dcor_accum holding the exact reference of `rec`, its sums rounded to (hi, lo) pairs."""
    from dcor import _lib
    ex = R.exact_accum(rec, rho, meth)
    a = _lib.Accum()
    for k in ("n",) + R.COUNTERS:
        setattr(a, k, ex[k])
    for k in R.SUMS:
        w = getattr(a, k)
        w[0], w[1] = dd_pair(ex[k])
    return a


def split_points(count, parts):
    """Cut points of `parts` consecutive ranges, some of them empty (the first, and every third)."""
    if parts == 1:
        return [0, count]
    cuts = sorted((count * j) // (parts - 1) for j in range(parts - 1))
    cuts = [0, 0] + cuts[1:] + [count]
    for j in range(3, len(cuts) - 1, 3):
        cuts[j] = cuts[j - 1]
    return cuts


@pytest.mark.parametrize("parts", (1, 2, 3, 7))
@pytest.mark.parametrize("name", ALL)
def test_host_merge_vs_exact(name, parts):
    from dcor.sim import merge
    rho = 0.5
    rec = _records(name, rho)
    cuts = split_points(rec.shape[0], parts)
    assert len(cuts) == parts + 1 and cuts[0] == 0 and cuts[-1] == rec.shape[0]
    assert parts == 1 or any(a == b for a, b in zip(cuts, cuts[1:]))
    for meth in (0, 1):
        got = merge([accum_of(rec[a:b], rho, meth) for a, b in zip(cuts, cuts[1:])])
        ex, sabs = R.exact_accum_abs(rec, rho, meth)
        what = f"{name} in {parts} parts, method {meth}"
        R.assert_counts(got, ex, what)
        R.assert_normalised(got, what)
        R.assert_sums(got, ex, sabs, parts, what)


def test_host_merge_keeps_the_low_words():
    """1 + 2^-80 merged with -1: the sum is the low word alone."""
    from dcor import _lib
    from dcor.sim import merge
    a, b = _lib.Accum(), _lib.Accum()
    a.n, b.n = 1, 1
    for k in R.SUMS:
        getattr(a, k)[0], getattr(a, k)[1] = 1.0, 2.0 ** -80
        getattr(b, k)[0] = -1.0
    m = merge([a, b])
    assert m.n == 2 and all(R.stored(m, k) == (2.0 ** -80, 0.0) for k in R.SUMS)


def _finalize(rec, rho, meth):
    from dcor.sim import finalize
    return finalize(accum_of(rec, rho, meth), rho)


@pytest.mark.parametrize("rho", RHOS)
@pytest.mark.parametrize("name", ("benign", "cancelling", "giant", "na_classes"))
def test_host_finalize_vs_exact_summary(name, rho):
    """finalize on the builders' records: as built (NA estimates, covers and endpoints present, so
    the NA rules decide), without the records that hold a NaN (every column finite, so the bounds
    decide), and on prefixes of 0, 1 and 2 records."""
    rec = _records(name, rho)
    for meth in (0, 1):
        clean = rec[~np.isnan(rec[:, 3 * meth:3 * meth + 3]).any(axis=1)]
        assert 0 < clean.shape[0] < rec.shape[0]
        for r, tag in ((rec, "as built"), (clean, "finite"), (clean[:0], "n=0"), (clean[:1], "n=1"), (clean[:2], "n=2")):
            got = _finalize(r, rho, meth)
            R.assert_summary(got, r, rho, meth, f"{name} {tag} rho {rho} method {meth}")
        assert all(math.isnan(v) for v in _finalize(clean[:0], rho, meth).values())
        one = _finalize(clean[:1], rho, meth)
        assert math.isnan(one["var"]) and not math.isnan(one["mse"]) and not math.isnan(one["coverage"])
        full = _finalize(clean, rho, meth)
        assert not any(math.isnan(v) for v in full.values())
        raw = _finalize(rec, rho, meth)
        assert math.isnan(raw["mse"]) and math.isnan(raw["bias"]) and math.isnan(raw["var"])
        assert math.isnan(raw["ci_length"])


def test_host_finalize_na_rules_one_at_a_time():
    """Each NA source alone: an NA estimate beside a finite CI, lo NA with hi < rho (cover FALSE,
    not NA), lo NA with hi > rho (cover NA)."""
    rho = 0.5
    base = R.benign(300, rho)
    base = base[~np.isnan(base).any(axis=1)][:200]
    for row, na in (([NAN, 0.25, 0.75], {"mse", "bias", "var"}),
                    ([0.5, NAN, 0.25], {"ci_length"}),
                    ([0.5, NAN, 0.75], {"ci_length", "coverage"}),
                    ([0.5, 0.75, NAN], {"ci_length"}),
                    ([NAN, NAN, NAN], set(R.SUMMARY))):
        rec = base.copy()
        rec[100, 0:3] = row
        got = _finalize(rec, rho, 0)
        assert {k for k, v in got.items() if math.isnan(v)} == na, (row, got)
        R.assert_summary(got, rec, rho, 0, str(row))
        R.assert_summary(_finalize(rec, rho, 1), rec, rho, 1, str(row))   # the INT columns are untouched


@pytest.mark.parametrize("rho", (0.0, 0.5))
def test_host_finalize_tiny(rho):
    """Results in double's subnormal range (means of +-2^-1060 and subnormals against rho = 0): the
    long-double quotient is exact to 2^-64 but its conversion to double rounds to a multiple of
    2^-1074, so half of that is added to the relative bounds here, and only here."""
    rec = R.tiny(COUNT, rho)
    for meth in (0, 1):
        clean = rec[~np.isnan(rec[:, 3 * meth:3 * meth + 3]).any(axis=1)]
        R.assert_summary(_finalize(clean, rho, meth), clean, rho, meth, f"tiny rho {rho}", floor=F(1, 2 ** 1075))
        R.assert_summary(_finalize(rec, rho, meth), rec, rho, meth, f"tiny as built rho {rho}", floor=F(1, 2 ** 1075))


def test_host_finalize_near_constant_estimates(capsys):
    """1,000 estimates of mean 0.9 and spread 1e-7.  var comes from the one-pass formula
    (sum est^2 - (sum est)^2 / n) / (n - 1), whose two terms are each about 810 while their
    difference is about 1e-11: the bound 2^-52 var + 2^-60 sum est^2 / (n - 1) is about
    2^-60 * 0.81 = 7.0e-19 absolute against var = 1e-14, so it leaves var a relative accuracy of
    about 7e-5 here (the long-double arithmetic itself, 2^-64 per operation, measures about 1e-6 or
    better; printed below).  That is the known limit of the one-pass formula, not changed here."""
    g = np.random.default_rng(77)
    n, rho = 1000, 0.9
    rec = np.empty((n, 6))
    for meth in (0, 1):
        est = 0.9 + 1e-7 * g.standard_normal(n)
        rec[:, 3 * meth:3 * meth + 3] = np.stack([est, est - 0.05 * (meth + 1), np.minimum(est + 0.05, 1.0)], axis=1)
    for meth in (0, 1):
        got = _finalize(rec, rho, meth)
        R.assert_summary(got, rec, rho, meth, "near-constant")
        s, b = R.summary_bounds(rec, rho, meth)
        rel_bound, rel_got = float(b["var"] / s["var"]), float(abs(F(got["var"]) - s["var"]) / s["var"])
        assert 3e-5 < rel_bound < 2e-4 and 0.5e-14 < float(s["var"]) < 2e-14
        with capsys.disabled():
            print(f"\n  near-constant var, method {meth}: bound {rel_bound:.2e} relative, measured {rel_got:.2e}")
