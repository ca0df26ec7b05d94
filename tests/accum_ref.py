"""Exact-rational reference of the summary accumulators (dcor_accum), hand-made record builders
and the checks the accumulator tests share ("Accumulators against an exact reference").

The device forms six float64 terms per record and method (acc_record, compiled without
contraction) and adds them as double-double; here the same float64 terms are formed with numpy and
added exactly as integers, so the reference has no rounding of its own beyond the terms'.  The cover
flag is R's three-valued `rho >= lo & rho <= hi` written as a truth table (vert-cor.R:405;
ver-cor-subG.R:203), independent of dcor.sim.r_cover.  No GPU and no library call in this file."""
import math
from fractions import Fraction

import numpy as np

SUMS = ("est", "est2", "se2", "len", "lo", "hi")
COUNTERS = ("n_cover", "n_cover_na", "n_na_est", "n_na_ci")
SUMMARY = ("mse", "bias", "var", "coverage", "ci_length")

# ------------------------------------------------------------- R's three-valued logic
TRUE, FALSE, NA = 1, 0, 2
# R's `&`: FALSE if either side is FALSE, else NA if either side is NA, else TRUE.
AND3 = {
    (TRUE, TRUE): TRUE, (TRUE, FALSE): FALSE, (TRUE, NA): NA,
    (FALSE, TRUE): FALSE, (FALSE, FALSE): FALSE, (FALSE, NA): FALSE,
    (NA, TRUE): NA, (NA, FALSE): FALSE, (NA, NA): NA,
}
_AND3_TABLE = np.array([[AND3[(a, b)] for b in (FALSE, TRUE, NA)] for a in (FALSE, TRUE, NA)])


def cover3(rho, lo, hi):
    """R's `rho >= lo & rho <= hi` for one record: TRUE, FALSE or NA (a comparison with NaN is NA)."""
    a = NA if lo != lo else (TRUE if rho >= lo else FALSE)
    b = NA if hi != hi else (TRUE if rho <= hi else FALSE)
    return AND3[(a, b)]


def _cover_codes(rho, lo, hi):
    with np.errstate(invalid="ignore"):
        a = np.where(np.isnan(lo), NA, np.where(rho >= lo, TRUE, FALSE))
        b = np.where(np.isnan(hi), NA, np.where(rho <= hi, TRUE, FALSE))
    return _AND3_TABLE[a, b]


# ------------------------------------------------------------------- exact sums
def exact_sums(v):
    """(sum, sum of magnitudes) of finite float64 values, exactly, as Fractions.  A value's bits
    give it as +-mant * 2^(e - 1075) with an integer mant < 2^53 (e = the biased exponent, 1 for
    subnormals); the mantissas are split into 27 + 26 bits and added per exponent in float64, which
    is exact below 2^53 (up to 2^21 values of at most 2^27), then the per-exponent totals are added
    as Python integers."""
    v = np.ascontiguousarray(v, dtype=np.float64).ravel()
    if v.size == 0:
        return Fraction(0), Fraction(0)
    assert v.size <= 1 << 21
    bits = v.view(np.int64)
    e = (bits >> 52) & 0x7FF
    assert not np.any(e == 0x7FF), "exact_sums: NaN or infinity among the terms"
    mant = (bits & ((1 << 52) - 1)) | ((e != 0).astype(np.int64) << 52)
    slot = np.maximum(e, 1) + ((bits >> 63) & 2048)            # negative values 2048 slots up
    hi = np.bincount(slot, weights=(mant >> 26).astype(np.float64), minlength=4096)
    lo = np.bincount(slot, weights=(mant & ((1 << 26) - 1)).astype(np.float64), minlength=4096)
    pos, neg = 0, 0
    for ex in np.nonzero(hi + lo)[0].tolist():                 # as integers scaled by 2^1074
        w = ((int(hi[ex]) << 26) + int(lo[ex])) << ((ex & 2047) - 1)
        if ex < 2048:
            pos += w
        else:
            neg += w
    return Fraction(pos - neg, 1 << 1074), Fraction(pos + neg, 1 << 1074)


def exact_sum(v):
    return exact_sums(v)[0]


def terms(records, rho, meth):
    """The six float64 term arrays acc_record adds for method `meth` (0 NI, 1 INT): est, fl(est^2),
    fl(fl(est - rho)^2) over the records whose estimate is not NaN; fl(hi - lo), lo, hi over the
    records with both endpoints not NaN."""
    rec = np.asarray(records, dtype=np.float64).reshape(-1, 6)
    est, lo, hi = rec[:, 3 * meth], rec[:, 3 * meth + 1], rec[:, 3 * meth + 2]
    oke = ~np.isnan(est)
    okc = ~(np.isnan(lo) | np.isnan(hi))
    e, l, h = est[oke], lo[okc], hi[okc]
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        d = e - np.float64(rho)
        return {"est": e, "est2": e * e, "se2": d * d, "len": h - l, "lo": l, "hi": h}


def exact_counts(records, rho, meth):
    """n and the four counters of method `meth` from the truth table."""
    rec = np.asarray(records, dtype=np.float64).reshape(-1, 6)
    est, lo, hi = rec[:, 3 * meth], rec[:, 3 * meth + 1], rec[:, 3 * meth + 2]
    cv = _cover_codes(np.float64(rho), lo, hi)
    return {"n": int(rec.shape[0]), "n_cover": int((cv == TRUE).sum()), "n_cover_na": int((cv == NA).sum()),
            "n_na_est": int(np.isnan(est).sum()), "n_na_ci": int((np.isnan(lo) | np.isnan(hi)).sum())}


def exact_accum(records, rho, meth):
    """The accumulator of method `meth` over float64 records [count, 6]: n, the four counters, and
    the six sums as Fractions."""
    return exact_accum_abs(records, rho, meth)[0]


def sum_abs(records, rho, meth):
    """Sum |term| of each of the six sums (the magnitude the error bounds are relative to)."""
    return exact_accum_abs(records, rho, meth)[1]


def exact_accum_abs(records, rho, meth):
    """(exact_accum, sum_abs) from one pass over the terms."""
    out, mag = exact_counts(records, rho, meth), {}
    for name, t in terms(records, rho, meth).items():
        out[name], mag[name] = exact_sums(t)
    return out, mag


def exact_summary(ex, rho):
    """run_sim_one's summary row from exact sums (vert-cor.R:422-430), None for NA: mean and
    var (n - 1) as R computes them, no na.rm -- any NA estimate makes mse, bias and var NA, any NA
    cover makes coverage NA, any NA endpoint makes ci_length NA, n = 0 makes everything NA and
    n = 1 makes var NA."""
    n = ex["n"]
    out = dict.fromkeys(SUMMARY)
    if n == 0:
        return out
    if ex["n_na_est"] == 0:
        out["mse"] = ex["se2"] / n
        out["bias"] = ex["est"] / n - Fraction(float(rho))
        if n >= 2:
            out["var"] = (ex["est2"] - ex["est"] * ex["est"] / n) / (n - 1)
    if ex["n_cover_na"] == 0:
        out["coverage"] = Fraction(ex["n_cover"], n)
    if ex["n_na_ci"] == 0:
        out["ci_length"] = ex["len"] / n
    return out


# ------------------------------------------------------ the launch's partition
def acc_nblocks(count):
    """Blocks dcor_accumulate_launch uses for `count` records: ceil(count / 2048) within [1, 512]."""
    return min(max(-(-count // 2048), 1), 512)


def acc_per(count):
    """Records per block: ceil(count / nblocks)."""
    return -(-count // acc_nblocks(count))


def boundary_indices(count):
    """The record indices at which the work split changes, below count: the first and last lane of
    a wave (0, 63, 64), the last thread of a workgroup and the first record of its second trip
    (255, 256), the last record of block 0 and the first of block 1 (per - 1, per), the last
    record."""
    per = acc_per(count) if count > 0 else 0
    return sorted({i for i in (0, 63, 64, 255, 256, per - 1, per, count - 1) if 0 <= i < count})


# ------------------------------------------------------------ record builders
_NAN = float("nan")
# (est, lo, hi) overwrites of a special record: None keeps the builder's value, "rho" writes rho
_SPECIALS = ((_NAN, None, None), (None, _NAN, None), (None, None, _NAN), (None, _NAN, _NAN),
             (_NAN, _NAN, _NAN), (None, "rho", None), (None, None, "rho"), (_NAN, "rho", None))


def _put_specials(rec, rho, with_rho=True):
    """Overwrite the records at boundary_indices with special ones, the NI and INT columns from
    different places of the cycle."""
    pats = _SPECIALS if with_rho else _SPECIALS[:5]
    for j, i in enumerate(boundary_indices(rec.shape[0])):
        for meth, shift in ((0, 0), (1, 3)):
            for f, v in enumerate(pats[(j + shift) % len(pats)]):
                if v is not None:
                    rec[i, 3 * meth + f] = rho if isinstance(v, str) else v
    return rec


def _benign_raw(count, seed):
    g = np.random.default_rng([seed, 11])
    rec = np.empty((count, 6))
    for meth, width in ((0, 0.5), (1, 0.2)):
        est = g.uniform(-1.0, 1.0, count)
        w = g.uniform(0.01, width, count)
        rec[:, 3 * meth] = est
        rec[:, 3 * meth + 1] = np.clip(est - w, -1.0, 1.0)
        rec[:, 3 * meth + 2] = np.clip(est + w, -1.0, 1.0)
    return rec


def benign(count, rho, seed=1):
    """Estimates in [-1, 1], CIs clipped to [-1, 1] (what the engine emits)."""
    return _put_specials(_benign_raw(count, seed), rho)


def cancelling(count, rho, seed=1):
    """est = +-2^27 + d, |d| < 2^-20, signs alternating (NI starts +, INT starts -), endpoints built
    the same way: the sums are tiny beside the sums of magnitudes."""
    g = np.random.default_rng([seed, 12])
    rec = np.empty((count, 6))
    big, small = 2.0 ** 27, 2.0 ** -20
    alt = np.where(np.arange(count) % 2 == 0, 1.0, -1.0)
    for meth, first in ((0, 1.0), (1, -1.0)):
        s = first * alt * big
        rec[:, 3 * meth] = s + g.uniform(-small, small, count)
        rec[:, 3 * meth + 1] = s - g.uniform(0.0, small, count)
        rec[:, 3 * meth + 2] = s + g.uniform(0.0, small, count)
    return _put_specials(rec, rho)


def giant_indices(count):
    """Where giant() puts +2^60 and -2^60: the last record of block 0 and the first of block 1 when
    there are several blocks; in one block lanes 0 of waves 0 and 1 (records 0 and 64); below 65
    records the first and the last; one record holds +2^60 alone."""
    if count > 2048:
        return acc_per(count) - 1, acc_per(count)
    if count > 64:
        return 0, 64
    return (0, count - 1) if count >= 2 else (0, None) if count == 1 else (None, None)


def giant(count, rho, seed=1):
    """Values of order 1 with one +2^60 and one -2^60 record (giant_indices)."""
    g = np.random.default_rng([seed, 13])
    rec = _benign_raw(count, seed + 100)
    rec[:, 0] = g.uniform(-2.0, 2.0, count)
    rec[:, 3] = g.normal(0.0, 1.0, count)
    _put_specials(rec, rho)
    big = 2.0 ** 60
    for i, s in zip(giant_indices(count), (1.0, -1.0)):
        if i is not None:
            rec[i, 0:3] = (s * big, s * big - 2.0 ** 10, s * big + 2.0 ** 10)
            rec[i, 3:6] = (-s * big, -s * big - 2.0 ** 12, -s * big + 2.0 ** 11)
    return rec


def tiny(count, rho, seed=1):
    """+-2^-1060, +-0.0, the least normal and subnormals: est * est underflows, the sums are exact
    multiples of 2^-1074.  Specials here are the NaN patterns only (a value of rho's size would
    hide the tiny terms under the bound)."""
    g = np.random.default_rng([seed, 14])
    pal = np.array([2.0 ** -1060, -(2.0 ** -1060), 0.0, -0.0, 5e-324, -5e-324, 2.0 ** -1022,
                    -(2.0 ** -1022), 2.0 ** -1030, -3 * 2.0 ** -1074])
    rec = np.empty((count, 6))
    for meth in (0, 1):
        v = pal[g.integers(0, pal.size, (count, 3))]
        sub = g.integers(1, 1 << 20, (count, 3)) * 5e-324 * np.where(g.integers(0, 2, (count, 3)) == 0, 1.0, -1.0)
        v = np.where(g.integers(0, 3 + meth, (count, 3)) == 0, sub, v)
        rec[:, 3 * meth] = v[:, 0]
        rec[:, 3 * meth + 1] = np.minimum(v[:, 1], v[:, 2])
        rec[:, 3 * meth + 2] = np.maximum(v[:, 1], v[:, 2])
    return _put_specials(rec, rho, with_rho=False)


BUILDERS = {"benign": benign, "cancelling": cancelling, "giant": giant, "tiny": tiny}

# rho against the finite endpoints: (lo - rho, hi - rho) in units of a width
POSITIONS = {"below_lo": (1.0, 2.0), "equal_lo": (0.0, 1.0), "inside": (-1.0, 1.0),
             "equal_hi": (-1.0, 0.0), "above_hi": (-2.0, -1.0)}
NAN_PATTERNS = [(e, l, h) for e in (False, True) for l in (False, True) for h in (False, True)]


def na_class_list():
    """The 40 classes: (est NaN, lo NaN, hi NaN, position name)."""
    return [(e, l, h, p) for (e, l, h) in NAN_PATTERNS for p in POSITIONS]


def na_class_runs(r):
    """Run length of each of the 40 classes in na_classes(rho, r): r - 2 .. r + 2, every offset eight
    times, so the total is 40 r and no two classes' counts are tied by construction."""
    assert r >= 3
    return [r + (7 * c) % 5 - 2 for c in range(40)]


def na_classes(rho, r, seed=1):
    """40 r records: every NaN pattern of (est, lo, hi) crossed with the five positions of rho
    against the finite endpoints, class c in a contiguous run of na_class_runs(r)[c] records; the
    INT columns walk the classes in another order ((11 c + 5) mod 40), so the two methods differ
    everywhere.  Widths and estimates are drawn, the endpoints that must equal rho equal it
    exactly."""
    g = np.random.default_rng([seed, 15])
    classes, runs = na_class_list(), na_class_runs(r)
    count = 40 * r
    rec = np.empty((count, 6))
    for meth in (0, 1):
        order = list(range(40)) if meth == 0 else [(11 * c + 5) % 40 for c in range(40)]
        row = 0
        for slot, c in enumerate(order):
            ne, nl, nh, pos = classes[c]
            a, b = POSITIONS[pos]
            for _ in range(runs[slot]):
                w = g.uniform(0.125, 0.375)
                est, lo, hi = rho + g.uniform(-0.25, 0.25), rho + a * w, rho + b * w
                if a == 0.0:
                    lo = rho
                if b == 0.0:
                    hi = rho
                rec[row, 3 * meth:3 * meth + 3] = (_NAN if ne else est, _NAN if nl else lo, _NAN if nh else hi)
                row += 1
        assert row == count
    return rec


def na_class_counts(rho, r, meth):
    """The counters of na_classes(rho, r) by class arithmetic alone (run lengths times the truth
    table of each class), for checking exact_counts and the kernels against a count that was not
    made by scanning records."""
    classes, runs = na_class_list(), na_class_runs(r)
    order = list(range(40)) if meth == 0 else [(11 * c + 5) % 40 for c in range(40)]
    out = dict.fromkeys(("n",) + COUNTERS, 0)
    for slot, c in enumerate(order):
        ne, nl, nh, pos = classes[c]
        a, b = POSITIONS[pos]
        ge = NA if nl else (TRUE if a <= 0.0 else FALSE)      # rho >= lo  <=>  lo - rho <= 0
        le = NA if nh else (TRUE if b >= 0.0 else FALSE)      # rho <= hi  <=>  hi - rho >= 0
        cv = AND3[(ge, le)]
        k = runs[slot]
        out["n"] += k
        out["n_cover"] += k * (cv == TRUE)
        out["n_cover_na"] += k * (cv == NA)
        out["n_na_est"] += k * ne
        out["n_na_ci"] += k * (nl or nh)
    return out


# ------------------------------------------------------------------- the checks
TWO100 = Fraction(1, 2 ** 100)


def stored(got, name):
    """The (hi, lo) words of sum `name` of a dcor_accum (ctypes) as floats."""
    w = getattr(got, name)
    return float(w[0]), float(w[1])


def assert_counts(got, want, what=""):
    g = {k: int(getattr(got, k)) for k in ("n",) + COUNTERS}
    w = {k: want[k] for k in ("n",) + COUNTERS}
    assert g == w, f"{what}: counters {g}, exact {w}"
    assert list(got.reserved) == [0, 0, 0], f"{what}: reserved {list(got.reserved)}"


def assert_normalised(got, what=""):
    for name in SUMS:
        hi, lo = stored(got, name)
        assert math.isfinite(hi) and math.isfinite(lo), f"{what}: {name} = ({hi!r}, {lo!r})"
        assert Fraction(abs(lo)) * 2 ** 53 <= Fraction(abs(hi)), f"{what}: {name} not normalised ({hi!r}, {lo!r})"


def assert_sums(got, exact, sabs, scale, what=""):
    """|hi + lo - exact| <= scale * 2^-100 * sum|term| for each sum; returns the largest
    error / bound seen (0 where the bound is 0 and met)."""
    worst = 0.0
    for name in SUMS:
        hi, lo = stored(got, name)
        err = abs(Fraction(hi) + Fraction(lo) - exact[name])
        bound = scale * TWO100 * sabs[name]
        assert err <= bound, (f"{what}: {name} = {hi!r} + {lo!r}, exact {float(exact[name])!r}, error "
                              f"{float(err):.3e} > bound {float(bound):.3e}")
        if bound:
            worst = max(worst, float(err / bound))
    return worst


def assert_accum(got, records, rho, meth, what=""):
    """A dcor_accum against the exact reference of its records: n and the four counters exact,
    reserved zero, every (hi, lo) pair normalised (|lo| <= 2^-53 |hi|) and every sum within
    max(count, 1024) * 2^-100 * sum|term| -- the engine's own error model (the compensated
    per-thread sums: count * 2^-106; the wave and workgroup folds: order 2^-100 of the sum's
    magnitude) with a 64x margin; a sum whose low word was lost misses it by more than 2^40.
    Returns the largest error / bound."""
    count = np.asarray(records).reshape(-1, 6).shape[0]
    ex, sabs = exact_accum_abs(records, rho, meth)
    assert_counts(got, ex, what)
    assert_normalised(got, what)
    return assert_sums(got, ex, sabs, max(count, 1024), what)


def summary_bounds(records, rho, meth):
    """(exact summary, bound per column) for dcor_accum_finalize's x86-64 long-double arithmetic
    (64-bit significands, one rounding to double at the end):
      mse, ci_length: 2^-52 |exact| + 2^-62 sum|term| / n
      bias:           2^-52 (|mean| + |bias|)
      var:            2^-52 |var| + 2^-60 sum est^2 / (n - 1)
      coverage:       the correctly rounded quotient of the two integers, exactly (bound 0 on the
                      distance from float(n_cover / n))."""
    ex, sabs = exact_accum_abs(records, rho, meth)
    s = exact_summary(ex, rho)
    n = ex["n"]
    u52, u60, u62 = Fraction(1, 2 ** 52), Fraction(1, 2 ** 60), Fraction(1, 2 ** 62)
    b = dict.fromkeys(SUMMARY)
    if s["mse"] is not None:
        b["mse"] = u52 * abs(s["mse"]) + u62 * sabs["se2"] / n
        b["bias"] = u52 * (abs(ex["est"] / n) + abs(s["bias"]))
    if s["var"] is not None:
        b["var"] = u52 * abs(s["var"]) + u60 * ex["est2"] / (n - 1)
    if s["coverage"] is not None:
        b["coverage"] = Fraction(0)
    if s["ci_length"] is not None:
        b["ci_length"] = u52 * abs(s["ci_length"]) + u62 * sabs["len"] / n
    return s, b


def assert_summary(got, records, rho, meth, what="", floor=Fraction(0)):
    """A finalised summary (dict of floats, NaN for NA) against exact_summary within
    summary_bounds; NA exactly where R has NA.  `floor` is added to every bound: 0 except for
    results in double's subnormal range, whose own rounding is half of 2^-1074."""
    s, b = summary_bounds(records, rho, meth)
    for k in SUMMARY:
        g = float(got[k])
        if s[k] is None:
            assert g != g, f"{what}: {k} = {g!r}, R gives NA"
            continue
        assert math.isfinite(g), f"{what}: {k} = {g!r}, exact {float(s[k])!r}"
        if k == "coverage":
            assert g == float(s[k]), f"{what}: coverage = {g!r}, exact {float(s[k])!r}"
            continue
        err = abs(Fraction(g) - s[k])
        assert err <= b[k] + floor, (f"{what}: {k} = {g!r}, exact {float(s[k])!r}, error {float(err):.3e} > "
                                     f"bound {float(b[k] + floor):.3e}")
