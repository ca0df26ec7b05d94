"""Reference and adversarial key families for the engine's order-statistic selectors
(value_select, reg_select, wave_select, wave_select_lds in csrc/dcor_device.h), which the test
entry dcor_diag_select runs on caller keys.

The reference is sort(keys without NaN)[pos], NaN when pos is outside [0, valid).  A selector returns
one of its inputs, so the comparison is exact: equal as values (-0.0 == +0.0), NaN matches NaN, no
tolerance.

A family builder takes the set size n and returns Case(name, keys, pos): one key set and the
positions asked of it.  placed() adds the arrangements (ascending, descending, a fixed permutation;
for the crowded families also the crowd packed into few lanes / few slots of the wave layout, where
key i sits at lane i % 64, slot i // 64).

emulate_wave_select restates the round loop of the two wave selectors in numpy (same IEEE
operations, same bins), so the round cap's history stays checkable without a GPU."""
import math
from collections import namedtuple

import numpy as np

Case = namedtuple("Case", "name keys pos")

WHICH = {0: "value_select", 1: "reg_select", 2: "wave_select<16>", 3: "wave_select<32>",
         4: "wave_select_lds<16>", 5: "wave_select_lds<32>"}
SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 1000, 1023, 1024, 1025, 2000, 2047, 2048)
TINY = 2.0 ** -1074
HUGE = 1.7e308


def max_keys(which):
    return 1024 if which in (2, 4) else 2048


def reference(keys, pos):
    k = np.asarray(keys, dtype=np.float64)
    s = np.sort(k[~np.isnan(k)])
    return float(s[pos]) if 0 <= pos < len(s) else math.nan


def same(got, ref):
    """Exact: equal as values, or both NaN."""
    return bool(got == ref) or (math.isnan(got) and math.isnan(ref))


def valid_count(keys):
    return int(np.count_nonzero(~np.isnan(keys)))


def positions(valid):
    """-1, 0, 1, the middle, mixquant's 97.5% element, the last, one past the last."""
    return sorted({-1, 0, 1, valid // 2, math.ceil(0.975 * valid) - 1, valid - 1, valid})


def _bits(a):
    return np.asarray(a, dtype=np.int64).view(np.float64)


def _draws(seed, n, c=0.0):
    g = np.random.default_rng(seed)
    u = g.uniform(-0.5, 0.5, n)
    return g.standard_normal(n) + c * (-np.sign(u) * np.log1p(-2.0 * np.abs(u)))


# ------------------------------------------------------------------ families
def fam_sizes(n=None):
    """Every set size where a layout changes: part-filled slots, one key, the 16 / 32 keys-per-lane
    limits.  n is ignored (the sizes are the point)."""
    return [Case(f"size{nk}", _draws(100 + nk, nk), positions(nk)) for nk in SIZES]


def _crowded_bin(n, x, tied):
    """x keys inside one bin of a wider range: keys 0 and 256 pin the range, so value_select's bin
    100 is [100, 101) and the wave selectors' bin 50 is [100, 102); the rest stay outside [99, 103]."""
    g = np.random.default_rng(1000 + x)
    below = (n - x - 2) // 3
    above = n - x - 2 - below
    crowd = np.full(x, 100.5) if tied else 100.0 + 0.9 * np.arange(x) / x
    keys = np.concatenate([[0.0], g.uniform(0.5, 98.0, below), crowd, g.uniform(104.0, 255.5, above), [256.0]])
    first = 1 + below
    return Case(f"bin{x}{'tied' if tied else ''}", keys, [first - 1, first, first + x // 2, first + x - 1, first + x, n])


def fam_ties(n):
    g = np.random.default_rng(11)
    out = [Case("all-equal", np.full(n, 2.5), positions(n))]
    for pos in (n // 2, math.ceil(0.975 * n) - 1):
        for a in (pos - 1, pos, pos + 1):   # a copies of 1.0, then 2.0: the split around pos
            out.append(Case(f"two-split{a}", np.r_[np.full(a, 1.0), np.full(n - a, 2.0)], [-1, pos - 1, pos, pos + 1, n]))
    for d in (3, 7):
        out.append(Case(f"{d}-distinct", g.choice(g.standard_normal(d), n), positions(n)))
    for x in (64, 65, 256, 257):
        out.append(_crowded_bin(n, x, False))
        out.append(_crowded_bin(n, x, True))
    return out


def fam_nan(n):
    base = _draws(21, n)
    out = [Case("nan-none", base.copy(), positions(n))]

    def add(name, idx):
        k = base.copy()
        k[idx] = np.nan
        out.append(Case(name, k, positions(valid_count(k))))

    add("nan-first", [0])
    add("nan-middle", [n // 2])
    add("nan-last", [n - 1])
    add("nan-all-but-one", np.arange(n) != n // 3)
    add("nan-all", np.arange(n))
    add("nan-slot0", np.arange(min(64, n)))              # the whole first slot of the wave layout
    add("nan-slot0-part", np.arange(0, min(64, n), 3))
    add("nan-tail-slot", np.arange(64 * ((n - 1) // 64), n))   # the last, part-filled slot
    add("nan-interleaved", np.arange(0, n, 2))
    return out


def fam_inf(n):
    out = []

    def add(name, a, b, mid, nnan=0):
        k = np.r_[np.full(a, -np.inf), mid, np.full(b, np.inf), np.full(nnan, np.nan)]
        v = len(k) - nnan
        out.append(Case(name, k, sorted({-1, 0, a - 1, a, v - b - 1, v - b, v - 1, v})))

    for a, b in ((1, 1), (3, 70), (70, 3), (100, 100), (0, 5), (5, 0)):
        add(f"inf-{a}-{b}", a, b, _draws(31 + a, n - a - b))
    add("inf-only", n // 2, n - n // 2, [])
    add("inf-only-plus", 0, n, [])
    add("inf-only-minus", n, 0, [])
    add("inf-nan", 40, 90, _draws(32, n - 140), nnan=10)
    add("inf-one-finite", n // 3, n - 1 - n // 3, [-2.75])
    return out


def fam_range(n):
    g = np.random.default_rng(41)
    h = n // 2
    out = [
        Case("zeros-mixed", np.where(g.integers(0, 2, n) == 1, 0.0, -0.0), positions(n)),
        Case("consecutive-from-1", _bits(np.float64(1.0).view(np.int64) + np.arange(n)), positions(n)),
        Case("consecutive-from-tiny", _bits(1 + np.arange(n)), positions(n)),
        # ..., -2 TINY, -TINY, +0.0, TINY, ...: consecutive doubles through zero
        Case("consecutive-straddle", np.r_[-_bits(np.arange(h, 0, -1)), _bits(np.arange(n - h))], positions(n)),
        # the same with both zeros present (equal values, two integer keys)
        Case("consecutive-straddle-2zeros", np.r_[-_bits(np.arange(h, -1, -1)), _bits(np.arange(n - h - 1))],
             sorted(set(positions(n)) | {h - 1, h, h + 1, h + 2})),
        Case("subnormal-range", _bits(g.integers(1, 1 << 52, n)), positions(n)),
        Case("subnormal-narrow", _bits((1 << 40) + g.integers(0, 300, n)), positions(n)),
        Case("tiny-over-zero", np.where(np.arange(n) < h, 0.0, TINY), [-1, 0, h - 1, h, n - 1, n]),
        Case("tiny-over-zeros-mixed", np.r_[np.where(g.integers(0, 2, h) == 1, 0.0, -0.0), np.full(n - h, TINY)],
             [-1, 0, h - 1, h, n - 1, n]),
        Case("minus-tiny-under-zeros-mixed", np.r_[np.full(h, -TINY), np.where(g.integers(0, 2, n - h) == 1, 0.0, -0.0)],
             [-1, 0, h - 1, h, n - 1, n]),
        Case("huge-range", np.r_[-HUGE, g.uniform(-1.0, 1.0, n - 2) * HUGE, HUGE], positions(n)),
        Case("huge-ends-crowded", np.r_[np.full(h, -HUGE), np.full(n - h, HUGE)], [-1, 0, h - 1, h, n - 1, n]),
        Case("cluster-1e300", _bits(np.float64(1e300).view(np.int64) + g.integers(0, 50, n)), positions(n)),
        Case("cluster-1e300-distinct", _bits(np.float64(1e300).view(np.int64) + np.arange(n)), positions(n)),
    ]
    return out


LADDER_J = (79, 80, 81, 200)


def ladder_keys(n, j, cluster=0.0, sign=1.0):
    """n - j copies of `cluster` and the rungs sign * 2^(-1000 + 8 i), i < j: each rung is 2^8 times
    the one before, more than a by-value round's bin ratio of 2^7."""
    return np.r_[np.full(n - j, cluster), sign * 2.0 ** (-1000.0 + 8.0 * np.arange(j))]


def key_ladder_keys(n, step):
    """The by-key rounds' worst case.  Five value rungs 4 * 2^(8 i) keep the four by-value rounds busy
    (one rung each) and leave 4.0 on top, 2^62 integer keys above the crowd at 2^-1022.  Below it sit
    keys at crowd + 2^(63 - step j) - 1: with step = 8 the chosen bin [0, 2^sh) keeps the next of them
    each round, so d loses exactly 8 bits a round and the select returns in the last round the cap
    allows; step = 7 is the same for a map that would keep only 7 bits a round."""
    k0 = int(np.float64(2.0 ** -1022).view(np.int64))
    spread = [k0 + (1 << (63 - step * j)) - 1 for j in range(1, 64 // step + 1) if 63 - step * j > 0]
    top = 4.0 * 2.0 ** (8.0 * np.arange(5))
    return np.r_[np.full(n - len(spread) - 5, 2.0 ** -1022), _bits(sorted(spread)), top]


def fam_ladder(n):
    """The round-cap family.  A by-value round over [0, top rung] puts every other key in bin 0, so it
    peels one rung a round; the rank sits in the crowd of more than 64 equal keys."""
    out = []
    for j in LADDER_J:
        c = n - j
        pos = [-1, 0, c // 2, c - 1, c, c + j // 2, n - 1, n]   # crowd: first, middle, last copy; rungs: first, middle, last
        up = ladder_keys(n, j)
        out.append(Case(f"ladder{j}", up, pos))
        # mirror image: the crowd (-0.0) on top of a ladder of negative rungs
        out.append(Case(f"ladder{j}-mirror", -up, sorted({-1, n} | {n - 1 - p for p in pos if 0 <= p < n})))
        # a crowd at -3.5 inside a ladder of negative rungs (those beyond -3.5 sort below the crowd)
        neg = ladder_keys(n, j, cluster=-3.5, sign=-1.0)
        nb = int(np.count_nonzero(neg < -3.5))
        posn = sorted({-1, 0, nb - 1, nb, nb + c // 2, nb + c - 1, nb + c, n - 1, n})
        out.append(Case(f"ladder{j}-neg", neg, posn))
        out.append(Case(f"ladder{j}-neg-mirror", -neg, sorted({-1, n} | {n - 1 - p for p in posn if 0 <= p < n})))
    for step in (8, 7):
        k = key_ladder_keys(n, step)
        c = int(np.count_nonzero(k == 2.0 ** -1022))
        out.append(Case(f"ladder-bykey{step}", k, [-1, 0, c // 2, c - 1, c, n - 6, n - 1, n]))
    return out


def fam_radix(n):
    g = np.random.default_rng(61)
    one = int(np.float64(1.0).view(np.int64))
    low = one + (np.arange(n) % 256)                      # differ in the lowest byte only: eight passes
    uniq = one + np.r_[np.arange(n - 1) % 255, 255]       # the top value once: cnt == 1 at the last digit
    sign = np.where(g.integers(0, 2, n) == 1, 1.0, -1.0)
    pats = g.integers(0, 1 << 64, n, dtype=np.uint64, endpoint=False)
    pats[:: 97] = np.uint64(0x7FF8000000000000)           # quiet NaN
    pats[1:: 89] = np.uint64(0xFFF0000000000001)          # a negative signalling NaN pattern
    pats[2:: 83] = np.uint64(0x7FF0000000000000)          # +inf
    pats[3:: 79] = np.uint64(0xFFF0000000000000)          # -inf
    rnd = pats.view(np.float64)
    return [
        Case("low-byte", _bits(low), positions(n)),
        Case("low-byte-unique-top", _bits(uniq), sorted(set(positions(n)) | {n - 2})),
        Case("sign-bit", sign * _bits(low), positions(n)),
        Case("sign-bit-wide", sign * 2.0 ** g.integers(-1000, 1000, n).astype(np.float64), positions(n)),
        Case("random-patterns", rnd, positions(valid_count(rnd))),
    ]


def fam_baseline(n):
    """What the suite fed the selectors before: standard_normal + c * laplace."""
    return [Case(f"normal+{c}lap-seed{s}", _draws(70 + s, n, c), positions(n))
            for c in (0.0, 0.01, 1.0, 100.0) for s in (1, 2, 3)]


FAMILIES = {"sizes": fam_sizes, "ties": fam_ties, "nan": fam_nan, "inf": fam_inf, "range": fam_range,
            "ladder": fam_ladder, "radix": fam_radix, "baseline": fam_baseline}
CROWDED = ("ladder7", "ladder8", "ladder2", "bin65")   # cases that also get the lane- and slot-packed arrangements


# ---------------------------------------------------------------- placement
def _crowd_first(keys):
    """The crowd first -- the copies of the most frequent value, or the keys of _crowded_bin's bin
    [100, 101) when no value repeats -- and the rest in their order."""
    k = np.asarray(keys)
    vals, cnt = np.unique(k[~np.isnan(k)], return_counts=True)
    crowd = (k == vals[np.argmax(cnt)]) if cnt.max() > 1 else ((k >= 100.0) & (k < 101.0))
    return np.r_[k[crowd], k[~crowd]]


def placed(case):
    """The arrangements of one case: as built, ascending (NaN last), descending (NaN first), a fixed
    permutation; crowded cases also with the crowd packed into the fewest lanes (indices ordered by
    lane, then slot) and into the fewest slots (the lowest indices)."""
    k = np.asarray(case.keys, dtype=np.float64)
    n = len(k)
    asc = np.sort(k)
    perm = np.random.default_rng(5).permutation(n)
    out = [case, Case(case.name + "/asc", asc, case.pos), Case(case.name + "/desc", asc[::-1].copy(), case.pos),
           Case(case.name + "/perm", k[perm], case.pos)]
    if any(case.name.startswith(c) for c in CROWDED):
        cf = _crowd_first(k)
        by_lane = np.lexsort((np.arange(n) // 64, np.arange(n) % 64))   # index order: lane 0's slots, lane 1's, ...
        lanes = np.empty(n)
        lanes[by_lane] = cf
        out += [Case(case.name + "/lanes", lanes, case.pos), Case(case.name + "/slots", cf, case.pos)]
    return out


def family_cases(family, n):
    """Every arrangement of every case of a family at set size n."""
    return [p for c in FAMILIES[family](n) for p in placed(c)]


# ---------------------------------------------------- the wave selectors' round loop
def _sel_key(v):
    u = np.asarray(v, dtype=np.float64).view(np.uint64)
    neg = (u >> np.uint64(63)) == 1
    return np.where(neg, ~u, u | np.uint64(1 << 63))


def emulate_wave_select(keys, pos, value_rounds=None, cap=80, key_bits=8):
    """wave_select / wave_select_lds in numpy: (result, rounds run).  value_rounds = None and cap = 80
    is the loop before the round-cap fix (by-key binning only when 128 / h overflows); value_rounds = 4,
    cap = 13 is the loop now (by-key binning from round 4 on).  key_bits: the bits of d a by-key round
    keeps (8 in the engine)."""
    v = np.asarray(keys, dtype=np.float64)
    act = ~np.isnan(v)
    k = pos
    if k < 0 or k >= act.sum():
        return math.nan, 0
    nlo, nhi = int((v == -np.inf).sum()), int((v == np.inf).sum())
    if k < nlo:
        return -math.inf, 0
    if k >= act.sum() - nhi:
        return math.inf, 0
    act &= np.isfinite(v)
    k -= nlo
    with np.errstate(over="ignore", divide="ignore", invalid="ignore"):
        for it in range(cap):
            a = v[act]
            ka = _sel_key(a)
            lo, hi = a[np.argmin(ka)], a[np.argmax(ka)]   # -0.0 below +0.0, as v_min_f64 / v_max_f64 order them
            if not hi > lo:
                return float(lo), it
            h = 0.5 * hi - 0.5 * lo
            scale = np.float64(128.0) / h
            by_value = h > 0.0 and scale < np.inf and (value_rounds is None or it < value_rounds)
            if by_value:
                t = (0.5 * a - 0.5 * lo) * scale
                b = np.where(t < 255.0, t, 255.0).astype(np.int64)
            else:
                klo = ka.min()
                d = int(ka.max() - klo)
                sh = max(d.bit_length() - key_bits, 0)
                b = ((ka - klo) >> np.uint64(sh)).astype(np.int64) & 255
            hist = np.bincount(b, minlength=256)
            cum = np.cumsum(hist)
            B = int(np.searchsorted(cum, k, side="right"))
            kk = k - (int(cum[B - 1]) if B > 0 else 0)
            if hist[B] <= 64:
                return float(np.sort(a[b == B])[kk]), it + 1
            idx = np.flatnonzero(act)
            act[idx[b != B]] = False
            k = kk
    return math.nan, cap
