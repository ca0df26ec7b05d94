"""GPU tests of the private pairwise HRS table path (dcor_hrs_private_pairwise_launch,
dcor.hrs.private_pairwise_segments / corr_matrix_private_pairwise / corr_matrix_sweep_private_pairwise,
dcor.dist.hrs_private_pairwise_distributed) on tests/test_gpu_hrs_private.py's table with gaps.

The yardstick is the composition of the entries that existed before it, one replicate number r at a
time -- what a user had to loop over on the host: dcor_draws_launch(0, seed_std, 17, r, 1, 2 p) ->
per column api.dp_sd on the NaN-holding column (which drops the column's own gaps), api.standardize_dp
and api.lambda_from_priv -> one hrs.pairwise_segments call holding every segment at rep_begin = r,
reps = 1 with the same masks.  Full masks are compared with hrs.private_segments.  Records are compared
as uint64; the new path is never its own reference.  One anchor does not go through the shared
reduction code at all: a released mean against exact rational arithmetic.

Every column of every pair of the main table has more present rows than the pair (asserted), so a
release scaled by n_ab instead of the column's own count cannot pass."""
import ctypes as C
import os
import socket
from fractions import Fraction

import numpy as np
import pytest

from test_gpu_hrs_private import BOUNDS, P, PAIRS, REP_BEGIN, REPS, SEED_STD, SENTINEL
from test_gpu_hrs_private import _bits, _draws, _named, _raw, _segments

pytestmark = pytest.mark.gpu


def _present(n, seed=91):
    """bool [P, n]: every column drops 10-30 % of its rows independently (12, 28, 18 and 22 %)."""
    g = np.random.default_rng(seed + n)
    return np.stack([g.random(n) >= q for q in (0.12, 0.28, 0.18, 0.22)])


def _pack(V, junk=True):
    """bool [p, n] -> uint64 [p, nw]; junk: the last word's bits at i >= n set (they are ignored)."""
    p, n = V.shape
    bits = np.zeros((p, 64 * ((n + 63) // 64)), dtype=np.uint8)
    bits[:, :n] = V
    if junk:
        bits[:, n:] = 1
    return np.packbits(bits, axis=1, bitorder="little").view("<u8").astype(np.uint64).reshape(p, -1)


def _launch(raw, bounds, V, segs, rows, ld=None, seed_std=SEED_STD, eps_mean=0.1, eps_m2=0.1, delta=float("nan"),
            fill=np.nan, want_priv=True, junk=True, expect=0):
    """dcor_hrs_private_pairwise_launch on the (n, p) array raw laid out with `ld` elements between
    columns, the rows V leaves out overwritten with `fill`; the record and d_priv buffers start out as
    SENTINEL.  -> (records, priv)."""
    import torch
    from dcor import _lib
    n, p = raw.shape
    ld = n if ld is None else ld
    host = np.full((p, ld), -123.0)   # the gap between columns is never read
    host[:, :n] = np.where(V, raw.T, fill)
    Dd = torch.as_tensor(host.reshape(-1), device="cuda")
    out = torch.full((max(rows, 1), 6), SENTINEL, dtype=torch.float64, device="cuda")
    priv = torch.full((max(rows, 1), 6), SENTINEL, dtype=torch.float64, device="cuda")
    lo = np.array([b[0] for b in bounds], dtype=np.float64)
    hi = np.array([b[1] for b in bounds], dtype=np.float64)
    valid = _pack(V, junk)
    D = C.POINTER(C.c_double)
    desc = _lib.HrsPrivateNaDesc(n=n, p=p, ld=ld, D=Dd.data_ptr(), lo=lo.ctypes.data_as(D), hi=hi.ctypes.data_as(D),
                                 valid=valid.ctypes.data_as(C.POINTER(C.c_uint64)), eps_mean=eps_mean, eps_m2=eps_m2,
                                 seed_std=seed_std, alpha=0.05, delta=delta, nsim=2000)
    arr = (_lib.HrsPairSegment * max(len(segs), 1))(*[
        _lib.HrsPairSegment(eps=e, seed_ni=sn, seed_int=si, rep_begin=rb, reps=c, out_row=row, col_x=a, col_y=b)
        for a, b, e, sn, si, rb, c, row in segs])
    st = _lib.lib.dcor_hrs_private_pairwise_launch(
        C.byref(desc), arr, len(segs), C.c_void_p(out.data_ptr()),
        C.c_void_p(priv.data_ptr()) if want_priv else None,
        C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert st == expect, _lib.last_error()
    return out.cpu().numpy(), priv.cpu().numpy()


def _yardstick(raw, bounds, V, segs, rows, seed_std=SEED_STD, eps_mean=0.1, eps_m2=0.1):
    """Records and d_priv rows of `segs` from the existing entries, the host loop over replicate
    numbers: per distinct r one draws launch, per column the helpers' trio on the NaN-holding column,
    and one pairwise_segments call of single-replicate segments under the same masks (delta = NaN:
    1 / n_ab)."""
    from dcor import api, hrs
    n, p = raw.shape
    holes = np.where(V.T, raw, np.nan)
    valid = _pack(V)
    want = np.full((rows, 6), np.nan)
    wpriv = np.full((rows, 6), np.nan)
    reps = sorted({rb + j for *_, rb, c, _row in segs for j in range(c)})
    for r in reps:
        lap = _draws(seed_std, r, p)
        cols, prow = [], []
        for c, (lo, hi) in enumerate(bounds):
            col = np.ascontiguousarray(holes[:, c])
            pv = api.dp_sd(col, lo, hi, eps_mean, eps_m2, lap=lap[2 * c:2 * c + 2])
            cols.append(api.standardize_dp(col, pv, lo, hi))
            prow.append((pv["mean"], pv["sd"], api.lambda_from_priv(lo, hi, pv)))
        prow = np.array(prow)
        Z, lam = np.asfortranarray(np.stack(cols, axis=1)), prow[:, 2].copy()
        one, where = [], []
        for a, b, e, sn, si, rb, c, row in segs:
            if rb <= r < rb + c:
                one.append((a, b, e, sn, si, r, 1))
                where.append((row + (r - rb), a, b))
        if not one:
            continue
        got = hrs.pairwise_segments(Z, lam, one, valid=valid)
        for rec, (row, a, b) in zip(got, where):
            want[row] = rec
            wpriv[row] = np.concatenate([prow[a], prow[b]])
    return want, wpriv, len(reps)


_CACHE = {}


def _main_case(n):
    """The main segment list in one call (columns at 8-B offsets: ld = n + 3) and its yardstick,
    computed once per n and left unchanged."""
    if n not in _CACHE:
        raw, V, segs = _raw(n), _present(n), _segments()
        rows = (REPS + 1) * len(segs)
        got, priv = _launch(raw, BOUNDS, V, segs, rows, ld=n + 3)
        want, wpriv, nrep = _yardstick(raw, BOUNDS, V, segs, rows)
        for a in (got, priv, want, wpriv):
            a.setflags(write=False)
        _CACHE[n] = (got, priv, want, wpriv, nrep)
    return _CACHE[n]


def _counts_differ(V, pairs):
    """Every column of every pair of different columns has more present rows than the pair."""
    for a, b in pairs:
        nab = int((V[a] & V[b]).sum())
        assert nab >= 2
        if a != b:
            assert V[a].sum() > nab and V[b].sum() > nab, (a, b)


# ---------------------------------------------------------------- 1. the yardstick, byte for byte
@pytest.mark.parametrize("n", [1000, 1001])
def test_records_and_releases_equal_the_host_loop_bitwise(n):
    V, segs = _present(n), _segments()
    for c in range(P):
        assert 0.10 <= 1.0 - V[c].mean() <= 0.30, c
    _counts_differ(V, PAIRS + [(1, 2)])
    assert {s[5] for s in segs} == set(REP_BEGIN) and 2**32 - 4 in REP_BEGIN
    got, priv, want, wpriv, nrep = _main_case(n)
    assert nrep == 9
    named = _named(segs, len(got))
    assert named.sum() == REPS * len(segs)
    assert np.isfinite(want[named]).all() and np.isfinite(wpriv[named]).all()
    assert np.array_equal(_bits(got[named]), _bits(want[named]))
    assert np.array_equal(_bits(priv[named]), _bits(wpriv[named]))
    # shuffled out_row blocks: the row after each block survives in both buffers
    assert np.all(got[~named] == SENTINEL) and np.all(priv[~named] == SENTINEL)
    s = segs[5]
    assert not np.array_equal(got[s[7]], got[s[7] + 1])     # the replicate's release matters


def test_other_budgets_against_the_host_loop():
    n = 1001
    raw, V = _raw(n), _present(n)
    segs = [(0, 1, 1.0, 2**33 + 5, 2**34 + 6, 7, 2, 0), (3, 2, 2.0, 2**33 + 8, 2**34 + 9, 7, 2, 3)]
    kw = dict(seed_std=2**40 + 3, eps_mean=0.3, eps_m2=0.7)
    got, priv = _launch(raw, BOUNDS, V, segs, 6, **kw)
    want, wpriv, _ = _yardstick(raw, BOUNDS, V, segs, 6, **kw)
    named = _named(segs, 6)
    assert np.isfinite(want[named]).all()
    assert np.array_equal(_bits(got[named]), _bits(want[named]))
    assert np.array_equal(_bits(priv[named]), _bits(wpriv[named]))
    assert np.all(got[~named] == SENTINEL) and np.all(priv[~named] == SENTINEL)


# ---------------------------------------------------------------- 2. full masks: the private entry
@pytest.mark.parametrize("n", [1000, 1001])
def test_full_masks_equal_the_private_entry_bitwise(n):
    from dcor import hrs
    raw = _raw(n)
    segs = _segments()[:8]
    rows = (REPS + 1) * 16
    got, priv = _launch(raw, BOUNDS, np.ones((P, n), dtype=bool), segs, rows, ld=n + 3, delta=1.0 / n)
    res, pv = hrs.private_segments(raw, BOUNDS, [s[:7] for s in segs], seed_std=SEED_STD, return_priv=True)
    for j, s in enumerate(segs):
        assert np.array_equal(_bits(got[s[7]:s[7] + REPS]), _bits(res[REPS * j:REPS * (j + 1)])), s
        assert np.array_equal(_bits(priv[s[7]:s[7] + REPS]), _bits(pv[REPS * j:REPS * (j + 1)])), s
    assert np.isfinite(res).all()


# ---------------------------------------------------------------- 3. absent rows are never read
def test_value_at_an_absent_row_reaches_no_result():
    n = 1001
    raw, V = _raw(n), _present(n)
    segs = _segments()[:8]
    rows = (REPS + 1) * 16
    base = _launch(raw, BOUNDS, V, segs, rows, fill=np.nan)
    got = _main_case(n)
    named = _named(segs, rows)
    assert np.array_equal(_bits(base[0][named]), _bits(got[0][named]))      # ld = n against ld = n + 3 too
    for fill in (1e300, -1e300, 50.0):
        other = _launch(raw, BOUNDS, V, segs, rows, fill=fill)
        assert np.array_equal(_bits(other[0]), _bits(base[0])), fill
        assert np.array_equal(_bits(other[1]), _bits(base[1])), fill
    # and the masks' bits at i >= n are ignored
    other = _launch(raw, BOUNDS, V, segs, rows, junk=False)
    assert np.array_equal(_bits(other[0]), _bits(base[0])) and np.array_equal(_bits(other[1]), _bits(base[1]))


# ---------------------------------------------------------------- 4. a column has one release
def test_column_release_ignores_the_partner_and_its_mask():
    n, r = 1001, 1001
    raw, V = _raw(n), _present(n)
    pairs = [(0, 1), (1, 0), (1, 2), (1, 1)]
    segs = [(a, b, 1.0, 70 + j, 80 + j, r, 2, 2 * j) for j, (a, b) in enumerate(pairs)]
    got, priv = _launch(raw, BOUNDS, V, segs, 8)
    triple = lambda pv, j, side, k: pv[2 * j + k, 3 * side:3 * side + 3].tobytes()
    for k in range(2):
        ones = {triple(priv, 0, 1, k), triple(priv, 1, 0, k), triple(priv, 2, 0, k), triple(priv, 3, 0, k),
                triple(priv, 3, 1, k)}
        assert len(ones) == 1, k
    assert triple(priv, 0, 1, 0) != triple(priv, 0, 1, 1)                   # it differs between replicates
    V2 = V.copy()
    V2[2, ::2] &= np.random.default_rng(5).random(len(V2[2, ::2])) >= 0.5    # only column 2's mask changes
    assert V2[2].sum() < V[2].sum() and np.array_equal(V2[[0, 1, 3]], V[[0, 1, 3]])
    got2, priv2 = _launch(raw, BOUNDS, V2, segs, 8)
    for j in (0, 1, 3):                                                      # pairs without column 2: unchanged
        assert np.array_equal(_bits(got2[2 * j:2 * j + 2]), _bits(got[2 * j:2 * j + 2]))
        assert np.array_equal(_bits(priv2[2 * j:2 * j + 2]), _bits(priv[2 * j:2 * j + 2]))
    assert np.array_equal(_bits(priv2[4:6, :3]), _bits(priv[4:6, :3]))       # column 1's release in (1, 2)
    assert not np.array_equal(_bits(priv2[4:6, 3:]), _bits(priv[4:6, 3:]))   # column 2's moved
    assert not np.array_equal(_bits(got2[4:6]), _bits(got[4:6]))


# ---------------------------------------------------------------- 5. NaN at a present row
def test_nan_at_a_present_row_reaches_only_the_pairs_that_name_its_column():
    n = 1001
    raw, V = _raw(n).copy(order="F"), _present(n)
    segs = [(a, b, 1.0, 50 + j, 60 + j, 3, 2, 2 * j) for j, (a, b) in enumerate(PAIRS + [(3, 3), (0, 2), (3, 1)])]
    clean, cpriv = _launch(raw, BOUNDS, V, segs, 2 * len(segs))
    i = int(np.flatnonzero(V[3] & ~V[1])[0])          # present in column 3, absent in column 1
    raw[i, 3] = np.nan
    got, priv = _launch(raw, BOUNDS, V, segs, 2 * len(segs))
    assert np.isfinite(clean).all() and np.isfinite(cpriv).all()
    for a, b, *_, row in segs:
        rows = slice(row, row + 2)
        if 3 in (a, b):                               # (3, 1) too: the row is not in its pair, but in its column
            assert np.isnan(got[rows]).all(), (a, b)
            for side, col in ((slice(0, 3), a), (slice(3, 6), b)):
                if col == 3:
                    assert np.isnan(priv[rows, side]).all()
                else:
                    assert np.array_equal(_bits(priv[rows, side]), _bits(cpriv[rows, side]))
        else:
            assert np.array_equal(_bits(got[rows]), _bits(clean[rows])), (a, b)
            assert np.array_equal(_bits(priv[rows]), _bits(cpriv[rows])), (a, b)


# ---------------------------------------------------------------- 6. compaction edges
def _edge_table(n):
    """Six columns at n rows.  0: full.  1: about 80 % at random.  2: rows {0, n - 1} only.  3: row 0 and
    the last row of a mask word (row 63, or the last row below it).  4: row 0 only.  5: row n - 1 only.
    A pair of a one-row column and the full one has n_ab = 1, which the entry's own check refuses (2 <=
    n_ab), so columns 4 and 5 go through the column preparation unnamed and the refusal is asserted;
    the named edge columns keep two rows, at the same edges."""
    g = np.random.default_rng(600 + n)
    raw = np.asfortranarray(np.stack([np.round(67.5 + 11.25 * g.standard_normal(n)) for _ in range(6)], axis=1))
    V = np.zeros((6, n), dtype=bool)
    V[0] = True
    V[1] = g.random(n) >= 0.2
    V[2, [0, n - 1]] = True
    V[3, [0, min(63, n - 2)]] = True
    V[4, 0] = True
    V[5, n - 1] = True
    return raw, V, [(45.0, 90.0)] * 6


@pytest.mark.parametrize("n", [63, 64, 65, 129])
def test_compaction_edges_equal_the_host_loop_bitwise(n):
    from dcor import _lib
    raw, V, bounds = _edge_table(n)
    pairs = [(0, 1), (1, 0), (2, 0), (0, 3), (3, 3), (1, 1), (2, 1)]
    segs = [(a, b, (1.0, 2.0)[j % 2], 300 + j, 400 + j, 11, 2, 3 * j) for j, (a, b) in enumerate(pairs)]
    rows = 3 * len(segs)
    got, priv = _launch(raw, bounds, V, segs, rows, ld=n + 1)
    want, wpriv, _ = _yardstick(raw, bounds, V, segs, rows)
    named = _named(segs, rows)
    assert np.array_equal(_bits(got[named]), _bits(want[named]))
    assert np.array_equal(_bits(priv[named]), _bits(wpriv[named]))
    assert np.isfinite(wpriv[named]).all() and np.isfinite(want[:2]).all()
    assert np.all(got[~named] == SENTINEL)
    for col in (4, 5):
        bad, bpriv = _launch(raw, bounds, V, segs[:1] + [(col, 0, 1.0, 1, 2, 0, 1, 0)], rows, expect=_lib.DCOR_EINVAL)
        assert "segment 1" in _lib.last_error() and "n_ab = 1 " in _lib.last_error()
        assert np.all(bad == SENTINEL) and np.all(bpriv == SENTINEL)


def test_compaction_past_one_pack_trip_equals_the_host_loop_bitwise():
    """n = 256 * 64 + 65: the mask words of a column span two trips of the compaction.  Column 0 is
    full (its own compaction is the long one); columns 1 and 2 are sparse, so every n_ab stays small,
    with present rows on both sides of the trip boundary and in the last, partial word."""
    n = 256 * 64 + 65
    g = np.random.default_rng(44)
    raw = np.asfortranarray(np.stack([np.round(67.5 + 11.25 * g.standard_normal(n)),
                                      np.round(25.0 + 5.0 * g.standard_normal(n), 1),
                                      0.8 * g.standard_normal(n)], axis=1))
    bounds = [BOUNDS[0], BOUNDS[1], BOUNDS[3]]
    V = np.zeros((3, n), dtype=bool)
    V[0] = True
    V[1, ::41] = V[1, 256 * 64 - 3:256 * 64 + 5] = V[1, n - 7:] = True
    V[2, ::29] = V[2, 256 * 64 - 1:256 * 64 + 2] = V[2, n - 30:n - 2] = True
    nab = {pr: int((V[pr[0]] & V[pr[1]]).sum()) for pr in [(0, 1), (1, 2), (2, 0)]}
    assert all(8 <= v <= 700 for v in nab.values()), nab
    assert (V[1] & V[2])[256 * 64:].any() and (V[1] & V[2])[:256 * 64].any()
    segs = [(a, b, 1.0, 500 + j, 600 + j, 2**32 - 4, 2, 3 * j) for j, (a, b) in enumerate(nab)]
    got, priv = _launch(raw, bounds, V, segs, 9, ld=n + 1)
    want, wpriv, _ = _yardstick(raw, bounds, V, segs, 9)
    named = _named(segs, 9)
    assert np.isfinite(want[named]).all()
    assert np.array_equal(_bits(got[named]), _bits(want[named]))
    assert np.array_equal(_bits(priv[named]), _bits(wpriv[named]))


# ---------------------------------------------------------------- 7. split and order
def test_split_and_order_invariance():
    n = 1001
    raw, V = _raw(n), _present(n)
    a, b, e, sn, si = 0, 1, 1.0, 2**33 + 77, 2**34 + 78
    rb, c = 1001, 5
    one, p1 = _launch(raw, BOUNDS, V, [(a, b, e, sn, si, rb, c, 0)], c, ld=n + 3)
    singles = [(a, b, e, sn, si, rb + j, 1, j) for j in range(c)][::-1]
    rev, p2 = _launch(raw, BOUNDS, V, singles, c)
    assert np.array_equal(_bits(rev), _bits(one)) and np.array_equal(_bits(p2), _bits(p1))
    g1, _ = _launch(raw, BOUNDS, V, [(a, b, e, sn, si, rb, 2, 0)], c, want_priv=False)
    g2, q2 = _launch(raw, BOUNDS, V, [(a, b, e, sn, si, rb + 2, 3, 2)], c, want_priv=False)
    assert np.all(g1[2:] == SENTINEL) and np.all(g2[:2] == SENTINEL) and np.all(q2 == SENTINEL)
    assert np.array_equal(_bits(np.concatenate([g1[:2], g2[2:]])), _bits(one))
    # other segments around it, other out_row blocks with gap rows between them
    mixed = [(2, 3, 2.0, 5, 6, 0, 2, 9), (a, b, e, sn, si, rb, c, 3), (1, 1, 0.1, 7, 8, 4, 1, 0)]
    g3, p3 = _launch(raw, BOUNDS, V, mixed, 12)
    assert np.array_equal(_bits(g3[3:8]), _bits(one)) and np.array_equal(_bits(p3[3:8]), _bits(p1))
    assert np.all(g3[[1, 2, 8, 11]] == SENTINEL) and np.all(p3[[1, 2, 8, 11]] == SENTINEL)


# ---------------------------------------------------------------- 8. Python surface, distributed
def _holes(n):
    return np.asfortranarray(np.where(_present(n).T, _raw(n), np.nan))


def test_python_surface_matches_the_native_call():
    from dcor import hrs
    n = 1001
    V = _present(n)
    T = _holes(n)
    segs = _segments()[:6]
    flat = [s[:7] for s in segs]
    got, priv = _main_case(n)[:2]
    res, pv = hrs.private_pairwise_segments(T, BOUNDS, flat, seed_std=SEED_STD, return_priv=True)
    assert res.shape == (REPS * len(flat), 6) and pv.shape == res.shape
    for j, s in enumerate(segs):
        assert np.array_equal(_bits(res[REPS * j:REPS * (j + 1)]), _bits(got[s[7]:s[7] + REPS]))
        assert np.array_equal(_bits(pv[REPS * j:REPS * (j + 1)]), _bits(priv[s[7]:s[7] + REPS]))
    # explicit masks over a table without NaN give the same
    again = hrs.private_pairwise_segments(_raw(n), BOUNDS, flat, seed_std=SEED_STD, valid=_pack(V, junk=False))
    assert np.array_equal(_bits(again), _bits(res))
    npair = (V.astype(np.int64) @ V.astype(np.int64).T)
    cm = hrs.corr_matrix_private_pairwise(T[:, :3], BOUNDS[:3], 1.0, 4, seed_std=SEED_STD)
    assert cm["pairs"] == [(0, 1), (0, 2), (1, 2)] and cm["runs"].shape == (3, 4, 6)
    assert np.isfinite(cm["runs"]).all() and np.array_equal(cm["n_pair"], npair[:3, :3])
    want = hrs.private_pairwise_segments(T[:, :3], BOUNDS[:3], [(0, 2, 1.0, 10 + 2000, 20 + 2000, 0, 4)],
                                         seed_std=SEED_STD)
    assert np.array_equal(_bits(cm["runs"][1]), _bits(want))
    sw = hrs.corr_matrix_sweep_private_pairwise(T[:, :2], BOUNDS[:2], (0.25, 2.0), 3, seed_std=SEED_STD)
    assert sw["runs"].shape == (1, 2, 3, 6) and np.isfinite(sw["runs"]).all() and len(sw["summaries"]) == 1
    assert np.array_equal(sw["n_pair"], npair[:2, :2])
    want = hrs.private_pairwise_segments(T[:, :2], BOUNDS[:2], [(0, 1, 2.0, 10 + 2000, 20 + 2000, 0, 3)],
                                         seed_std=SEED_STD)
    assert np.array_equal(_bits(sw["runs"][0, 1]), _bits(want))


RANK_SEGS = [(0, 1, 1.0, 61, 71, 0, 7), (3, 1, 0.1, 62, 72, 1001, 3), (2, 2, 2.0, 63, 73, 5, 0),
             (1, 2, 2.45, 64, 74, 2, 4)]


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def test_hrs_private_pairwise_distributed_rccl_world1():
    import torch
    import torch.distributed as dist
    from dcor import hrs
    from dcor.dist import hrs_private_pairwise_distributed
    T = _holes(1001)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()))
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    try:
        got = [hrs_private_pairwise_distributed(T, BOUNDS, RANK_SEGS, seed_std=SEED_STD).tobytes(),
               hrs_private_pairwise_distributed(T, BOUNDS, []).tobytes()]
    finally:
        dist.destroy_process_group()
    want = [hrs.private_pairwise_segments(T, BOUNDS, RANK_SEGS, seed_std=SEED_STD).tobytes(), b""]
    assert len(want[0]) == 14 * 48 and got == want


# ---------------------------------------------------------------- 9. the released mean, independently
def test_released_mean_against_exact_rational_arithmetic():
    """api.dp_sd runs the same reduction code as the new preparation, so one anchor avoids it: for one
    column, m1 = the mean of the clipped present rows and the noise term s lap, s = (hi - lo) / (n_c
    eps_mean), in exact rationals (fractions, as tests/accum_ref.py), lap the replicate's first site-17
    draw of the column.  |mean - (m1 + s lap)| <= 4 * 2^-53 * max(|m1|, |s lap|): three roundings (s, s
    lap, the sum) on top of a double-double sum whose own error is far below that.  n_c, not n_ab and
    not n, is the count: with either of the others the mean is off by more than 1e-3 of the noise term."""
    n, c, r = 1001, 1, 1001
    raw, V = _raw(n), _present(n)
    lo, hi = BOUNDS[c]
    segs = [(c, 0, 1.0, 1, 2, r, 1, 0), (2, c, 1.0, 3, 4, r, 1, 1)]
    _, priv = _launch(raw, BOUNDS, V, segs, 2)
    lap = float(_draws(SEED_STD, r, P)[2 * c])
    xs = raw[V[c], c]
    n_c = len(xs)
    assert n_c == V[c].sum() and n_c > (V[c] & V[0]).sum() and n_c > (V[c] & V[2]).sum() and n_c < n
    m1 = sum(Fraction(min(max(float(x), lo), hi)) for x in xs) / n_c
    term = Fraction(hi - lo) / (n_c * Fraction(0.1)) * Fraction(lap)
    exact = m1 + term
    bound = 4 * Fraction(1, 2**53) * max(abs(m1), abs(term))
    for mean in (priv[0, 0], priv[1, 3]):
        err = abs(Fraction(float(mean)) - exact)
        print(f"released mean {mean!r}: |error| = {float(err):.3e}, bound {float(bound):.3e}")
        assert err <= bound
    wrong = m1 + term * n_c / int((V[c] & V[0]).sum())
    assert abs(wrong - exact) > 1000 * bound
