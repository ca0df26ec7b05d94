"""GPU tests of the private HRS table path (dcor_hrs_private_table_launch, dcor.hrs.private_segments /
corr_matrix_private, dcor.dist.hrs_private_distributed).  The yardstick is always the composition of
the entries that existed before it, one replicate number r at a time: dcor_draws_launch(0, seed_std,
17, r, 1, 2 p) -> hrs.standardize_table(raw, bounds, lap) (or the api.dp_sd / standardize_dp /
lambda_from_priv trio at other budgets) -> one hrs.table_segments call holding every segment at
rep_begin = r, reps = 1.  Records are compared as uint64; the new path is never its own reference.

Replicate ranges: the segment entries run replicates up to 2^32 - 2 (rep_begin + reps <= 2^32 - 1,
the table entry's own check, which the yardstick call obeys too), so the top block is rep_begin =
2^32 - 4 with 3 replicates: the last legal range."""
import ctypes as C
import os
import socket

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

P = 4
# age-like, bmi-like, a coarse grid, and bounds that clip about 10 % of the column
BOUNDS = [(45.0, 90.0), (15.0, 35.0), (0.0, 8.0), (-1.3, 1.3)]
PAIRS = [(0, 1), (1, 0), (2, 3), (1, 1)]
# at n = 1000 / 1001: the k < 2 guard (k = 2, m = 500), m = 8, and the m == 2 path twice
EPS = [0.1, 1.0, 2.0, 2.45]
REP_BEGIN = [0, 1001, 2**32 - 4]
REPS = 3
SEED_STD = 2**35 + 12345
SENTINEL = -7.25


def _raw(n, seed=31):
    g = np.random.default_rng(seed + n)
    age = np.round(67.5 + 11.25 * g.standard_normal(n))
    bmi = np.round(25.0 + 5.0 * (-0.3 * (age - 67.5) / 11.25 + np.sqrt(0.91) * g.standard_normal(n)), 1)
    grid = np.clip(np.round(4.0 + 2.0 * g.standard_normal(n)), -1.0, 9.0)        # a few values outside [0, 8]
    wide = 0.8 * g.standard_normal(n)                                            # ~10 % outside +-1.3
    cut = np.mean((wide < -1.3) | (wide > 1.3))
    assert 0.05 < cut < 0.15 and len(np.unique(grid)) <= 11
    return np.asfortranarray(np.stack([age, bmi, grid, wide], axis=1))


def _segments():
    """(col_x, col_y, eps, seed_ni, seed_int, rep_begin, reps, out_row): every pair x every eps, keys
    above 2^32, the three replicate offsets in turn, output blocks in a shuffled order with one
    unnamed row after each block."""
    cells = [(a, b, e) for a, b in PAIRS for e in EPS]
    order = np.random.default_rng(4).permutation(len(cells))
    return [(a, b, e, 2**33 + 1010 + 7 * j, 2**34 + 1020 + 11 * j, REP_BEGIN[(j + j // 4) % 3], REPS,
             (REPS + 1) * int(order[j])) for j, (a, b, e) in enumerate(cells)]


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def _launch(raw, bounds, segs, rows, ld=None, seed_std=SEED_STD, eps_mean=0.1, eps_m2=0.1, want_priv=True,
            expect=0):
    """dcor_hrs_private_table_launch on the (n, p) array raw laid out with `ld` elements between
    columns; the record and d_priv buffers start out as SENTINEL.  -> (records, priv)."""
    import torch
    from dcor import _lib
    n, p = raw.shape
    ld = n if ld is None else ld
    host = np.full((p, ld), -123.0)   # the gap between columns is never read
    host[:, :n] = raw.T
    Dd = torch.as_tensor(host.reshape(-1), device="cuda")
    out = torch.full((max(rows, 1), 6), SENTINEL, dtype=torch.float64, device="cuda")
    priv = torch.full((max(rows, 1), 6), SENTINEL, dtype=torch.float64, device="cuda")
    lo = np.array([b[0] for b in bounds], dtype=np.float64)
    hi = np.array([b[1] for b in bounds], dtype=np.float64)
    D = C.POINTER(C.c_double)
    desc = _lib.HrsPrivateDesc(n=n, p=p, ld=ld, D=Dd.data_ptr(), lo=lo.ctypes.data_as(D), hi=hi.ctypes.data_as(D),
                               eps_mean=eps_mean, eps_m2=eps_m2, seed_std=seed_std, alpha=0.05, delta=1.0 / n,
                               nsim=2000)
    arr = (_lib.HrsPairSegment * max(len(segs), 1))(*[
        _lib.HrsPairSegment(eps=e, seed_ni=sn, seed_int=si, rep_begin=rb, reps=c, out_row=row, col_x=a, col_y=b)
        for a, b, e, sn, si, rb, c, row in segs])
    st = _lib.lib.dcor_hrs_private_table_launch(
        C.byref(desc), arr, len(segs), C.c_void_p(out.data_ptr()),
        C.c_void_p(priv.data_ptr()) if want_priv else None,
        C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert st == expect, _lib.last_error()
    return out.cpu().numpy(), priv.cpu().numpy()


def _draws(seed_std, r, p):
    """The site-17 unit Laplace draws of replicate r: [mean, m2] of column 0, of column 1, ..."""
    import torch
    from dcor import _lib
    t = torch.empty(2 * p, dtype=torch.float64, device="cuda")
    _lib.check(_lib.lib.dcor_draws_launch(0, seed_std, _lib.SITE_STD, r, 1, 2 * p, C.c_void_p(t.data_ptr()),
                                          C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    return t.cpu().numpy()


def _release(raw, bounds, lap, eps_mean, eps_m2):
    """The helpers' trio per column -> (Z column-major, lam [p], priv rows [p, 3] = mean, sd, lam)."""
    from dcor import api
    cols, rows = [], []
    for c, (lo, hi) in enumerate(bounds):
        col = np.ascontiguousarray(raw[:, c])
        pv = api.dp_sd(col, lo, hi, eps_mean, eps_m2, lap=lap[2 * c:2 * c + 2])
        cols.append(api.standardize_dp(col, pv, lo, hi))
        rows.append((pv["mean"], pv["sd"], api.lambda_from_priv(lo, hi, pv)))
    rows = np.array(rows)
    return np.asfortranarray(np.stack(cols, axis=1)), rows[:, 2].copy(), rows


def _yardstick(raw, bounds, segs, rows, seed_std=SEED_STD, eps_mean=0.1, eps_m2=0.1, skip_cols=()):
    """Records and d_priv rows of `segs` from the existing entries: per distinct replicate number one
    draws launch, one standardisation on the host helpers and one table call of single-replicate
    segments.  skip_cols: columns whose pairs have no yardstick (a NaN release); their rows stay NaN."""
    from dcor import hrs
    n, p = raw.shape
    want = np.full((rows, 6), np.nan)
    wpriv = np.full((rows, 6), np.nan)
    reps = sorted({rb + j for *_, rb, c, _row in segs for j in range(c)})
    for r in reps:
        lap = _draws(seed_std, r, p)
        if eps_mean == hrs.EPS_MEAN and eps_m2 == hrs.EPS_M2 and not skip_cols:
            t = hrs.standardize_table(raw, bounds, lap=lap)
            Z, lam = t["Z"], t["lam"]
            prow = np.array([(pv["mean"], pv["sd"], l) for pv, l in zip(t["priv"], lam)])
        else:
            Z, lam, prow = _release(raw, bounds, lap, eps_mean, eps_m2)
        keep = [c for c in range(p) if c not in skip_cols]
        idx = {c: i for i, c in enumerate(keep)}
        one, where = [], []
        for a, b, e, sn, si, rb, c, row in segs:
            if rb <= r < rb + c and a not in skip_cols and b not in skip_cols:
                one.append((idx[a], idx[b], e, sn, si, r, 1))
                where.append((row + (r - rb), a, b))
        if not one:
            continue
        got = hrs.table_segments(np.asfortranarray(Z[:, keep]), lam[keep], one, delta=1.0 / n)
        for rec, (row, a, b) in zip(got, where):
            want[row] = rec
            wpriv[row] = np.concatenate([prow[a], prow[b]])
    return want, wpriv, len(reps)


_CACHE = {}


def _main_case(n):
    """The main segment list in one private call (columns at 8-B offsets: ld = n + 3) and its
    yardstick, computed once per n and left unchanged."""
    if n not in _CACHE:
        raw, segs = _raw(n), _segments()
        rows = (REPS + 1) * len(segs)
        got, priv = _launch(raw, BOUNDS, segs, rows, ld=n + 3)
        want, wpriv, nrep = _yardstick(raw, BOUNDS, segs, rows)
        for a in (got, priv, want, wpriv):
            a.setflags(write=False)
        _CACHE[n] = (got, priv, want, wpriv, nrep)
    return _CACHE[n]


def _named(segs, rows):
    m = np.zeros(rows, dtype=bool)
    for *_, c, row in segs:
        m[row:row + c] = True
    return m


# ---------------------------------------------------------------- 1. records, byte for byte
@pytest.mark.parametrize("n", [1000, 1001])
def test_records_equal_the_composed_entries_bitwise(n):
    from dcor import api
    assert [api.batch_geometry(1000, e, e, "subG", hrs=True) for e in EPS] == [(2, 500), (125, 8), (500, 2), (500, 2)]
    segs = _segments()
    assert {s[5] for s in segs} == set(REP_BEGIN)
    # every pair meets every replicate offset across its four eps
    for pr in PAIRS:
        assert {s[5] for s in segs if s[:2] == pr} == set(REP_BEGIN), pr
    got, _, want, _, nrep = _main_case(n)
    assert nrep == 9                                   # 9 distinct replicate numbers: 9 yardstick calls
    named = _named(segs, len(got))
    assert named.sum() == REPS * len(segs)
    assert np.isfinite(want[named]).all()
    assert np.array_equal(_bits(got[named]), _bits(want[named]))
    assert np.all(got[~named] == SENTINEL)             # the row after each block survives
    # the replicate's release matters: two replicates of one segment differ
    s = segs[5]
    assert not np.array_equal(got[s[7]], got[s[7] + 1])


# ---------------------------------------------------------------- 2. one release for every pair
@pytest.mark.parametrize("n", [1000, 1001])
def test_d_priv_is_the_helpers_release_and_the_same_for_every_pair(n):
    segs = _segments()
    _, priv, _, wpriv, _ = _main_case(n)
    named = _named(segs, len(priv))
    assert np.array_equal(_bits(priv[named]), _bits(wpriv[named]))
    assert np.all(priv[~named] == SENTINEL)
    # column 1's triple at one replicate number: identical in (0, 1), (1, 0), (1, 1) and across eps
    seen = {}
    for a, b, e, sn, si, rb, c, row in segs:
        for j in range(c):
            for side, col in ((0, a), (1, b)):
                if col == 1:
                    seen.setdefault(rb + j, []).append(priv[row + j, 3 * side:3 * side + 3].tobytes())
    assert len(seen) == 9
    for r, triples in seen.items():
        assert len(triples) >= 4 and len(set(triples)) == 1, r
    assert len({t[0] for t in seen.values()}) == 9     # and it differs between replicates


def test_other_budgets_against_the_helper_trio():
    """eps_mean, eps_m2 other than the study's 0.1: the yardstick standardises with api.dp_sd /
    standardize_dp / lambda_from_priv directly."""
    n = 1001
    raw = _raw(n)
    segs = [(0, 1, 1.0, 2**33 + 5, 2**34 + 6, 7, 2, 0), (3, 2, 2.0, 2**33 + 8, 2**34 + 9, 7, 2, 3)]
    kw = dict(seed_std=2**40 + 3, eps_mean=0.3, eps_m2=0.7)
    got, priv = _launch(raw, BOUNDS, segs, 6, ld=n, **kw)
    want, wpriv, _ = _yardstick(raw, BOUNDS, segs, 6, **kw)
    named = _named(segs, 6)
    assert np.isfinite(want[named]).all()
    assert np.array_equal(_bits(got[named]), _bits(want[named]))
    assert np.array_equal(_bits(priv[named]), _bits(wpriv[named]))
    assert np.all(got[~named] == SENTINEL) and np.all(priv[~named] == SENTINEL)


# ---------------------------------------------------------------- 3. split invariance
def test_split_and_order_invariance():
    n = 1001
    raw = _raw(n)
    a, b, e, sn, si = 0, 1, 1.0, 2**33 + 77, 2**34 + 78
    rb, c = 1001, 5
    one, p1 = _launch(raw, BOUNDS, [(a, b, e, sn, si, rb, c, 0)], c, ld=n + 3)
    singles = [(a, b, e, sn, si, rb + j, 1, j) for j in range(c)][::-1]
    rev, p2 = _launch(raw, BOUNDS, singles, c, ld=n)
    assert np.array_equal(_bits(rev), _bits(one)) and np.array_equal(_bits(p2), _bits(p1))
    g1, _ = _launch(raw, BOUNDS, [(a, b, e, sn, si, rb, 2, 0)], c, ld=n + 3, want_priv=False)
    g2, _ = _launch(raw, BOUNDS, [(a, b, e, sn, si, rb + 2, 3, 2)], c, ld=n + 3, want_priv=False)
    assert np.all(g1[2:] == SENTINEL) and np.all(g2[:2] == SENTINEL)
    assert np.array_equal(_bits(np.concatenate([g1[:2], g2[2:]])), _bits(one))


RANK_SEGS = [(0, 1, 1.0, 61, 71, 0, 7), (3, 1, 0.1, 62, 72, 1001, 3), (2, 2, 2.0, 63, 73, 5, 0),
             (1, 2, 2.45, 64, 74, 2, 4)]


def _rank_runs():
    from dcor.dist import hrs_private_distributed
    raw = _raw(1001)
    return [hrs_private_distributed(raw, BOUNDS, RANK_SEGS, seed_std=SEED_STD).tobytes(),
            hrs_private_distributed(raw, BOUNDS, [(1, 0, 1.0, 65, 75, 9, 1)], seed_std=SEED_STD).tobytes(),
            hrs_private_distributed(raw, BOUNDS, []).tobytes()]


def _rank_expected():
    from dcor import hrs
    raw = _raw(1001)
    return [hrs.private_segments(raw, BOUNDS, RANK_SEGS, seed_std=SEED_STD).tobytes(),
            hrs.private_segments(raw, BOUNDS, [(1, 0, 1.0, 65, 75, 9, 1)], seed_std=SEED_STD).tobytes(), b""]


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def test_hrs_private_distributed_rccl_world1():
    import torch
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()))
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    try:
        got = _rank_runs()
    finally:
        dist.destroy_process_group()
    want = _rank_expected()
    assert len(want[0]) == 14 * 48 and got == want


def _rank_worker(rank, world, port, q):
    import torch
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    q.put((rank, _rank_runs()))
    dist.destroy_process_group()


def test_hrs_private_distributed_two_ranks_on_gpu():
    """World size 2: two gloo ranks sharing cuda:0, each running its contiguous part of the flattened
    (segment, replicate) space (the split falls inside a segment); the gathered records are the
    one-process call's bytes."""
    import torch.multiprocessing as mp
    world, port = 2, _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_rank_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    got = dict(q.get(timeout=200) for _ in range(world))
    for p in procs:
        p.join(timeout=30)
        assert p.exitcode == 0
    want = _rank_expected()
    assert got[0] == want and got[1] == want


# ---------------------------------------------------------------- 4. degenerate sd
def test_constant_column_with_negative_variance_draw_takes_the_floor_denominator():
    """A constant column (xc all equal, so m2 = m1^2 up to rounding) at a replicate whose draws make
    m2p - mean^2 < 0: sd = 0 and den = 1e-8.  The replicate is picked from the oracle's restatement of
    the draws, on the CPU, and checked to be degenerate."""
    import oracle.oracle as orc
    n, seed_std = 1000, 2**36 + 99
    lo, hi, v = 15.0, 35.0, 27.5
    raw = _raw(n).copy(order="F")
    raw[:, 1] = v
    nd = float(n)
    pick = None
    for r in range(64):
        lap = orc.gen_laplace(seed_std, r, 17, 2 * P)
        mean = v + ((hi - lo) / (nd * 0.1)) * lap[2]
        m2p = v * v + ((hi * hi - lo * lo) / (nd * 0.1)) * lap[3]
        if m2p - mean * mean < -1e-6:
            pick = r
            break
    assert pick is not None
    assert np.array_equal(_bits(_draws(seed_std, pick, P)), _bits(orc.gen_laplace(seed_std, pick, 17, 2 * P)))
    segs = [(0, 1, 1.0, 2**33 + 1, 2**34 + 2, pick, 1, 0), (1, 0, 2.0, 2**33 + 3, 2**34 + 4, pick, 1, 1),
            (1, 1, 0.1, 2**33 + 5, 2**34 + 6, pick, 1, 2)]
    got, priv = _launch(raw, BOUNDS, segs, 3, ld=n, seed_std=seed_std)
    want, wpriv, _ = _yardstick(raw, BOUNDS, segs, 3, seed_std=seed_std)
    assert priv[0, 4] == 0.0 and priv[1, 1] == 0.0          # sd of column 1: the case is degenerate
    assert priv[0, 5] > 1e8                                  # lam = |bound - mean| / 1e-8
    assert np.isfinite(got).all() and np.isfinite(want).all()
    assert np.array_equal(_bits(got), _bits(want)) and np.array_equal(_bits(priv), _bits(wpriv))


# ---------------------------------------------------------------- 5. NaN
def test_nan_reaches_only_the_pairs_that_name_its_column():
    from dcor import hrs
    n = 1001
    raw = _raw(n).copy(order="F")
    raw[500, 3] = np.nan
    segs = [(a, b, 1.0, 50 + j, 60 + j, 3, 2, 2 * j) for j, (a, b) in enumerate(PAIRS + [(3, 3), (0, 2)])]
    got, priv = _launch(raw, BOUNDS, segs, 2 * len(segs), ld=n + 3)
    want, wpriv, _ = _yardstick(raw, BOUNDS, segs, 2 * len(segs), skip_cols=(3,))
    for a, b, *_, row in segs:
        rows = slice(row, row + 2)
        if 3 in (a, b):
            assert np.isnan(got[rows]).all(), (a, b)
            side = slice(0, 3) if a == 3 else slice(3, 6)
            assert np.isnan(priv[rows, side]).all()
        else:
            assert np.isfinite(want[rows]).all()
            assert np.array_equal(_bits(got[rows]), _bits(want[rows])), (a, b)
            assert np.array_equal(_bits(priv[rows]), _bits(wpriv[rows])), (a, b)
    with pytest.raises(ValueError, match="corr_matrix_pairwise"):
        hrs.private_segments(raw, BOUNDS, [(0, 1, 1.0, 1, 2, 0, 1)])


# ---------------------------------------------------------------- 6. top of the index range
def test_largest_table_matches_the_composed_entries():
    """n = 65536: the u16 index row at its last value and the preparation at the largest column."""
    n = 65536
    g = np.random.default_rng(8)
    raw = np.asfortranarray(np.stack([np.round(67.5 + 11.25 * g.standard_normal(n)),
                                      np.round(25.0 + 5.0 * g.standard_normal(n), 1)], axis=1))
    bounds = BOUNDS[:2]
    segs = [(0, 1, 2.0, 2**33 + 9, 2**34 + 9, 12, 1, 0)]
    got, priv = _launch(raw, bounds, segs, 2, ld=n)
    want, wpriv, _ = _yardstick(raw, bounds, segs, 2)
    assert np.isfinite(want[0]).all()
    assert np.array_equal(_bits(got[0]), _bits(want[0])) and np.array_equal(_bits(priv[0]), _bits(wpriv[0]))
    assert np.all(got[1] == SENTINEL) and np.all(priv[1] == SENTINEL)


# ---------------------------------------------------------------- 7. empty, invalid, Python surface
def test_empty_and_invalid_calls_leave_both_outputs_untouched():
    from dcor import _lib
    n = 1000
    raw = _raw(n)
    ok = (0, 1, 1.0, 1, 2, 0, REPS, 0)

    def untouched(res):
        return np.all(res[0] == SENTINEL) and np.all(res[1] == SENTINEL)
    assert untouched(_launch(raw, BOUNDS, [], 4))
    assert untouched(_launch(raw, BOUNDS, [(0, 1, 1.0, 1, 2, 0, 0, 0), (2, 3, 2.0, 3, 4, 5, 0, 1)], 4))
    for bad in ((0, P, 1.0, 1, 2, 0, 1, 3), (0, 1, 0.0, 1, 2, 0, 1, 3), (0, 1, 1.0, 1, 2, 2**32 - 3, 3, 3),
                (0, 1, 1.0, 1, 2, 0, -1, 3)):
        assert untouched(_launch(raw, BOUNDS, [ok, bad], 4, expect=_lib.DCOR_EINVAL)), bad
        assert "segment 1" in _lib.last_error()
    bounds = list(BOUNDS)
    bounds[2] = (8.0, 8.0)
    assert untouched(_launch(raw, bounds, [ok], 4, expect=_lib.DCOR_EINVAL))
    assert "column 2" in _lib.last_error()
    assert untouched(_launch(raw, BOUNDS, [ok], 4, eps_m2=0.0, expect=_lib.DCOR_EINVAL))


def test_python_surface_matches_the_native_call():
    from dcor import hrs
    n = 1001
    raw = _raw(n)
    segs = _segments()[:6]
    flat = [s[:7] for s in segs]
    got, priv = _main_case(n)[:2]
    res, pv = hrs.private_segments(raw, BOUNDS, flat, seed_std=SEED_STD, return_priv=True)
    assert res.shape == (REPS * len(flat), 6) and pv.shape == res.shape
    for j, s in enumerate(segs):
        assert np.array_equal(_bits(res[REPS * j:REPS * (j + 1)]), _bits(got[s[7]:s[7] + REPS]))
        assert np.array_equal(_bits(pv[REPS * j:REPS * (j + 1)]), _bits(priv[s[7]:s[7] + REPS]))
    assert np.array_equal(_bits(hrs.private_segments(raw, BOUNDS, flat, seed_std=SEED_STD)), _bits(res))
    cm = hrs.corr_matrix_private(raw[:, :3], BOUNDS[:3], 1.0, 4, seed_std=SEED_STD)
    assert cm["pairs"] == [(0, 1), (0, 2), (1, 2)] and cm["runs"].shape == (3, 4, 6)
    assert np.isfinite(cm["runs"]).all()
    want = hrs.private_segments(raw[:, :3], BOUNDS[:3], [(0, 2, 1.0, 10 + 2000, 20 + 2000, 0, 4)], seed_std=SEED_STD)
    assert np.array_equal(_bits(cm["runs"][1]), _bits(want))
    sw = hrs.corr_matrix_sweep_private(raw[:, :2], BOUNDS[:2], (0.25, 2.0), 3, seed_std=SEED_STD)
    assert sw["runs"].shape == (1, 2, 3, 6) and np.isfinite(sw["runs"]).all() and len(sw["summaries"]) == 1


# ---------------------------------------------------------------- 8. untouched paths
_UNTOUCHED = """
import sys
import numpy as np
sys.path[:0] = {paths!r}
from dcor import hrs
g = np.random.default_rng(3)
Z = np.asfortranarray(g.standard_normal((1001, 3)))
if {call_new}:
    raw = np.asfortranarray(60.0 + 10.0 * g.standard_normal((1001, 2)))
    hrs.private_segments(raw, [(45.0, 90.0), (45.0, 90.0)], [(0, 1, 1.0, 1, 2, 0, 2)])
from dcor import api
pv = api.dp_sd(Z[:, 0], -2.0, 2.0, 0.1, 0.1, lap=np.array([0.3, -0.2]))
out = hrs.table_segments(Z, [2.2, 1.9, 2.4], [(0, 1, 1.0, 5, 6, 0, 3), (2, 0, 0.1, 7, 8, 1001, 2)])
sys.stdout.write(out.tobytes().hex() + " " + np.array([pv["mean"], pv["sd"]]).tobytes().hex())
"""


def test_existing_table_entry_is_unchanged_by_the_new_entry():
    """table_segments on a fixed Z (and dp_sd, whose sum the new preparation shares) gives the same
    bytes in a process that has and one that has not called the new entry: two fresh processes,
    since the property is about a process's history."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    paths = [root, os.path.join(root, "distributed-correlation_amd")]
    outs = []
    for call_new in (False, True):
        r = subprocess.run([sys.executable, "-c", _UNTOUCHED.format(paths=paths, call_new=call_new)],
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        outs.append(r.stdout.strip())
    assert outs[0] == outs[1] and len(outs[0]) > 2 * 5 * 48
