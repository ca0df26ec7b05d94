"""GPU tests of the HRS table path (dcor_hrs_table_launch, dcor.hrs.table_segments / corr_matrix /
corr_matrix_sweep / standardize_table, dcor.dist.hrs_table_distributed).  The yardstick is the
panel entry (dcor_hrs_fused_launch through dcor.hrs.hrs_replicates(mode='fused')) on the pair's two
columns and clip bounds, compared as uint64, and the oracle's estimators on its own restatement of
the Philox streams -- never the table path itself."""
import ctypes as C
import os
import socket

import numpy as np
import pytest

from helpers import assert_close

pytestmark = pytest.mark.gpu

P = 4
LAM = np.array([2.2, 2.6, 1.9, 2.4])      # distinct per column; each clips some of its column
PAIRS = [(0, 1), (1, 0), (2, 3), (0, 2), (1, 1)]
# at n = 1000 / 1001: the k < 2 guard (k = 2, m = 500), m = 128, m = 8, and the m == 2 path twice
EPS = [0.1, 0.25, 1.0, 2.0, 2.45]
REP_BEGIN = [0, 1001, 2**32 - 6]
REPS = 3
SENTINEL = -7.25


def _table(n, seed=23):
    """Columns 0-1 continuous (no dictionary: the panel entry runs its L2-gather kernel), columns 2-3
    of dcor.signpanel.standin_table (a coarse grid, at most 256 distinct values: the coded kernel)."""
    from dcor import signpanel
    g = np.random.default_rng(seed + n)
    x = g.standard_normal(n)
    y = -0.3 * x + np.sqrt(1 - 0.09) * g.standard_normal(n)
    T = signpanel.standin_table(n, 4, 0.5, seed=seed)
    assert all(len(np.unique(T[:, c])) <= 256 for c in (2, 3)) and len(np.unique(x)) == n
    return np.asfortranarray(np.stack([x, y, T[:, 2], T[:, 3]], axis=1))


def _segments():
    """(col_x, col_y, eps, seed_ni, seed_int, rep_begin, reps, out_row): every pair x every eps, keys
    above 2^32, the three replicate offsets in turn, output blocks in a shuffled order with one
    unnamed row after each block."""
    cells = [(a, b, e) for a, b in PAIRS for e in EPS]
    order = np.random.default_rng(4).permutation(len(cells))
    return [(a, b, e, 2**33 + 1010 + 7 * j, 2**34 + 1020 + 11 * j, REP_BEGIN[j % 3], REPS,
             (REPS + 1) * int(order[j])) for j, (a, b, e) in enumerate(cells)]


def _launch(Z, lam, segs, rows, ld=None, sentinel=SENTINEL, expect=0):
    """dcor_hrs_table_launch on the (n, p) array Z laid out with `ld` elements between columns; the
    record buffer starts out as `sentinel`."""
    import torch
    from dcor import _lib
    n, p = Z.shape
    ld = n if ld is None else ld
    host = np.full((p, ld), -123.0)   # the gap between columns is never read
    host[:, :n] = Z.T
    Dd = torch.as_tensor(host.reshape(-1), device="cuda")
    out = torch.full((max(rows, 1), 6), sentinel, dtype=torch.float64, device="cuda")
    lam = np.ascontiguousarray(lam, dtype=np.float64)
    desc = _lib.HrsTableDesc(n=n, p=p, ld=ld, D=Dd.data_ptr(), lam=lam.ctypes.data_as(C.POINTER(C.c_double)),
                             alpha=0.05, delta=1.0 / n, nsim=2000)
    arr = (_lib.HrsPairSegment * max(len(segs), 1))(*[
        _lib.HrsPairSegment(eps=e, seed_ni=sn, seed_int=si, rep_begin=rb, reps=c, out_row=row, col_x=a, col_y=b)
        for a, b, e, sn, si, rb, c, row in segs])
    st = _lib.lib.dcor_hrs_table_launch(C.byref(desc), arr, len(segs), C.c_void_p(out.data_ptr()),
                                        C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert st == expect, _lib.last_error()
    return out.cpu().numpy()


def _panel(Z, lam, seg):
    """The yardstick: the panel entry on the segment's two columns and their clip bounds."""
    from dcor import hrs
    a, b, e, sn, si, rb, c = seg[:7]
    return hrs.hrs_replicates(np.ascontiguousarray(Z[:, a]), np.ascontiguousarray(Z[:, b]), float(lam[a]),
                              float(lam[b]), e, c, seed_ni=sn, seed_int=si, rep_begin=rb, mode="fused")


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


_CACHE = {}


def _one_call(n):
    """Test 1's segment list in one table call (columns at 8-B offsets: ld = n + 3), computed once
    per n and left unchanged."""
    if n not in _CACHE:
        segs = _segments()
        _CACHE[n] = _launch(_table(n), LAM, segs, (REPS + 1) * len(segs), ld=n + 3)
        _CACHE[n].setflags(write=False)
    return _CACHE[n]


# ---------------------------------------------------------------- 1. byte equality per pair
@pytest.mark.parametrize("n", [1001, 1000])
def test_every_segment_equals_the_panel_entry_bitwise(n):
    """Odd and even n (the local-noise tail), continuous and coded reference panels and a mixed one,
    (a, b) and (b, a), (a, a), every geometry, replicate offsets up to the last legal range."""
    from dcor import api
    assert [api.batch_geometry(1000, e, e, "subG", hrs=True) for e in EPS] == [
        (2, 500), (7, 128), (125, 8), (500, 2), (500, 2)]
    Z, segs = _table(n), _segments()
    got = _one_call(n)
    named = np.zeros(len(got), dtype=bool)
    for seg in segs:
        rows = slice(seg[7], seg[7] + REPS)
        named[rows] = True
        want = _panel(Z, LAM, seg)
        assert np.isfinite(want).all()
        assert np.array_equal(_bits(got[rows]), _bits(want)), seg
    assert named.sum() == REPS * len(segs) and np.all(got[~named] == SENTINEL)
    # the pairs differ from one another: (0, 1) and (1, 0) are different segments' data
    s01, s10 = segs[2], segs[len(EPS) + 2]
    assert s01[:3] == (0, 1, 1.0) and s10[:3] == (1, 0, 1.0)
    assert not np.array_equal(got[s01[7]:s01[7] + REPS, 3:], got[s10[7]:s10[7] + REPS, 3:])


def test_split_and_order_invariance():
    n = 1001
    Z, segs = _table(n), _segments()
    rows = (REPS + 1) * len(segs)
    one = _one_call(n)
    # one range in two calls: segment 13's replicates [rb, rb + 1) and [rb + 1, rb + 3)
    a, b, e, sn, si, rb, c, row = segs[13]
    first = segs[:13] + [(a, b, e, sn, si, rb, 1, row)]
    second = [(a, b, e, sn, si, rb + 1, 2, row + 1)] + segs[14:]
    g1 = _launch(Z, LAM, first, rows, ld=n + 3)
    g2 = _launch(Z, LAM, second, rows, ld=n + 3)
    named1 = np.zeros(rows, dtype=bool)
    for seg in first:
        named1[seg[7]:seg[7] + seg[6]] = True
    assert np.all(g1[~named1] == SENTINEL) and np.all(g2[named1] == SENTINEL)
    assert np.array_equal(_bits(np.where(named1[:, None], g1, g2)), _bits(one))
    # the same range as two segments of one call
    both = segs[:13] + [(a, b, e, sn, si, rb, 1, row), (a, b, e, sn, si, rb + 1, 2, row + 1)] + segs[14:]
    assert np.array_equal(_bits(_launch(Z, LAM, both, rows, ld=n + 3)), _bits(one))
    # reversed segment order, and another column pitch
    assert np.array_equal(_bits(_launch(Z, LAM, segs[::-1], rows, ld=n)), _bits(one))


# ---------------------------------------------------------------- 2. oracle
@pytest.mark.parametrize("n", [257, 1001])
@pytest.mark.parametrize("eps", [0.25, 2.0])
def test_pair_matches_oracle(n, eps):
    """One pair with lam_a != lam_b against oracle.ni_subg / int_subg (hrs = 1) fed the oracle's own
    restatement of the streams at the HRS sites, within the project's 1e-12 / 1e-13 contract."""
    import oracle.oracle as orc
    from dcor import api, hrs
    Z = _table(n)
    a, b, sn, si, rb, reps = 1, 0, 1010, 1020, 3, 4
    got = hrs.table_segments(Z, LAM, [(a, b, eps, sn, si, rb, reps)])
    assert got.shape == (reps, 6) and np.isfinite(got).all()
    X, Y = np.ascontiguousarray(Z[:, a]), np.ascontiguousarray(Z[:, b])
    k, m = api.batch_geometry(n, eps, eps, "subG", hrs=True)
    delta = 1.0 / n
    lam_r = api.lambda_receiver_from_noise(LAM[a], LAM[b], eps, delta)
    for r in range(reps):
        rep = rb + r
        st, ni, _ = orc.ni_subg(X, Y, eps, eps, hrs=1, lam_x=LAM[a], lam_y=LAM[b],
                                perm=orc.perm(sn, 8, rep, n, k * m),
                                lap_x=orc.gen_laplace(sn, rep, hrs.SITE_NI_LAP_X, k),
                                lap_y=orc.gen_laplace(sn, rep, hrs.SITE_NI_LAP_Y, k))
        st2, it, _ = orc.int_subg(X, Y, eps, eps, hrs=1, lam_s=LAM[a], lam_o=LAM[b], lam_r=lam_r, delta=delta,
                                  lap_local=orc.gen_laplace(si, rep, hrs.SITE_INT_LOCAL, n),
                                  lap_central=orc.gen_laplace(si, rep, hrs.SITE_INT_CENTRAL, 1)[0],
                                  mix_z=orc.gen_normals(si, rep, hrs.SITE_MIX_Z, 2000),
                                  mix_l=orc.gen_laplace(si, rep, hrs.SITE_MIX_L, 2000))
        assert st == 0 and st2 == 0
        assert_close(got[r], np.concatenate([ni, it]), what=f"pair ({a}, {b}) n={n} eps={eps} rep {rep}")


# ---------------------------------------------------------------- 3. NaN isolation
def test_nan_reaches_only_the_pairs_that_name_its_column():
    """A NaN in one sample of column 1.  Pairs without column 1: the clean table's records byte for
    byte; pairs with it: the panel entry on the same columns, NaN pattern included."""
    n = 1001
    clean = _table(n)
    Z = clean.copy(order="F")
    Z[500, 1] = np.nan
    segs = [(a, b, 1.0, 50 + j, 60 + j, 0, REPS, REPS * j) for j, (a, b) in enumerate(PAIRS)]
    got = _launch(Z, LAM, segs, REPS * len(segs), ld=n + 3)
    ref = _launch(clean, LAM, segs, REPS * len(segs), ld=n + 3)
    assert np.isfinite(ref).all()
    for seg in segs:
        rows = slice(seg[7], seg[7] + REPS)
        if 1 in seg[:2]:
            want = _panel(Z, LAM, seg)
            assert np.isnan(want[:, 3:]).all()          # INT reads every sample
            assert np.array_equal(got[rows], want, equal_nan=True), seg
        else:
            assert np.array_equal(_bits(got[rows]), _bits(ref[rows])), seg


# ---------------------------------------------------------------- 4. empty and invalid
def test_empty_and_invalid_calls_leave_the_records_untouched():
    from dcor import _lib
    n = 1000
    Z = _table(n)
    ok = (0, 1, 1.0, 1, 2, 0, REPS, 0)
    assert np.all(_launch(Z, LAM, [], 4) == SENTINEL)
    assert np.all(_launch(Z, LAM, [(0, 1, 1.0, 1, 2, 0, 0, 0), (2, 3, 2.0, 3, 4, 5, 0, 1)], 4) == SENTINEL)
    for bad in ((0, P, 1.0, 1, 2, 0, 1, 3), (0, 1, 0.0, 1, 2, 0, 1, 3), (0, 1, 1.0, 1, 2, 2**32 - 1, 2, 3),
                (0, 1, 1.0, 1, 2, 0, -1, 3)):
        assert np.all(_launch(Z, LAM, [ok, bad], 4, expect=_lib.DCOR_EINVAL) == SENTINEL), bad
        assert "segment 1" in _lib.last_error()
    lam = LAM.copy()
    lam[3] = np.inf
    assert np.all(_launch(Z, lam, [ok], 4, expect=_lib.DCOR_EINVAL) == SENTINEL)
    assert "column 3" in _lib.last_error()


# ---------------------------------------------------------------- 5. Python surface
def test_corr_matrix_shapes_and_sweep_equals_eps_sweep():
    from dcor import hrs
    n = 1001
    Z, lam = _table(n)[:, :3], LAM[:3]
    res = hrs.corr_matrix(Z, lam, 1.0, 4)
    assert res["pairs"] == [(0, 1), (0, 2), (1, 2)] and res["runs"].shape == (3, 4, 6)
    for j, (a, b) in enumerate(res["pairs"]):
        for m, c in (("ni", 0), ("int", 3)):
            for i, key in enumerate(("rho_hat", "ci_low", "ci_high")):
                M = res[m][key]
                assert M.shape == (3, 3) and M[a, b] == M[b, a] == res["runs"][j][:, c + i].mean()
    for m in ("ni", "int"):
        for M in res[m].values():
            assert np.isnan(np.diag(M)).all() and np.array_equal(M, M.T, equal_nan=True)
            assert not np.isnan(M[~np.eye(3, dtype=bool)]).any()
    grid = (0.25, 1.05, 2.0)
    sw = hrs.corr_matrix_sweep(Z, lam, grid, 5, pairs=[(1, 2), (0, 1)])
    assert sw["runs"].shape == (2, 3, 5, 6) and len(sw["summaries"]) == 2 and sw["eps"] == list(grid)
    es = hrs.eps_sweep(np.ascontiguousarray(Z[:, 1]), np.ascontiguousarray(Z[:, 2]), lam[1], lam[2], grid, 5,
                       mode="fused")
    assert np.array_equal(_bits(sw["runs"][0]), _bits(es["runs"]))
    assert sw["summaries"][0]["int_mean"] == es["int_mean"] and sw["summaries"][0]["ni_mean"] == es["ni_mean"]


def test_standardize_table_equals_standardize_panel():
    from dcor import hrs
    age, bmi = hrs.standin_panel(2001, -0.3, seed=5)
    age[7], bmi[11] = np.nan, np.nan
    lap = np.array([0.3, -0.2, 0.1, 0.4])
    z = hrs.standardize_panel(age, bmi, lap=lap)
    t = hrs.standardize_table(np.stack([age, bmi], axis=1),
                              [(hrs.AGE_LO, hrs.AGE_HI), (hrs.BMI_LO, hrs.BMI_HI)], lap=lap)
    assert t["Z"].shape == (1999, 2) and t["Z"].flags.f_contiguous
    assert np.array_equal(_bits(t["Z"][:, 0]), _bits(z["age_z"])) and np.array_equal(_bits(t["Z"][:, 1]), _bits(z["bmi_z"]))
    assert t["lam"].tolist() == [z["lambda_age_z"], z["lambda_bmi_z"]]
    assert t["priv"] == [z["age_priv"], z["bmi_priv"]]


# ---------------------------------------------------------------- 6. allocations
def test_warm_second_call_allocates_nothing():
    from dcor import _lib, hrs
    Z = _table(1000)
    segs = [(0, 1, 2.0, 1, 2, 0, 6), (2, 3, 0.25, 3, 4, 2, 3)]
    first = hrs.table_segments(Z, LAM, segs)
    count = _lib.lib.dcor_alloc_count()
    second = hrs.table_segments(Z, LAM, segs)
    assert _lib.lib.dcor_alloc_count() == count
    assert np.array_equal(_bits(first), _bits(second))


# ---------------------------------------------------------------- 7. ranks
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def test_hrs_table_distributed_rccl_world1():
    import torch
    import torch.distributed as dist
    from dcor import hrs
    from dcor.dist import hrs_table_distributed
    Z = _table(1001)
    segs = [(0, 1, 1.0, 61, 71, 0, 7), (3, 1, 0.25, 62, 72, 1001, 3), (2, 2, 2.0, 63, 73, 5, 0),
            (1, 2, 2.45, 64, 74, 2, 4)]
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()))
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    try:
        got = hrs_table_distributed(Z, LAM, segs)
        empty = hrs_table_distributed(Z, LAM, [])
    finally:
        dist.destroy_process_group()
    want = hrs.table_segments(Z, LAM, segs)
    assert want.shape == (14, 6) and got.tobytes() == want.tobytes() and empty.shape == (0, 6)
