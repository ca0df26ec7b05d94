"""GPU tests of the sub-G panel path (dcor_subg_panel_launch, dcor.subgpanel): against the oracle
on the restated draw contract, against the fused engine on its own DGP samples, the segment
semantics, the NaN rule, invalid calls, the warm-call scratch and a cheap law check."""
import ctypes as C

import numpy as np
import pytest

import subg_panel_ref as R
from helpers import assert_close

pytestmark = pytest.mark.gpu

W_NMAX = 16384   # SUBG_W_NMAX (csrc/dcor_engine.h): up to this n a replicate is one wave


def _panel(n, seed=11, rho=0.5):
    """N(0.5, 2^2) pairs, as tests/test_gpu_sign_panel.py's: both clips bind."""
    g = np.random.default_rng(seed)
    xy = g.multivariate_normal([0.5, 0.5], [[4.0, 4.0 * rho], [4.0 * rho, 4.0]], size=n)
    return np.ascontiguousarray(xy[:, 0]), np.ascontiguousarray(xy[:, 1])


def _orc():
    import oracle.oracle as orc
    return orc


def _launch(Xd, Yd, segs, rows, sentinel=None, eta1=1.0, eta2=1.0, alpha=0.05, nsim=1000, n=None):
    """dcor_subg_panel_launch over device tensors; segs: (eps1, eps2, seed, rep_begin, reps, out_row).
    Returns (status, out [rows, 6])."""
    import torch
    from dcor import _lib
    out = torch.full((rows, 6), float("nan") if sentinel is None else sentinel, dtype=torch.float64, device="cuda")
    desc = _lib.SubgPanelDesc(n=int(Xd.shape[0]) if n is None else n, X=Xd.data_ptr(), Y=Yd.data_ptr(),
                              eta1=eta1, eta2=eta2, alpha=alpha, nsim=nsim)
    arr = (_lib.SubgSegment * len(segs))(*[
        _lib.SubgSegment(eps1=a, eps2=b, seed=s, rep_begin=rb, reps=c, out_row=row) for a, b, s, rb, c, row in segs])
    st = _lib.lib.dcor_subg_panel_launch(C.byref(desc), arr, len(segs), C.c_void_p(out.data_ptr()),
                                         C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return st, out.cpu().numpy()


def _dev(X, Y):
    import torch
    return (torch.as_tensor(X, dtype=torch.float64, device="cuda"),
            torch.as_tensor(Y, dtype=torch.float64, device="cuda"))


def _u64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ---------------------------------------------------------------- 1. against the oracle
# (n, eps1, eps2): m > n (5), k = 1 (12), a tail of 5 (37), odd and even n, m = 2, m = 200 (k = 2,
# 5), m = 11 with either sender, and either side of the wave / workgroup threshold
ORACLE_SHAPES = [(5, 1.0, 1.0), (12, 1.0, 1.0), (37, 1.0, 1.0), (1001, 1.0, 1.0), (4099, 1.0, 1.0),
                 (1001, 2.0, 2.0), (401, 0.2, 0.2), (1001, 0.2, 0.2), (1001, 1.5, 0.5), (1001, 0.5, 1.5),
                 (W_NMAX, 1.0, 1.0), (W_NMAX + 1, 1.0, 1.0)]
# (rep_begin, reps, nsim, seed, eta1, eta2)
ORACLE_RUNS = [(0, 3, 1000, 1_000_003, 1.0, 1.0), (1001, 3, 2000, (5 << 32) + 9, 0.5, 0.8),
               (1001, 2, 1000, 77, 0.5, 0.8)]


@pytest.mark.parametrize("n,eps1,eps2", ORACLE_SHAPES)
def test_matches_oracle_on_restated_streams(n, eps1, eps2):
    from dcor import subgpanel
    orc = _orc()
    X, Y = _panel(n, seed=n)
    for rep_begin, reps, nsim, seed, eta1, eta2 in ORACLE_RUNS:
        got = subgpanel.replicates(X, Y, eps1, eps2, reps, seed, rep_begin=rep_begin, eta1=eta1, eta2=eta2, nsim=nsim)
        ref = R.oracle_records(orc, X, Y, eps1, eps2, seed, rep_begin, reps, eta1=eta1, eta2=eta2, nsim=nsim)
        assert got.shape == (reps, 6)
        assert_close(got, ref, what=f"n={n} eps=({eps1},{eps2}) eta=({eta1},{eta2}) nsim={nsim}")
        assert np.array_equal(np.isnan(got), np.isnan(ref))
        if R.geometry(n, eps1, eps2)[0] == 1:   # k = 1: the NI CI is NA exactly where the oracle's is
            assert np.isnan(got[:, 1:3]).all() and not np.isnan(got[:, [0, 3, 4, 5]]).any()
        else:
            assert not np.isnan(got).any()


def test_matches_oracle_large_panel():
    """n = 70,001: a workgroup per replicate, many trips of both loops per thread."""
    from dcor import subgpanel
    X, Y = _panel(70_001, seed=5)
    got = subgpanel.replicates(X, Y, 1.0, 1.0, 3, 42, rep_begin=7)
    assert_close(got, R.oracle_records(_orc(), X, Y, 1.0, 1.0, 42, 7, 3), what="n=70001")
    got = subgpanel.replicates(X, Y, 0.5, 1.5, 2, 42, eta1=0.5, eta2=0.8)
    assert_close(got, R.oracle_records(_orc(), X, Y, 0.5, 1.5, 42, 0, 2, eta1=0.5, eta2=0.8), what="n=70001 m=11")


def test_zero_column_matches_oracle():
    """Y all zero: sd(Uc) = 0, c* infinite -- the oracle's NaN and infinity pattern."""
    from dcor import subgpanel
    X, _ = _panel(1001, seed=9)
    Y = np.zeros_like(X)
    for e1, e2 in ((1.0, 1.0), (0.5, 1.5)):
        got = subgpanel.replicates(X, Y, e1, e2, 4, 31)
        ref = R.oracle_records(_orc(), X, Y, e1, e2, 31, 0, 4)
        assert np.array_equal(np.isnan(got), np.isnan(ref)) and np.array_equal(np.isinf(got), np.isinf(ref))
        assert_close(got, ref, what=f"zero Y eps=({e1},{e2})")


# ---------------------------------------------------------------- 2. against the fused engine
@pytest.mark.parametrize("dgp", ["bounded_factor", "gaussian"])
@pytest.mark.parametrize("n", [1000, 20_000])
def test_matches_fused_engine_on_its_own_samples(n, dgp):
    import torch
    from dcor import _lib
    from dcor.sim import CellSpec, simulate
    cell = CellSpec(n=n, rho=0.4, eps1=1.5, eps2=0.5, family="subG", dgp=dgp, seed=1_000_123)
    c = cell.to_c()
    reps = [0, 1, 5, 1001]
    sim = {r: simulate(cell, 1, rep_begin=r).cpu().numpy()[0] for r in reps}
    Xd = torch.empty(n, dtype=torch.float64, device="cuda")
    Yd = torch.empty(n, dtype=torch.float64, device="cuda")
    sp = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for r in reps:
        _lib.check(_lib.lib.dcor_dgp_launch(C.byref(c), r, 1, C.c_void_p(Xd.data_ptr()), C.c_void_p(Yd.data_ptr()), sp))
        st, got = _launch(Xd, Yd, [(cell.eps1, cell.eps2, c.seed, r, 1, 0)], 1, eta1=c.eta1, eta2=c.eta2,
                          alpha=c.alpha, nsim=c.nsim)
        assert st == 0
        assert not np.isnan(got).any()
        assert_close(got[0], sim[r], what=f"{dgp} n={n} rep={r}")


# ---------------------------------------------------------------- 3. segments
SEGS = [  # (eps1, eps2, seed, rep_begin, reps, out_row): mixed eps pairs, seeds, ranges, shuffled rows
    (1.0, 1.0, 11, 0, 7, 20), (0.2, 0.2, 12, 1001, 3, 0), (2.0, 2.0, 13, 5, 6, 30), (1.5, 0.5, 14, 0, 4, 5),
    (1.0, 1.0, 15, 3, 0, 99), (0.5, 1.5, 16, 2**32 - 6, 5, 12), (2.0, 0.5, (9 << 32) + 1, 2, 2, 36)]
ROWS = 40


@pytest.mark.parametrize("n", [1001, W_NMAX + 3])
def test_segments_equal_per_segment_calls_bitwise(n):
    X, Y = _panel(n, seed=3)
    Xd, Yd = _dev(X, Y)
    sentinel = -7.25
    segs = SEGS if n == 1001 else [s[:4] + (min(s[4], 2),) + s[5:] for s in SEGS]
    st, got = _launch(Xd, Yd, segs, ROWS, sentinel=sentinel, eta1=0.5, eta2=0.8)
    assert st == 0
    named = np.zeros(ROWS, dtype=bool)
    for e1, e2, seed, rb, c, row in segs:
        if c == 0:
            continue
        assert not named[row:row + c].any()
        named[row:row + c] = True
        st1, one = _launch(Xd, Yd, [(e1, e2, seed, rb, c, 0)], c, eta1=0.5, eta2=0.8)
        assert st1 == 0
        assert np.array_equal(_u64(got[row:row + c]), _u64(one)), (e1, e2, seed)
        # the segment split into two calls
        h = c // 2
        _, a = _launch(Xd, Yd, [(e1, e2, seed, rb, h, 0)], max(h, 1), eta1=0.5, eta2=0.8)
        _, b = _launch(Xd, Yd, [(e1, e2, seed, rb + h, c - h, 0)], c - h, eta1=0.5, eta2=0.8)
        assert np.array_equal(_u64(np.concatenate([a[:h], b])), _u64(one)), (e1, e2, seed, "split")
    assert np.all(got[~named] == sentinel)   # rows no segment names keep the sentinel
    st, rev = _launch(Xd, Yd, segs[::-1], ROWS, sentinel=sentinel, eta1=0.5, eta2=0.8)
    assert st == 0 and np.array_equal(_u64(rev), _u64(got))


def test_segments_sharing_a_batch_size_bitwise():
    """(1, 1) and (2, 0.5) both have m = 8 and share one means array; their eps-dependent constants
    differ.  Both equal their single calls."""
    X, Y = _panel(1001, seed=4)
    Xd, Yd = _dev(X, Y)
    segs = [(1.0, 1.0, 21, 0, 3, 0), (2.0, 0.5, 21, 0, 3, 3), (1.0, 1.0, 22, 4, 2, 6)]
    st, got = _launch(Xd, Yd, segs, 8)
    assert st == 0
    for e1, e2, seed, rb, c, row in segs:
        _, one = _launch(Xd, Yd, [(e1, e2, seed, rb, c, 0)], c)
        assert np.array_equal(_u64(got[row:row + c]), _u64(one))
    assert not np.array_equal(_u64(got[0:3]), _u64(got[3:6]))
    assert_close(got[3:6], R.oracle_records(_orc(), X, Y, 2.0, 0.5, 21, 0, 3), what="(2, .5)")


# ---------------------------------------------------------------- 4. NaN
def _premat_nan_mask(X, Y, eps1, eps2, reps, nsim=1000):
    """The NaN mask of dcor_premat_subg_launch (hrs = 0) on the shared panel with arbitrary noise."""
    import torch
    from dcor import _lib
    n = len(X)
    k, _ = R.geometry(n, eps1, eps2)
    g = torch.Generator(device="cuda").manual_seed(5)
    rnd = lambda *s: torch.rand(*s, dtype=torch.float64, device="cuda", generator=g) - 0.5
    Xd, Yd = _dev(X, Y)
    bufs = dict(lap_ni_x=rnd(reps, k), lap_ni_y=rnd(reps, k), lap_local=rnd(reps, n), lap_central=rnd(reps),
                mix_z=rnd(reps, nsim), mix_l=rnd(reps, nsim))
    nan = float("nan")
    d = _lib.PrematSubg(n=n, reps=reps, eps1=eps1, eps2=eps2, eta1=1.0, eta2=1.0, alpha=0.05, hrs=0,
                        lam_x=nan, lam_y=nan, lam_s=nan, lam_o=nan, lam_r=nan, delta=nan, nsim=nsim,
                        X=Xd.data_ptr(), Y=Yd.data_ptr(), xy_stride=0, perm=None,
                        **{k_: v.data_ptr() for k_, v in bufs.items()})
    out = torch.zeros((reps, 6), dtype=torch.float64, device="cuda")
    _lib.check(_lib.lib.dcor_premat_subg_launch(C.byref(d), C.c_void_p(out.data_ptr()),
                                                C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    return np.isnan(out.cpu().numpy())


@pytest.mark.parametrize("n", [1003, W_NMAX + 5])
def test_nan_rule(n):
    from dcor import subgpanel
    k, m = R.geometry(n, 1.0, 1.0)
    assert k * m < n   # a tail
    X0, Y0 = _panel(n, seed=8)
    for col in (0, 1):
        for idx, ni_nan in ((k * m - 1, True), (n - 1, False), (0, True)):
            X, Y = X0.copy(), Y0.copy()
            (X if col == 0 else Y)[idx] = np.nan
            got = subgpanel.replicates(X, Y, 1.0, 1.0, 2, 5)
            assert np.isnan(got[:, 3:6]).all(), (col, idx)
            assert np.isnan(got[:, 0:3]).all() == ni_nan and np.isnan(got[:, 0:3]).any() == ni_nan, (col, idx)
            assert np.array_equal(np.isnan(got), _premat_nan_mask(X, Y, 1.0, 1.0, 2)), (col, idx)
    got = subgpanel.replicates(X0, Y0, 1.0, 1.0, 2, 5)
    assert not np.isnan(got).any()


# ---------------------------------------------------------------- 5. invalid calls on the device
def test_invalid_calls_leave_output_untouched():
    from dcor import _lib
    X, Y = _panel(100, seed=2)
    Xd, Yd = _dev(X, Y)
    good = (1.0, 1.0, 1, 0, 2, 0)
    for segs, kw in (([good, (0.0, 1.0, 1, 0, 2, 2)], {}), ([good, (1.0, float("inf"), 1, 0, 2, 2)], {}),
                     ([good, (1.0, 1.0, 1, -1, 2, 2)], {}), ([good, (1.0, 1.0, 1, 2**32 - 2, 4, 2)], {}),
                     ([good, (1.0, 1.0, 1, 0, 2, -1)], {}), ([good], dict(nsim=2049)), ([good], dict(alpha=2.0)),
                     ([good], dict(eta1=0.0)), ([good], dict(eta2=float("nan"))), ([good], dict(n=0))):
        st, out = _launch(Xd, Yd, segs, 6, sentinel=-3.5, **kw)
        assert st == _lib.DCOR_EINVAL, (segs, kw)
        assert np.all(out == -3.5), (segs, kw)
    st, out = _launch(Xd, Yd, [(1.0, 1.0, 1, 0, 0, 0)], 2, sentinel=-3.5)
    assert st == 0 and np.all(out == -3.5)


# ---------------------------------------------------------------- 6. scratch
def test_warm_second_call_adds_no_device_bytes():
    from dcor import _lib
    X, Y = _panel(5000, seed=2)
    Xd, Yd = _dev(X, Y)
    segs = [(1.0, 1.0, 1, 0, 40, 0), (0.5, 0.5, 2, 0, 40, 40)]
    st, a = _launch(Xd, Yd, segs, 80)
    assert st == 0
    bytes0, allocs0 = _lib.lib.dcor_device_bytes(), _lib.lib.dcor_alloc_count()
    st, b = _launch(Xd, Yd, segs, 80)
    assert st == 0 and np.array_equal(_u64(a), _u64(b))
    assert _lib.lib.dcor_device_bytes() == bytes0 and _lib.lib.dcor_alloc_count() == allocs0


# ---------------------------------------------------------------- 7. law
def test_law_matches_restatement():
    """n = 256, eps = (1, 1): 4,096 GPU replicates against 2,000 replicates of the numpy restatement
    under an unrelated seed; Welch tests on mean ni_hat, mean int_hat and the mean INT width, each
    |t| < 5 (false-alarm rate below 2e-6 for the three together).  tests/test_subg_panel_abi.py
    shows that a restatement with the local noise scale halved fails the same test."""
    from dcor import subgpanel
    X, Y = R.law_panel()
    got = subgpanel.replicates(X, Y, 1.0, 1.0, 4096, 20_261_020)
    ref = R.oracle_records(_orc(), X, Y, 1.0, 1.0, 777, 0, 2000)
    assert not np.isnan(got).any() and not np.isnan(ref).any()
    ts = [R.welch_t(u, v) for u, v in zip(R.law_stats(got), R.law_stats(ref))]
    print("welch t (ni_hat, int_hat, int width):", ts)
    assert all(abs(t) < 5.0 for t in ts), ts


def test_eps_sweep_surface():
    """eps_sweep takes scalars and pairs, keys seed + idx, and equals sweep_segments' rows."""
    from dcor import subgpanel
    X, Y = _panel(501, seed=6)
    grid = [0.5, (1.5, 0.5), 2.0]
    sw = subgpanel.eps_sweep(X, Y, grid, 3, seed=900)
    assert sw["runs"].shape == (3, 3, 6) and len(sw["ni_mean"]) == 3 and len(sw["int_mean"]) == 3
    for idx, (e1, e2) in enumerate([(0.5, 0.5), (1.5, 0.5), (2.0, 2.0)], start=1):
        one = subgpanel.replicates(X, Y, e1, e2, 3, 900 + idx)
        assert np.array_equal(_u64(sw["runs"][idx - 1]), _u64(one))
