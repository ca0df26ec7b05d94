"""GPU tests of the sign-family panel path (dcor_sign_panel_launch, dcor.signpanel): against the
oracle on the restated draw contract, against the fused engine on its own DGP samples, the segment
semantics, the NaN / zero / boundary rules, and a cheap law check."""
import ctypes as C

import numpy as np
import pytest

import sign_panel_ref as R
from helpers import assert_close

pytestmark = pytest.mark.gpu


def _panel(n, seed=11, rho=0.5):
    g = np.random.default_rng(seed)
    xy = g.multivariate_normal([0.5, 0.5], [[4.0, 4.0 * rho], [4.0 * rho, 4.0]], size=n)
    return np.ascontiguousarray(xy[:, 0]), np.ascontiguousarray(xy[:, 1])


def _orc():
    import oracle.oracle as orc
    return orc


def _launch(Xd, Yd, segs, rows, sentinel=None, alpha=0.05, normalise=1, ci_mode=0, nsim=1000):
    """dcor_sign_panel_launch over device tensors; segs: (eps1, eps2, seed, rep_begin, reps, out_row).
    Returns (status, out [rows, 6])."""
    import torch
    from dcor import _lib
    out = torch.full((rows, 6), float("nan") if sentinel is None else sentinel, dtype=torch.float64, device="cuda")
    desc = _lib.SignPanelDesc(n=int(Xd.shape[0]), X=Xd.data_ptr(), Y=Yd.data_ptr(), alpha=alpha,
                              normalise=normalise, ci_mode=ci_mode, nsim=nsim)
    arr = (_lib.SignSegment * len(segs))(*[
        _lib.SignSegment(eps1=a, eps2=b, seed=s, rep_begin=rb, reps=c, out_row=row) for a, b, s, rb, c, row in segs])
    st = _lib.lib.dcor_sign_panel_launch(C.byref(desc), arr, len(segs), C.c_void_p(out.data_ptr()),
                                         C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return st, out.cpu().numpy()


def _dev(X, Y):
    import torch
    return (torch.as_tensor(X, dtype=torch.float64, device="cuda"),
            torch.as_tensor(Y, dtype=torch.float64, device="cuda"))


# ---------------------------------------------------------------- 1. against the oracle
# (n, eps1, eps2): the smallest shapes that reach each path -- k = 1 (n = 12), one partial flip
# block and a tail (37, 1001, 4099), m = 2 and m = 200 (k = 2, 5), m = 11 with either sender
ORACLE_SHAPES = [(12, 1.0, 1.0), (37, 1.0, 1.0), (1001, 1.0, 1.0), (4099, 1.0, 1.0), (1001, 2.0, 2.0),
                 (401, 0.2, 0.2), (1001, 0.2, 0.2), (1001, 1.5, 0.5), (1001, 0.5, 1.5)]


@pytest.mark.parametrize("n,eps1,eps2", ORACLE_SHAPES)
@pytest.mark.parametrize("normalise", [1, 0])
def test_matches_oracle_on_restated_streams(n, eps1, eps2, normalise):
    from dcor import signpanel
    orc = _orc()
    X, Y = _panel(n, seed=n)
    for rep_begin, reps, mode, nsim, seed in ((0, 5, "normal", 1000, 1_000_003), (1001, 6, "laplace", 1000, 77),
                                              (1001, 5, "normal", 2000, (5 << 32) + 9), (0, 5, "auto", 1000, 3)):
        got = signpanel.replicates(X, Y, eps1, eps2, reps, seed, rep_begin=rep_begin, normalise=bool(normalise),
                                   mode=mode, nsim=nsim)
        ref = R.oracle_records(orc, X, Y, eps1, eps2, seed, rep_begin, reps, normalise=bool(normalise),
                               mode={"auto": 0, "normal": 1, "laplace": 2}[mode], nsim=nsim)
        assert got.shape == (reps, 6)
        assert_close(got, ref, what=f"n={n} eps=({eps1},{eps2}) normalise={normalise} {mode} nsim={nsim}")
        if n == 12:   # k = 1: the NI CI is NA exactly where the oracle's is, the rest finite
            assert np.isnan(got[:, 1:3]).all() and not np.isnan(got[:, [0, 3, 4, 5]]).any()
            assert np.array_equal(np.isnan(got), np.isnan(ref))


def test_matches_oracle_large_panel():
    """n = 70,001: many trips of the sample loop per thread, three passes of the batch counters."""
    from dcor import signpanel
    X, Y = _panel(70_001, seed=5)
    got = signpanel.replicates(X, Y, 1.0, 1.0, 3, 42, rep_begin=7)
    ref = R.oracle_records(_orc(), X, Y, 1.0, 1.0, 42, 7, 3)
    assert_close(got, ref, what="n=70001")
    got = signpanel.replicates(X, Y, 2.0, 2.0, 2, 42)   # m = 2, k = 35,000: nine counter passes
    assert_close(got, R.oracle_records(_orc(), X, Y, 2.0, 2.0, 42, 0, 2), what="n=70001 m=2")


# ---------------------------------------------------------------- 2. against the fused engine
@pytest.mark.parametrize("n", [1000, 20_000])
def test_matches_fused_engine_on_its_own_samples(n):
    import torch
    from dcor import _lib
    from dcor.sim import CellSpec, simulate
    cell = CellSpec(n=n, rho=0.4, eps1=1.0, eps2=1.0, family="sign", dgp="bounded_factor", seed=1_000_123)
    c = cell.to_c()
    reps = [0, 1, 5, 1001]
    sim = {r: simulate(cell, 1, rep_begin=r).cpu().numpy()[0] for r in reps}
    Xd = torch.empty(n, dtype=torch.float64, device="cuda")
    Yd = torch.empty(n, dtype=torch.float64, device="cuda")
    sp = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for r in reps:
        _lib.check(_lib.lib.dcor_dgp_launch(C.byref(c), r, 1, C.c_void_p(Xd.data_ptr()), C.c_void_p(Yd.data_ptr()), sp))
        st, got = _launch(Xd, Yd, [(cell.eps1, cell.eps2, c.seed, r, 1, 0)], 1, alpha=c.alpha,
                          normalise=c.normalise, ci_mode=c.ci_mode, nsim=c.nsim)
        assert st == 0
        assert not np.isnan(got).any()
        assert_close(got[0], sim[r], what=f"n={n} rep={r}")


# ---------------------------------------------------------------- 3. segments
SEGS = [  # (eps1, eps2, seed, rep_begin, reps, out_row): mixed eps pairs, seeds, ranges, shuffled rows
    (1.0, 1.0, 11, 0, 7, 20), (0.2, 0.2, 12, 1001, 3, 0), (2.0, 2.0, 13, 5, 6, 30), (1.5, 0.5, 14, 0, 4, 5),
    (1.0, 1.0, 15, 3, 0, 99), (0.5, 1.5, 16, 2**32 - 6, 5, 12)]
ROWS = 40


def test_segments_equal_per_segment_calls_bitwise():
    X, Y = _panel(1001, seed=3)
    Xd, Yd = _dev(X, Y)
    sentinel = -7.25
    st, got = _launch(Xd, Yd, SEGS, ROWS, sentinel=sentinel)
    assert st == 0
    named = np.zeros(ROWS, dtype=bool)
    for a, b, s, rb, c, row in SEGS:
        if c == 0:
            continue
        st1, one = _launch(Xd, Yd, [(a, b, s, rb, c, 0)], c)
        assert st1 == 0
        assert np.array_equal(got[row:row + c], one, equal_nan=True), (a, b, s)
        assert not np.isnan(one[:, [0, 3, 4, 5]]).any()
        named[row:row + c] = True
    assert np.all(got[~named] == sentinel), "rows no segment names must keep the sentinel"
    # one range in two calls, and the same range as two segments of one call
    _, whole = _launch(Xd, Yd, [(1.0, 1.0, 11, 0, 7, 0)], 7)
    _, a = _launch(Xd, Yd, [(1.0, 1.0, 11, 0, 3, 0)], 3)
    _, b = _launch(Xd, Yd, [(1.0, 1.0, 11, 3, 4, 0)], 4)
    assert np.array_equal(np.concatenate([a, b]), whole)
    _, two = _launch(Xd, Yd, [(1.0, 1.0, 11, 3, 4, 3), (1.0, 1.0, 11, 0, 3, 0)], 7)
    assert np.array_equal(two, whole)


def test_invalid_last_segment_leaves_output_untouched():
    from dcor import _lib
    Xd, Yd = _dev(*_panel(1001, seed=3))
    for bad, code in (((0.0, 1.0, 1, 0, 2, 30), _lib.DCOR_EINVAL), ((0.05, 0.05, 1, 0, 2, 30), _lib.DCOR_EKLT1),
                      ((1.0, 1.0, 1, 2**32 - 1, 2, 30), _lib.DCOR_EINVAL)):
        st, got = _launch(Xd, Yd, SEGS[:4] + [bad], ROWS, sentinel=-7.25)
        assert st == code
        assert np.all(got == -7.25)


def test_python_sweep_surface():
    from dcor import signpanel
    X, Y = _panel(1001, seed=3)
    segs = [(1.0, 1.0, 11, 0, 7), (0.2, 0.2, 12, 1001, 3), (1.5, 0.5, 14, 0, 4)]
    runs = signpanel.sweep_segments(X, Y, segs)
    assert runs.shape == (14, 6)
    row = 0
    for e1, e2, seed, rb, c in segs:
        assert np.array_equal(runs[row:row + c], signpanel.replicates(X, Y, e1, e2, c, seed, rep_begin=rb))
        row += c
    sw = signpanel.eps_sweep(X, Y, (0.5, 1.0, 2.0), 6, seed=100)
    assert sw["runs"].shape == (3, 6, 6) and len(sw["ni_mean"]) == 3 and len(sw["int_mean"]) == 3
    assert np.array_equal(sw["runs"][1], signpanel.replicates(X, Y, 1.0, 1.0, 6, 102))
    assert sw["int_mean"][2]["rho_hat_mean"] == float(np.mean(sw["runs"][2][:, 3]))
    assert signpanel.sweep_segments(X, Y, []).shape == (0, 6)


# ---------------------------------------------------------------- 4. edge semantics
def test_raw_signs_of_exact_zeros():
    """normalise = 0 on a panel holding exact zeros (and -0.0): sign(0) = 0, as the oracle."""
    from dcor import signpanel
    X, Y = _panel(203, seed=8)
    X[::3] = 0.0
    Y[1::5] = 0.0
    Y[2::7] = -0.0
    got = signpanel.replicates(X, Y, 1.0, 1.0, 6, 21, normalise=False)
    assert_close(got, R.oracle_records(_orc(), X, Y, 1.0, 1.0, 21, 0, 6, normalise=False), what="zeros")
    assert not np.isnan(got).any()


def test_nan_rules():
    """n = 43 at eps = (1, 1): m = 8, k = 5, tail = samples 40..42.  normalise = 0: a NaN in the tail
    makes INT NaN and leaves NI finite (and equal to the clean panel's NI); a NaN in the first k m
    samples makes both NaN.  normalise = 1: the NaN reaches the means, so both are NaN wherever it
    lies (R's priv_standardize; dcor_premat_sign_launch likewise)."""
    from dcor import signpanel
    orc = _orc()
    X, Y = _panel(43, seed=9)
    clean = signpanel.replicates(X, Y, 1.0, 1.0, 4, 5, normalise=False)
    assert not np.isnan(clean).any()
    for col in (0, 1):
        for idx, ni_nan in ((41, False), (40, False), (39, True), (0, True), (17, True)):
            P = [X.copy(), Y.copy()]
            P[col][idx] = np.nan
            got = signpanel.replicates(P[0], P[1], 1.0, 1.0, 4, 5, normalise=False)
            ref = R.oracle_records(orc, P[0], P[1], 1.0, 1.0, 5, 0, 4, normalise=False)
            assert np.array_equal(np.isnan(got), np.isnan(ref)), (col, idx)
            assert np.isnan(got[:, 3:]).all(), (col, idx)
            assert np.isnan(got[:, :3]).all() == ni_nan and np.isnan(got[:, :3]).any() == ni_nan, (col, idx)
            if not ni_nan:
                assert np.array_equal(got[:, :3], clean[:, :3])
            got1 = signpanel.replicates(P[0], P[1], 1.0, 1.0, 2, 5, normalise=True)
            assert np.isnan(got1).all(), (col, idx)


@pytest.mark.parametrize("n,eps", [(1001, 1.0), (4099, 1.0), (1003, 2.0), (1001, 0.2), (39, 1.0)])
def test_flip_block_and_tail_boundaries(n, eps):
    """n neither a multiple of 4 (a partial last flip block) nor of m (a tail), explicitly: the
    record equals the oracle's, and differs from the record of the panel cut to k m samples only in
    its INT half when the tail is cut (the NI batches are the same samples)."""
    from dcor import signpanel
    k, m = R.geometry(n, eps, eps)
    assert n % 4 != 0 and n % m != 0 and k >= 1
    X, Y = _panel(n, seed=n + 1)
    got = signpanel.replicates(X, Y, eps, eps, 5, 31, normalise=False)
    assert_close(got, R.oracle_records(_orc(), X, Y, eps, eps, 31, 0, 5, normalise=False), what=f"n={n}")
    cut = signpanel.replicates(X[:k * m], Y[:k * m], eps, eps, 5, 31, normalise=False)
    assert_close(cut, R.oracle_records(_orc(), X[:k * m], Y[:k * m], eps, eps, 31, 0, 5, normalise=False),
                 what=f"n={k * m}")
    # with raw signs the NI half reads the first k m samples only: eta-hat is the same up to the
    # Laplace scale's n-free constants, so the two NI triples are bit-equal
    assert np.array_equal(got[:, :3], cut[:, :3])
    assert not np.array_equal(got[:, 3], cut[:, 3])


# ---------------------------------------------------------------- 5. law check
def test_law_agrees_with_oracle_replicates():
    """Mean NI and INT estimates over 10,000 engine replicates (keys and replicate indices disjoint
    from the oracle's) against 2,000 oracle replicates on the restated streams: Welch t inside the
    Bonferroni bound of tests/mc_stats.py for the two statistics tested."""
    import mc_stats as S
    from dcor import signpanel
    X, Y = R.law_panel()
    ref = R.oracle_records(_orc(), X, Y, 1.0, 1.0, 777, 0, 2000)
    assert not np.isnan(ref).any(), "the oracle side must be well-defined for this input"
    got = signpanel.replicates(X, Y, 1.0, 1.0, 10_000, 778, rep_begin=5000)
    assert not np.isnan(got).any()
    th = S.thresholds(2)
    for name, col in (("ni_hat", 0), ("int_hat", 3)):
        t = S.welch_t(got[:, col], ref[:, col])
        print(f"{name}: engine mean {got[:, col].mean():.6f} oracle mean {ref[:, col].mean():.6f} t {t:.3f} "
              f"(bound {th['z_max']:.3f})")
        assert t is not S.UNDEFINED and abs(t) < th["z_max"], (name, t)
