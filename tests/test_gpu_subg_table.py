"""GPU tests of the sub-G table path (dcor_subg_table_launch, dcor.subgpanel.table_segments /
corr_matrix / corr_matrix_sweep): byte equality with the panel entry on every pair's two columns,
one direct oracle comparison, the NaN rule per column, invalid and empty calls, the warm-call
scratch, the Python surface and the segment cursor."""
import ctypes as C
import functools

import numpy as np
import pytest

import subg_panel_ref as R
from helpers import assert_close
from test_gpu_subg_panel import _launch as _panel_launch
from test_gpu_subg_panel import _panel, _u64

pytestmark = pytest.mark.gpu

W_NMAX = 16384   # SUBG_W_NMAX (csrc/dcor_engine.h): up to this n a replicate is one wave
ETA = (1.0, 0.5, 0.8, 1.3)
P = 4


def _orc():
    import oracle.oracle as orc
    return orc


@functools.lru_cache(maxsize=None)
def _table(n):
    """p = 4 columns of test_gpu_subg_panel._panel's data, (n, 4) column-major; shared, never
    written (the tests that change a value copy it)."""
    a, b = _panel(n, seed=n)
    c, d = _panel(n, seed=n + 1, rho=0.2)
    return np.asfortranarray(np.stack([a, b, c, d], axis=1))


def _upload(D, ld):
    """The table on the device with `ld` elements between column starts (the gaps hold a value no
    column has), as a flat tensor."""
    import torch
    n, p = D.shape
    flat = np.full(p * ld, 1e300)
    for c in range(p):
        flat[c * ld:c * ld + n] = D[:, c]
    return torch.as_tensor(flat, device="cuda")


def _launch(Dd, n, ld, segs, rows, sentinel=None, eta=ETA, p=P, alpha=0.05, nsim=1000):
    """dcor_subg_table_launch over a device tensor; segs: (col_x, col_y, eps1, eps2, seed, rep_begin,
    reps, out_row).  Returns (status, out [rows, 6])."""
    import torch
    from dcor import _lib
    out = torch.full((rows, 6), float("nan") if sentinel is None else sentinel, dtype=torch.float64, device="cuda")
    eta_c = (C.c_double * len(eta))(*eta)
    desc = _lib.SubgTableDesc(n=n, p=p, ld=ld, D=Dd.data_ptr(), eta=eta_c, alpha=alpha, nsim=nsim)
    arr = (_lib.SubgPairSegment * len(segs))(*[
        _lib.SubgPairSegment(col_x=a, col_y=b, eps1=e1, eps2=e2, seed=s, rep_begin=rb, reps=c, out_row=row)
        for a, b, e1, e2, s, rb, c, row in segs])
    st = _lib.lib.dcor_subg_table_launch(C.byref(desc), arr, len(segs), C.c_void_p(out.data_ptr()),
                                         C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return st, out.cpu().numpy()


def _panel_rows(D, a, b, e1, e2, seed, rb, c, eta=ETA, nsim=1000):
    """The segment's reference call: dcor_subg_panel_launch on the two contiguous columns."""
    import torch
    Xd = torch.as_tensor(np.ascontiguousarray(D[:, a]), device="cuda")
    Yd = torch.as_tensor(np.ascontiguousarray(D[:, b]), device="cuda")
    st, one = _panel_launch(Xd, Yd, [(e1, e2, seed, rb, c, 0)], c, eta1=eta[a], eta2=eta[b], nsim=nsim)
    assert st == 0
    return one


# ---------------------------------------------------------------- 1. byte equality with the panel entry
# (col_x, col_y, eps1, eps2, seed, rep_begin, reps, out_row): m = 8 shared by (0,1) and (1,0), m = 11
# with either sender, 64-bit seeds, rep_begin = 2^32 - 6, a zero-rep segment, shuffled rows
SEGS = [(0, 1, 1.0, 1.0, (7 << 32) + 11, 0, 3, 12), (1, 0, 2.0, 0.5, (9 << 32) + 1, 2, 2, 0),
        (2, 2, 0.2, 0.2, 12, 1001, 3, 20), (3, 1, 0.5, 1.5, (5 << 32) + 16, 2**32 - 6, 5, 4),
        (1, 3, 1.0, 1.0, 15, 3, 0, 99), (0, 3, 1.5, 0.5, 14, 0, 4, 15)]
ROWS = 26


@pytest.mark.parametrize("n", [5, 12, 37, 1001, W_NMAX, W_NMAX + 1])
def test_segments_equal_the_panel_entry_bytewise(n):
    """m > n (5), k = 1 (12), a tail (37), an odd n whose last pair reads the zero padding, both
    sides of the wave / workgroup switch; ld = n + 1 (for even n columns 1 and 3 start only 8-byte
    aligned) and ld = n."""
    D = _table(n)
    Dd = _upload(D, n + 1)
    sentinel = -7.25
    segs = SEGS if n <= 1001 else [s[:6] + (min(s[6], 2),) + s[7:] for s in SEGS]
    st, got = _launch(Dd, n, n + 1, segs, ROWS, sentinel=sentinel)
    assert st == 0
    named = np.zeros(ROWS, dtype=bool)
    for a, b, e1, e2, seed, rb, c, row in segs:
        if c == 0:
            continue
        assert not named[row:row + c].any()
        named[row:row + c] = True
        one = _panel_rows(D, a, b, e1, e2, seed, rb, c)
        assert np.array_equal(_u64(got[row:row + c]), _u64(one)), (a, b, e1, e2)
        # the segment split into two calls by rep_begin
        h = c // 2
        _, x = _launch(Dd, n, n + 1, [(a, b, e1, e2, seed, rb, h, 0)], max(h, 1))
        _, y = _launch(Dd, n, n + 1, [(a, b, e1, e2, seed, rb + h, c - h, 0)], c - h)
        assert np.array_equal(_u64(np.concatenate([x[:h], y])), _u64(one)), (a, b, "split")
    assert named.sum() == sum(s[6] for s in segs)
    assert np.all(got[~named] == sentinel)   # rows no segment names keep the sentinel
    st, rev = _launch(Dd, n, n + 1, segs[::-1], ROWS, sentinel=sentinel)
    assert st == 0 and np.array_equal(_u64(rev), _u64(got))
    st, tight = _launch(_upload(D, n), n, n, segs, ROWS, sentinel=sentinel)
    assert st == 0 and np.array_equal(_u64(tight), _u64(got))


# ---------------------------------------------------------------- 2. against the oracle
def test_matches_oracle_directly():
    n = 1001
    D = _table(n)
    segs = [(3, 1, 0.5, 1.5, (5 << 32) + 16, 1001, 3, 0), (2, 2, 1.0, 1.0, 77, 0, 3, 3)]
    st, got = _launch(_upload(D, n + 1), n, n + 1, segs, 6)
    assert st == 0
    for a, b, e1, e2, seed, rb, c, row in segs:
        ref = R.oracle_records(_orc(), D[:, a], D[:, b], e1, e2, seed, rb, c, eta1=ETA[a], eta2=ETA[b])
        assert_close(got[row:row + c], ref, what=f"pair ({a},{b}) eps=({e1},{e2})")
        assert np.array_equal(np.isnan(got[row:row + c]), np.isnan(ref))
        assert np.array_equal(np.isinf(got[row:row + c]), np.isinf(ref))
        assert not np.isnan(ref).any()


# ---------------------------------------------------------------- 3. NaN
def test_nan_reaches_only_the_pairs_that_name_the_column():
    n = 1003
    k, m = R.geometry(n, 1.0, 1.0)
    assert k * m < n   # a tail
    D0 = _table(n)
    segs = [(0, 1, 1.0, 1.0, 5, 0, 2, 0), (1, 0, 1.0, 1.0, 5, 0, 2, 2), (0, 2, 1.0, 1.0, 6, 0, 2, 4),
            (1, 1, 1.0, 1.0, 7, 0, 2, 6), (3, 1, 1.0, 1.0, 8, 0, 2, 8)]
    st, clean = _launch(_upload(D0, n + 1), n, n + 1, segs, 10)
    assert st == 0 and not np.isnan(clean).any()
    for idx, ni_nan in ((k * m - 1, True), (n - 1, False), (0, True)):
        D = D0.copy()
        D[idx, 1] = np.nan
        st, got = _launch(_upload(D, n + 1), n, n + 1, segs, 10)
        assert st == 0
        for a, b, e1, e2, seed, rb, c, row in segs:
            rows = got[row:row + c]
            if 1 not in (a, b):   # (0, 2): untouched by column 1's NaN
                assert np.array_equal(_u64(rows), _u64(clean[row:row + c])), idx
                continue
            assert np.isnan(rows[:, 3:6]).all(), (a, b, idx)
            assert np.isnan(rows[:, 0:3]).all() == ni_nan and np.isnan(rows[:, 0:3]).any() == ni_nan, (a, b, idx)
            one = _panel_rows(D, a, b, e1, e2, seed, rb, c)   # the panel entry's rule, and its bits elsewhere
            assert np.array_equal(np.isnan(rows), np.isnan(one)), (a, b, idx)
            keep = ~np.isnan(one)
            assert np.array_equal(_u64(rows[keep]), _u64(one[keep])), (a, b, idx)


# ---------------------------------------------------------------- 4, 5. invalid and empty calls
def test_invalid_and_empty_calls_leave_output_untouched():
    from dcor import _lib
    n = 100
    Dd = _upload(_table(n), n + 1)
    good = (0, 1, 1.0, 1.0, 1, 0, 2, 0)
    nan, inf = float("nan"), float("inf")
    for segs, kw in (([good, (0, 4, 1.0, 1.0, 1, 0, 2, 2)], {}), ([good, (-1, 1, 1.0, 1.0, 1, 0, 2, 2)], {}),
                     ([good], dict(eta=(1.0, nan, 0.8, 1.3))), ([good], dict(ld=n - 1)),
                     ([good, (0, 1, 1.0, inf, 1, 0, 2, 2)], {}), ([good, (0, 1, 1.0, 1.0, 1, 0, 2, -1)], {}),
                     ([good, (0, 1, 1.0, 1.0, 1, 2**32 - 2, 4, 2)], {}), ([good], dict(nsim=2049))):
        kw = {"ld": n + 1, **kw}
        st, out = _launch(Dd, n, kw.pop("ld"), segs, 6, sentinel=-3.5, **kw)
        assert st == _lib.DCOR_EINVAL, (segs, kw)
        if "nsim" not in kw:   # alpha and nsim are refused by the shared checks, which name no entry
            assert "subg_table" in _lib.last_error()
        assert np.all(out == -3.5), (segs, kw)
    # every segment without replicates: DCOR_OK, nothing written
    st, out = _launch(Dd, n, n + 1, [(0, 1, 1.0, 1.0, 1, 0, 0, 0), (2, 3, 0.5, 1.5, 2, 7, 0, 1)], 2, sentinel=-3.5)
    assert st == 0 and np.all(out == -3.5)


# ---------------------------------------------------------------- 6. scratch
def test_warm_second_call_adds_no_device_bytes():
    from dcor import _lib
    n = 5000
    Dd = _upload(_table(n), n + 1)
    segs = [(0, 1, 1.0, 1.0, 1, 0, 40, 0), (2, 3, 0.5, 0.5, 2, 0, 40, 40), (1, 1, 1.5, 0.5, 3, 0, 8, 80)]
    st, a = _launch(Dd, n, n + 1, segs, 88)
    assert st == 0
    bytes0, allocs0 = _lib.lib.dcor_device_bytes(), _lib.lib.dcor_alloc_count()
    st, b = _launch(Dd, n, n + 1, segs, 88)
    assert st == 0 and np.array_equal(_u64(a), _u64(b))
    assert _lib.lib.dcor_device_bytes() == bytes0 and _lib.lib.dcor_alloc_count() == allocs0


# ---------------------------------------------------------------- 7. the Python surface
def test_python_surface():
    from dcor import subgpanel
    n = 501
    D = np.array(_table(n))
    eta = np.array(ETA)
    segs = [(0, 1, 1.0, 1.0, 31, 0, 3), (3, 1, 0.5, 1.5, 32, 4, 2), (2, 2, 2.0, 0.5, 33, 0, 2)]
    got = subgpanel.table_segments(D, segs, eta=eta)
    assert got.shape == (7, 6)
    row = 0
    for a, b, e1, e2, seed, rb, c in segs:
        one = subgpanel.replicates(D[:, a], D[:, b], e1, e2, c, seed, rep_begin=rb, eta1=eta[a], eta2=eta[b])
        assert np.array_equal(_u64(got[row:row + c]), _u64(one)), (a, b)
        row += c
    # a row-major table is the same table
    assert np.array_equal(_u64(subgpanel.table_segments(np.ascontiguousarray(D), segs, eta=eta)), _u64(got))
    # a scalar eta is the vector of that scalar
    assert np.array_equal(_u64(subgpanel.table_segments(D, segs, eta=0.7)),
                          _u64(subgpanel.table_segments(D, segs, eta=[0.7] * P)))
    # corr_matrix: shapes, symmetry, NaN diagonal, keys seed + j + 1
    cm = subgpanel.corr_matrix(D, 1.5, 0.5, 3, seed=900, eta=eta)
    pairs = subgpanel.all_pairs(P)
    assert cm["pairs"] == pairs and cm["runs"].shape == (6, 3, 6)
    for meth in ("ni", "int"):
        for key in ("rho_hat", "ci_low", "ci_high"):
            M = cm[meth][key]
            assert M.shape == (P, P) and np.isnan(np.diag(M)).all()
            off = ~np.eye(P, dtype=bool)
            assert np.array_equal(M[off], M.T[off]) and not np.isnan(M[off]).any()
    for j, (a, b) in enumerate(pairs):
        one = subgpanel.replicates(D[:, a], D[:, b], 1.5, 0.5, 3, 900 + j + 1, eta1=eta[a], eta2=eta[b])
        assert np.array_equal(_u64(cm["runs"][j]), _u64(one)), (a, b)
        assert cm["int"]["rho_hat"][a, b] == one[:, 3].mean()
    cm = subgpanel.corr_matrix(D, 1.0, 1.0, 2, pairs=[(1, 1), (3, 0)], eta=eta)
    assert not np.isnan(cm["ni"]["rho_hat"][1, 1]) and np.isnan(cm["ni"]["rho_hat"][0, 0])
    assert cm["ni"]["rho_hat"][0, 3] == cm["ni"]["rho_hat"][3, 0] == cm["runs"][1][:, 0].mean()
    # corr_matrix_sweep: pair j equals eps_sweep on its columns under seed + j len(eps_grid)
    grid = [0.5, (1.5, 0.5), 2.0]
    sw = subgpanel.corr_matrix_sweep(D, grid, 2, seed=5000, pairs=[(0, 1), (2, 1), (3, 3)], eta=eta)
    assert sw["runs"].shape == (3, 3, 2, 6) and sw["eps"] == grid and len(sw["summaries"]) == 3
    for j, (a, b) in enumerate(sw["pairs"]):
        one = subgpanel.eps_sweep(D[:, a], D[:, b], grid, 2, seed=5000 + j * len(grid), eta1=eta[a], eta2=eta[b])
        assert np.array_equal(_u64(sw["runs"][j]), _u64(one["runs"])), (a, b)
        assert np.array_equal(sw["summaries"][j]["int_mean"], one["int_mean"])


# ---------------------------------------------------------------- 8. the cursor
def _cursor_segments(nseg, seed):
    g = np.random.default_rng(seed)
    eps = [(1.0, 1.0), (2.0, 0.5), (0.2, 0.2), (0.5, 1.5), (1.5, 0.5), (2.0, 2.0)]
    segs, row = [], 0
    for j in range(nseg):
        a, b = (int(v) for v in g.integers(0, P, 2))
        e1, e2 = eps[int(g.integers(0, len(eps)))]
        c = int(g.integers(0, 4))
        segs.append((a, b, e1, e2, 1000 + j, int(g.integers(0, 50)), c, row))
        row += c
    return segs, row


def test_many_short_segments_equal_per_segment_calls():
    """200 segments of 0 - 3 replicates at n = 37 against one call per segment, bit for bit."""
    n = 37
    Dd = _upload(_table(n), n + 1)
    segs, rows = _cursor_segments(200, seed=1)
    st, got = _launch(Dd, n, n + 1, segs, rows)
    assert st == 0
    for s in segs:
        if s[6] == 0:
            continue
        st, one = _launch(Dd, n, n + 1, [s[:7] + (0,)], s[6])
        assert st == 0
        assert np.array_equal(_u64(got[s[7]:s[7] + s[6]]), _u64(one)), s


def test_cursor_advances_through_segments_within_a_unit():
    """6,000 segments of 0 - 3 replicates at n = 37: about 9,000 items, more than one pass of the
    wave form's units on a 256-CU device (3 workgroups of 4 waves per CU: 3,072), so a unit's later
    items lie many segments on.  Against the panel entry, one call per pair holding that pair's
    segments, bit for bit."""
    import torch
    n = 37
    D = _table(n)
    segs, rows = _cursor_segments(6000, seed=2)
    assert rows > 2 * 3072
    st, got = _launch(_upload(D, n + 1), n, n + 1, segs, rows)
    assert st == 0
    for a in range(P):
        for b in range(P):
            mine = [s for s in segs if (s[0], s[1]) == (a, b)]
            Xd = torch.as_tensor(np.ascontiguousarray(D[:, a]), device="cuda")
            Yd = torch.as_tensor(np.ascontiguousarray(D[:, b]), device="cuda")
            st, ref = _panel_launch(Xd, Yd, [s[2:] for s in mine], rows, eta1=ETA[a], eta2=ETA[b])
            assert st == 0
            for s in mine:
                sl = slice(s[7], s[7] + s[6])
                assert np.array_equal(_u64(got[sl]), _u64(ref[sl])), s
