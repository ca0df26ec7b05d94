"""GPU tests of the pairwise-complete HRS table path (dcor_hrs_table_pairwise_launch,
dcor.hrs.pairwise_segments / corr_matrix_pairwise / corr_matrix_sweep_pairwise,
dcor.dist.hrs_table_pairwise_distributed).  The yardsticks are the panel entry
(dcor.hrs.hrs_replicates(mode='fused')) on the pair's host-compacted columns, compared as uint64,
the present table entry on full masks, and the oracle's estimators on its own restatement of the
Philox streams -- never the pairwise path itself."""
import ctypes as C
import os
import socket

import numpy as np
import pytest

from helpers import assert_close

pytestmark = pytest.mark.gpu

N, P = 1001, 4
LAM = np.array([2.2, 2.6, 1.9, 2.4])      # distinct per column; each clips some of its column
PAIRS = [(0, 1), (1, 0), (2, 3), (1, 2), (1, 1)]
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
    return np.asfortranarray(np.stack([x, y, T[:, 2], T[:, 3]], axis=1))


def _present(n=N):
    """bool [P, n]: column 0 complete; column 1 about 20 % missing at random; column 2 missing rows
    60..70, the whole word 128..191 and 250..260; column 3 missing rows 0 and 1000 and every third
    row -- and row 1: with the masks as first written every pair's count was even (806, 608, 730),
    so one more bit of column 3 is cleared, which makes (2, 3) odd (607)."""
    V = np.ones((P, n), dtype=bool)
    V[1] = np.random.default_rng(77).random(n) >= 0.2
    V[2, 60:71] = V[2, 128:192] = V[2, 250:261] = False
    V[3, 0] = V[3, n - 1] = V[3, ::3] = False
    V[3, 1] = False
    return V


def _pack(V, junk=True):
    """bool [p, n] -> uint64 [p, nw]; junk: the last word's bits at i >= n set (they are ignored)."""
    p, n = V.shape
    bits = np.zeros((p, 64 * ((n + 63) // 64)), dtype=np.uint8)
    bits[:, :n] = V
    if junk:
        bits[:, n:] = 1
    return np.packbits(bits, axis=1, bitorder="little").view("<u8").astype(np.uint64).reshape(p, -1)


def _n_ab(V, a, b):
    return int((V[a] & V[b]).sum())


def _check_geometry():
    """On the CPU, at import: the (pair, eps) set covers the k < 2 guard, the m == 2 path and a general
    m at an even and at an odd n_ab."""
    from dcor import api
    V = _present()
    counts = {pr: _n_ab(V, *pr) for pr in PAIRS}
    assert counts == {(0, 1): 806, (1, 0): 806, (2, 3): 607, (1, 2): 730, (1, 1): 806}
    geo = {nab: [api.batch_geometry(nab, e, e, "subG", hrs=True) for e in EPS] for nab in (806, 607, 730)}
    assert geo[806] == [(2, 403), (6, 128), (100, 8), (403, 2), (403, 2)]
    assert geo[607] == [(2, 303), (4, 128), (75, 8), (303, 2), (303, 2)]
    assert geo[730] == [(2, 365), (5, 128), (91, 8), (365, 2), (365, 2)]
    for nab in (806, 607):   # even and odd: the guard (k = 2 from eps = 0.1), m == 2, a general m
        ms = [m for _, m in geo[nab]]
        assert geo[nab][0] == (2, nab // 2) and 2 in ms and 8 in ms and 128 in ms


_check_geometry()


def _segments():
    """(col_x, col_y, eps, seed_ni, seed_int, rep_begin, reps, out_row): every pair x every eps, keys
    above 2^32, the three replicate offsets in turn, output blocks in a shuffled order with one
    unnamed row after each block."""
    cells = [(a, b, e) for a, b in PAIRS for e in EPS]
    order = np.random.default_rng(4).permutation(len(cells))
    return [(a, b, e, 2**33 + 1010 + 7 * j, 2**34 + 1020 + 11 * j, REP_BEGIN[j % 3], REPS,
             (REPS + 1) * int(order[j])) for j, (a, b, e) in enumerate(cells)]


def _launch(Z, lam, V, segs, rows, ld=None, delta=float("nan"), fill=np.nan, junk=True, expect=0):
    """dcor_hrs_table_pairwise_launch on the (n, p) array Z laid out with `ld` elements between
    columns, the rows V leaves out overwritten with `fill`; the record buffer starts out as SENTINEL."""
    import torch
    from dcor import _lib
    n, p = Z.shape
    ld = n if ld is None else ld
    host = np.full((p, ld), -123.0)   # the gap between columns is never read
    host[:, :n] = np.where(V, Z.T, fill)
    Dd = torch.as_tensor(host.reshape(-1), device="cuda")
    out = torch.full((max(rows, 1), 6), SENTINEL, dtype=torch.float64, device="cuda")
    lam = np.ascontiguousarray(lam, dtype=np.float64)
    valid = _pack(V, junk)
    desc = _lib.HrsTableNaDesc(n=n, p=p, ld=ld, D=Dd.data_ptr(), lam=lam.ctypes.data_as(C.POINTER(C.c_double)),
                               valid=valid.ctypes.data_as(C.POINTER(C.c_uint64)), alpha=0.05, delta=delta,
                               nsim=2000)
    arr = (_lib.HrsPairSegment * max(len(segs), 1))(*[
        _lib.HrsPairSegment(eps=e, seed_ni=sn, seed_int=si, rep_begin=rb, reps=c, out_row=row, col_x=a, col_y=b)
        for a, b, e, sn, si, rb, c, row in segs])
    st = _lib.lib.dcor_hrs_table_pairwise_launch(C.byref(desc), arr, len(segs), C.c_void_p(out.data_ptr()),
                                                 C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert st == expect, _lib.last_error()
    return out.cpu().numpy()


def _panel(Z, lam, V, seg):
    """The yardstick: the panel entry on the segment's two columns compacted on the host to the rows
    both have, with their clip bounds (its delta_clip is 1 / len = 1 / n_ab)."""
    from dcor import hrs
    a, b, e, sn, si, rb, c = seg[:7]
    ok = V[a] & V[b]
    return hrs.hrs_replicates(np.ascontiguousarray(Z[ok, a]), np.ascontiguousarray(Z[ok, b]), float(lam[a]),
                              float(lam[b]), e, c, seed_ni=sn, seed_int=si, rep_begin=rb, mode="fused")


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


_CACHE = {}


def _one_call():
    """Test 1's segment list in one call (columns at 8-B offsets: ld = n + 3, missing rows NaN),
    computed once and left unchanged."""
    if "one" not in _CACHE:
        segs = _segments()
        _CACHE["one"] = _launch(_table(N), LAM, _present(), segs, (REPS + 1) * len(segs), ld=N + 3)
        _CACHE["one"].setflags(write=False)
    return _CACHE["one"]


# ---------------------------------------------------------------- 1. byte equality per pair
def test_every_segment_equals_the_panel_entry_on_compacted_columns_bitwise():
    Z, V, segs = _table(N), _present(), _segments()
    got = _one_call()
    named = np.zeros(len(got), dtype=bool)
    for seg in segs:
        rows = slice(seg[7], seg[7] + REPS)
        named[rows] = True
        want = _panel(Z, LAM, V, seg)
        assert np.isfinite(want).all()
        assert np.array_equal(_bits(got[rows]), _bits(want)), seg
    assert named.sum() == REPS * len(segs) and np.all(got[~named] == SENTINEL)
    s01, s10 = segs[2], segs[len(EPS) + 2]
    assert s01[:3] == (0, 1, 1.0) and s10[:3] == (1, 0, 1.0)
    assert not np.array_equal(got[s01[7]:s01[7] + REPS, 3:], got[s10[7]:s10[7] + REPS, 3:])


# ---------------------------------------------------------------- 2. full masks
@pytest.mark.parametrize("n", [1001, 1000])
def test_full_masks_equal_the_table_entry_bitwise(n):
    """Every mask bit set and delta = 1 / n (and the NaN default, which is the same here): the present
    table entry's records byte for byte."""
    from test_gpu_hrs_table import _launch as table_launch
    Z, segs = _table(n), _segments()
    rows = (REPS + 1) * len(segs)
    want = table_launch(Z, LAM, segs, rows, ld=n + 3)
    full = np.ones((P, n), dtype=bool)
    assert np.isfinite(want[want != SENTINEL]).all()
    assert np.array_equal(_bits(_launch(Z, LAM, full, segs, rows, ld=n + 3, delta=1.0 / n)), _bits(want))
    assert np.array_equal(_bits(_launch(Z, LAM, full, segs, rows, ld=n, junk=False)), _bits(want))


# ---------------------------------------------------------------- 3. missing rows are never used
def test_values_at_missing_rows_are_ignored():
    Z, V, segs = _table(N), _present(), _segments()
    rows = (REPS + 1) * len(segs)
    one = _one_call()   # NaN at the missing rows
    assert np.isfinite(one[one != SENTINEL]).all()
    for fill in (1e300, -123.0):
        assert np.array_equal(_bits(_launch(Z, LAM, V, segs, rows, ld=N + 3, fill=fill)), _bits(one)), fill


# ---------------------------------------------------------------- 4. NaN at a present row
def test_nan_at_a_present_row_reaches_only_the_pairs_that_name_its_column():
    Z, V = _table(N).copy(order="F"), _present()
    segs = [(a, b, 1.0, 50 + j, 60 + j, 0, REPS, REPS * j) for j, (a, b) in enumerate(PAIRS)]
    ref = _launch(Z, LAM, V, segs, REPS * len(segs), ld=N + 3)
    assert np.isfinite(ref).all()
    row = int(np.flatnonzero(V.all(axis=0))[250])   # present in every column: in every pair's ok
    Z[row, 2] = np.nan
    got = _launch(Z, LAM, V, segs, REPS * len(segs), ld=N + 3)
    for seg in segs:
        rows = slice(seg[7], seg[7] + REPS)
        if 2 in seg[:2]:
            want = _panel(Z, LAM, V, seg)
            assert np.isnan(want[:, 3:]).all()          # INT reads every sample
            assert np.isnan(got[rows, 3:]).all()
            assert np.array_equal(got[rows], want, equal_nan=True), seg
        else:
            assert np.array_equal(_bits(got[rows]), _bits(ref[rows])), seg


# ---------------------------------------------------------------- 5. oracle
@pytest.mark.parametrize("pair", [(2, 3), (1, 0)])
@pytest.mark.parametrize("eps", [0.25, 2.0])
def test_pair_matches_oracle_on_compacted_columns(pair, eps):
    """oracle.ni_subg / int_subg (hrs = 1) on the pair's compacted columns, fed the oracle's own
    restatement of the streams at the HRS sites with n = n_ab, within the project's 1e-12 / 1e-13
    contract: (2, 3) has an odd count (607) and coded columns, (1, 0) an even one (806)."""
    import oracle.oracle as orc
    from dcor import api, hrs
    Z, V = _table(N), _present()
    a, b = pair
    sn, si, rb, reps = 1010, 1020, 3, 3
    Zna = np.where(V.T, Z, np.nan)
    got = hrs.pairwise_segments(Zna, LAM, [(a, b, eps, sn, si, rb, reps)], valid=_pack(V))
    assert got.shape == (reps, 6) and np.isfinite(got).all()
    ok = V[a] & V[b]
    n = int(ok.sum())
    X, Y = np.ascontiguousarray(Z[ok, a]), np.ascontiguousarray(Z[ok, b])
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
        assert_close(got[r], np.concatenate([ni, it]), what=f"pair ({a}, {b}) n_ab={n} eps={eps} rep {rep}")


# ---------------------------------------------------------------- 6. compaction edges
def _edge_masks(n):
    """name -> bool [n] for column 1 (column 0 is complete).  A whole word can go missing only where
    at least two rows remain: word 1 (rows 64..127) at n >= 255; at n = 63, 64 and 65 it would leave
    0, 0 and 1 row."""
    i = np.arange(n)
    m = {"alternate": i % 2 == 0, "first": i != 0, "last": i != n - 1, "ends_only": (i == 0) | (i == n - 1),
         "three": (i == 0) | (i == n // 2) | (i == n - 1)}
    if n >= 255:
        m["word"] = (i < 64) | (i >= 128)
    return m


@pytest.mark.parametrize("n", [63, 64, 65, 255, 256, 257, 513])
def test_compaction_edges_equal_the_panel_entry_bitwise(n):
    """p = 2, one pair, eps = 2.0 and 0.25, every edge mask (n_ab = 2 and 3 run under the guard's k =
    2, m = 1); the missing rows of the table hold NaN."""
    from dcor import api
    Z = _table(n)[:, :2]
    lam = LAM[:2]
    assert api.batch_geometry(2, 2.0, 2.0, "subG", hrs=True) == (2, 1)
    assert api.batch_geometry(3, 0.25, 0.25, "subG", hrs=True) == (2, 1)
    for name, m1 in _edge_masks(n).items():
        V = np.stack([np.ones(n, dtype=bool), m1])
        segs = [(0, 1, e, 2**33 + 5 + j, 2**34 + 9 + j, REP_BEGIN[j], REPS, (REPS + 1) * (1 - j))
                for j, e in enumerate((2.0, 0.25))]
        got = _launch(Z, lam, V, segs, 2 * (REPS + 1), ld=n + 1)
        for seg in segs:
            want = _panel(Z, lam, V, seg)
            assert np.array_equal(_bits(got[seg[7]:seg[7] + REPS]), _bits(want)), (n, name, seg[2])
            assert np.all(got[seg[7] + REPS] == SENTINEL)
        # the reversed pair reads the same rows with the other column as the sender
        rev = [(1, 0) + segs[0][2:]]
        assert np.array_equal(_bits(_launch(Z, lam, V, rev, 2 * (REPS + 1), ld=n)[segs[0][7]:segs[0][7] + REPS]),
                              _bits(_panel(Z, lam, V, rev[0]))), (n, name)


# ---------------------------------------------------------------- 7. split and order invariance
def test_split_and_order_invariance():
    """Test 1's segments reversed, each split into 1 + 2 replicates across two calls: per replicate
    the same bits."""
    Z, V, segs = _table(N), _present(), _segments()
    rows = (REPS + 1) * len(segs)
    one = _one_call()
    first = [(a, b, e, sn, si, rb, 1, row) for a, b, e, sn, si, rb, c, row in segs[::-1]]
    second = [(a, b, e, sn, si, rb + 1, 2, row + 1) for a, b, e, sn, si, rb, c, row in segs[::-1]]
    g1 = _launch(Z, LAM, V, first, rows, ld=N)
    g2 = _launch(Z, LAM, V, second, rows, ld=N + 3)
    named1 = np.zeros(rows, dtype=bool)
    for seg in first:
        named1[seg[7]] = True
    assert np.all(g1[~named1] == SENTINEL) and np.all(g2[named1] == SENTINEL)
    assert np.array_equal(_bits(np.where(named1[:, None], g1, g2)), _bits(one))


# ---------------------------------------------------------------- 8. Python layer
def test_corr_matrix_pairwise_and_sweep():
    from dcor import hrs
    Z, V = _table(N), _present()
    Zna = np.asfortranarray(np.where(V.T, Z, np.nan))
    want_n = (V.astype(np.int64) @ V.T.astype(np.int64))
    assert np.array_equal(hrs.valid_mask(Zna), _pack(V, junk=False))
    grid = (0.25, 1.05, 2.0)
    res = hrs.corr_matrix_pairwise(Zna, LAM, 1.05, 4)
    assert res["pairs"] == [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)] and res["runs"].shape == (6, 4, 6)
    assert res["n_pair"].shape == (P, P) and np.issubdtype(res["n_pair"].dtype, np.integer)
    assert np.array_equal(res["n_pair"], want_n)
    segs = [(a, b, 1.05, 10 + 1000 * (j + 1), 20 + 1000 * (j + 1), 0, 4) for j, (a, b) in enumerate(res["pairs"])]
    assert np.array_equal(_bits(res["runs"].reshape(-1, 6)), _bits(hrs.pairwise_segments(Zna, LAM, segs)))
    for j, (a, b) in enumerate(res["pairs"]):
        assert res["int"]["rho_hat"][a, b] == res["int"]["rho_hat"][b, a] == res["runs"][j][:, 3].mean()
    # the runs are the panel entry's on the compacted columns
    j = res["pairs"].index((2, 3))
    assert np.array_equal(_bits(res["runs"][j]), _bits(_panel(Z, LAM, V, segs[j])))
    pairs = [(1, 2), (3, 0)]
    sw = hrs.corr_matrix_sweep_pairwise(Zna, LAM, grid, 4, pairs=pairs)
    assert sw["runs"].shape == (2, 3, 4, 6) and len(sw["summaries"]) == 2 and sw["eps"] == list(grid)
    assert np.array_equal(sw["n_pair"], want_n)
    segs = [(a, b, e, 10 + 1000 * (j * 3 + idx), 20 + 1000 * (j * 3 + idx), 0, 4)
            for j, (a, b) in enumerate(pairs) for idx, e in enumerate(grid, start=1)]
    assert np.array_equal(_bits(sw["runs"].reshape(-1, 6)), _bits(hrs.pairwise_segments(Zna, LAM, segs)))
    # an explicit mask narrower than the NaN pattern is honoured
    V2 = V.copy()
    V2[0, 10:20] = False
    r2 = hrs.corr_matrix_pairwise(Zna, LAM, 1.05, 2, pairs=[(0, 1)], valid=_pack(V2))
    assert r2["n_pair"][0, 1] == _n_ab(V2, 0, 1) == want_n[0, 1] - int(V[1, 10:20].sum())
    assert np.array_equal(_bits(r2["runs"][0]), _bits(_panel(Z, LAM, V2, (0, 1, 1.05, 1010, 1020, 0, 2))))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def test_hrs_table_pairwise_distributed_rccl_world1():
    import torch
    import torch.distributed as dist
    from dcor import hrs
    from dcor.dist import hrs_table_pairwise_distributed
    Z, V = _table(N), _present()
    Zna = np.asfortranarray(np.where(V.T, Z, np.nan))
    segs = [(0, 1, 1.0, 61, 71, 0, 7), (3, 1, 0.25, 62, 72, 1001, 3), (2, 2, 2.0, 63, 73, 5, 0),
            (1, 2, 2.45, 64, 74, 2, 4)]
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()))
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    try:
        got = hrs_table_pairwise_distributed(Zna, LAM, segs)
        empty = hrs_table_pairwise_distributed(Zna, LAM, [])
    finally:
        dist.destroy_process_group()
    want = hrs.pairwise_segments(Zna, LAM, segs)
    assert want.shape == (14, 6) and got.tobytes() == want.tobytes() and empty.shape == (0, 6)
