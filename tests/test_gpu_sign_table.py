"""GPU tests of the sign-family table path (dcor_sign_table_launch, dcor.signpanel.table_segments /
corr_matrix, dcor.dist.sign_table_distributed).  The yardstick is the panel entry
(dcor_sign_panel_launch through dcor.signpanel.sweep_segments) on the pair's two columns, compared
as uint64, and through tests/sign_panel_ref.py the oracle -- never the table path itself."""
import ctypes as C
import os
import socket

import numpy as np
import pytest

import sign_panel_ref as R
from helpers import assert_close

pytestmark = pytest.mark.gpu

N, P, LD = 1003, 4, 1011   # odd n, not a multiple of 4; columns at 8-B offsets in the caller's table
PAIRS = [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3), (3, 1), (2, 2)]
EPS = [(2.0, 2.0), (1.0, 1.0), (0.2, 0.2), (1.5, 0.7)]   # m = 2, 8, 200 (k = 5, k m = 1000 < n), 8
REPS = 5


def _table(n=N, p=P, seed=17):
    """Correlated columns of different location and scale (some clipped at sqrt(2 log n), some not)."""
    g = np.random.default_rng(seed)
    f = g.standard_normal(n)
    cols = [(0.3 + 0.2 * c) + (0.6 + 0.5 * c) * (np.sqrt(0.5) * f + np.sqrt(0.5) * g.standard_normal(n))
            for c in range(p)]
    return np.asfortranarray(np.stack(cols, axis=1))


def _segments():
    """(col_x, col_y, eps1, eps2, seed, rep_begin, reps, out_row): every pair x every eps pair, five
    replicates each, rep_begin 0 or 7, distinct seeds, output blocks in a shuffled order."""
    cells = [(a, b, e1, e2) for a, b in PAIRS for e1, e2 in EPS]
    order = np.random.default_rng(4).permutation(len(cells))
    return [(a, b, e1, e2, 1_000 + 13 * j, (0, 7)[(j + j // 4) % 2], REPS, REPS * int(order[j]))
            for j, (a, b, e1, e2) in enumerate(cells)]


def _launch(D, segs, rows, ld=None, normalise=1, sentinel=float("nan")):
    """dcor_sign_table_launch on the (n, p) array D laid out with `ld` elements between columns."""
    import torch
    from dcor import _lib
    n, p = D.shape
    ld = n if ld is None else ld
    host = np.full((p, ld), -123.0)   # the gap between columns is never read
    host[:, :n] = D.T
    Dd = torch.as_tensor(host.reshape(-1), device="cuda")
    out = torch.full((rows, 6), sentinel, dtype=torch.float64, device="cuda")
    desc = _lib.SignTableDesc(n=n, p=p, ld=ld, D=Dd.data_ptr(), alpha=0.05, normalise=normalise, ci_mode=0,
                              nsim=1000)
    arr = (_lib.SignPairSegment * len(segs))(*[
        _lib.SignPairSegment(eps1=e1, eps2=e2, seed=s, rep_begin=rb, reps=c, out_row=row, col_x=a, col_y=b)
        for a, b, e1, e2, s, rb, c, row in segs])
    st = _lib.lib.dcor_sign_table_launch(C.byref(desc), arr, len(segs), C.c_void_p(out.data_ptr()),
                                         C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert st == 0, _lib.last_error()
    return out.cpu().numpy()


def _panel(D, seg, normalise=True):
    """The yardstick: the panel entry on the segment's two columns."""
    from dcor import signpanel
    a, b, e1, e2, s, rb, c = seg[:7]
    return signpanel.sweep_segments(np.ascontiguousarray(D[:, a]), np.ascontiguousarray(D[:, b]),
                                    [(e1, e2, s, rb, c)], normalise=normalise)


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


_CACHE = {}


def _one_call():
    """Test 1's segment list in one table call, computed once and left unchanged."""
    if "one" not in _CACHE:
        segs = _segments()
        _CACHE["one"] = _launch(_table(), segs, REPS * len(segs), ld=LD)
        _CACHE["one"].setflags(write=False)
    return _CACHE["one"]


# ---------------------------------------------------------------- 1. bit equality per pair
def test_every_segment_equals_the_panel_entry_bitwise():
    D, segs = _table(), _segments()
    got = _one_call()
    assert sorted(s[7] for s in segs) == list(range(0, REPS * len(segs), REPS))
    for seg in segs:
        want = _panel(D, seg)
        assert not np.isnan(want[:, [0, 3, 4, 5]]).any()
        assert np.array_equal(_bits(got[seg[7]:seg[7] + REPS]), _bits(want)), seg
    # the pairs differ from one another: (1, 3) and (3, 1) are different segments' data
    s13, s31 = segs[4 * 4 + 1], segs[6 * 4 + 1]
    assert s13[:2] == (1, 3) and s31[:2] == (3, 1)
    assert not np.array_equal(got[s13[7]:s13[7] + REPS], got[s31[7]:s31[7] + REPS])


# ---------------------------------------------------------------- 2. counter passes
@pytest.mark.parametrize("n,eps", [(9001, 2.0), (40_001, 0.0156)])
def test_counter_passes_equal_the_panel_entry(n, eps):
    """n = 9,001 at eps = (2, 2): k = 4,500 batches, more than one pass of the LDS counters;
    n = 40,001 at eps = 0.0156: m = 32,873 > 32,767, the two-word counters, k = 1."""
    k, m = R.geometry(n, eps, eps)
    assert (k > 4096) if eps == 2.0 else (m > 32767 and k == 1)
    D = _table(n, 2, seed=n)
    segs = [(0, 1, eps, eps, 31, 2, 3, 0), (1, 0, eps, eps, 32, 0, 3, 3)]
    got = _launch(D, segs, 6)
    for seg in segs:
        assert np.array_equal(_bits(got[seg[7]:seg[7] + 3]), _bits(_panel(D, seg))), seg


# ---------------------------------------------------------------- 3. oracle
@pytest.mark.parametrize("normalise", [True, False])
def test_pair_matches_oracle(normalise):
    import oracle.oracle as orc
    from dcor import signpanel
    D = _table()
    got = signpanel.table_segments(D, [(0, 2, 1.0, 1.0, 77, 3, 4)], normalise=normalise)
    ref = R.oracle_records(orc, np.ascontiguousarray(D[:, 0]), np.ascontiguousarray(D[:, 2]), 1.0, 1.0, 77, 3, 4,
                           normalise=normalise)
    assert got.shape == (4, 6) and not np.isnan(got).any()
    assert_close(got, ref, what=f"pair (0, 2) normalise={normalise}")


# ---------------------------------------------------------------- 4. NaN isolation
@pytest.mark.parametrize("normalise,idx", [(1, 500), (0, 500), (0, 1001)])
def test_nan_reaches_only_the_pairs_that_name_its_column(normalise, idx):
    """A NaN in one sample of column 2 (idx 1001: in the tail past k m = 1000 at eps = (1, 1), where
    raw signs leave NI finite).  Pairs without column 2: the clean table's records byte for byte;
    pairs with it: the panel entry on the same columns, NaN pattern included."""
    clean = _table()
    D = clean.copy(order="F")
    D[idx, 2] = np.nan
    segs = [(a, b, 1.0, 1.0, 50 + j, 0, 3, 3 * j) for j, (a, b) in enumerate(PAIRS)]
    got = _launch(D, segs, 3 * len(segs), ld=LD, normalise=normalise)
    ref = _launch(clean, segs, 3 * len(segs), ld=LD, normalise=normalise)
    assert not np.isnan(ref).any()
    for seg in segs:
        rows = slice(seg[7], seg[7] + 3)
        if 2 in seg[:2]:
            want = _panel(D, seg, normalise=bool(normalise))
            assert np.isnan(want[:, 3:]).all()
            assert np.isnan(want[:, :3]).all() == (idx < 1000 or normalise == 1)
            assert np.array_equal(_bits(got[rows]), _bits(want)), seg
        else:
            assert np.array_equal(_bits(got[rows]), _bits(ref[rows])), seg


# ---------------------------------------------------------------- 5. split and order invariance
def test_split_and_order_invariance():
    D, segs = _table(), _segments()
    rows = REPS * len(segs)
    one = _one_call()
    # two calls, split inside segment 13 by rep_begin: replicates [rb, rb + 2) and [rb + 2, rb + 5)
    a, b, e1, e2, s, rb, c, row = segs[13]
    first = segs[:13] + [(a, b, e1, e2, s, rb, 2, row)]
    second = [(a, b, e1, e2, s, rb + 2, 3, row + 2)] + segs[14:]
    g1 = _launch(D, first, rows, ld=LD, sentinel=-7.25)
    g2 = _launch(D, second, rows, ld=LD, sentinel=-7.25)
    named1 = np.zeros(rows, dtype=bool)
    for seg in first:
        named1[seg[7]:seg[7] + seg[6]] = True
    assert np.all(g1[~named1] == -7.25) and np.all(g2[named1] == -7.25)
    assert np.array_equal(_bits(np.where(named1[:, None], g1, g2)), _bits(one))
    # reversed segment order
    assert np.array_equal(_bits(_launch(D, segs[::-1], rows, ld=LD)), _bits(one))


# ---------------------------------------------------------------- 6. corr_matrix
def test_corr_matrix_runs_and_matrices():
    from dcor import signpanel
    D = _table(N, 3)
    res = signpanel.corr_matrix(D, 1.0, 1.0, 50, seed=500)
    assert res["pairs"] == [(0, 1), (0, 2), (1, 2)] and res["runs"].shape == (3, 50, 6)
    for j, (a, b) in enumerate(res["pairs"]):
        want = signpanel.replicates(np.ascontiguousarray(D[:, a]), np.ascontiguousarray(D[:, b]), 1.0, 1.0, 50,
                                    500 + j + 1)
        assert np.array_equal(_bits(res["runs"][j]), _bits(want)), (a, b)
        for m, c in (("ni", 0), ("int", 3)):
            for i, k in enumerate(("rho_hat", "ci_low", "ci_high")):
                M = res[m][k]
                assert M.shape == (3, 3) and M[a, b] == M[b, a] == res["runs"][j][:, c + i].mean()
    for m in ("ni", "int"):
        for M in res[m].values():
            assert np.isnan(np.diag(M)).all() and np.array_equal(M, M.T, equal_nan=True)
            assert not np.isnan(M[~np.eye(3, dtype=bool)]).any()
    # asked-for pairs only, the diagonal among them; the sweep form keys pair j, eps idx as documented
    sub = signpanel.corr_matrix(D, 1.0, 1.0, 4, seed=500, pairs=[(1, 1), (2, 0)])
    assert not np.isnan(sub["int"]["rho_hat"][1, 1]) and np.isnan(sub["int"]["rho_hat"][0, 0])
    assert sub["ni"]["rho_hat"][0, 2] == sub["ni"]["rho_hat"][2, 0] == sub["runs"][1][:, 0].mean()
    assert np.isnan(sub["ni"]["rho_hat"][0, 1])
    sw = signpanel.corr_matrix_sweep(D, (0.5, 1.0), 4, seed=900, pairs=[(0, 1), (1, 2)])
    assert sw["runs"].shape == (2, 2, 4, 6) and len(sw["summaries"]) == 2
    es = signpanel.eps_sweep(np.ascontiguousarray(D[:, 1]), np.ascontiguousarray(D[:, 2]), (0.5, 1.0), 4, seed=902)
    assert np.array_equal(_bits(sw["runs"][1]), _bits(es["runs"]))
    assert sw["summaries"][1]["int_mean"] == es["int_mean"]


# ---------------------------------------------------------------- 7. ranks
RANK_SEGS = [(0, 1, 1.0, 1.0, 61, 0, 7), (3, 1, 0.2, 0.2, 62, 1001, 3), (2, 2, 2.0, 2.0, 63, 5, 0),
             (1, 2, 1.5, 0.7, 64, 2, 4)]   # 14 replicates: the two ranks split inside a segment


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rank_runs():
    from dcor.dist import sign_table_distributed
    D = _table()
    return [sign_table_distributed(D, RANK_SEGS).tobytes(),
            sign_table_distributed(D, [(0, 2, 1.0, 1.0, 65, 9, 1)]).tobytes(),   # fewer items than ranks
            sign_table_distributed(D, []).tobytes()]


def _rank_expected():
    from dcor import signpanel
    D = _table()
    return [signpanel.table_segments(D, RANK_SEGS).tobytes(),
            signpanel.table_segments(D, [(0, 2, 1.0, 1.0, 65, 9, 1)]).tobytes(), b""]


def test_sign_table_distributed_rccl_world1():
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


def test_sign_table_distributed_two_ranks_on_gpu():
    """Two gloo ranks sharing cuda:0: each runs its contiguous part of the flattened (segment,
    replicate) space in one native call; the gathered records are the one-process call's bytes."""
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
