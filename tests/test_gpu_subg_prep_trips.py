"""GPU tests of the sub-G preparation kernels (k_subg_panel_prep, k_subg_table_prep,
csrc/dcor_subgpanel.hip) at sizes where their grid-stride loops take more than one trip.  Both
launchers cap the preparation grid at 1,024 blocks of 256 threads; below that cap (every other
sub-G test) each loop body runs once per thread or block, so a loop that stopped after its first
trip, a tile split that went wrong from the second trip on, or a launcher whose cap differed from
the kernel's stride would pass.  Here every loop takes a second trip (a third for the long table):

  panel  n = 300,007   copy: 1,172 tiles of 256 > 1,024 blocks; means at m = 1: k = n > 262,144
  table  n = 70,001    p = 4: 4 x 274 = 1,096 tiles, copy and (at m = 1) means; p = 5: the second
                       trip runs from inside column 3 across the boundary into column 4
  table  n = 300,007   p = 2: 2 x 1,172 = 2,344 tiles, three trips

Every call is checked against the oracle on the restated draw contract (helpers.assert_close, the
suite's 1e-12 / 1e-13), the table's records are bit-equal to the panel entry's on the two contiguous
columns, and every call runs after a call of the same layout on 1e300 data: the entries reuse their
call scratch, so a value the real call fails to rewrite is a value no estimator survives."""
import functools

import numpy as np
import pytest

import subg_panel_ref as R
from helpers import ATOL, RTOL, assert_close
from test_gpu_subg_panel import _dev, _panel, _u64
from test_gpu_subg_panel import _launch as _panel_launch
from test_gpu_subg_table import _launch as _table_launch
from test_gpu_subg_table import _upload

pytestmark = pytest.mark.gpu

PREP_NT, PREP_MAXGRID = 256, 1024   # SGP_PREP_NT, SGP_PREP_MAXGRID (csrc/dcor_subgpanel.hip)
GS = PREP_NT * PREP_MAXGRID         # the panel loops' stride at the cap: 262,144
N_BIG, N_TAB = 300_007, 70_001
EPS_K1 = (0.005, 0.005)             # ceil(8 / (eps1 eps2)) = 320,000 >= n: m = n, k = 1
POISON = 1e300


def _npad(n):
    return (n + 3) & ~3


def _tiles(v):
    return -(-v // PREP_NT)


# the geometry the cases below rely on, restated and checked without a device
for _n in (N_BIG, N_TAB):
    assert _n % 2 == 1 and _n % 4 != 0 and _npad(_n) > _n   # the last pair reads the zero padding
assert _tiles(_npad(N_BIG)) == 1172 > PREP_MAXGRID          # panel copy: blocks 0..147 take two trips
assert _tiles(_npad(N_BIG)) - PREP_MAXGRID == 148
assert R.geometry(N_BIG, 1.0, 1.0) == (37_500, 8)
assert R.geometry(N_BIG, 0.5, 1.5) == (27_273, 11) and R.geometry(N_BIG, 1.5, 0.5)[1] == 11
assert R.geometry(N_BIG, 4.0, 2.0) == (N_BIG, 1) and N_BIG > GS   # panel means: a second trip of j += gs
assert R.geometry(N_BIG, 2.0, 2.0) == (150_003, 2) and 150_003 < GS   # one trip: the control
assert R.geometry(N_BIG, *EPS_K1) == (1, N_BIG)
assert _tiles(_npad(N_TAB)) == 274
assert 4 * 274 == 1096 > PREP_MAXGRID and 3 * 274 < PREP_MAXGRID      # p = 4: tiles 1,024..1,095, all in column 3
assert 4 * 274 < PREP_MAXGRID + 274 < 5 * 274                          # p = 5: the second trip enters column 4
assert R.geometry(N_TAB, 4.0, 2.0) == (N_TAB, 1) and 4 * _tiles(N_TAB) == 1096   # table means at m = 1
assert 2 * _tiles(_npad(N_BIG)) == 2344 > 2 * PREP_MAXGRID             # long table: three trips of the copy
assert 2 * _tiles(N_BIG) > 2 * PREP_MAXGRID                            # and of the means at m = 1

# ---------------------------------------------------------------- the calls
# panel: (eps1, eps2, seed, rep_begin, reps, out_row); 2 replicates a segment, rep_begin 0 or 1001
PANEL_CALLS = {
    # m = 1, 2 and 8 in one call: three mean slots at offsets 0, n and n + 150,003
    "means_m1_m2_m8": dict(segs=[(4.0, 2.0, 101, 0, 2, 4), (2.0, 2.0, 102, 1001, 2, 0),
                                 (1.0, 1.0, (7 << 32) + 11, 0, 2, 2)], eta=(1.0, 1.0)),
    # m = 11 with either sender
    "copy_m11_senders": dict(segs=[(0.5, 1.5, 103, 1001, 2, 0), (1.5, 0.5, 104, 0, 2, 2)], eta=(0.5, 0.8)),
    # k = 1: one thread adds all n clipped samples in index order
    "k1": dict(segs=[(EPS_K1[0], EPS_K1[1], 105, 1001, 2, 0)], eta=(1.0, 1.0)),
}
# table: (col_x, col_y, eps1, eps2, seed, rep_begin, reps, out_row)
ETA5 = (1.0, 0.5, 0.8, 1.3, 0.9)
TABLE_CALLS = {
    # copy and means (m = 1: kt = 274) past the cap, m = 8 and m = 11 in the same call.  Column 3's
    # last 4,000 rows lie in second-trip tiles and above every clip: the four segments naming column 3
    # depend on them (NI through its last batches' clipped means, INT through the copied rows); the
    # (1, 0) segment does not.
    "p4": dict(n=N_TAB, p=4, segs=[(0, 3, 4.0, 2.0, 201, 0, 2, 8), (3, 1, 1.0, 1.0, (9 << 32) + 1, 1001, 2, 0),
                                   (3, 3, 0.5, 1.5, 203, 0, 2, 2), (2, 3, 1.5, 0.5, 204, 1001, 2, 4),
                                   (1, 0, 2.0, 2.0, 205, 0, 2, 6)]),
    # a fifth column: second-trip tiles 1,024..1,369 span the boundary between columns 3 and 4
    "p5": dict(n=N_TAB, p=5, segs=[(3, 4, 1.0, 1.0, 211, 0, 2, 0), (4, 3, 4.0, 2.0, 212, 1001, 2, 2),
                                   (4, 4, 0.5, 1.5, 213, 0, 2, 4)]),
    # three trips of both loops
    "long_p2": dict(n=N_BIG, p=2, segs=[(0, 1, 1.0, 1.0, 221, 0, 2, 0), (1, 0, 4.0, 2.0, 222, 1001, 2, 2),
                                        (1, 1, 0.5, 1.5, 223, 0, 2, 4)]),
}


def _orc():
    import oracle.oracle as orc
    return orc


@functools.lru_cache(maxsize=None)
def _big_panel():
    X, Y = _panel(N_BIG, seed=5)
    X.setflags(write=False)
    Y.setflags(write=False)
    return X, Y


@functools.lru_cache(maxsize=None)
def _table_data(n, p):
    """Column-major (n, p).  n = 70,001: test_gpu_subg_table's four columns (a fifth for p = 5), the
    last 4,000 rows of column 3 replaced by values between 9 and 9.006, above every clip.
    n = 300,007: the big panel's two columns."""
    if n == N_BIG:
        D = np.asfortranarray(np.stack(_big_panel(), axis=1))
    else:
        a, b = _panel(n, seed=n)
        c, d = _panel(n, seed=n + 1, rho=0.2)
        e, _ = _panel(n, seed=n + 2)
        d[-4000:] = 9.0 + 0.001 * (np.arange(4000) % 7)
        D = np.asfortranarray(np.stack([a, b, c, d, e][:p], axis=1))
    D.setflags(write=False)
    return D


def _rows(segs):
    return sum(s[-2] for s in segs)


@functools.lru_cache(maxsize=None)
def _panel_run(name):
    """(records after a poison call, records of the same call repeated)."""
    call = PANEL_CALLS[name]
    segs, (eta1, eta2) = call["segs"], call["eta"]
    X, Y = _big_panel()
    Pd = _dev(np.full(N_BIG, POISON), np.full(N_BIG, POISON))
    st, _ = _panel_launch(*Pd, segs, _rows(segs), eta1=eta1, eta2=eta2)
    assert st == 0
    Xd, Yd = _dev(X, Y)
    st, got = _panel_launch(Xd, Yd, segs, _rows(segs), eta1=eta1, eta2=eta2)
    assert st == 0
    st, again = _panel_launch(Xd, Yd, segs, _rows(segs), eta1=eta1, eta2=eta2)
    assert st == 0
    return got, again


@functools.lru_cache(maxsize=None)
def _table_run(name):
    call = TABLE_CALLS[name]
    n, p, segs = call["n"], call["p"], call["segs"]
    D, ld = _table_data(n, p), n + 3
    st, _ = _table_launch(_upload(np.full((n, p), POISON), ld), n, ld, segs, _rows(segs), eta=ETA5[:p], p=p)
    assert st == 0
    Dd = _upload(D, ld)
    st, got = _table_launch(Dd, n, ld, segs, _rows(segs), eta=ETA5[:p], p=p)
    assert st == 0
    st, again = _table_launch(Dd, n, ld, segs, _rows(segs), eta=ETA5[:p], p=p)
    assert st == 0
    return got, again


def _check_oracle(got, ref, what):
    dev = np.abs(got - ref) / np.maximum(np.abs(got), np.abs(ref))
    print(f"{what}: worst relative deviation from the oracle {np.nanmax(dev):.3e}")
    assert np.array_equal(np.isnan(got), np.isnan(ref)), what
    assert np.array_equal(np.isinf(got), np.isinf(ref)), what
    assert_close(got, ref, rtol=RTOL, atol=ATOL, what=what)


# ---------------------------------------------------------------- the panel
@pytest.mark.parametrize("name", list(PANEL_CALLS))
def test_panel_matches_oracle_after_poison(name):
    call = PANEL_CALLS[name]
    X, Y = _big_panel()
    got, _ = _panel_run(name)
    for e1, e2, seed, rb, c, row in call["segs"]:
        ref = R.oracle_records(_orc(), X, Y, e1, e2, seed, rb, c, eta1=call["eta"][0], eta2=call["eta"][1])
        _check_oracle(got[row:row + c], ref, f"panel {name} eps=({e1},{e2})")
        if R.geometry(N_BIG, e1, e2)[0] == 1:   # k = 1: the NI CI is NA exactly where the oracle's is
            assert np.isnan(got[row:row + c, 1:3]).all() and not np.isnan(got[row:row + c][:, [0, 3, 4, 5]]).any()
        else:
            assert not np.isnan(got[row:row + c]).any()


@pytest.mark.parametrize("name", list(PANEL_CALLS))
def test_panel_records_do_not_depend_on_the_call_before(name):
    """The call after the 1e300 panel and the call after itself: the same bits."""
    got, again = _panel_run(name)
    assert np.array_equal(_u64(got), _u64(again))


def test_panel_segments_equal_their_single_calls():
    """Three mean slots in one call (offsets 0, n, n + 150,003) against one call per segment."""
    call = PANEL_CALLS["means_m1_m2_m8"]
    got, _ = _panel_run("means_m1_m2_m8")
    Xd, Yd = _dev(*_big_panel())
    for e1, e2, seed, rb, c, row in call["segs"]:
        st, one = _panel_launch(Xd, Yd, [(e1, e2, seed, rb, c, 0)], c)
        assert st == 0 and np.array_equal(_u64(got[row:row + c]), _u64(one)), (e1, e2)


# ---------------------------------------------------------------- the table
@pytest.mark.parametrize("name", list(TABLE_CALLS))
def test_table_matches_oracle_after_poison(name):
    call = TABLE_CALLS[name]
    D = _table_data(call["n"], call["p"])
    got, _ = _table_run(name)
    for a, b, e1, e2, seed, rb, c, row in call["segs"]:
        ref = R.oracle_records(_orc(), D[:, a], D[:, b], e1, e2, seed, rb, c, eta1=ETA5[a], eta2=ETA5[b])
        _check_oracle(got[row:row + c], ref, f"table {name} pair ({a},{b}) eps=({e1},{e2})")
        assert not np.isnan(got[row:row + c]).any()


@pytest.mark.parametrize("name", list(TABLE_CALLS))
def test_table_equals_panel_entry_bytewise(name):
    import torch
    call = TABLE_CALLS[name]
    D = _table_data(call["n"], call["p"])
    got, again = _table_run(name)
    assert np.array_equal(_u64(got), _u64(again))   # after the 1e300 table, and after itself
    for a, b, e1, e2, seed, rb, c, row in call["segs"]:
        Xd = torch.as_tensor(np.ascontiguousarray(D[:, a]), device="cuda")
        Yd = torch.as_tensor(np.ascontiguousarray(D[:, b]), device="cuda")
        st, one = _panel_launch(Xd, Yd, [(e1, e2, seed, rb, c, 0)], c, eta1=ETA5[a], eta2=ETA5[b])
        assert st == 0 and np.array_equal(_u64(got[row:row + c]), _u64(one)), (a, b, e1, e2)


def test_table_last_rows_reach_the_records():
    """The 4,000 marked rows of column 3 (second-trip tiles of the copy, the last batches of the
    means) move every record that names column 3 and none of the (1, 0) segment's."""
    call = TABLE_CALLS["p4"]
    n, p, segs = call["n"], call["p"], call["segs"]
    got, _ = _table_run("p4")
    D = np.array(_table_data(n, p))
    D[-4000:, 3] = _panel(n, seed=n + 1, rho=0.2)[1][-4000:]
    st, plain = _table_launch(_upload(D, n + 3), n, n + 3, segs, _rows(segs), eta=ETA5[:p], p=p)
    assert st == 0
    for a, b, e1, e2, seed, rb, c, row in segs:
        same = _u64(got[row:row + c]) == _u64(plain[row:row + c])
        if 3 in (a, b):
            assert not same[:, [0, 1, 3, 4]].any(), (a, b)   # estimates and lower ends (upper ends clamp at 1)
        else:
            assert same.all(), (a, b)
