"""GPU tests of sign_panel_item (csrc/dcor_signpanel.hip), the replicate both k_sign_panel and
k_sign_table run, at the batch geometry the other sign-panel tests leave out, against the oracle on
the restated draws (sign_panel_ref.oracle_records): the two-word counters (m > 32,767), the packing
boundary m = 32,767 | 32,768 with batch counts of exactly +-m, the small and the large batch sizes,
the edges of the counter passes (k around multiples of 4,096), and workgroups that run several
items across segments of different kinds.  The shapes are the tables of sign_edges_ref.py, pinned
on the CPU by test_sign_edges_ref.py.

Tolerance: helpers.assert_close for m <= 200, as everywhere; sign_edges_ref.assert_close_ni_conditioned
for m > 200, where one ulp of T_j = m xt yt is more than helpers' bound allows the NI numbers."""
import functools

import numpy as np
import pytest

import sign_edges_ref as E
import sign_panel_ref as R
from helpers import assert_close
from test_gpu_sign_panel import _dev, _launch as _launch_panel
from test_gpu_sign_table import _bits, _launch as _launch_table

pytestmark = pytest.mark.gpu

MODES = {"auto": 0, "normal": 1, "laplace": 2}
SENTINEL = -7.25


def _orc():
    import oracle.oracle as orc
    return orc


@functools.lru_cache(maxsize=None)
def _panel(n):
    """(X, Y) of n samples, drawn once; the tests only read it."""
    return E.edge_panel(n, seed=n)


@functools.lru_cache(maxsize=None)
def _ref(n, eps1, eps2, normalise, mode, rep_begin, swap=False):
    """The oracle's records on _panel(n) (swap: on (Y, X)), computed once per case, shared and
    left unchanged."""
    X, Y = _panel(n)[::-1] if swap else _panel(n)
    ref = R.oracle_records(_orc(), X, Y, eps1, eps2, E.EDGE_SEED, rep_begin, E.EDGE_REPS,
                           normalise=bool(normalise), mode=MODES[mode])
    ref.setflags(write=False)
    return ref


def _check(got, ref, n, eps1, eps2, seed, rep_begin, what):
    """got against the oracle's ref at the tolerance the batch size calls for; the NaN pattern is the
    oracle's: the NI interval NaN exactly when k = 1, everything else finite."""
    k, m = R.geometry(n, eps1, eps2)
    assert got.shape == ref.shape, what
    assert np.array_equal(np.isnan(got), np.isnan(ref)), (what, got, ref)
    assert np.isnan(got[:, 1:3]).all() == (k == 1) and not np.isnan(got[:, [0, 3, 4, 5]]).any(), (what, got)
    if m <= 200:
        assert_close(got, ref, what=what)
    else:
        E.assert_close_ni_conditioned(got, ref, E.ni_T_bounds(_orc(), n, eps1, eps2, seed, rep_begin, len(got)), what)


def _ids(shape):
    return f"{shape[0]}-{shape[1]:.6g}-{shape[2]:.6g}"


# ---------------------------------------------------------------- a. wide counters
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("normalise", [1, 0])
@pytest.mark.parametrize("shape", list(E.WIDE_SHAPES), ids=_ids)
def test_wide_counters_match_oracle(shape, normalise, mode):
    """m = 33,334: cx and cy in two counter words.  k = 2: two threads' flushes meet in both words of
    a batch; eps swapped: bx != by the other way round, so a swap of the two words cannot hide."""
    from dcor import signpanel
    n, eps1, eps2 = shape
    k, m = R.geometry(n, eps1, eps2)
    assert (k, m) == E.WIDE_SHAPES[shape] and m > 32_767
    X, Y = _panel(n)
    for rep_begin in E.EDGE_REP_BEGINS:
        got = signpanel.replicates(X, Y, eps1, eps2, E.EDGE_REPS, E.EDGE_SEED, rep_begin=rep_begin,
                                   normalise=bool(normalise), mode=mode)
        _check(got, _ref(n, eps1, eps2, normalise, mode, rep_begin), n, eps1, eps2, E.EDGE_SEED, rep_begin,
               f"wide {shape} normalise={normalise} {mode} rep_begin={rep_begin}")


@pytest.mark.parametrize("shape", list(E.WIDE_SHAPES), ids=_ids)
def test_wide_counters_table_shell_matches_oracle(shape):
    """The same shapes through k_sign_table, columns (0, 1) and (1, 0) of a two-column table, against
    the oracle on those columns: the table shell pinned to the oracle at wide m, not to the panel."""
    from dcor import signpanel
    n, eps1, eps2 = shape
    X, Y = _panel(n)
    D = np.asfortranarray(np.stack([X, Y], axis=1))
    rb0, rb1 = E.EDGE_REP_BEGINS
    got = signpanel.table_segments(D, [(0, 1, eps1, eps2, E.EDGE_SEED, rb0, E.EDGE_REPS),
                                       (1, 0, eps1, eps2, E.EDGE_SEED, rb1, E.EDGE_REPS)])
    assert got.shape == (2 * E.EDGE_REPS, 6)
    _check(got[:E.EDGE_REPS], _ref(n, eps1, eps2, 1, "auto", rb0), n, eps1, eps2, E.EDGE_SEED, rb0,
           f"table (0,1) {shape}")
    _check(got[E.EDGE_REPS:], _ref(n, eps1, eps2, 1, "auto", rb1, swap=True), n, eps1, eps2, E.EDGE_SEED, rb1,
           f"table (1,0) {shape}")


# ---------------------------------------------------------------- b. packing boundary
@pytest.mark.parametrize("kind", E.PACK_PANELS)
@pytest.mark.parametrize("shape", list(E.PACK_SHAPES), ids=lambda s: str(s[0]))
def test_packing_boundary_exact_counts(shape, kind):
    """m = 32,767 (the last one-word m: cx + 65536 cy, read back through int16) and m = 32,768 (the
    first two-word m) on raw signs of constant-sign panels: every batch count is exactly (+-m, +-m),
    the extreme the packed word must hold.  A count off by one moves T by |yt| >= ~0.3, far outside
    any tolerance here.  "half": each batch's counts cancel to (-1, 1) or (0, 0) from +-16,383 up."""
    from dcor import signpanel
    n, eps1, eps2 = shape
    k, m = R.geometry(n, eps1, eps2)
    assert (k, m) == E.PACK_SHAPES[shape]
    X, Y = E.pack_panel(n, m, kind)
    cx, cy = E.pack_counts(X, Y, k, m)
    assert np.all(np.abs(cx) == (m if kind != "half" else m % 2)) and np.all(np.abs(cy) == np.abs(cx))
    for rep_begin in E.EDGE_REP_BEGINS:
        got = signpanel.replicates(X, Y, eps1, eps2, E.EDGE_REPS, E.EDGE_SEED, rep_begin=rep_begin, normalise=False)
        ref = R.oracle_records(_orc(), X, Y, eps1, eps2, E.EDGE_SEED, rep_begin, E.EDGE_REPS, normalise=False)
        _check(got, ref, n, eps1, eps2, E.EDGE_SEED, rep_begin, f"pack {shape} {kind} rep_begin={rep_begin}")


@pytest.mark.parametrize("shape", list(E.PACK_SHAPES), ids=lambda s: str(s[0]))
def test_packing_boundary_random_panel(shape):
    from dcor import signpanel
    n, eps1, eps2 = shape
    assert R.geometry(n, eps1, eps2) == E.PACK_SHAPES[shape]
    X, Y = _panel(n)
    for rep_begin in E.EDGE_REP_BEGINS:
        got = signpanel.replicates(X, Y, eps1, eps2, E.EDGE_REPS, E.EDGE_SEED, rep_begin=rep_begin, normalise=True)
        _check(got, _ref(n, eps1, eps2, 1, "auto", rep_begin), n, eps1, eps2, E.EDGE_SEED, rep_begin,
               f"pack {shape} random rep_begin={rep_begin}")


# ---------------------------------------------------------------- c. batch sizes and pass edges
@pytest.mark.parametrize("normalise", [1, 0])
@pytest.mark.parametrize("shape", list(E.BATCH_SHAPES), ids=_ids)
def test_batch_sizes_and_pass_edges(shape, normalise):
    """m = 1, 3, 4, 5 (up to four flushes per flip block), m = 1,024 (a thread's offset never
    moves), m = 1,025 and 3,200 (its batch moves only by the carry; a batch spans trips of the
    sample loop), and k = 4,096, 4,097, 8,192, 8,193: a last pass that is full, or one batch, with
    and without a tail past k m."""
    from dcor import signpanel
    n, eps1, eps2 = shape
    assert R.geometry(n, eps1, eps2) == E.BATCH_SHAPES[shape]
    X, Y = _panel(n)
    for rep_begin in E.EDGE_REP_BEGINS:
        got = signpanel.replicates(X, Y, eps1, eps2, E.EDGE_REPS, E.EDGE_SEED, rep_begin=rep_begin,
                                   normalise=bool(normalise))
        _check(got, _ref(n, eps1, eps2, normalise, "auto", rep_begin), n, eps1, eps2, E.EDGE_SEED, rep_begin,
               f"batch {shape} normalise={normalise} rep_begin={rep_begin}")


# ---------------------------------------------------------------- d, e. several items per workgroup
def _items():
    """3 G one-replicate items, G = 8 x CUs.  A workgroup of the replicate kernels holds SpLds, just
    over 20 KB (20,192 B) of a CU's 160 KB of LDS, so at most 8 fit a CU and the persistent grid
    (CUs x resident workgroups per CU) cannot exceed G: every workgroup runs at least three items."""
    import torch
    return 3 * 8 * torch.cuda.get_device_properties(0).multi_processor_count


def _ends(count, h):
    """The first h and the last h replicate indices of a kind with `count` items."""
    assert count >= 2 * h
    return [(0, h), (count - h, h)]


@pytest.mark.parametrize("normalise", [1, 0])
def test_panel_workgroups_cross_segment_kinds(normalise):
    """One launch of one-replicate segments whose kind -- wide counters (m = 33,334), five counter
    passes (m = 2, k = 20,000) or m = 200 -- is drawn per item, so a workgroup goes from any kind to
    any other with the counters, lap and sel of the item before.  Yardsticks that never cross kinds
    inside a workgroup: a single-segment call per kind (bit equality) and the oracle."""
    n = E.MIX_N
    X, Y = _panel(n)
    Xd, Yd = _dev(X, Y)
    kinds = list(E.MIX_KINDS)
    for (e1, e2, _), km in E.MIX_KINDS.items():
        assert R.geometry(n, e1, e2) == km
    items = _items()
    kind, rep = E.mix_items(items, len(kinds))
    segs = [kinds[q][:3] + (int(r), 1, i) for i, (q, r) in enumerate(zip(kind, rep))]
    st, got = _launch_panel(Xd, Yd, segs, items + 5, sentinel=SENTINEL, normalise=normalise)
    assert st == 0
    assert np.all(got[items:] == SENTINEL), "rows no segment names must keep the sentinel"
    for q, (e1, e2, seed) in enumerate(kinds):
        mine = got[:items][kind == q]
        count = len(mine)
        st, one = _launch_panel(Xd, Yd, [(e1, e2, seed, 0, count, 0)], count, normalise=normalise)
        assert st == 0
        assert np.array_equal(_bits(mine), _bits(one)), (e1, e2)
        for rb, h in _ends(count, 4):
            ref = R.oracle_records(_orc(), X, Y, e1, e2, seed, rb, h, normalise=bool(normalise))
            _check(mine[rb:rb + h], ref, n, e1, e2, seed, rb, f"mixed ({e1},{e2}) normalise={normalise} rep {rb}")


@pytest.mark.parametrize("normalise", [1, 0])
def test_table_workgroups_cross_pairs_and_eps(normalise):
    """The same for k_sign_table: twelve kinds (four column pairs x three eps pairs), so a workgroup
    reloads xa, yb and the four means for another pair between items.  Yardsticks: the panel entry
    on the kind's two columns (bit equality) and the oracle."""
    from dcor import signpanel
    D = E.edge_table()
    n = E.TABLE_N
    for (e1, e2), km in E.TABLE_EPS.items():
        assert R.geometry(n, e1, e2) == km
    kinds = [(a, b, e1, e2, 200 + 3 * j + i) for j, (a, b) in enumerate(E.TABLE_PAIRS)
             for i, (e1, e2) in enumerate(E.TABLE_EPS)]
    items = _items()
    kind, rep = E.mix_items(items, len(kinds))
    segs = [kinds[q] + (int(r), 1, i) for i, (q, r) in enumerate(zip(kind, rep))]
    got = _launch_table(D, segs, items + 5, ld=E.TABLE_LD, normalise=normalise, sentinel=SENTINEL)
    assert np.all(got[items:] == SENTINEL), "rows no segment names must keep the sentinel"
    for q, (a, b, e1, e2, seed) in enumerate(kinds):
        mine = got[:items][kind == q]
        count = len(mine)
        Xa, Yb = np.ascontiguousarray(D[:, a]), np.ascontiguousarray(D[:, b])
        one = signpanel.sweep_segments(Xa, Yb, [(e1, e2, seed, 0, count)], normalise=bool(normalise))
        assert np.array_equal(_bits(mine), _bits(one)), kinds[q]
        for rb, h in _ends(count, 2):
            ref = R.oracle_records(_orc(), Xa, Yb, e1, e2, seed, rb, h, normalise=bool(normalise))
            assert not np.isnan(ref).any()
            assert_close(mine[rb:rb + h], ref, what=f"table {kinds[q]} normalise={normalise} rep {rb}")
