"""CPU pins of the inputs of tests/test_gpu_sign_edges.py: every shape's (k, m) as
sign_panel_ref.geometry gives it, the NaN pattern of the oracle's records on it (the NI interval NaN
exactly when k = 1, everything else finite), the exact batch counts of the packing-boundary panels,
and the conditioned NI bound's arithmetic.  The GPU file reads its shapes from the same tables, so
it cannot quietly test something else."""
import math

import numpy as np
import pytest

import helpers
import sign_edges_ref as E
import sign_panel_ref as R


def _orc():
    import oracle.oracle as orc
    return orc


def _check_pattern(ref, k, what):
    assert ref.shape == (E.EDGE_REPS, 6), what
    nan = np.isnan(ref)
    want = np.zeros_like(nan)
    want[:, 1:3] = (k == 1)
    assert np.array_equal(nan, want), (what, ref)


ORACLE_SHAPES = {**E.WIDE_SHAPES, **E.BATCH_SHAPES,
                 **{(E.MIX_N, e1, e2): km for (e1, e2, _), km in E.MIX_KINDS.items()}}


@pytest.mark.parametrize("shape", list(ORACLE_SHAPES), ids=lambda s: f"{s[0]}-{s[1]:.6g}-{s[2]:.6g}")
def test_geometry_and_oracle_nan_pattern(shape):
    n, eps1, eps2 = shape
    k, m = ORACLE_SHAPES[shape]
    assert R.geometry(n, eps1, eps2) == (k, m)
    assert k * m <= n < (k + 1) * m
    X, Y = E.edge_panel(n, seed=n)
    for normalise, rep_begin in ((True, 0), (False, 1001)):
        ref = R.oracle_records(_orc(), X, Y, eps1, eps2, E.EDGE_SEED, rep_begin, E.EDGE_REPS, normalise=normalise)
        _check_pattern(ref, k, (shape, normalise))


def test_wide_and_mixed_shapes_lie_where_the_kernel_branches():
    """The constants the shapes are chosen around: one-word counters up to m = 32,767, 4,096 (2,048
    two-word) batches per pass, 1,024 samples per trip of a workgroup's sample loop."""
    for (n, e1, e2), (k, m) in E.WIDE_SHAPES.items():
        assert m > 32_767 and k <= 2048
    ks = sorted(k for k, m in E.BATCH_SHAPES.values())
    assert {4096, 4097, 8192, 8193} <= set(ks)
    ms = {m for k, m in E.BATCH_SHAPES.values()}
    assert {1, 3, 4, 5, 1024, 1025, 3200} <= ms
    (kw, mw), (kp, mp), (k2, m2) = E.MIX_KINDS.values()
    assert mw > 32_767 and kw == 1 and (kp, mp) == (20_000, 2) and (k2, m2) == (200, 200)
    assert divmod(kp, 4096) == (4, 3616)   # five counter passes: four full ones and 3,616 batches


@pytest.mark.parametrize("shape", list(E.PACK_SHAPES), ids=lambda s: str(s[0]))
def test_packing_boundary_panels(shape):
    n, eps1, eps2 = shape
    k, m = E.PACK_SHAPES[shape]
    assert R.geometry(n, eps1, eps2) == (k, m)
    assert m in (32_767, 32_768) and n - k * m == (0 if k == 1 else 1)
    orc = _orc()
    for kind in E.PACK_PANELS:
        X, Y = E.pack_panel(n, m, kind)
        cx, cy = E.pack_counts(X, Y, k, m)
        if kind == "half":
            assert np.all(cx == m // 2 - (m - m // 2)) and np.all(cy == -cx)
        else:
            sx, sy = (1 if c == "+" else -1 for c in kind)
            assert np.all(cx == sx * m) and np.all(cy == sy * m)   # exactly +-m in every batch
        ref = R.oracle_records(orc, X, Y, eps1, eps2, E.EDGE_SEED, 0, E.EDGE_REPS, normalise=False)
        _check_pattern(ref, k, (shape, kind))
    X, Y = E.edge_panel(n, seed=n)
    ref = R.oracle_records(orc, X, Y, eps1, eps2, E.EDGE_SEED, 1001, E.EDGE_REPS, normalise=True)
    _check_pattern(ref, k, (shape, "random"))


def test_table_shapes():
    D = E.edge_table()
    assert D.shape == (E.TABLE_N, E.TABLE_P) and E.TABLE_LD > E.TABLE_N
    orc = _orc()
    for (e1, e2), (k, m) in E.TABLE_EPS.items():
        assert R.geometry(E.TABLE_N, e1, e2) == (k, m)
    for a, b in E.TABLE_PAIRS:
        ref = R.oracle_records(orc, np.ascontiguousarray(D[:, a]), np.ascontiguousarray(D[:, b]), 0.2, 0.2,
                               E.EDGE_SEED, 0, E.EDGE_REPS)
        _check_pattern(ref, 5, (a, b))


def test_mix_items_are_not_periodic_and_count_their_kind():
    kinds, reps = E.mix_items(6144, 3)
    assert np.array_equal(kinds, E.mix_items(6144, 3)[0])
    for q in range(3):
        assert np.array_equal(reps[kinds == q], np.arange(np.sum(kinds == q)))
        assert np.sum(kinds == q) > 1800
    for period in range(1, 65):   # no short period a grid stride could align with
        assert not np.array_equal(kinds[period:], kinds[:-period])


def test_ni_T_bound_and_conditioned_assert():
    orc = _orc()
    n, eps1, eps2 = 70_001, 0.02, 0.012
    k, m = R.geometry(n, eps1, eps2)
    b = E.ni_T_bound(orc, n, eps1, eps2, E.EDGE_SEED, 1)
    bl = orc.gen_laplace(E.EDGE_SEED, 1, R.SITE_NI_LAP, 2 * k)
    want = max(m * (1 + 2 / (m * eps1) * abs(bl[2 * j])) * (1 + 2 / (m * eps2) * abs(bl[2 * j + 1])) for j in range(k))
    assert b >= m and abs(b - want) <= 1e-12 * want
    # the bound dominates |T_j| whatever the batch means in [-1, 1] are (equal, up to this line's
    # own rounding, where both means are +-1 with the draws' signs)
    for sx, sy in ((1.0, 1.0), (-1.0, 1.0), (0.25, -0.5)):
        T = m * (sx + 2 / (m * eps1) * bl[0::2]) * (sy + 2 / (m * eps2) * bl[1::2])
        assert np.all(np.abs(T) <= b * (1 + 4 * 2.0 ** -52))
    # the assert: INT at helpers' bound, NI at the conditioned one, NaN patterns identical
    tol = (math.pi / 2) * 64 * 2.0 ** -53 * b
    assert tol > helpers.ATOL + helpers.RTOL   # the conditioned term is the larger one at this m
    ref = np.array([[0.25, -0.5, 0.75, 0.1, 0.0, 0.2]])
    E.assert_close_ni_conditioned(ref.copy(), ref, b, "same")
    ok = ref.copy()
    ok[0, :3] += 0.9 * tol
    E.assert_close_ni_conditioned(ok, ref, b, "inside")
    for col, d in ((0, 1.1 * tol), (2, -1.1 * tol), (3, 1e-11), (5, 1e-11)):
        bad = ref.copy()
        bad[0, col] += d
        with pytest.raises(AssertionError):
            E.assert_close_ni_conditioned(bad, ref, b, "outside")
    nan = ref.copy()
    nan[0, 1] = np.nan
    with pytest.raises(AssertionError):
        E.assert_close_ni_conditioned(nan, ref, b, "nan")
    E.assert_close_ni_conditioned(nan, nan.copy(), b, "both nan")
    # one bound per row
    two = np.vstack([ref, ref])
    off = two.copy()
    off[1, 0] += 0.9 * tol
    E.assert_close_ni_conditioned(off, two, np.array([b, b]), "rows")
    with pytest.raises(AssertionError):
        E.assert_close_ni_conditioned(off, two, np.array([b, b / 2]), "rows")
