"""Tests of the pairwise table path's host helpers: dcor.hrs.valid_mask's bit order (no device) and
dcor.hrs.standardize_table(na=...), whose dp_sd / standardize_dp run on the device like every
estimator of the engine, so those two tests carry the gpu mark."""
import numpy as np
import pytest


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def test_valid_mask_bit_order_hand_written():
    """n = 70, p = 2: two words per column.  Column 0 misses rows 0, 5, 63 and 64; column 1 misses
    row 69 only.  Bit i & 63 of word i >> 6 is row i; the bits at i >= 70 are zero."""
    from dcor import hrs
    Z = np.zeros((70, 2))
    Z[[0, 5, 63, 64], 0] = np.nan
    Z[69, 1] = np.nan
    got = hrs.valid_mask(Z)
    assert got.dtype == np.uint64 and got.shape == (2, 2)
    want = [[0xFFFFFFFFFFFFFFFF & ~(1 << 0) & ~(1 << 5) & ~(1 << 63), 0b111110],
            [0xFFFFFFFFFFFFFFFF, 0b011111]]
    assert got.tolist() == want
    # a row-major and a column-major table give the same masks; inf is present
    Z[3, 1] = np.inf
    assert hrs.valid_mask(np.asfortranarray(Z)).tolist() == want
    assert hrs.valid_mask(np.zeros((64, 1))).tolist() == [[0xFFFFFFFFFFFFFFFF]]
    assert hrs.valid_mask(np.zeros((1, 3))).tolist() == [[1], [1], [1]]
    with pytest.raises(ValueError):
        hrs.valid_mask(np.zeros(8))


def _raw():
    from dcor import hrs
    age, bmi = hrs.standin_panel(501, -0.3, seed=5)
    third = 0.5 * age + 0.1 * bmi
    age[[7, 100]], bmi[[11, 100, 500]], third[0] = np.nan, np.nan, np.nan
    raw = np.stack([age, bmi, third], axis=1)
    bounds = [(hrs.AGE_LO, hrs.AGE_HI), (hrs.BMI_LO, hrs.BMI_HI), (20.0, 60.0)]
    lap = np.array([0.3, -0.2, 0.1, 0.4, -0.6, 0.05])
    return raw, bounds, lap


@pytest.mark.gpu
def test_standardize_table_pairwise_keeps_rows_and_equals_standardize_dp_per_column():
    from dcor import api, hrs
    raw, bounds, lap = _raw()
    t = hrs.standardize_table(raw, bounds, lap=lap, na="pairwise")
    assert t["Z"].shape == raw.shape and t["Z"].flags.f_contiguous
    assert np.array_equal(np.isnan(t["Z"]), np.isnan(raw))
    for c, (lo, hi) in enumerate(bounds):
        col = np.ascontiguousarray(raw[:, c])
        priv = api.dp_sd(col, lo, hi, hrs.EPS_MEAN, hrs.EPS_M2, lap=lap[2 * c:2 * c + 2])
        assert t["priv"][c] == priv
        assert np.array_equal(_bits(t["Z"][:, c]), _bits(api.standardize_dp(col, priv, lo, hi)))
        assert t["lam"][c] == api.lambda_from_priv(lo, hi, priv)
    # the masks of the kept table are the raw table's gaps
    assert hrs.valid_mask(t["Z"]).tolist() == hrs.valid_mask(raw).tolist()
    with pytest.raises(ValueError, match="na must be"):
        hrs.standardize_table(raw, bounds, lap=lap, na="rowwise")


@pytest.mark.gpu
def test_standardize_table_listwise_default_unchanged():
    """na='listwise' is the default: the same result as the call with the keyword omitted, which
    drops every row with a gap in any column; the pairwise table's complete rows are those rows."""
    from dcor import hrs
    raw, bounds, lap = _raw()
    want = hrs.standardize_table(raw, bounds, lap=lap)
    got = hrs.standardize_table(raw, bounds, lap=lap, na="listwise")
    ok = ~np.isnan(raw).any(axis=1)
    assert want["Z"].shape == (int(ok.sum()), 3) == (raw.shape[0] - 5, 3) and want["Z"].flags.f_contiguous
    assert np.array_equal(_bits(got["Z"]), _bits(want["Z"])) and got["Z"].flags.f_contiguous
    assert got["lam"].tolist() == want["lam"].tolist() and got["priv"] == want["priv"]
    pw = hrs.standardize_table(raw, bounds, lap=lap, na="pairwise")
    assert np.array_equal(_bits(pw["Z"][ok]), _bits(want["Z"]))
