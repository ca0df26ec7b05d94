"""The accumulate kernels against the exact-rational reference of tests/accum_ref.py (DESIGN.md,
"Accumulators against an exact reference"): dcor_accumulate_launch on hand-made records at every
count where its work split changes, the 40 NaN / rho-position classes, infinite endpoints, order
invariance, and the accumulators and summaries the grid drivers return against the exact reference
of their own detail records."""
import ctypes as C
import math

import numpy as np
import pytest

import accum_ref as R

pytestmark = pytest.mark.gpu

RHOS = (0.0, 0.5, -1.0, 1.0)
# wave, workgroup-trip and block edges; 2^20 = 512 blocks of 2,048 records, one more: per = 2,049
COUNTS = (0, 1, 2, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 4097, 1 << 20, (1 << 20) + 1)
INF = float("inf")


@pytest.fixture(scope="module")
def dc():
    import torch
    assert torch.cuda.is_available()
    import dcor
    return dcor


def launch(rec, rho, count=None, null=False):
    """dcor_accumulate_launch on host records -> [NI, INT] accumulators (host copies)."""
    import torch
    from dcor import _lib
    from dcor.sim import accum_from_bytes
    rec = np.ascontiguousarray(rec, dtype=np.float64).reshape(-1, 6)
    count = rec.shape[0] if count is None else count
    dev = torch.as_tensor(rec if rec.shape[0] else np.zeros((1, 6)), device="cuda")
    acc = torch.full((2 * C.sizeof(_lib.Accum),), 0xA5, dtype=torch.uint8, device="cuda")
    _lib.check(_lib.lib.dcor_accumulate_launch(None if null else C.c_void_p(dev.data_ptr()), count, float(rho),
                                               C.c_void_p(acc.data_ptr()),
                                               C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    return accum_from_bytes(acc.cpu().numpy().tobytes())


_REF = {}


def reference(name, count, rho):
    """(records, [(exact accumulator, sum |term|) per method]) of a builder, computed once."""
    key = (name, count, rho)
    if key in _REF:
        return _REF[key]
    rec = R.BUILDERS[name](count, rho)
    out = (rec, [R.exact_accum_abs(rec, rho, m) for m in (0, 1)])
    if count <= 4097:       # the large ones are used once
        _REF[key] = out
    return out


def check(got, ref, count, what):
    for m in (0, 1):
        ex, sabs = ref[m]
        w = f"{what} method {m}"
        R.assert_counts(got[m], ex, w)
        R.assert_normalised(got[m], w)
        R.assert_sums(got[m], ex, sabs, max(count, 1024), w)


CASES = [(name, count, RHOS[(i + j) % 4]) for i, name in enumerate(R.BUILDERS) for j, count in enumerate(COUNTS)]


@pytest.mark.parametrize("name,count,rho", CASES)
def test_accumulate_launch_vs_exact(dc, name, count, rho):
    rec, ref = reference(name, count, rho)
    check(launch(rec, rho), ref, count, f"{name} count {count} rho {rho}")


@pytest.mark.parametrize("rho", RHOS)
def test_accumulate_launch_count_zero(dc, rho):
    """No records, with a null and with a non-null record pointer: every field zero."""
    for null in (True, False):
        got = launch(np.full((1, 6), 7.0), rho, count=0, null=null)
        for m in (0, 1):
            R.assert_counts(got[m], dict.fromkeys(("n",) + R.COUNTERS, 0), f"count 0 null {null}")
            assert all(R.stored(got[m], k) == (0.0, 0.0) for k in R.SUMS)


@pytest.mark.parametrize("r,rho", [(3, 0.5), (7, 0.0), (52, -1.0), (103, 1.0), (52, 0.5)])
def test_na_classes_counters_and_sums(dc, r, rho):
    """Every NaN pattern of (est, lo, hi) crossed with rho below lo, on lo, inside, on hi, above hi,
    in runs that straddle the wave edge (40 r = 120), the second trip of a workgroup (280) and the
    blocks (2,080: two of 1,040; 4,120: three of 1,374): the counters equal the class arithmetic
    of the truth table, the sums the exact reference."""
    rec = R.na_classes(rho, r)
    got = launch(rec, rho)
    for m in (0, 1):
        R.assert_counts(got[m], R.na_class_counts(rho, r, m), f"na_classes r {r} rho {rho} method {m}")
        R.assert_accum(got[m], rec, rho, m, f"na_classes r {r} rho {rho} method {m}")


def test_infinite_endpoints_counters(dc):
    """lo = -Inf, hi = +Inf or both, beside finite and NaN neighbours: R's rule fixes the counters
    (an infinity is not NA).  Only n and the counters are asserted: TwoSum of an infinity leaves
    NaN in the low word, and the engine never emits an infinite endpoint."""
    rho = 0.5
    rec = R.benign(600, rho)
    for meth, step in ((0, 3), (1, 5)):
        lo, hi = rec[:, 3 * meth + 1], rec[:, 3 * meth + 2]
        lo[0::step] = -INF
        hi[1::step] = INF
        lo[2::7], hi[2::7] = -INF, INF
        hi[4::11] = -INF          # rho <= -Inf is FALSE
    got = launch(rec, rho)
    for m in (0, 1):
        want = R.exact_counts(rec, rho, m)
        R.assert_counts(got[m], want, f"infinite endpoints method {m}")
        lo, hi = rec[:, 3 * m + 1], rec[:, 3 * m + 2]
        both = int(((lo == -INF) & (hi == INF)).sum())
        assert both > 50 and want["n_cover"] >= both
    one = launch(np.array([[0.0, -INF, INF, 0.0, INF, INF]]), rho)
    assert (one[0].n_cover, one[0].n_cover_na, one[0].n_na_ci) == (1, 0, 0)
    assert (one[1].n_cover, one[1].n_cover_na, one[1].n_na_ci) == (0, 0, 0)


@pytest.mark.parametrize("name", tuple(R.BUILDERS))
def test_order_invariance(dc, name):
    """The same records reversed and rotated by one block: the same counters, and sums within the
    same bound of the same exact values."""
    count = 4097
    rho = next(r for n, c, r in CASES if (n, c) == (name, count))    # shares that case's reference
    rec, ref = reference(name, count, rho)
    base = launch(rec, rho)
    for tag, perm in (("reversed", rec[::-1]), ("rotated", np.roll(rec, R.acc_per(count), axis=0))):
        got = launch(perm, rho)
        check(got, ref, count, f"{name} {tag}")
        for m in (0, 1):
            assert all(getattr(got[m], k) == getattr(base[m], k) for k in ("n",) + R.COUNTERS)


# ------------------------------------------------------------ through the drivers
B = 257


def _cells():
    from dcor.sim import CellSpec
    return [CellSpec(n=400, rho=0.3, eps1=0.5, eps2=0.5, family="sign", dgp="gaussian", mu=(0.5, 0.5),
                     sigma=(2.0, 2.0), seed=1_000_001),
            CellSpec(n=500, rho=0.5, eps1=1.0, eps2=1.0, family="subG", dgp="bounded_factor", seed=1_000_002),
            CellSpec(n=200, rho=0.0, eps1=0.2, eps2=0.2, family="sign", dgp="gaussian", seed=1_000_003)]  # k = 1


def _run(kind):
    from dcor import rstream
    from dcor.sim import run_grid
    cells = _cells()
    if kind == "grid":
        return cells, run_grid(cells, B, detail=True, devices=[0])
    if kind == "shards":
        return cells, run_grid(cells, B, detail=True, devices=[0, 0, 0])
    return cells, rstream.run_grid(cells, B, detail=True)


@pytest.mark.parametrize("kind", ("grid", "rstream", "shards"))
def test_drivers_vs_exact_reference_of_their_records(dc, kind):
    """run_grid on one device, the R-stream grid, and run_grid over three shards of one device: each
    cell's accumulators against the exact reference of the detail records the same call returned,
    its summary within the finalize bounds, and the tables' summary row equal to finalize's."""
    from dcor.tables import grid_summary
    cells, res = _run(kind)
    rows = grid_summary(cells, res)
    assert len(rows) == 2 * len(cells)
    for i, (c, r) in enumerate(zip(cells, res)):
        rec = np.asarray(r["records"], dtype=np.float64).reshape(-1, 6)
        assert rec.shape == (B, 6)
        for m, meth in enumerate(("NI", "INT")):
            what = f"{kind} cell {i} {meth}"
            R.assert_accum(r["accum"][m], rec, c.rho, m, what)
            s = r["summary"][meth]
            R.assert_summary(s, rec, c.rho, m, what)
            row = rows[m * len(cells) + i]
            assert (row["n"], row["rho_true"], row["method"]) == (float(c.n), float(c.rho), meth)
            for k_row, k_sum in (("mse", "mse"), ("bias", "bias"), ("coverage", "coverage"), ("ci_len", "ci_length")):
                a, b = row[k_row], s[k_sum]
                assert a == b or (math.isnan(a) and math.isnan(b)), (what, k_row, a, b)
    # the k = 1 cell: every NI CI is NA, the estimate is not (the pattern the engine itself makes)
    ni = res[2]["accum"][0]
    assert (ni.n, ni.n_na_ci, ni.n_cover_na, ni.n_cover, ni.n_na_est) == (B, B, B, 0, 0)
    assert math.isnan(res[2]["summary"]["NI"]["coverage"]) and math.isfinite(res[2]["summary"]["NI"]["mse"])
