"""GPU tests of the fused HRS sweep (dcor_hrs_fused_sweep_launch; mode='fused' of
hrs.sweep_segments / eps_sweep / dist.eps_sweep_distributed): every segment's records against the
per-segment entry, hrs_replicates(mode='fused') with that segment's eps, keys and rep_begin, bit
for bit."""
import ctypes as C
import math
import os
import socket

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SENTINEL = -7.25
# (eps, reps, rep_begin): m = 2; m = 8; m = 27 with no replicates; m > n (the k < 2 guard:
# k = 2, m = n // 2)
RAGGED = ((2.0, 37, 0), (1.05, 1, 1001), (0.55, 0, 5), (0.05, 11, 3))
# output rows out of segment order, rows 11 .. 12 and 51 .. 52 left over
RAGGED_ROWS = (13, 50, 7, 0)
RAGGED_TOTAL = 53


def _coded(n):
    from dcor import hrs
    age, bmi = hrs.standin_panel(n, -0.3, seed=5)
    return hrs.standardize_panel(age, bmi, lap=np.array([0.3, -0.2, 0.1, 0.4]))


def _continuous(n, seed=1):
    """A panel no dictionary codes: every value distinct (standardised normal draws)."""
    g = np.random.default_rng(seed)
    x = g.standard_normal(n)
    y = -0.3 * x + math.sqrt(1 - 0.09) * g.standard_normal(n)
    return {"age_z": x, "bmi_z": y, "lambda_age_z": 2.2, "lambda_bmi_z": 2.6}


def _args(z):
    return (z["age_z"], z["bmi_z"], z["lambda_age_z"], z["lambda_bmi_z"])


def _per_segment(z, eps, idx, reps, rb):
    """The reference: the existing per-segment fused path with the sweep's keys for eps index idx."""
    from dcor import hrs
    return hrs.hrs_replicates(*_args(z), eps, reps, seed_ni=10 + 1000 * idx, seed_int=20 + 1000 * idx,
                              rep_begin=rb, mode="fused")


class _Panel:
    """X, Y on the device and the prepared panel of one z, for direct C-ABI calls."""

    def __init__(self, z):
        import torch
        from dcor import _lib
        self.z = z
        self.X = torch.as_tensor(np.ascontiguousarray(z["age_z"], dtype=np.float64), device="cuda")
        self.Y = torch.as_tensor(np.ascontiguousarray(z["bmi_z"], dtype=np.float64), device="cuda")
        self.n = int(self.X.shape[0])
        self.sp = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        self.pn = C.c_void_p()
        _lib.check(_lib.lib.dcor_panel_create(C.c_void_p(self.X.data_ptr()), C.c_void_p(self.Y.data_ptr()),
                                              self.n, self.sp, C.byref(self.pn)))

    def base(self):
        from dcor import _lib
        z = self.z
        return _lib.PrematSubg(n=self.n, reps=0, eps1=1.0, eps2=1.0, eta1=1.0, eta2=1.0, alpha=0.05, hrs=1,
                               lam_x=z["lambda_age_z"], lam_y=z["lambda_bmi_z"], lam_s=z["lambda_age_z"],
                               lam_o=z["lambda_bmi_z"], lam_r=float("nan"), delta=1.0 / self.n, nsim=2000,
                               X=self.X.data_ptr(), Y=self.Y.data_ptr(), xy_stride=0)

    def sweep(self, segs, rows, total):
        """(status, out [total, 6]) of one dcor_hrs_fused_sweep_launch; segs: (eps, reps, rep_begin)
        with keys 10 / 20 + 1000 (position + 1); out pre-filled with SENTINEL."""
        import torch
        from dcor import _lib
        out = torch.full((total, 6), SENTINEL, dtype=torch.float64, device="cuda")
        arr = (_lib.HrsSegment * len(segs))(*[
            _lib.HrsSegment(eps=e, seed_ni=10 + 1000 * (i + 1), seed_int=20 + 1000 * (i + 1), rep_begin=rb,
                            reps=c, out_row=row) for i, ((e, c, rb), row) in enumerate(zip(segs, rows))])
        base = self.base()
        st = _lib.lib.dcor_hrs_fused_sweep_launch(C.byref(base), self.pn, arr, len(segs),
                                                  C.c_void_p(out.data_ptr()), self.sp)
        torch.cuda.synchronize()
        return st, out.cpu().numpy()

    def close(self):
        from dcor import _lib
        _lib.lib.dcor_panel_destroy(self.pn)


def _expected(z, segs, rows, total):
    want = np.full((total, 6), SENTINEL)
    for i, ((e, c, rb), row) in enumerate(zip(segs, rows)):
        if c:
            want[row:row + c] = _per_segment(z, e, i + 1, c, rb)
    return want


def _check_ragged(z, variants=None):
    from dcor import _lib
    want = _expected(z, RAGGED, RAGGED_ROWS, RAGGED_TOTAL)
    assert np.isfinite(want).all()
    p = _Panel(z)
    try:
        with _lib.variants(**(variants or {})):
            st, got = p.sweep(RAGGED, RAGGED_ROWS, RAGGED_TOTAL)
    finally:
        p.close()
    assert st == _lib.DCOR_OK, _lib.last_error()
    np.testing.assert_array_equal(got.view(np.int64), want.view(np.int64))
    gap = np.ones(RAGGED_TOTAL, dtype=bool)
    for (e, c, rb), row in zip(RAGGED, RAGGED_ROWS):
        gap[row:row + c] = False
    assert gap.sum() == 4 and (got[gap] == SENTINEL).all()


@pytest.mark.parametrize("n", [2501, 2500])
def test_ragged_sweep_coded_panel(n):
    """m = 2, m = 8, an empty segment and the k < 2 guard in one call, odd and even n, replicate
    offsets, permuted output rows with gaps that keep their sentinel."""
    from dcor import api
    assert api.batch_geometry(n, 0.05, 0.05, "subG", hrs=True) == (2, n // 2)
    assert api.batch_geometry(n, 2.0, 2.0, "subG", hrs=True)[1] == 2
    _check_ragged(_coded(n))


@pytest.mark.parametrize("n", [3001, 3000])
def test_ragged_sweep_continuous_panel(n):
    """The uncoded kernel (k_hrs_sweep_fused_l2): the same segment list against the per-segment
    fused calls, which test_gpu_hrs pins to the oracle."""
    _check_ragged(_continuous(n))


def test_l2_kernel_equals_coded_kernel_on_coded_panel():
    """DCOR_HRS_FUSED_L2=1: the coded panel through the uncoded sweep kernel, the same bits (the
    reference is computed on the coded path)."""
    _check_ragged(_coded(2501), variants=dict(DCOR_HRS_FUSED_L2="1"))


@pytest.fixture(scope="module")
def full_grid_reference():
    from dcor import hrs
    z = _coded(2501)
    return z, np.stack([_per_segment(z, e, i, 60, 0) for i, e in enumerate(hrs.EPS_GRID, start=1)])


@pytest.mark.parametrize("wpe", [None, "4"])
def test_workgroups_cross_segments(full_grid_reference, wpe):
    """23 eps x 60 runs = 1380 replicates: more than the 1024 resident 512-thread workgroups of a
    256-CU device, so the persistent loop wraps and workgroups move from one segment to another."""
    from dcor import _lib, hrs
    z, want = full_grid_reference
    segs = [(e, 0, 60) for e in range(len(hrs.EPS_GRID))]
    with _lib.variants(**({"DCOR_HRS_WPE": wpe} if wpe else {})):
        got = hrs.sweep_segments(*_args(z), hrs.EPS_GRID, segs, mode="fused")
    np.testing.assert_array_equal(got.view(np.int64), want.reshape(-1, 6).view(np.int64))


@pytest.mark.parametrize("kind", ["coded", "continuous"])
def test_survey_geometry(kind):
    """n = 19,433 (39 KB of LDS codes per workgroup), m = 2 and m = 128."""
    from dcor import hrs
    z = _coded(19433) if kind == "coded" else _continuous(19433)
    grid = (2.0, 0.25)
    got = hrs.sweep_segments(*_args(z), grid, [(0, 0, 4), (1, 0, 4)], mode="fused")
    want = np.concatenate([_per_segment(z, e, i, 4, 0) for i, e in enumerate(grid, start=1)])
    np.testing.assert_array_equal(got.view(np.int64), want.view(np.int64))


def test_validates_every_segment_first():
    """A bad last segment (eps = 0) or a bad base: DCOR_EINVAL and d_out unchanged; all-empty
    segments: DCOR_OK and d_out unchanged."""
    import torch
    from dcor import _lib
    p = _Panel(_coded(2501))
    try:
        st, out = p.sweep(((2.0, 4, 0), (0.0, 4, 0)), (0, 4), 8)
        assert st == _lib.DCOR_EINVAL and (out == SENTINEL).all()
        st, out = p.sweep(((2.0, 4, 0), (1.0, 4, 2**32 - 2)), (0, 4), 8)
        assert st == _lib.DCOR_EINVAL and (out == SENTINEL).all()
        st, out = p.sweep(((2.0, 0, 0), (1.0, 0, 3)), (0, 4), 8)
        assert st == _lib.DCOR_OK and (out == SENTINEL).all()
        out = torch.full((4, 6), SENTINEL, dtype=torch.float64, device="cuda")
        arr = (_lib.HrsSegment * 1)(_lib.HrsSegment(eps=2.0, seed_ni=1, seed_int=2, rep_begin=0, reps=4, out_row=0))
        for field, value in (("n", p.n - 1), ("nsim", 0), ("delta", 0.0), ("hrs", 0)):
            other = p.base()
            setattr(other, field, value)
            st = _lib.lib.dcor_hrs_fused_sweep_launch(C.byref(other), p.pn, arr, 1, C.c_void_p(out.data_ptr()), p.sp)
            assert st == _lib.DCOR_EINVAL, field
        torch.cuda.synchronize()
        assert bool((out == SENTINEL).all())
    finally:
        p.close()


def test_large_uncoded_panel_runs_per_segment():
    """n = 65,537 with no dictionary has no fused kernel: the segments go one by one through the
    per-segment entry's materialised path."""
    from dcor import hrs
    z = _continuous(65537, seed=3)
    grid = (2.0, 0.75)
    got = hrs.sweep_segments(*_args(z), grid, [(0, 1, 2), (1, 0, 2)], mode="fused")
    want = np.concatenate([_per_segment(z, 2.0, 1, 2, 1), _per_segment(z, 0.75, 2, 2, 0)])
    np.testing.assert_array_equal(got.view(np.int64), want.view(np.int64))


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_python_surface():
    """eps_sweep(mode='fused'): runs equal the per-eps fused calls stacked, summaries equal
    sweep_summaries of them; eps_sweep_distributed(mode='fused') at world size 1 equals it."""
    import torch.distributed as dist
    from dcor import hrs
    from dcor.dist import eps_sweep_distributed
    z = _coded(2501)
    sw = hrs.eps_sweep(*_args(z), reps=5, mode="fused")
    one = np.stack([_per_segment(z, e, i, 5, 0) for i, e in enumerate(hrs.EPS_GRID, start=1)])
    np.testing.assert_array_equal(sw["runs"].view(np.int64), one.view(np.int64))
    ref = hrs.sweep_summaries(hrs.EPS_GRID, one)
    np.testing.assert_equal(sw["ni_mean"], ref["ni_mean"])
    np.testing.assert_equal(sw["int_mean"], ref["int_mean"])
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()))
    dist.init_process_group("gloo", rank=0, world_size=1)
    try:
        ds = eps_sweep_distributed(*_args(z), reps=5, mode="fused")
    finally:
        dist.destroy_process_group()
    assert ds["runs"].tobytes() == sw["runs"].tobytes()
    np.testing.assert_equal(ds["ni_mean"], sw["ni_mean"])
    np.testing.assert_equal(ds["int_mean"], sw["int_mean"])


def test_warm_second_call_allocates_like_the_per_segment_entry():
    """A second identical call adds to dcor_alloc_count() no more than the first did, and exactly
    what a warm dcor_hrs_fused_launch adds: its one stream-ordered scratch buffer."""
    import torch
    from dcor import _lib
    p = _Panel(_coded(2501))
    try:
        segs, rows = ((2.0, 6, 0), (0.55, 3, 2)), (0, 6)
        counts = [_lib.lib.dcor_alloc_count()]
        outs = []
        for _ in range(2):
            st, out = p.sweep(segs, rows, 9)
            assert st == _lib.DCOR_OK
            outs.append(out)
            counts.append(_lib.lib.dcor_alloc_count())
        first, second = counts[1] - counts[0], counts[2] - counts[1]
        np.testing.assert_array_equal(outs[0].view(np.int64), outs[1].view(np.int64))
        d = p.base()
        d.reps, d.eps1, d.eps2 = 6, 2.0, 2.0
        d.lam_r = float("nan")
        rec = torch.empty((6, 6), dtype=torch.float64, device="cuda")
        per = []
        for _ in range(2):
            c0 = _lib.lib.dcor_alloc_count()
            _lib.check(_lib.lib.dcor_hrs_fused_launch(C.byref(d), p.pn, 1010, 1020, 0, C.c_void_p(rec.data_ptr()), p.sp))
            torch.cuda.synchronize()
            per.append(_lib.lib.dcor_alloc_count() - c0)
        assert second <= first and second == per[1]
    finally:
        p.close()
