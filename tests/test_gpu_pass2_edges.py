"""Pass 2's m = 8 loop at the batch counts where its peeled, 32-bit form can go wrong.

The loop runs steady trips (two batches per thread and two prefetched, all in range, nothing
guarded) and then at most two guarded trips.  A trip is 2 NT batches per wave set: 512 in the
workgroup kernels (NT = 256), 128 in the wave-per-replicate kernels (NT = 64).  Sign family,
Gaussian DGP, eps = (1, 1), so m = 8; every case against the oracle fed the same Philox streams
at tests/helpers.py's tolerances, through simulate() as test_fused_vs_oracle.

k = floor(n / 8) takes 1, 63, 64, 65, 255, 256, 257, 511, 512, 513, 767, 768, 769, 1024, 1537:
below one wave, below one workgroup, exactly 1, 1.5, 2 and 3 trips of 512 and one either side of
each; n = 8 k and n = 8 k + 5 (five records past the last batch, which only the INT sum reads).
All of these n are below the wave-per-replicate limit (SIGN_W_NMAX = 16384), and the engine has no
switch that sends such a cell through the workgroup kernels of simulate(): these cases run the wave
kernels' loop (the same source, NT = 64, where the same k are 0.5 to 12 trips of 128 and their
neighbours).  The workgroup kernel k_sign_pass2<DGP, true> is reached through public entries in
two ways: the cases above SIGN_W_NMAX (k = 2049 ... 2561: 4, 4.5 and 5 trips of 512 and their
neighbours), and dcor_diag_sign_ties, which runs its replicates in the workgroup kernels whatever
their n (the tie case below, k = 1537).
"""
import ctypes as C

import numpy as np
import pytest

from helpers import assert_close

pytestmark = pytest.mark.gpu

K_SMALL = [1, 63, 64, 65, 255, 256, 257, 511, 512, 513, 767, 768, 769, 1024, 1537]
K_WORKGROUP = [2049, 2303, 2304, 2305, 2559, 2560, 2561]     # n > SIGN_W_NMAX: NT = 256


@pytest.fixture(scope="module")
def dc():
    import torch
    assert torch.cuda.is_available()
    import dcor
    return dcor


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle
    return oracle


def m8_cell(n):
    from dcor.sim import CellSpec
    cell = CellSpec(n=n, rho=0.5, eps1=1.0, eps2=1.0, family="sign", dgp="gaussian", mu=(0.5, 0.5),
                    sigma=(2.0, 2.0), seed=1_000_000 + n % 97)
    return cell


def check_vs_oracle(dc, orc, k, tail, reps):
    from dcor.sim import simulate
    n = 8 * k + tail
    cell = m8_cell(n)
    assert dc.api.batch_geometry(n, 1.0, 1.0, "sign") == (k, 8)
    got = simulate(cell, reps, rep_begin=3).cpu().numpy()
    ref = orc.sim_reps(cell.to_c(), 3, 3 + reps)
    assert_close(got, ref, what=f"m = 8, k = {k}, n = {n}")


@pytest.mark.parametrize("tail", [0, 5])
@pytest.mark.parametrize("k", K_SMALL)
def test_m8_trip_edges_wave_kernels(dc, orc, k, tail):
    check_vs_oracle(dc, orc, k, tail, 12)


@pytest.mark.parametrize("tail", [0, 5])
@pytest.mark.parametrize("k", K_WORKGROUP)
def test_m8_trip_edges_workgroup_kernels(dc, orc, k, tail):
    assert 8 * k + tail > 16384      # the engine's SIGN_W_NMAX
    check_vs_oracle(dc, orc, k, tail, 8)


def test_m8_common_ties_against_peeled_loop(dc, orc):
    """Ties made common (DCOR_CODE_WINDOW=wide: about a third of the batches tie), k = 1537: the
    deferral queue fills inside the loop, so drain_if_full and the final drain both run beside the
    steady and the guarded trips.  Against the default window the INT columns are bit-equal (exact
    integer counts) and the NI columns differ at most in the order of their compensated T sums
    (1e-14): test_headline_wide_code_window's criterion; both against the oracle at 1e-12.  The tie
    batches are counted by dcor_diag_sign_ties, which runs the same replicates in the workgroup
    kernel k_sign_pass2<DGP, true>."""
    from dcor import _lib
    from dcor.sim import simulate
    k, R, r0 = 1537, 16, 5
    cell = m8_cell(8 * k)
    c = cell.to_c()

    def ties():
        t = np.zeros(R, dtype=np.int64)
        _lib.check(_lib.lib.dcor_diag_sign_ties(C.byref(c), r0, R, t.ctypes.data_as(C.POINTER(C.c_int64))))
        return t

    try:
        narrow, t_narrow = simulate(cell, R, r0).cpu().numpy(), ties()
        _lib.set_variant("DCOR_CODE_WINDOW", "wide")
        wide, t_wide = simulate(cell, R, r0).cpu().numpy(), ties()
    finally:
        _lib.set_variant("DCOR_CODE_WINDOW", None)
    print(f"tie batches per replicate of {k}: default window {t_narrow.tolist()}, wide {t_wide.tolist()}")
    assert np.array_equal(narrow[:, 3:].view(np.int64), wide[:, 3:].view(np.int64))
    assert_close(wide[:, :3], narrow[:, :3], rtol=1e-14, what="NI, wide vs default window")
    ref = orc.sim_reps(c, r0, r0 + R)
    assert_close(narrow, ref, what="k = 1537, default code window")
    assert_close(wide, ref, what="k = 1537, wide code window")
    assert t_wide.sum() > 0 and t_wide.max() <= k
