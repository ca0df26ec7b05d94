"""Pass 1's Gaussian workgroup loop at the group counts where its peeled, 32-bit form can go wrong.

The loop of sign_pass1_core (workgroup form, NT = 256) runs steady trips of 2 NT = 512 four-sample
groups while the whole trip lies below G = floor(n / 4) -- nothing guarded, the slow samples' pend
bits shifted into a register that is decoded every four trips -- then at most one guarded trip, then
the n % 4 group.  Headline family (sign, Gaussian, eps = (1, 1)) at n just above the
wave-per-replicate limit (SIGN_W_NMAX = 16384) so that simulate() runs the workgroup kernels; every
replicate against the oracle fed the same Philox streams, at tests/helpers.py's tolerances.

G takes: a multiple of 512 and one either side (4607, 4608, 4609); a multiple + 255, + 256, + 257
(the guarded trip's second group: 4863, 4864, 4865); 8 steady trips and one group (4097), 9, 10 and
12 steady trips (4608, 5120, 6144: a trip count that is and is not a multiple of 4, so the partial
quad word of pend bits is empty, one, two and three bytes); one group short of 12 trips and one past
(6143, 6145); and each n % 4 in {0, 1, 2, 3}.

Each case also counts, on the CPU, the samples of its replicates whose ziggurat normals miss the fast
path (about 0.85 %: some 140 to 210 per replicate here) and asserts there are some: those samples'
records and sums are rewritten by the in-kernel regeneration that the pend bits feed.
"""
import numpy as np
import pytest

import zig_ref
from helpers import assert_close

pytestmark = pytest.mark.gpu

# (G, n % 4)
CASES = [(4097, 0), (4607, 1), (4608, 0), (4608, 3), (4609, 2), (4863, 1), (4864, 0), (4865, 3),
         (5120, 2), (6143, 3), (6144, 0), (6145, 1), (6400, 2)]
REPS = 6
REP0 = 3


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


@pytest.fixture(scope="module")
def zig_tab():
    return zig_ref.zig_tab()


@pytest.mark.parametrize("G,tail", CASES)
def test_pass1_trip_edges_workgroup_kernels(dc, orc, zig_tab, G, tail):
    from dcor.sim import CellSpec, simulate
    n = 4 * G + tail
    assert n > 16384      # the engine's SIGN_W_NMAX: the workgroup kernels run
    cell = CellSpec(n=n, rho=0.5, eps1=1.0, eps2=1.0, family="sign", dgp="gaussian", mu=(0.5, 0.5),
                    sigma=(2.0, 2.0), seed=1_000_000 + n % 89)
    assert dc.api.batch_geometry(n, 1.0, 1.0, "sign")[1] == 8
    slow = [zig_ref.slow_samples(cell.seed, REP0 + r, n, zig_tab) for r in range(REPS)]
    print(f"G = {G}, n = {n}: slow samples per replicate {slow}")
    assert min(slow) > 0
    got = simulate(cell, REPS, rep_begin=REP0).cpu().numpy()
    ref = orc.sim_reps(cell.to_c(), REP0, REP0 + REPS)
    assert_close(got, ref, what=f"pass 1, G = {G}, n = {n}")
