"""The Gaussian DGP's slow-path draws, bit for bit: one replicate of n = 2^18 samples (2^19 ziggurat
normals, about 2,200 of them off the fast path) through dcor_dgp_launch against the oracle's gen_xy.

The oracle side first shows that the replicate exercises every branch of zig_slow.  Each normal's
attempt 0 is classified on the host (tests/zig_ref.py: the fast-path value x0 and whether it misses);
for a miss in a layer L >= 1 the oracle's orc_zig returns x0 exactly when the wedge test accepted
attempt 0 and another value when it rejected and drew again; a miss in layer 0 takes the base
layer's tail.  All three must occur.  Unit covariance factor (mu = 0, sigma = 1, rho = 0), so the
samples are the normals themselves up to the factor's arithmetic.
"""
import ctypes as C

import numpy as np
import pytest

import zig_ref

pytestmark = pytest.mark.gpu

N = 1 << 18
REP = 11
SEED = 1_000_033


def classify(orc, seed, rep, n, tab):
    zig = orc.lib.orc_zig
    zig.restype = C.c_double
    zig.argtypes = [C.c_uint64] + [C.c_uint32] * 5
    accept = reject = tail = 0
    for which, (A, H, x0, miss) in enumerate(zig_ref.attempt0(seed, rep, n, tab)):
        for i in np.flatnonzero(miss):
            if int(H[i]) >> 6 == 0:
                tail += 1
                continue
            z = zig(seed, int(i), which, rep, int(A[i]), int(H[i]))
            if z == x0[i]:
                accept += 1
            else:
                reject += 1
    return accept, reject, tail


def test_slow_path_draws_bitexact():
    import torch
    assert torch.cuda.is_available()
    from dcor import _lib
    from dcor.sim import CellSpec
    from oracle import oracle as orc
    tab = zig_ref.zig_tab()
    accept, reject, tail = classify(orc, SEED, REP, N, tab)
    print(f"slow normals of the replicate: {accept} wedge accepts, {reject} wedge rejects (retry), {tail} base-layer tails")
    assert accept > 0 and reject > 0 and tail > 0
    assert 1500 < accept + reject + tail < 3000
    cell = CellSpec(n=N, eps1=1.0, eps2=1.0, family="sign", seed=SEED, dgp="gaussian", rho=0.0,
                    mu=(0.0, 0.0), sigma=(1.0, 1.0))
    cs = cell.to_c()
    X = torch.empty((1, N), dtype=torch.float64, device="cuda")
    Y = torch.empty_like(X)
    _lib.check(_lib.lib.dcor_dgp_launch(C.byref(cs), REP, 1, C.c_void_p(X.data_ptr()), C.c_void_p(Y.data_ptr()), None))
    ox, oy = orc.gen_xy(cs, REP)
    gx, gy = X.cpu().numpy()[0], Y.cpu().numpy()[0]
    assert np.array_equal(gx.view(np.int64), ox.view(np.int64))
    assert np.array_equal(gy.view(np.int64), oy.view(np.int64))
