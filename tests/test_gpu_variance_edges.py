"""GPU tests of the one-pass sample variance (dd_var, csrc/dcor_device.h) at its edge, through the
pre-materialised entries, whose contract is the reference's numbers on the caller's arrays:
dcor_premat_subg_launch with hrs = 0 and hrs = 1 and dcor_premat_sign_launch, on hand-made inputs
with all-zero Laplace noise and clips that do not bind.

The kernels round each square before it enters the compensated sum of squares, so on a constant the
numerator of the variance is rounding residue n (fl(c^2) - c^2) of either sign where R's two-pass
var (orc_r_var) gives 0.  A negative residue under the square root made every CI endpoint of the
family NaN; a positive one left an sd of about 1e-9, which with hrs = 1 misses the reference's
sd == 0 branch (real-data-sims.R:237-238).  dd_var now recognises the sums of a constant sample
exactly (variance 0) and returns 0 for a negative value.  On nearly constant data the residue stays,
within the bound of tests/ddvar_ref.py:  |sd_kernel - sd_exact| <= sqrt B,
B = 4 * 2^-53 * sum T^2 / (k - 1), so an NI endpoint may sit crit * sqrt B / sqrt k from the
reference's (a derived allowance, not a measured one); everything else is held to
helpers.assert_close."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import ddvar_ref as V
from helpers import ATOL, RTOL, assert_close, unit_laplace

pytestmark = pytest.mark.gpu

W_NMAX = 16384   # SUBG_W_NMAX (csrc/dcor_engine.h)
NS = [1001, W_NMAX + 5]
CONSTANTS = [0.3, 0.7, 1.1, 1.7, 2.0 / 3.0]
EPS = (1.0, 1.0)   # m = 8: k = 125 and 2,048
NSIM = 1000
LAM = 5.0          # the hrs = 1 clips: above every |x| used here; lam_r = 50 above every |x y|
LAM_R = 50.0


def _orc():
    import oracle.oracle as orc
    return orc


@functools.lru_cache(maxsize=None)
def _mix():
    """Benign mixquant draws: no NaN, no zero in l (c* = inf gives +-inf keys, never inf * 0)."""
    g = np.random.default_rng(20261021)
    z, l = g.standard_normal(NSIM), unit_laplace(g, NSIM)
    assert np.all(l != 0.0)
    return z, l


def _geometry(n, hrs):
    m = math.ceil(8.0 / (EPS[0] * EPS[1]))
    k = n // m
    assert k >= 3
    return k, m


def _perm(n, hrs):
    k, m = _geometry(n, hrs)
    return np.random.default_rng(n).permutation(n)[:k * m].astype(np.int32) if hrs else None


def _t(a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a), device="cuda")


def _subg_gpu(X, Y, hrs):
    """One replicate of dcor_premat_subg_launch on (X, Y) with zero Laplace noise."""
    import torch
    from dcor import _lib
    n = len(X)
    k, m = _geometry(n, hrs)
    z, l = _mix()
    perm = _perm(n, hrs)
    nan = float("nan")
    T = dict(X=_t(X), Y=_t(Y), lx=_t(np.zeros(k)), ly=_t(np.zeros(k)), ll=_t(np.zeros(n)), lc=_t(np.zeros(1)),
             mz=_t(z), ml=_t(l))
    if hrs:
        T["perm"] = _t(perm)
    lam = LAM if hrs else nan
    d = _lib.PrematSubg(n=n, reps=1, eps1=EPS[0], eps2=EPS[1], eta1=1.0, eta2=1.0, alpha=0.05, hrs=hrs,
                        lam_x=lam, lam_y=lam, lam_s=lam, lam_o=lam, lam_r=LAM_R if hrs else nan, delta=nan,
                        nsim=NSIM, X=T["X"].data_ptr(), Y=T["Y"].data_ptr(), xy_stride=0,
                        perm=T["perm"].data_ptr() if hrs else None, lap_ni_x=T["lx"].data_ptr(),
                        lap_ni_y=T["ly"].data_ptr(), lap_local=T["ll"].data_ptr(), lap_central=T["lc"].data_ptr(),
                        mix_z=T["mz"].data_ptr(), mix_l=T["ml"].data_ptr())
    out = torch.full((1, 6), -7.0, dtype=torch.float64, device="cuda")
    _lib.check(_lib.lib.dcor_premat_subg_launch(C.byref(d), C.c_void_p(out.data_ptr()),
                                                C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    return out.cpu().numpy()[0]


def _subg_ref(X, Y, hrs):
    """(the reference's six numbers, the T values of oracle/dcor_oracle.c's orc_ni_subg recomputed
    in double: rowMeans in long double, T[j] = m * xt * yt with zero noise)."""
    orc = _orc()
    n = len(X)
    k, m = _geometry(n, hrs)
    z, l = _mix()
    perm = _perm(n, hrs)
    lam = LAM if hrs else np.nan
    st, ni, km = orc.ni_subg(X, Y, *EPS, hrs=hrs, lam_x=lam, lam_y=lam, perm=perm, lap_x=np.zeros(k),
                             lap_y=np.zeros(k))
    assert st == 0 and (int(km[0]), int(km[1])) == (k, m)
    st, it, lams = orc.int_subg(X, Y, *EPS, hrs=hrs, lam_s=lam, lam_o=lam, lam_r=LAM_R if hrs else np.nan,
                                lap_local=np.zeros(n), lap_central=0.0, mix_z=z, mix_l=l)
    assert st == 0
    # the clips do not bind
    lx = LAM if hrs else orc.lambda_n(n, 1.0)
    assert max(np.abs(X).max(), np.abs(Y).max()) < min(lx, lams[0]) and np.abs(X * Y).max() < lams[2]
    idx = perm if hrs else np.arange(k * m)
    xb = (X[idx].astype(np.longdouble).reshape(k, m).sum(axis=1) / np.longdouble(m)).astype(np.float64)
    yb = (Y[idx].astype(np.longdouble).reshape(k, m).sum(axis=1) / np.longdouble(m)).astype(np.float64)
    return np.concatenate([ni, it]), float(m) * xb * yb


def _int_allowance(Uc, hrs):
    """What sqrt B of the Uc values (no clip binds, zero noise: Uc = x y) lets an unclamped INT endpoint
    move.  width = q(c*) f(sd) / sqrt n with c* = a / sd, q the mixquant of z + c* l, and f = sqrt(sd^2 +
    2 sn^2) (hrs = 0) or sd (hrs = 1).  With |d sd| <= sqrt B:  |d c*| <= c* sqrt B / (sd - sqrt B),
    |d q| <= max |l| |d c*| (an order statistic of z + c l moves no faster in c than its steepest
    member) and |d f| <= sqrt B, so  |d width| <= (|d q| (f + sqrt B) + |q| sqrt B) / sqrt n.
    Every term comes from the reference's quantities."""
    orc = _orc()
    n = len(Uc)
    z, l = _mix()
    sd, sb = math.sqrt(float(V.exact_var(list(Uc)))), V.sd_bound(list(Uc))
    assert sd > 2.0 * sb
    eps_r = min(EPS)
    lr = LAM_R if hrs else orc.lambda_int_n(n, 1.0, 1.0, max(EPS))[1]
    cstar = (2.0 * lr if hrs else 2.0) / (math.sqrt(n) * sd * eps_r)
    f = sd if hrs else math.sqrt(sd * sd + 2.0 * (2.0 * lr / (n * eps_r)) ** 2)
    q = orc.mixquant(z, l, cstar, 0.975)
    dq = np.abs(l).max() * cstar * sb / (sd - sb)
    return (dq * (f + sb) + abs(q) * sb) / math.sqrt(n)


def _check(got, ref, T, what, crit_scale=1.0, plain=False, int_allow=0.0):
    """The NaN and Inf pattern and everything but the NI endpoints under assert_close (the INT
    endpoints within int_allow where one is given: _int_allowance); the NI endpoints within
    max(assert_close's bound, crit * sqrt B / sqrt k) -- plain: assert_close on everything too."""
    k = len(T)
    allow = crit_scale * _orc().qnorm(0.975) * V.sd_bound(T) / math.sqrt(k)
    dev = np.abs(got[1:3] - ref[1:3])
    print(f"{what}: got {got!r}\n  ref {ref!r}\n  NI endpoint deviation {dev.max():.3e} "
          f"(relative {np.max(dev / np.abs(ref[1:3])):.3e}), crit sqrt(B / k) {allow:.3e}")
    assert np.array_equal(np.isnan(got), np.isnan(ref)), f"{what}: NaN pattern\n got {got!r}\n ref {ref!r}"
    assert np.array_equal(np.isinf(got), np.isinf(ref)), what
    assert_close(got[[0, 3]], ref[[0, 3]], what=what + " (estimates)")
    idev = np.abs(got[4:6] - ref[4:6])
    ibound = np.maximum(ATOL + RTOL * np.maximum(np.abs(got[4:6]), np.abs(ref[4:6])), int_allow)
    print(f"  INT endpoint deviation {idev.max():.3e}, allowance {int_allow:.3e}")
    assert np.all((idev <= ibound) | (got[4:6] == ref[4:6])), \
        f"{what}: INT endpoints got {got[4:6]!r} ref {ref[4:6]!r} off by {idev!r}, allowed {ibound!r}"
    bound = np.maximum(ATOL + RTOL * np.maximum(np.abs(got[1:3]), np.abs(ref[1:3])), allow)
    assert np.all(dev <= bound), f"{what}: NI endpoints off by {dev!r}, allowed {bound!r}"
    if plain:
        assert_close(got, ref, what=what)
    return dev.max()


# ---------------------------------------------------------------- sub-G entries
@pytest.mark.parametrize("hrs", [0, 1])
@pytest.mark.parametrize("n", NS)
def test_subg_constant_columns(n, hrs):
    """X = Y = c and X = c, Y = -c: var(T) = var(Uc) = 0 in the reference, so its NI endpoints equal
    the estimate and its INT interval is [-1, 1] (hrs = 0: c* infinite) or the sd == 0 width
    (hrs = 1, real-data-sims.R:237-238).

    Before dd_var treated these sums, c = 0.7 and c = 1.1 (negative residue) gave NaN endpoints at
    both n, with either sign of Y and either hrs, as did the sign entry on the constant
    T = 11 fl(1/11) fl(3/11); with the negative residue clamped only, c = 0.3, 1.7 and 2/3 (positive
    residue) still missed the hrs = 1 reference: sd(Uc) about 1e-9, the mixquant branch instead of
    sd == 0, INT endpoints off by 0.040 (n = 1,001) and 0.0025 (n = 16,389)."""
    worst, failed = 0.0, []
    for c in CONSTANTS:
        for sy in (1.0, -1.0):
            X, Y = np.full(n, c), np.full(n, sy * c)
            ref, T = _subg_ref(X, Y, hrs)
            assert ref[1] == ref[0] == ref[2] or abs(ref[0]) > 1.0   # the reference's variance is 0
            assert not np.isnan(ref).any()
            try:   # every constant is run; the failures are reported together
                worst = max(worst, _check(_subg_gpu(X, Y, hrs), ref, T, f"n={n} hrs={hrs} c={c} Y={sy:+.0f}c"))
            except AssertionError as e:
                failed.append(str(e))
    print(f"n={n} hrs={hrs}: worst NI endpoint deviation on constants {worst:.3e}")
    assert not failed, f"{len(failed)} of {2 * len(CONSTANTS)} constant inputs:\n" + "\n".join(failed)


@pytest.mark.parametrize("hrs", [0, 1])
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("cv", [1e-3, 1e-5])
def test_subg_nearly_constant_columns(cv, n, hrs):
    g = np.random.default_rng(20261021)
    X = 1.3 * (1.0 + cv * g.standard_normal(n))
    Y = 0.9 * (1.0 + cv * g.standard_normal(n))
    ref, T = _subg_ref(X, Y, hrs)
    _check(_subg_gpu(X, Y, hrs), ref, T, f"n={n} hrs={hrs} cv={cv}", plain=cv == 1e-3,
           int_allow=_int_allowance(X * Y, hrs))


@pytest.mark.parametrize("hrs", [0, 1])
@pytest.mark.parametrize("n", NS)
def test_subg_cancelling_sums(n, hrs):
    """The sender alternates +v, -v against a constant receiver, the odd last row is 0: the sum of
    Uc is 0 exactly while the sum of its squares is (n - 1) (1.7 * 0.9)^2."""
    X = 1.7 * (1.0 - 2.0 * (np.arange(n) % 2))
    X[-1] = 0.0
    Y = np.full(n, 0.9)
    ref, T = _subg_ref(X, Y, hrs)
    _check(_subg_gpu(X, Y, hrs), ref, T, f"n={n} hrs={hrs} cancelling", plain=True)


# ---------------------------------------------------------------- sign entry
SIGN_EPS = (0.5, 1.5)   # m = 11: batch means of signs are multiples of 1 / 11, not dyadic


def _sign_run(X, Y):
    """(GPU record, reference record, T values) of dcor_premat_sign_launch, normalise = 0, zero noise."""
    import torch
    from dcor import _lib
    orc = _orc()
    n = len(X)
    m = math.ceil(8.0 / (SIGN_EPS[0] * SIGN_EPS[1]))
    k = n // m
    assert m == 11 and k >= 3
    z, l = _mix()
    flips = np.ones(n, dtype=np.uint8)
    bits = np.zeros(32 * ((n + 31) // 32), dtype=np.uint8)
    bits[:n] = flips
    words = np.packbits(bits, bitorder="little").view(np.uint32)   # sample i: bit i & 31 of word i >> 5
    T = dict(X=_t(X), Y=_t(Y), sc=_t(np.zeros(4)), lx=_t(np.zeros(k)), ly=_t(np.zeros(k)), isc=_t(np.zeros(4)),
             fl=_t(words.view(np.int32)), lz=_t(np.zeros(1)), mz=_t(z), ml=_t(l))
    d = _lib.PrematSign(n=n, reps=1, eps1=SIGN_EPS[0], eps2=SIGN_EPS[1], alpha=0.05, normalise=0, ci_mode=0,
                        nsim=NSIM, X=T["X"].data_ptr(), Y=T["Y"].data_ptr(), xy_stride=n,
                        lap_ni_sc=T["sc"].data_ptr(), lap_ni_x=T["lx"].data_ptr(), lap_ni_y=T["ly"].data_ptr(),
                        lap_int_sc=T["isc"].data_ptr(), flips=T["fl"].data_ptr(), lap_z=T["lz"].data_ptr(),
                        mix_z=T["mz"].data_ptr(), mix_l=T["ml"].data_ptr())
    out = torch.full((1, 6), -7.0, dtype=torch.float64, device="cuda")
    _lib.check(_lib.lib.dcor_premat_sign_launch(C.byref(d), C.c_void_p(out.data_ptr()),
                                                C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    _, ni = orc.ci_ni_signbatch(X, Y, *SIGN_EPS, 0.05, 0, np.zeros(4), np.zeros(k), np.zeros(k))
    _, it, _ = orc.ci_int_signflip(X, Y, *SIGN_EPS, 0.05, 0, 0, np.zeros(4), flips, 0.0, z, l)
    xb = np.sign(X[:k * m]).reshape(k, m).sum(axis=1) / float(m)
    yb = np.sign(Y[:k * m]).reshape(k, m).sum(axis=1) / float(m)
    return out.cpu().numpy()[0], np.concatenate([ni, it]), float(m) * xb * yb


@pytest.mark.parametrize("n", NS)
def test_sign_constant_batches(n):
    """Constant columns (every T = +-11, squares exact) and two period-11 sign patterns whose every
    batch has the same sign sums (1 and 3 of 11: T = 11 * fl(1 / 11) * fl(3 / 11), constant and
    inexact).  The endpoints are sin(pi / 2 * (eta -+ crit S / sqrt k)): sin is 1-Lipschitz, so the
    allowance is pi / 2 times the sub-G one."""
    i = np.arange(n) % 11
    pat_x = np.where(i < 6, 0.7, -0.7)
    pat_y = np.where(i < 7, 1.1, -1.1)
    cases = [(np.full(n, c), np.full(n, s * c), f"c={c} Y={s:+.0f}c") for c in CONSTANTS for s in (1.0, -1.0)]
    cases.append((pat_x, pat_y, "sign sums 1/11, 3/11"))
    cases.append((pat_y, -pat_x, "sign sums 3/11, -1/11"))
    for X, Y, what in cases:
        got, ref, T = _sign_run(X, Y)
        assert np.all(T == T[0]) and not np.isnan(ref).any()
        _check(got, ref, T, f"sign n={n} {what}", crit_scale=math.pi / 2.0)
