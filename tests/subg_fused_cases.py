"""Case table of the fused sub-G engine's edge tests (subg_fused_core, csrc/dcor_fused.hip): no HIP.

Each case names the batch geometry it is meant to hit, m = min(ceil(8 / (eps1 eps2)), n),
k = floor(n / m), tail = n - k m (make_subg, csrc/dcor_plan.cpp), and the kernel form that n
selects: "wave" (one wave per replicate, k_subg_fused_w / k_grid_subg_w) up to SUBG_W_NMAX, "wg"
(one 256-thread workgroup per replicate, k_subg_fused / k_grid_subg) above it.  assert_geometry()
checks every case against the host planner, so a case cannot drift off its edge.

Why eta is small in the cases with few batches.  The NI interval's half width is
crit sd(T) / sqrt(k) with T = m xt yt, and with m = 8 / (eps1 eps2) the variance of T is about
(lambda1^2 eps2 / eps1 + 1) (lambda2^2 eps1 / eps2 + 1), at least (lambda^2 + 1)^2 = 169 at
eta = 1 (lambda = 2 sqrt 3): below k of about 700 both NI bounds then clamp to -1 and +1 in every
replicate and say nothing about se, sd(T) or the batch sums.  The lane-wrap cases pin k to 63..65,
so n cannot grow; eta (lambda = 2 eta sqrt(log n)) shrinks the noise instead and keeps the edge.
The INT interval's width falls with eta of the sender the same way (bs = 2 lambda_s / eps_s).
"""
from collections import namedtuple

# csrc/dcor_engine.h: #define SUBG_W_NMAX 16384 (test_subg_fused_cases reads the header against it)
SUBG_W_NMAX = 16384
WAVE_LANES, WG_THREADS = 64, 256

# the replicates every geometry case runs: five from 3 (not a multiple of the four waves of a
# wave-kernel workgroup, so its last workgroup is partial)
REP_BEGIN, REPS = 3, 5

Case = namedtuple("Case", "id n eps k m tail form spec why")

GAUSS = dict(dgp="gaussian", mu=(0.2, -0.1), sigma=(0.8, 0.9))                 # mu != 0, sigma != 1
GAUSS0 = dict(dgp="gaussian", mu=(0.0, 0.0), sigma=(1.1, 0.9))
BERN = dict(dgp="bernoulli")
BF = dict(dgp="bounded_factor")
MIX = dict(dgp="mix_gaussian", pi_mix=0.3, mix_mu1=(0.5, -0.5), mix_sigma1=(0.7, 1.3))  # pi not dyadic


def _eta(a, b):
    return dict(eta1=a, eta2=b)


_ROWS = [
    # id, n, (eps1, eps2), k, m, tail, form, cell arguments, what it hits
    ("n16384-last-wave", 16384, (1.0, 1.0), 2048, 8, 0, "wave", dict(BF, rho=0.3),
     "last wave-kernel n, m = 2^3, no tail"),
    ("n16385-first-wg", 16385, (1.0, 1.0), 2048, 8, 1, "wg", dict(GAUSS, rho=0.3, **_eta(2.0, 0.5)),
     "first workgroup-kernel n, one-sample tail; eta (2, .5), sender X"),
    ("n63-m1", 63, (4.0, 2.0), 63, 1, 0, "wave", dict(BERN, rho=0.3, **_eta(0.1, 0.15)),
     "m = 1: remainder branch only, one idle lane"),
    ("n64-m1", 64, (4.0, 2.0), 64, 1, 0, "wave", dict(GAUSS, rho=0.3, **_eta(0.15, 0.1)),
     "m = 1, k = the wave's lanes"),
    ("n65-m1", 65, (4.0, 2.0), 65, 1, 0, "wave", dict(MIX, rho=0.4, **_eta(0.1, 0.15)),
     "m = 1, k one past the wave's lanes"),
    ("n193-m3", 193, (2.0, 1.5), 64, 3, 1, "wave", dict(BF, rho=0.3, **_eta(0.15, 0.1)),
     "odd m: pair loop + remainder + tail"),
    ("n512-k64", 512, (1.0, 1.0), 64, 8, 0, "wave", dict(BERN, rho=0.3, **_eta(0.1, 0.15)),
     "k = 64 with the pair loop"),
    ("n520-k65", 520, (1.0, 1.0), 65, 8, 0, "wave", dict(GAUSS, rho=0.3, **_eta(0.15, 0.1)),
     "k = 65: lane 0 wraps to a second batch"),
    ("n527-k65-tail7", 527, (1.0, 1.0), 65, 8, 7, "wave", dict(MIX, rho=0.4, **_eta(0.1, 0.15)),
     "lane wrap and a 7-sample tail"),
    ("n3001-senderX", 3001, (1.5, 0.5), 272, 11, 9, "wave", dict(BF, rho=0.3, **_eta(0.3, 0.2)),
     "odd non-2^e m, sender X"),
    ("n3001-senderY", 3001, (0.5, 1.5), 272, 11, 9, "wave", dict(GAUSS, rho=0.3, **_eta(0.3, 0.2)),
     "odd non-2^e m, sender Y"),
    ("n15-k1", 15, (1.0, 1.0), 1, 8, 7, "wave", dict(BF, rho=0.3),
     "k = 1: the NI CI is NA, the INT side finite"),
    ("n7-m-clipped", 7, (1.0, 1.0), 1, 7, 0, "wave", dict(GAUSS, rho=0.3),
     "m clipped to n, k = 1"),
    ("n16385-m800", 16385, (0.1, 0.1), 20, 800, 385, "wg", dict(BF, rho=0.1, **_eta(0.1, 0.15)),
     "workgroup kernel, 236 idle threads, long tail"),
    ("n204800-k256", 204800, (0.1, 0.1), 256, 800, 0, "wg", dict(BF, rho=0.3, **_eta(0.15, 0.1)),
     "k = the workgroup's thread count"),
    ("n205605-k257", 205605, (0.1, 0.1), 257, 800, 5, "wg", dict(GAUSS0, rho=0.3, **_eta(0.1, 0.15)),
     "thread 0 takes a second batch"),
    # moved up from the issue's n = 20000 (k = 625): at eta (.5, 2) the NI bounds clamp below k of
    # about 1000; the edge (workgroup form, m = 2^5, no tail) is kept
    ("n64000-m32", 64000, (0.5, 0.5), 2000, 32, 0, "wg", dict(BF, rho=0.2, **_eta(0.5, 2.0)),
     "workgroup kernel, 2^e m; eta (.5, 2), sender X"),
    # beyond the issue's table.  eta (.5, 2) and (2, .5) need k of 1000 or more to leave an NI bound
    # unclamped, so the n = 3001 pair is repeated at the largest wave-form n with m = 11 and
    # tail 9 under both eta orders and both senders ...
    ("n16377-senderX-eta.5-2", 16377, (1.5, 0.5), 1488, 11, 9, "wave", dict(BF, rho=0.2, **_eta(0.5, 2.0)),
     "odd m, sender X, eta (.5, 2)"),
    ("n16377-senderX-eta2-.5", 16377, (1.5, 0.5), 1488, 11, 9, "wave", dict(MIX, rho=0.4, **_eta(2.0, 0.5)),
     "odd m, sender X, eta (2, .5)"),
    ("n16377-senderY-eta.5-2", 16377, (0.5, 1.5), 1488, 11, 9, "wave", dict(GAUSS, rho=0.3, **_eta(0.5, 2.0)),
     "odd m, sender Y, eta (.5, 2)"),
    ("n16377-senderY-eta2-.5", 16377, (0.5, 1.5), 1488, 11, 9, "wave", dict(BF, rho=0.2, **_eta(2.0, 0.5)),
     "odd m, sender Y, eta (2, .5)"),
    # ... the workgroup form gets the sender on the Y side (every workgroup row of the issue's table
    # has eps1 = eps2), and sub-G + Bernoulli in the workgroup form (m = 8: a larger m puts
    # m E[x] E[y] past 1)
    ("n20003-senderY-eta.5-2", 20003, (0.5, 1.5), 1818, 11, 5, "wg", dict(MIX, rho=0.4, **_eta(0.5, 2.0)),
     "workgroup kernel, odd m, sender Y, eta (.5, 2)"),
    ("n20003-senderY-eta2-.5", 20003, (0.5, 1.5), 1818, 11, 5, "wg", dict(GAUSS, rho=0.3, **_eta(2.0, 0.5)),
     "workgroup kernel, odd m, sender Y, eta (2, .5)"),
    ("n16399-wg-bernoulli", 16399, (1.0, 1.0), 2049, 8, 7, "wg", dict(BERN, rho=0.3, **_eta(0.05, 0.07)),
     "workgroup kernel, two-valued samples, 7-sample tail"),
]

CASES = [Case(*row) for row in _ROWS]
CASE_IDS = [c.id for c in CASES]

# The only cases allowed to have every CI bound of a side clamped or NA (at most five), each with
# its reason.  Every other case has, among its five replicates, one with both NI bounds and one
# with both INT bounds strictly inside (-1, 1) (test_subg_fused_cases).
DEGENERATE = {
    "n15-k1": "k = 1: var of one batch product is NA, so both NI bounds are NaN by construction; the INT "
              "side's central noise alone, 2 lambda_r / (n eps_r) = 1.8 at n = 15, clamps both its bounds",
    "n7-m-clipped": "k = 1 as well (m clipped to n = 7): NI bounds NaN, INT bounds clamped as at n = 15",
}
assert len(DEGENERATE) <= 5 and set(DEGENERATE) <= set(CASE_IDS)


def seed_of(case):
    return 7_000_000 + CASE_IDS.index(case.id)


def cell_of(case, **over):
    """The case's CellSpec (dcor.sim)."""
    from dcor.sim import CellSpec
    kw = dict(n=case.n, eps1=case.eps[0], eps2=case.eps[1], family="subG", seed=seed_of(case))
    kw.update(case.spec)
    kw.update(over)
    return CellSpec(**kw)


def form_of(n):
    return "wave" if n <= SUBG_W_NMAX else "wg"


def sender_of(case):
    """ver-cor-subG.R:76: the X side sends when eps1 >= eps2."""
    return "X" if case.eps[0] >= case.eps[1] else "Y"


def eta_of(case):
    return (case.spec.get("eta1", 1.0), case.spec.get("eta2", 1.0))


def assert_geometry(case, batch_geometry):
    """The case's (k, m, tail) and kernel form against the host planner (dc.api.batch_geometry)."""
    k, m = batch_geometry(case.n, case.eps[0], case.eps[1], "subG")
    assert (k, m, case.n - k * m) == (case.k, case.m, case.tail), (case.id, k, m, case.n - k * m)
    assert form_of(case.n) == case.form, case.id


def unclamped(rows, lo, up):
    """Replicates whose bounds in columns lo, up both lie strictly inside (-1, 1)."""
    import numpy as np
    rows = np.asarray(rows)
    with np.errstate(invalid="ignore"):
        return (np.abs(rows[:, lo]) < 1.0) & (np.abs(rows[:, up]) < 1.0)


# ---------------------------------------------------------------- key counts
# The mixquant key count nsim decides the wave selector's width (WaveMix<16> up to 1024 keys,
# WaveMix<32> above) and, with alpha, the order statistic's position.
KEY_NSIM = [1, 2, 3, 1023, 1024, 1025, 2047, 2048]
# alpha = 1.999 puts the position at 0 for 3 and 1025 keys but at 1 for 2048 (ceiling(0.0005 * 2048)
# = 2), so 2048 keys also run alpha = 1.9995 (ceiling(0.512) = 1); alpha = 1e-6: the last key
KEY_ALPHA_EDGES = [(3, 1.999), (1025, 1.999), (2048, 1.999), (2048, 1.9995), (3, 1e-6), (1025, 1e-6), (2048, 1e-6)]
KEY_RUNS = [(nsim, 0.05) for nsim in KEY_NSIM] + KEY_ALPHA_EDGES
KEY_REPS = 5
# one cell per kernel form; eta as in the few-batch cases keeps the INT bounds off +-1 at every
# key count, the largest order statistic of 2048 keys included
KEY_CELLS = {
    "wave": dict(n=1000, rho=0.2, eps1=1.0, eps2=1.0, family="subG", seed=7_100_001, **BF, **_eta(0.1, 0.1)),
    "wg": dict(n=20000, rho=0.2, eps1=1.0, eps2=1.0, family="subG", seed=7_100_002, **GAUSS, **_eta(0.1, 0.1)),
}


def mix_pos(nsim, alpha):
    """make_mix (csrc/dcor_plan.cpp): the 0-based position of sort(x)[ceiling((1 - alpha/2) nsim)]."""
    import math
    return math.ceil((1.0 - alpha / 2.0) * nsim) - 1
