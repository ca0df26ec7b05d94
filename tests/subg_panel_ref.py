"""The sub-G panel draw contract (include/dcor.h, dcor_subg_panel_launch) restated on the CPU for
tests/test_gpu_subg_panel.py and tests/test_subg_panel_abi.py: per replicate the oracle's Philox
streams (oracle.gen_laplace / gen_normals) at the contract's sites, fed to the oracle's
correlation_NI_subG and ci_INT_subG with hrs = 0."""
import math

import numpy as np

from sign_panel_ref import philox4x32_10

SITE_DGP_B, SITE_NI_LAP, SITE_SCALAR, SITE_MIX_Z, SITE_MIX_L = 2, 4, 5, 6, 7


def geometry(n, eps1, eps2):
    """(k, m) of correlation_NI_subG (ver-cor-subG.R:37-38): m = ceil(8 / (eps1 eps2)) capped at n."""
    m = min(math.ceil(8.0 / (eps1 * eps2)), n)
    return n // m, m


def local_laplace(orc, n, seed, rep):
    """Sample i's local unit Laplace, i < n: words 2,3 of block (i, rep, SITE_DGP_B, 0) -- the odd
    elements of the site's Laplace stream (element e: block e / 2, words (0,1) / (2,3))."""
    return orc.gen_laplace(seed, rep, SITE_DGP_B, 2 * n)[1::2]


def local_laplace_words(n, seed, rep):
    """The same draws from the block's words 2,3 by a numpy Philox and numpy's log: (2 x + 1) 2^-53
    with x the top 52 bits of (w2, w3), then -sign(u - .5) log(1 - 2 |u - .5|)."""
    w = philox4x32_10(np.arange(n, dtype=np.uint64), rep, SITE_DGP_B, 0, seed & 0xFFFFFFFF, seed >> 32)
    x = (w[2].astype(np.uint64) << np.uint64(20)) | (w[3].astype(np.uint64) >> np.uint64(12))
    u = (2.0 * x.astype(np.float64) + 1.0) * 2.0 ** -53
    up = u - 0.5
    return -np.sign(up) * np.log(1.0 - 2.0 * np.abs(up))


def oracle_record(orc, X, Y, eps1, eps2, seed, rep, eta1=1.0, eta2=1.0, alpha=0.05, nsim=1000,
                  local_scale=1.0):
    """One replicate's six numbers from the oracle on the restated streams.  local_scale != 1
    miscalibrates the local noise on purpose (the law test's negative control)."""
    n = len(X)
    k, _ = geometry(n, eps1, eps2)
    bl = orc.gen_laplace(seed, rep, SITE_NI_LAP, 2 * k)
    central = orc.gen_laplace(seed, rep, SITE_SCALAR, 10)[8]
    mz = orc.gen_normals(seed, rep, SITE_MIX_Z, nsim)
    ml = orc.gen_laplace(seed, rep, SITE_MIX_L, nsim)
    st, ni, km = orc.ni_subg(X, Y, eps1, eps2, eta1, eta2, alpha, 0, lap_x=bl[0::2], lap_y=bl[1::2])
    assert st == 0, f"oracle ni_subg status {st}"
    assert (int(km[0]), int(km[1])) == geometry(n, eps1, eps2)
    st, it, _ = orc.int_subg(X, Y, eps1, eps2, eta1, eta2, alpha, 0,
                             lap_local=local_scale * local_laplace(orc, n, seed, rep), lap_central=central,
                             mix_z=mz, mix_l=ml)
    assert st == 0, f"oracle int_subg status {st}"
    return np.concatenate([ni, it])


def oracle_records(orc, X, Y, eps1, eps2, seed, rep_begin, reps, **kw):
    return np.stack([oracle_record(orc, X, Y, eps1, eps2, seed, rep_begin + j, **kw) for j in range(reps)])


def law_panel():
    """The law check's panel: 256 samples drawn once from a bivariate normal with rho = .5 at a tenth
    of the unit scale, so that the INT interval stays inside [-1, 1] and its width is informative."""
    g = np.random.default_rng(20261020)
    xy = 0.1 * g.multivariate_normal([0.0, 0.0], [[1.0, 0.5], [0.5, 1.0]], size=256)
    return np.ascontiguousarray(xy[:, 0]), np.ascontiguousarray(xy[:, 1])


def welch_t(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return (a.mean() - b.mean()) / math.sqrt(a.var(ddof=1) / len(a) + b.var(ddof=1) / len(b))


def law_stats(rec):
    """The three per-replicate statistics the law test compares: ni_hat, int_hat, the INT width."""
    return rec[:, 0], rec[:, 3], rec[:, 5] - rec[:, 4]
