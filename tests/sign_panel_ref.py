"""The sign-panel draw contract (include/dcor.h, dcor_sign_panel_launch) restated on the CPU for
tests/test_gpu_sign_panel.py and tests/test_sign_panel_abi.py: per replicate the oracle's Philox
streams (oracle.gen_laplace / gen_normals) and the flips from a numpy Philox4x32-10, fed to the
oracle's ci_NI_signbatch and ci_INT_signflip."""
import math

import numpy as np

SITE_FLIP, SITE_NI_LAP, SITE_SCALAR, SITE_MIX_Z, SITE_MIX_L = 3, 4, 5, 6, 7
_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = 0x9E3779B9, 0xBB67AE85
_LO = np.uint64(0xFFFFFFFF)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Vectorised Philox4x32-10: counters as uint32 arrays (broadcast), key two ints -> four uint32
    arrays (w0, w1, w2, w3)."""
    c = [np.asarray(v, dtype=np.uint64) & _LO for v in np.broadcast_arrays(c0, c1, c2, c3)]
    k0, k1 = int(k0) & 0xFFFFFFFF, int(k1) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = _M0 * c[0], _M1 * c[2]
        c = [((p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0)) & _LO, p1 & _LO,
             ((p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1)) & _LO, p0 & _LO]
        k0, k1 = (k0 + _W0) & 0xFFFFFFFF, (k1 + _W1) & 0xFFFFFFFF
    return [v.astype(np.uint32) for v in c]


def flip_threshold(eps1, eps2):
    """ceil(p 2^32), p = e^eps_s / (e^eps_s + 1), eps_s = max(eps1, eps2) (vert-cor.R:174, 275)."""
    es = math.exp(max(eps1, eps2))
    return int(math.ceil(es / (es + 1.0) * 4294967296.0))


def flips(n, eps1, eps2, seed, rep):
    """S_i = (word i & 3 of block (i >> 2, rep, SITE_FLIP, 0) < ceil(p 2^32)), i < n, as uint8."""
    nb = (n + 3) // 4
    w = philox4x32_10(np.arange(nb, dtype=np.uint64), rep, SITE_FLIP, 0, seed & 0xFFFFFFFF, seed >> 32)
    words = np.stack(w, axis=1).reshape(-1)[:n].astype(np.uint64)
    return (words < np.uint64(flip_threshold(eps1, eps2))).astype(np.uint8)


def geometry(n, eps1, eps2):
    m = math.ceil(8.0 / (eps1 * eps2))
    return n // m, m


def oracle_record(orc, X, Y, eps1, eps2, seed, rep, alpha=0.05, normalise=True, mode=0, nsim=1000):
    """One replicate's six numbers from the oracle on the restated streams (NaN triple where the
    oracle refuses)."""
    n = len(X)
    k, _ = geometry(n, eps1, eps2)
    sc = orc.gen_laplace(seed, rep, SITE_SCALAR, 10)
    bl = orc.gen_laplace(seed, rep, SITE_NI_LAP, 2 * k)
    mz = orc.gen_normals(seed, rep, SITE_MIX_Z, nsim)
    ml = orc.gen_laplace(seed, rep, SITE_MIX_L, nsim)
    st, ni = orc.ci_ni_signbatch(X, Y, eps1, eps2, alpha, normalise, sc[0:4], bl[0::2], bl[1::2])
    assert st == 0, f"oracle ci_ni_signbatch status {st}"
    st, it, _ = orc.ci_int_signflip(X, Y, eps1, eps2, alpha, mode, normalise, sc[4:8],
                                    flips(n, eps1, eps2, seed, rep), sc[8], mz, ml)
    assert st == 0, f"oracle ci_int_signflip status {st}"
    return np.concatenate([ni, it])


def oracle_records(orc, X, Y, eps1, eps2, seed, rep_begin, reps, **kw):
    return np.stack([oracle_record(orc, X, Y, eps1, eps2, seed, rep_begin + j, **kw) for j in range(reps)])


def law_panel():
    """The law check's panel (tests/test_gpu_sign_panel.py, test 5): 4,000 samples drawn once from a
    bivariate normal with rho = .5."""
    g = np.random.default_rng(20261019)
    xy = g.multivariate_normal([0.0, 0.0], [[1.0, 0.5], [0.5, 1.0]], size=4000)
    return np.ascontiguousarray(xy[:, 0]), np.ascontiguousarray(xy[:, 1])
