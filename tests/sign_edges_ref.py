"""The inputs and the large-m NI tolerance of tests/test_gpu_sign_edges.py, pinned on the CPU by
tests/test_sign_edges_ref.py: the shape tables (n, eps1, eps2) -> (k, m), the panels, the draw of
item kinds, ni_T_bound and assert_close_ni_conditioned.  The draw contract itself (geometry,
oracle_records, the sites) is tests/sign_panel_ref.py's, used here unchanged."""
import math

import numpy as np

import helpers
from sign_panel_ref import SITE_NI_LAP, geometry


def ni_T_bound(orc, n, eps1, eps2, seed, rep):
    """m max_j (1 + bx |lap_x[j]|) (1 + by |lap_y[j]|) on the SITE_NI_LAP draws oracle_record makes,
    bx = 2 / (m eps1), by = 2 / (m eps2): an upper bound of max_j |T_j| of the replicate (a batch
    mean of signs is in [-1, 1]) that needs no signs, so it holds for normalise 0 and 1."""
    k, m = geometry(n, eps1, eps2)
    bl = np.abs(orc.gen_laplace(seed, rep, SITE_NI_LAP, 2 * k))
    bx, by = 2.0 / (m * eps1), 2.0 / (m * eps2)
    return float(m * np.max((1.0 + bx * bl[0::2]) * (1.0 + by * bl[1::2])))


def ni_T_bounds(orc, n, eps1, eps2, seed, rep_begin, reps):
    return np.array([ni_T_bound(orc, n, eps1, eps2, seed, rep_begin + j) for j in range(reps)])


NI_COND_ULPS = 64.0


def assert_close_ni_conditioned(got, ref, bound, what=""):
    """For m > 200 only.  Columns 3:6 (INT): helpers.assert_close unchanged.  Columns 0:3 (NI):
    |got - ref| <= max(helpers' bound, (pi / 2) 64 2^-53 bound), the NaN pattern identical; `bound`
    is ni_T_bound of the row (a scalar, or one value per row).

    The NI numbers are sin(pi / 2 x) of eta = mean(T) and of eta -+ crit S / sqrt(k), clamped to
    [-1, 1], with T_j = m xt yt of order m: one ulp of T moves them by (pi / 2) ulp(T), which at
    m > 3e4 is above helpers' 1e-13 + 1e-12 |.| with nothing wrong.  64 ulp of max |T| cover a
    one-ulp difference in each of cx / m, xt, yt, T, the sum of k <= 3 terms and S / sqrt(k); the
    clamp and sin are 1-Lipschitz after the pi / 2 factor."""
    got = np.atleast_2d(np.asarray(got, dtype=np.float64))
    ref = np.atleast_2d(np.asarray(ref, dtype=np.float64))
    assert got.shape == ref.shape and got.shape[1] == 6, (what, got.shape, ref.shape)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), f"{what}: NaN pattern\n got {got!r}\n ref {ref!r}"
    helpers.assert_close(got[:, 3:], ref[:, 3:], what=f"{what} INT")
    g, r = got[:, :3], ref[:, :3]
    b = np.broadcast_to(np.asarray(bound, dtype=np.float64).reshape(-1, 1), g.shape)
    tol = np.maximum(helpers.ATOL + helpers.RTOL * np.maximum(np.abs(g), np.abs(r)),
                     (math.pi / 2.0) * NI_COND_ULPS * 2.0 ** -53 * b)
    diff = np.abs(g - r)
    ok = (diff <= tol) | (np.isnan(g) & np.isnan(r)) | (g == r)
    if not np.all(ok):
        raise AssertionError(f"{what} NI: mismatch\n got {g!r}\n ref {r!r}\n diff {diff!r}\n tol {tol!r}")


# ------------------------------------------------ the shapes of tests/test_gpu_sign_edges.py,
# pinned on the CPU by tests/test_sign_edges_ref.py: (n, eps1, eps2) -> (k, m)
EDGE_SEED, EDGE_REPS, EDGE_REP_BEGINS = 31, 3, (0, 1001)

WIDE_SHAPES = {   # two-word counters (m > 32,767) against the oracle
    (40_001, 0.02, 0.012): (1, 33_334),
    (70_001, 0.02, 0.012): (2, 33_334),    # two threads' flushes meet in both words
    (70_001, 0.012, 0.02): (2, 33_334),    # the senders, so bx and by, swapped
}
EPS_PACK = (0.5, 16.0 / 32767.0)   # m = 32,767: the last one-word m
EPS_WIDE = (0.5, 16.0 / 32768.0)   # m = 32,768: the first two-word m
PACK_SHAPES = {
    (32_767,) + EPS_PACK: (1, 32_767),
    (65_535,) + EPS_PACK: (2, 32_767),     # tail 1
    (32_768,) + EPS_WIDE: (1, 32_768),
    (65_537,) + EPS_WIDE: (2, 32_768),     # tail 1
}
BATCH_SHAPES = {   # batch sizes and pass edges of the SP_CAP = 4,096 counter loop
    (4099, 4.0, 2.0): (4099, 1),           # two passes, the second with 3 batches
    (4096, 4.0, 2.0): (4096, 1),           # k = SP_CAP, no tail
    (12_291, 2.0, 1.5): (4097, 3),
    (4099, 2.0, 1.0): (1024, 4),
    (4099, 1.6, 1.0): (819, 5),
    (4099, 1.0, 8.0 / 1024.0): (4, 1024),  # dr = 0
    (4099, 1.0, 8.0 / 1025.0): (3, 1025),  # dq = 0: a batch spans trips of the sample loop
    (2049, 1.0, 8.0 / 1025.0): (1, 1025),
    (6401, 0.05, 0.05): (2, 3200),
    (8192, 2.0, 2.0): (4096, 2),
    (8194, 2.0, 2.0): (4097, 2),
    (16_385, 2.0, 2.0): (8192, 2),         # tail 1
    (16_386, 2.0, 2.0): (8193, 2),
}
MIX_N = 40_001   # the mixed-kind panel: (eps1, eps2, seed) -> (k, m)
MIX_KINDS = {(0.02, 0.012, 101): (1, 33_334), (2.0, 2.0, 102): (20_000, 2), (0.2, 0.2, 103): (200, 200)}
TABLE_N, TABLE_P, TABLE_LD = 1003, 3, 1011
TABLE_PAIRS = [(0, 1), (1, 2), (2, 0), (1, 1)]
TABLE_EPS = {(1.0, 1.0): (125, 8), (2.0, 2.0): (501, 2), (0.2, 0.2): (5, 200)}


def edge_panel(n, seed):
    """test_gpu_sign_panel's _panel: bivariate normal, mean .5, sd 2, rho .5."""
    g = np.random.default_rng(seed)
    xy = g.multivariate_normal([0.5, 0.5], [[4.0, 2.0], [2.0, 4.0]], size=n)
    return np.ascontiguousarray(xy[:, 0]), np.ascontiguousarray(xy[:, 1])


PACK_PANELS = ("++", "+-", "-+", "--", "half")


def pack_panel(n, m, kind):
    """The packing-boundary panels (normalise = 0).  "++" .. "--": X = +-1.25, Y = +-0.75
    throughout, every batch count exactly (+-m, +-m).  "half": the first m // 2 samples of each run
    of m positive in X, the rest negative, Y the opposite."""
    if kind == "half":
        s = np.where(np.arange(n) % m < m // 2, 1.0, -1.0)
        return 1.25 * s, -0.75 * s
    sx, sy = (1.0 if c == "+" else -1.0 for c in kind)
    return np.full(n, 1.25 * sx), np.full(n, 0.75 * sy)


def pack_counts(X, Y, k, m):
    """The per-batch sign counts of the raw panel, as the kernel's counters must hold them."""
    return (np.sign(X[:k * m]).reshape(k, m).sum(axis=1).astype(np.int64),
            np.sign(Y[:k * m]).reshape(k, m).sum(axis=1).astype(np.int64))


def mix_items(items, nkinds, seed=7):
    """Item i's kind from a fixed default_rng(seed) (not cycled: no grid stride can align with a
    period) and its replicate index, the number of earlier items of its kind."""
    kinds = np.random.default_rng(seed).integers(0, nkinds, size=items)
    reps = np.zeros(items, dtype=np.int64)
    seen = [0] * nkinds
    for i, q in enumerate(kinds):
        reps[i] = seen[q]
        seen[q] += 1
    return kinds, reps


def edge_table(n=TABLE_N, p=TABLE_P, seed=17):
    """test_gpu_sign_table's _table."""
    g = np.random.default_rng(seed)
    f = g.standard_normal(n)
    cols = [(0.3 + 0.2 * c) + (0.6 + 0.5 * c) * (np.sqrt(0.5) * f + np.sqrt(0.5) * g.standard_normal(n))
            for c in range(p)]
    return np.asfortranarray(np.stack(cols, axis=1))
