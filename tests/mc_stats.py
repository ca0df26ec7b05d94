"""Monte-Carlo law comparison of two replicate sets of one cell (tests/test_mc_oracle.py on the
CPU restatements, tests/test_gpu_mc.py on the engine): the fused Philox engine against the
R-stream replay, which share neither the draw transforms nor the kernels.

`compare(a, b, rho)` turns two [B, 6] record arrays (columns dcor.sim.DETAIL_COLS) into named
statistics; `thresholds(n_stats)` gives the Bonferroni bounds they are held to; `violations`
lists what is outside them.  A statistic that cannot be computed (no data on a side, pooled
variance 0) is UNDEFINED, which is never a pass: the caller names the ones it allows.
"""
from __future__ import annotations

import math
import warnings
from statistics import NormalDist

import numpy as np
from scipy.stats import ks_2samp

from dcor.sim import DETAIL_COLS, CellSpec, headline_cell, r_cover

UNDEFINED = None
METHODS = ("ni", "int")
Z_NAMES = ("cover_z", "hat_t", "width_t", "se2_t")
KS_NAMES = ("hat_ks_p", "low_ks_p", "up_ks_p")
PER_METHOD = len(Z_NAMES) + len(KS_NAMES)

B = 10_000

# ------------------------------------------------------------------ the cells of the suite
_SG = dict(mu=(0.5, 0.5), sigma=(2.0, 2.0))
GRID_CELLS = {
    "sign-gauss": CellSpec(n=1000, rho=0.5, eps1=1.0, eps2=1.0, seed=1_000_073, **_SG),
    "sign-gauss-asym": CellSpec(n=2000, rho=-0.3, eps1=1.5, eps2=0.5, seed=1_000_017, **_SG),
    "sign-bern": CellSpec(n=1000, rho=0.3, eps1=1.0, eps2=1.0, dgp="bernoulli", seed=1_000_042),
    "subG-bounded": CellSpec(n=1000, rho=0.3, eps1=1.0, eps2=1.0, family="subG", dgp="bounded_factor",
                             seed=2025),
    "subG-gauss": CellSpec(n=2000, rho=0.8, eps1=0.5, eps2=0.5, family="subG", dgp="gaussian",
                           seed=1_000_300),
    "subG-mix": CellSpec(n=1500, rho=0.5, eps1=1.0, eps2=1.0, family="subG", dgp="mix_gaussian",
                         seed=1_000_400),
    "sign-k1": CellSpec(n=200, rho=0.3, eps1=0.2, eps2=0.2, seed=7, **_SG),
}
GPU_ONLY_CELLS = {"sign-gauss-1e4": headline_cell(n=10_000)}
HRS_CELLS = ("hrs-eps-hi", "hrs-eps-lo")

# k = floor(n / ceil(8 / (eps1 eps2))) = 1 in sign-k1: the NI interval needs var(T) of one batch,
# so ni_low / ni_up are NA in every replicate of both engines and the four NI statistics built on
# them have no input.  At n = 200, eps = 0.2 the INT interval is so wide that it covers rho in all
# 10,000 replicates of both engines (measured on the CPU restatements of both), so int_cover_z has
# pooled variance 0: no z exists, and `violations` requires the two coverage counts to be equal
# instead.  Nothing else may be undefined, in any cell.
K1_UNDEFINED = frozenset({"ni_cover_z", "ni_width_t", "ni_low_ks_p", "ni_up_ks_p", "int_cover_z"})
ALLOWED_UNDEFINED = {"sign-k1": K1_UNDEFINED}


def expected_defined(name: str) -> int:
    """How many of compare()'s z / t / KS statistics are defined for the cell `name`."""
    return len(METHODS) * PER_METHOD - len(ALLOWED_UNDEFINED.get(name, ()))


# every statistic the suite asserts: the seven grid cells, the GPU-only n = 1e4 cell and the two
# HRS cells, both methods.  The tests check the count of defined statistics per cell against
# expected_defined, so this is counted, not guessed.  An NA-count z (defined only where an NA
# count is neither 0 nor B on both sides) would add to it; there is none at these cells, and the
# tests assert that too.
N_STATS = sum(expected_defined(c) for c in (*GRID_CELLS, *GPU_ONLY_CELLS, *HRS_CELLS))


# ------------------------------------------------------------------------------ statistics
def thresholds(n_stats: int, family_alpha: float = 0.01) -> dict:
    """Bonferroni bounds for n_stats statistics at family-wise level family_alpha: a z or t
    statistic (two-sided, normal: every one here has thousands of degrees of freedom) must stay
    under z_max = qnorm(1 - family_alpha / (2 n_stats)), a KS p-value above family_alpha / n_stats."""
    return {"z_max": NormalDist().inv_cdf(1.0 - family_alpha / (2.0 * n_stats)),
            "ks_p_min": family_alpha / n_stats, "n_stats": n_stats, "family_alpha": family_alpha}


def two_prop_z(k1: int, n1: int, k2: int, n2: int):
    """Pooled two-proportion z of k1/n1 against k2/n2."""
    if n1 == 0 or n2 == 0:
        return UNDEFINED
    p = (k1 + k2) / (n1 + n2)
    v = p * (1.0 - p) * (1.0 / n1 + 1.0 / n2)
    if not v > 0.0:
        return UNDEFINED
    return (k1 / n1 - k2 / n2) / math.sqrt(v)


def welch_t(x, y):
    """Welch t of the means of x and y, NA dropped on each side."""
    x = np.asarray(x, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    x, y = x[~np.isnan(x)], y[~np.isnan(y)]
    if len(x) < 2 or len(y) < 2:
        return UNDEFINED
    v = x.var(ddof=1) / len(x) + y.var(ddof=1) / len(y)
    if not v > 0.0:
        return UNDEFINED
    return float((x.mean() - y.mean()) / math.sqrt(v))


def ks_p(x, y):
    """Two-sample Kolmogorov-Smirnov p-value, NA dropped on each side."""
    x = np.asarray(x, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    x, y = x[~np.isnan(x)], y[~np.isnan(y)]
    if len(x) == 0 or len(y) == 0:
        return UNDEFINED
    with warnings.catch_warnings():     # with heavy ties (endpoints clamped at +-1) scipy falls back
        warnings.filterwarnings("ignore", "ks_2samp: Exact calculation unsuccessful")  # to the asymptotic p
        return float(ks_2samp(x, y).pvalue)


def _cover_counts(a, b, rho, off):
    ca, cb = (r_cover(rho, r[:, off + 1], r[:, off + 2]) for r in (a, b))
    ca, cb = ca[~np.isnan(ca)], cb[~np.isnan(cb)]
    return int(ca.sum()), len(ca), int(cb.sum()), len(cb)


def compare(a, b, rho: float) -> dict:
    """Two [B, 6] record arrays of one cell -> {'stats': {name: value or UNDEFINED},
    'na': {column: (NA count of a, of b)}, 'na_z': {column: two-proportion z of the NA counts, for
    the columns where it exists}, 'cover': {method: (covered, defined) of a, then of b},
    'rows': (len(a), len(b))}.  Per method m in ('ni', 'int'):
    m_cover_z (two-proportion z on r_cover, NA rows dropped per side), Welch t on the mean of hat,
    of the CI width up - low and of the squared error (hat - rho)^2, and the KS p-values of hat,
    low and up."""
    a = np.asarray(a, dtype=np.float64).reshape(-1, 6)
    b = np.asarray(b, dtype=np.float64).reshape(-1, 6)
    stats, cover = {}, {}
    for m, off in zip(METHODS, (0, 3)):
        cover[m] = _cover_counts(a, b, rho, off)
        stats[f"{m}_cover_z"] = two_prop_z(*cover[m])
        stats[f"{m}_hat_t"] = welch_t(a[:, off], b[:, off])
        stats[f"{m}_width_t"] = welch_t(a[:, off + 2] - a[:, off + 1], b[:, off + 2] - b[:, off + 1])
        stats[f"{m}_se2_t"] = welch_t((a[:, off] - rho) ** 2, (b[:, off] - rho) ** 2)
        for j, col in enumerate(("hat", "low", "up")):
            stats[f"{m}_{col}_ks_p"] = ks_p(a[:, off + j], b[:, off + j])
    na, na_z = {}, {}
    for j, col in enumerate(DETAIL_COLS):
        ka, kb = int(np.isnan(a[:, j]).sum()), int(np.isnan(b[:, j]).sum())
        na[col] = (ka, kb)
        z = two_prop_z(ka, len(a), kb, len(b))
        if z is not UNDEFINED:
            na_z[col] = z
    return {"stats": stats, "na": na, "na_z": na_z, "cover": cover, "rows": (len(a), len(b))}


def n_defined(res: dict) -> int:
    return sum(v is not UNDEFINED for v in res["stats"].values()) + len(res["na_z"])


def violations(res: dict, thr: dict, allow_undefined=()) -> list:
    """Everything in a compare() result that is outside the bounds `thr`: a z or t at or past
    z_max, a KS p at or under ks_p_min, an undefined statistic not in allow_undefined (or a defined
    one that is), an NA count or a coverage count that differs where no z of it exists."""
    bad = []
    for name, v in res["stats"].items():
        if v is UNDEFINED:
            if name not in allow_undefined:
                bad.append(f"{name} undefined")
        elif name in allow_undefined:
            bad.append(f"{name} = {v:.4g} is defined but listed as undefined")
        elif name.endswith("_ks_p"):
            if not v > thr["ks_p_min"]:
                bad.append(f"{name} = {v:.3g} <= {thr['ks_p_min']:.3g}")
        elif not abs(v) < thr["z_max"]:
            bad.append(f"|{name}| = {abs(v):.3f} >= {thr['z_max']:.3f}")
    for m, (ka, na_, kb, nb) in res["cover"].items():
        if res["stats"][f"{m}_cover_z"] is UNDEFINED and ka * nb != kb * na_:
            bad.append(f"{m} coverage {ka} of {na_} vs {kb} of {nb} with no z")
    for col, (ka, kb) in res["na"].items():
        if col in res["na_z"]:
            if not abs(res["na_z"][col]) < thr["z_max"]:
                bad.append(f"NA count of {col}: {ka} vs {kb}, |z| = {abs(res['na_z'][col]):.3f}")
        elif ka * res["rows"][1] != kb * res["rows"][0]:    # both all-NA or both NA-free
            bad.append(f"NA count of {col}: {ka} of {res['rows'][0]} vs {kb} of {res['rows'][1]}")
    return bad


def describe(res: dict) -> str:
    """Every statistic of a cell on one line each (assertion messages, the DESIGN table)."""
    lines = [f"  {k:14s} " + ("undefined" if v is UNDEFINED else f"{v: .6g}") for k, v in res["stats"].items()]
    lines += [f"  cover {m:8s} {c[0]}/{c[1]} vs {c[2]}/{c[3]}" for m, c in res["cover"].items()]
    lines += [f"  NA {c:11s} {ka} vs {kb}" + (f"  z = {res['na_z'][c]:.3f}" if c in res["na_z"] else "")
              for c, (ka, kb) in res["na"].items()]
    return "\n".join(lines)
