"""Sign-family replicates (ci_NI_signbatch + ci_INT_signflip) on the caller's own (X, Y) panel
with every noise draw made inside the kernel (dcor_sign_panel_launch): the sign family's
counterpart of the fused HRS sweep, and of running ver-cor-subG.R:179-195 with use_subG = FALSE on
one data set.  The panel is prepared once per call and shared by every replicate; a call takes any
mix of (eps1, eps2) segments.  A replicate's record depends only on (panel, eps1, eps2, seed,
replicate), so `rep_begin` makes any shard over calls, processes or GPUs exact.

For a table of several variables (vertically partitioned data), `table_segments`, `corr_matrix`
and `corr_matrix_sweep` run any column pairs in one call (dcor_sign_table_launch): one upload, one
preparation of every column, one replicate launch; a pair's records are the panel entry's on its
two columns bit for bit.
"""
from __future__ import annotations

import numpy as np

from . import _lib
from ._segcall import pack_segments, run_segment_call


def sweep_segments(X, Y, segs, alpha=0.05, normalise=True, mode="auto", nsim=1000, stream=None):
    """The replicates of several (eps1, eps2, seed, rep_begin, reps) segments on one shared panel
    in one native call -> float64 [sum(reps), 6] (ni_hat, ni_lo, ni_hi, int_hat, int_lo, int_hi) in
    segment order.  Each segment's records equal `replicates` with the same arguments bit for bit."""
    ci_mode = _lib.mode_code(mode)
    segs = list(segs)
    arr, total = pack_segments(_lib.SignSegment, segs, 4)
    import torch
    Xd = torch.as_tensor(np.ascontiguousarray(X, dtype=np.float64), device="cuda")
    Yd = torch.as_tensor(np.ascontiguousarray(Y, dtype=np.float64), device="cuda")
    if Xd.ndim != 1 or Xd.shape != Yd.shape:
        raise ValueError("X and Y must be vectors of one length")
    desc = _lib.SignPanelDesc(n=int(Xd.shape[0]), X=Xd.data_ptr(), Y=Yd.data_ptr(), alpha=float(alpha),
                              normalise=1 if normalise else 0, ci_mode=ci_mode, nsim=int(nsim))
    return run_segment_call(_lib.lib.dcor_sign_panel_launch, desc, arr, len(segs), total, stream)


def replicates(X, Y, eps1, eps2, reps, seed, rep_begin=0, alpha=0.05, normalise=True, mode="auto",
               nsim=1000, stream=None):
    """Replicates rep_begin .. rep_begin + reps - 1 of the sign family's NI and INT intervals on
    (X, Y) at (eps1, eps2) under Philox key `seed` -> float64 [reps, 6]."""
    return sweep_segments(X, Y, [(eps1, eps2, seed, rep_begin, reps)], alpha=alpha, normalise=normalise,
                          mode=mode, nsim=nsim, stream=stream)


def eps_sweep(X, Y, eps_grid, reps, seed=1_000_000, alpha=0.05, normalise=True, mode="auto", nsim=1000,
              stream=None):
    """`reps` replicates at eps1 = eps2 = eps for every eps of eps_grid (key seed + idx, idx 1-based)
    in one native call; returns the runs [n_eps, reps, 6] and the per-eps summaries in the shape of
    dcor.hrs.sweep_summaries."""
    from .hrs import sweep_summaries
    eps_grid = list(eps_grid)
    segs = [(e, e, seed + idx, 0, reps) for idx, e in enumerate(eps_grid, start=1)]
    runs = sweep_segments(X, Y, segs, alpha=alpha, normalise=normalise, mode=mode, nsim=nsim, stream=stream)
    return sweep_summaries(eps_grid, runs.reshape(len(eps_grid), reps, 6))


# ------------------------------------------------ every column pair of a shared table
def _table(D):
    """An (n, p) array -> (column-major float64 copy or view, n, p): column c is the contiguous run
    [c n, (c + 1) n) of its memory, so ld = n.  A column-major (Fortran-order) input is not copied."""
    D = np.asarray(D, dtype=np.float64)
    if D.ndim != 2 or D.shape[0] < 1 or D.shape[1] < 1:
        raise ValueError("D must be an (n, p) array with n, p >= 1")
    return np.asfortranarray(D), int(D.shape[0]), int(D.shape[1])


def table_segments(D, segs, alpha=0.05, normalise=True, mode="auto", nsim=1000, stream=None):
    """The replicates of several (col_x, col_y, eps1, eps2, seed, rep_begin, reps) segments on the
    columns of one shared (n, p) table in one native call (dcor_sign_table_launch): the table is
    uploaded and prepared once, every pair and eps shares one replicate launch -> float64
    [sum(reps), 6] in segment order.  Each segment's records equal `replicates(D[:, col_x],
    D[:, col_y], eps1, eps2, reps, seed, rep_begin)` bit for bit; X (col_x) is the sender side as
    there, so (a, b) and (b, a) are different segments."""
    ci_mode = _lib.mode_code(mode)
    segs = list(segs)
    F, n, p = _table(D)
    for a, b, *_ in segs:
        if not (0 <= int(a) < p and 0 <= int(b) < p):
            raise ValueError(f"columns ({a}, {b}) outside [0, {p})")
    arr, total = pack_segments(_lib.SignPairSegment, segs, 6)
    import torch
    Dd = torch.as_tensor(F.reshape(-1, order="F"), device="cuda")   # the one upload
    desc = _lib.SignTableDesc(n=n, p=p, ld=n, D=Dd.data_ptr(), alpha=float(alpha),
                              normalise=1 if normalise else 0, ci_mode=ci_mode, nsim=int(nsim))
    return run_segment_call(_lib.lib.dcor_sign_table_launch, desc, arr, len(segs), total, stream)


def all_pairs(p):
    """Every a < b of p columns in row-major order: (0, 1), (0, 2), ..., (p - 2, p - 1)."""
    return [(a, b) for a in range(p) for b in range(a + 1, p)]


def _pair_matrices(p, pairs, runs):
    """p x p matrices of the pairs' mean estimate and mean CI bounds, per method, filled
    symmetrically; NaN where no pair was asked for (the diagonal unless (a, a) was)."""
    names = (("ni", 0), ("int", 3))
    out = {m: {k: np.full((p, p), np.nan) for k in ("rho_hat", "ci_low", "ci_high")} for m, _ in names}
    for j, (a, b) in enumerate(pairs):
        for m, c in names:
            for i, k in enumerate(("rho_hat", "ci_low", "ci_high")):
                out[m][k][a, b] = out[m][k][b, a] = runs[j][:, c + i].mean() if runs.shape[1] else np.nan
    return out


def corr_matrix(D, eps1, eps2, reps, seed=1_000_000, pairs=None, alpha=0.05, normalise=True, mode="auto",
                nsim=1000, stream=None):
    """The private correlation of every column pair of the (n, p) table D at (eps1, eps2): `reps`
    replicates per pair in one native call.  pairs: every a < b in row-major order by default; pair
    j runs under Philox key seed + j + 1 (as eps_sweep keys its eps).  Returns {"pairs", "runs"
    [npairs, reps, 6], "ni", "int"}: per method the p x p matrices "rho_hat", "ci_low", "ci_high"
    of the runs' means, filled symmetrically (a pair listed in both orders keeps the later one), NaN
    on the diagonal unless that pair was asked for."""
    _, _, p = _table(D)
    pairs = all_pairs(p) if pairs is None else [(int(a), int(b)) for a, b in pairs]
    segs = [(a, b, eps1, eps2, seed + j + 1, 0, reps) for j, (a, b) in enumerate(pairs)]
    runs = table_segments(D, segs, alpha=alpha, normalise=normalise, mode=mode, nsim=nsim,
                          stream=stream).reshape(len(pairs), reps, 6)
    return {"pairs": pairs, "runs": runs, **_pair_matrices(p, pairs, runs)}


def corr_matrix_sweep(D, eps_grid, reps, seed=1_000_000, pairs=None, alpha=0.05, normalise=True, mode="auto",
                      nsim=1000, stream=None):
    """`reps` replicates at eps1 = eps2 = eps for every pair and every eps of eps_grid, pairs x eps
    in one native call.  Pair j at eps index idx (1-based) runs under key seed + j len(eps_grid) +
    idx, so one pair's part equals eps_sweep on its columns with seed + j len(eps_grid).  Returns
    {"pairs", "eps", "runs" [npairs, n_eps, reps, 6], "summaries"}: summaries[j] is
    dcor.hrs.sweep_summaries of pair j's runs."""
    from .hrs import sweep_summaries
    eps_grid = list(eps_grid)
    _, _, p = _table(D)
    pairs = all_pairs(p) if pairs is None else [(int(a), int(b)) for a, b in pairs]
    ne = len(eps_grid)
    segs = [(a, b, e, e, seed + j * ne + idx, 0, reps)
            for j, (a, b) in enumerate(pairs) for idx, e in enumerate(eps_grid, start=1)]
    runs = table_segments(D, segs, alpha=alpha, normalise=normalise, mode=mode, nsim=nsim,
                          stream=stream).reshape(len(pairs), ne, reps, 6)
    return {"pairs": pairs, "eps": eps_grid, "runs": runs,
            "summaries": [sweep_summaries(eps_grid, runs[j]) for j in range(len(pairs))]}


def standin_table(n, p, rho, seed=2):
    """A synthetic (n, p) table, column-major: equicorrelated normals (one common factor, pairwise
    correlation rho in [0, 1]) rounded in the manner of dcor.hrs.standin_panel -- even columns to
    whole years of an age-like scale, odd columns to one decimal of a BMI-like scale -- and put on
    the standard scale with the scales' own centre and sd, so the values stay on a coarse grid with
    many ties."""
    import math

    from .hrs import AGE_HI, AGE_LO, BMI_HI, BMI_LO
    if not 0.0 <= rho <= 1.0:
        raise ValueError("rho must be in [0, 1]")
    g = np.random.default_rng(seed)
    f = g.standard_normal(n)
    D = np.empty((n, p), dtype=np.float64, order="F")
    for c in range(p):
        z = math.sqrt(rho) * f + math.sqrt(1.0 - rho) * g.standard_normal(n)
        lo, hi, dec = (AGE_LO, AGE_HI, 0) if c % 2 == 0 else (BMI_LO, BMI_HI, 1)
        mid, sd = 0.5 * (lo + hi), 0.25 * (hi - lo)
        D[:, c] = (np.round(mid + sd * z, dec) - mid) / sd
    return D
