"""The simulation's sub-Gaussian estimators (correlation_NI_subG + ci_INT_subG,
ver-cor-subG.R:25-108: contiguous batches, lambda_n / lambda_INT_n, any (eps1, eps2), either
sender) on the caller's own (X, Y) panel with every noise draw made inside the kernel
(dcor_subg_panel_launch): the sub-G counterpart of dcor.signpanel, and of running
ver-cor-subG.R:179-195 on one data set.  The panel is prepared once per call and shared by every
replicate; a call takes any mix of (eps1, eps2) segments.  A replicate's record depends only on
(panel, eta1, eta2, eps1, eps2, seed, replicate), so `rep_begin` makes any shard over calls,
processes or GPUs exact.

For a table of several variables (vertically partitioned data), `table_segments`, `corr_matrix`
and `corr_matrix_sweep` run any column pairs in one call (dcor_subg_table_launch): one upload, one
preparation of every column (a column is clipped and its batch means formed once per distinct batch
size, not once per pair), one replicate launch; a pair's records are the panel entry's on its two
columns bit for bit.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._segcall import pack_segments, run_segment_call
from .signpanel import _pair_matrices, _table, all_pairs


def sweep_segments(X, Y, segs, eta1=1.0, eta2=1.0, alpha=0.05, nsim=1000, stream=None):
    """The replicates of several (eps1, eps2, seed, rep_begin, reps) segments on one shared panel
    in one native call -> float64 [sum(reps), 6] (ni_hat, ni_lo, ni_hi, int_hat, int_lo, int_hi) in
    segment order.  Each segment's records equal `replicates` with the same arguments bit for bit."""
    segs = list(segs)
    arr, total = pack_segments(_lib.SubgSegment, segs, 4)
    import torch
    Xd = torch.as_tensor(np.ascontiguousarray(X, dtype=np.float64), device="cuda")
    Yd = torch.as_tensor(np.ascontiguousarray(Y, dtype=np.float64), device="cuda")
    if Xd.ndim != 1 or Xd.shape != Yd.shape:
        raise ValueError("X and Y must be vectors of one length")
    desc = _lib.SubgPanelDesc(n=int(Xd.shape[0]), X=Xd.data_ptr(), Y=Yd.data_ptr(), eta1=float(eta1),
                              eta2=float(eta2), alpha=float(alpha), nsim=int(nsim))
    return run_segment_call(_lib.lib.dcor_subg_panel_launch, desc, arr, len(segs), total, stream)


def replicates(X, Y, eps1, eps2, reps, seed, rep_begin=0, eta1=1.0, eta2=1.0, alpha=0.05, nsim=1000,
               stream=None):
    """Replicates rep_begin .. rep_begin + reps - 1 of the sub-G NI and INT intervals on (X, Y) at
    (eps1, eps2) under Philox key `seed` -> float64 [reps, 6]."""
    return sweep_segments(X, Y, [(eps1, eps2, seed, rep_begin, reps)], eta1=eta1, eta2=eta2, alpha=alpha,
                          nsim=nsim, stream=stream)


def eps_sweep(X, Y, eps_grid, reps, seed=1_000_000, eta1=1.0, eta2=1.0, alpha=0.05, nsim=1000, stream=None):
    """`reps` replicates for every entry of eps_grid -- a scalar eps (eps1 = eps2 = eps) or an
    (eps1, eps2) pair -- under key seed + idx (idx 1-based) in one native call; returns the runs
    [n_eps, reps, 6] and the per-eps summaries in the shape of dcor.hrs.sweep_summaries (as
    dcor.signpanel.eps_sweep)."""
    from .hrs import sweep_summaries
    eps_grid = list(eps_grid)
    segs = [(e1, e2, seed + idx, 0, reps) for idx, (e1, e2) in enumerate(_eps_pairs(eps_grid), start=1)]
    runs = sweep_segments(X, Y, segs, eta1=eta1, eta2=eta2, alpha=alpha, nsim=nsim, stream=stream)
    return sweep_summaries(eps_grid, runs.reshape(len(eps_grid), reps, 6))


# ------------------------------------------------ every column pair of a shared table
def _eps_pairs(eps_grid):
    """eps_sweep's grid entries -- a scalar eps or an (eps1, eps2) pair -- as (eps1, eps2) floats."""
    return [(float(e[0]), float(e[1])) if np.ndim(e) else (float(e), float(e)) for e in eps_grid]


def table_segments(D, segs, eta=1.0, alpha=0.05, nsim=1000, stream=None):
    """The replicates of several (col_x, col_y, eps1, eps2, seed, rep_begin, reps) segments on the
    columns of one shared (n, p) table in one native call (dcor_subg_table_launch): the table is
    uploaded and prepared once, every pair and eps shares one replicate launch -> float64
    [sum(reps), 6] in segment order.  eta: column c's sub-Gaussian parameter, a scalar (every
    column's) or a length-p vector.  Each segment's records equal `replicates(D[:, col_x],
    D[:, col_y], eps1, eps2, reps, seed, rep_begin, eta1=eta[col_x], eta2=eta[col_y])` bit for bit;
    (a, b) and (b, a) are different segments."""
    segs = list(segs)
    F, n, p = _table(D)
    eta = np.ascontiguousarray(np.broadcast_to(np.asarray(eta, dtype=np.float64), (p,)) if np.ndim(eta) == 0
                               else eta, dtype=np.float64)
    if eta.shape != (p,):
        raise ValueError(f"eta must be a scalar or hold one value per column ({p})")
    for a, b, *_ in segs:
        if not (0 <= int(a) < p and 0 <= int(b) < p):
            raise ValueError(f"columns ({a}, {b}) outside [0, {p})")
    arr, total = pack_segments(_lib.SubgPairSegment, segs, 6)
    import torch
    Dd = torch.as_tensor(F.reshape(-1, order="F"), device="cuda")   # the one upload
    desc = _lib.SubgTableDesc(n=n, p=p, ld=n, D=Dd.data_ptr(), eta=eta.ctypes.data_as(C.POINTER(C.c_double)),
                              alpha=float(alpha), nsim=int(nsim))
    return run_segment_call(_lib.lib.dcor_subg_table_launch, desc, arr, len(segs), total, stream)


def corr_matrix(D, eps1, eps2, reps, seed=1_000_000, pairs=None, eta=1.0, alpha=0.05, nsim=1000, stream=None):
    """The private sub-G correlation of every column pair of the (n, p) table D at (eps1, eps2):
    `reps` replicates per pair in one native call.  pairs: every a < b in row-major order by default;
    pair j runs under Philox key seed + j + 1.  Returns {"pairs", "runs" [npairs, reps, 6], "ni",
    "int"}: per method the p x p matrices "rho_hat", "ci_low", "ci_high" of the runs' means, filled
    symmetrically, NaN on the diagonal unless that pair was asked for (as dcor.signpanel.corr_matrix)."""
    _, _, p = _table(D)
    pairs = all_pairs(p) if pairs is None else [(int(a), int(b)) for a, b in pairs]
    segs = [(a, b, eps1, eps2, seed + j + 1, 0, reps) for j, (a, b) in enumerate(pairs)]
    runs = table_segments(D, segs, eta=eta, alpha=alpha, nsim=nsim, stream=stream).reshape(len(pairs), reps, 6)
    return {"pairs": pairs, "runs": runs, **_pair_matrices(p, pairs, runs)}


def corr_matrix_sweep(D, eps_grid, reps, seed=1_000_000, pairs=None, eta=1.0, alpha=0.05, nsim=1000,
                      stream=None):
    """`reps` replicates for every pair and every entry of eps_grid (a scalar eps or an (eps1, eps2)
    pair, as eps_sweep), pairs x eps in one native call.  Pair j at eps index idx (1-based) runs
    under key seed + j len(eps_grid) + idx, so one pair's part equals eps_sweep on its columns with
    seed + j len(eps_grid).  Returns {"pairs", "eps", "runs" [npairs, n_eps, reps, 6], "summaries"}:
    summaries[j] is dcor.hrs.sweep_summaries of pair j's runs (as dcor.signpanel.corr_matrix_sweep)."""
    from .hrs import sweep_summaries
    eps_grid = list(eps_grid)
    _, _, p = _table(D)
    pairs = all_pairs(p) if pairs is None else [(int(a), int(b)) for a, b in pairs]
    ne = len(eps_grid)
    segs = [(a, b, e1, e2, seed + j * ne + idx, 0, reps)
            for j, (a, b) in enumerate(pairs) for idx, (e1, e2) in enumerate(_eps_pairs(eps_grid), start=1)]
    runs = table_segments(D, segs, eta=eta, alpha=alpha, nsim=nsim, stream=stream).reshape(len(pairs), ne, reps, 6)
    return {"pairs": pairs, "eps": eps_grid, "runs": runs,
            "summaries": [sweep_summaries(eps_grid, runs[j]) for j in range(len(pairs))]}
