"""The simulation's sub-Gaussian estimators (correlation_NI_subG + ci_INT_subG,
ver-cor-subG.R:25-108: contiguous batches, lambda_n / lambda_INT_n, any (eps1, eps2), either
sender) on the caller's own (X, Y) panel with every noise draw made inside the kernel
(dcor_subg_panel_launch): the sub-G counterpart of dcor.signpanel, and of running
ver-cor-subG.R:179-195 on one data set.  The panel is prepared once per call and shared by every
replicate; a call takes any mix of (eps1, eps2) segments.  A replicate's record depends only on
(panel, eta1, eta2, eps1, eps2, seed, replicate), so `rep_begin` makes any shard over calls,
processes or GPUs exact.
"""
from __future__ import annotations

import numpy as np

from . import _lib
from ._segcall import pack_segments, run_segment_call


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
    pairs = [(float(e[0]), float(e[1])) if np.ndim(e) else (float(e), float(e)) for e in eps_grid]
    segs = [(e1, e2, seed + idx, 0, reps) for idx, (e1, e2) in enumerate(pairs, start=1)]
    runs = sweep_segments(X, Y, segs, eta1=eta1, eta2=eta2, alpha=alpha, nsim=nsim, stream=stream)
    return sweep_summaries(eps_grid, runs.reshape(len(eps_grid), reps, 6))
