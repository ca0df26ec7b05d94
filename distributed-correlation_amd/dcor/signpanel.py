"""Sign-family replicates (ci_NI_signbatch + ci_INT_signflip) on the caller's own (X, Y) panel
with every noise draw made inside the kernel (dcor_sign_panel_launch): the sign family's
counterpart of the fused HRS sweep, and of running ver-cor-subG.R:179-195 with use_subG = FALSE on
one data set.  The panel is prepared once per call and shared by every replicate; a call takes any
mix of (eps1, eps2) segments.  A replicate's record depends only on (panel, eps1, eps2, seed,
replicate), so `rep_begin` makes any shard over calls, processes or GPUs exact.
"""
from __future__ import annotations

import numpy as np

from . import _lib


def _segments(segs):
    """[(eps1, eps2, seed, rep_begin, reps), ...] -> (ctypes array, rows, total): records in
    segment order."""
    rows = np.cumsum([0] + [int(s[4]) for s in segs])
    arr = (_lib.SignSegment * max(len(segs), 1))(*[
        _lib.SignSegment(eps1=float(e1), eps2=float(e2), seed=int(seed), rep_begin=int(rb), reps=int(c),
                         out_row=int(rows[j]))
        for j, (e1, e2, seed, rb, c) in enumerate(segs)])
    return arr, rows, int(rows[-1])


def sweep_segments(X, Y, segs, alpha=0.05, normalise=True, mode="auto", nsim=1000, stream=None):
    """The replicates of several (eps1, eps2, seed, rep_begin, reps) segments on one shared panel
    in one native call -> float64 [sum(reps), 6] (ni_hat, ni_lo, ni_hi, int_hat, int_lo, int_hi) in
    segment order.  Each segment's records equal `replicates` with the same arguments bit for bit."""
    import ctypes as C

    ci_mode = _lib.mode_code(mode)
    arr, _, total = _segments(list(segs))
    import torch
    Xd = torch.as_tensor(np.ascontiguousarray(X, dtype=np.float64), device="cuda")
    Yd = torch.as_tensor(np.ascontiguousarray(Y, dtype=np.float64), device="cuda")
    if Xd.ndim != 1 or Xd.shape != Yd.shape:
        raise ValueError("X and Y must be vectors of one length")
    st = torch.cuda.current_stream() if stream is None else stream
    out = torch.empty((max(total, 1), 6), dtype=torch.float64, device="cuda")
    desc = _lib.SignPanelDesc(n=int(Xd.shape[0]), X=Xd.data_ptr(), Y=Yd.data_ptr(), alpha=float(alpha),
                              normalise=1 if normalise else 0, ci_mode=ci_mode, nsim=int(nsim))
    with torch.cuda.stream(st):
        _lib.check(_lib.lib.dcor_sign_panel_launch(C.byref(desc), arr, len(segs),
                                                   C.c_void_p(out.data_ptr()), C.c_void_p(st.cuda_stream)))
        res = out[:total].cpu().numpy()   # waits for the stream: X, Y outlive the call's work
    return res


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
