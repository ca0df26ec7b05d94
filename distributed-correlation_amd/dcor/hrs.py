"""HRS BMI-vs-Age real-data study (real-data-sims.R) on the engine: panel ingest, DP
standardisation, the calibrated lambdas, and the replicate sweep of BASELINE config C5.

The reference loads `hrs_long_panel.rds`, keeps wave 2 complete cases of (agey_e, bmi)
(real-data-sims.R:13, 38-41), standardises both columns with a DP mean / sd
(real-data-sims.R:73-106, 273-287) and runs the NI and INT estimators on the standardised
panel (real-data-sims.R:290-323), then sweeps eps over seq(.25, 2.5, .1) with R = 200
replicates each (real-data-sims.R:345-448).

Ingesting the HRS panel itself waits for a data-licensing decision by the
project owner, so the repository ships no HRS microdata, nothing computed from them, and no
reader for them.  `standin_panel(n, rho)` is a generic synthetic panel of the same kind
(whole-year ages, one-decimal BMIs): each column is centred on its clip interval
(real-data-sims.R:260-261) with sd = interval width / 4; n and rho are the caller's.
"""
from __future__ import annotations

import math

import numpy as np

# real-data-sims.R:260-270
AGE_LO, AGE_HI = 45.0, 90.0
BMI_LO, BMI_HI = 15.0, 35.0
EPS_MEAN, EPS_M2 = 0.10, 0.10
EPS_CORR = 2.0
# seq(0.25, 2.5, by = 0.1): R's seq.default computes from + (0:n) * by without rounding, so
# e.g. the 7th value is 0.8500000000000001 (R prints 0.85); which(eps_grid == eps) matches these.
EPS_GRID = tuple(0.25 + i * 0.1 for i in range(23))
R_PER_EPS = 200
NI_SEED, INT_SEED = 231, 322                                     # set.seed (:289, :312)


def standin_panel(n: int, rho: float, seed: int = 2):
    """Synthetic raw (age, bmi): whole-year ages and one-decimal BMIs from a bivariate normal
    centred on the clip intervals with sd = width / 4 and correlation rho."""
    g = np.random.default_rng(seed)
    za = g.standard_normal(n)
    zb = rho * za + math.sqrt(1.0 - rho * rho) * g.standard_normal(n)
    age = np.round(0.5 * (AGE_LO + AGE_HI) + 0.25 * (AGE_HI - AGE_LO) * za)
    bmi = np.round(0.5 * (BMI_LO + BMI_HI) + 0.25 * (BMI_HI - BMI_LO) * zb, 1)
    return age, bmi


def standardize_panel(age, bmi, lap=None, rng=None):
    """dp_sd of both columns, standardize_dp, lambda_from_priv (real-data-sims.R:273-287).
    lap: optional unit Laplace draws [age mean, age m2, bmi mean, bmi m2]."""
    from . import api
    lap = np.asarray(api.unit_laplace(4, rng) if lap is None else lap, dtype=np.float64)
    age_priv = api.dp_sd(age, AGE_LO, AGE_HI, EPS_MEAN, EPS_M2, lap=lap[:2])
    bmi_priv = api.dp_sd(bmi, BMI_LO, BMI_HI, EPS_MEAN, EPS_M2, lap=lap[2:])
    age_z = api.standardize_dp(age, age_priv, AGE_LO, AGE_HI)
    bmi_z = api.standardize_dp(bmi, bmi_priv, BMI_LO, BMI_HI)
    ok = ~(np.isnan(age_z) | np.isnan(bmi_z))                      # drop_na (:282)
    return {"age_z": np.ascontiguousarray(age_z[ok]), "bmi_z": np.ascontiguousarray(bmi_z[ok]),
            "age_priv": age_priv, "bmi_priv": bmi_priv,
            "lambda_age_z": api.lambda_from_priv(AGE_LO, AGE_HI, age_priv),
            "lambda_bmi_z": api.lambda_from_priv(BMI_LO, BMI_HI, bmi_priv)}


# ------------------------------------------------------------ replicate sweep (a19 / C5)
# On-device unit-noise streams of one HRS replicate (dcor_draws_launch / dcor_perm_launch
# sites).  The reference reseeds per run with set.seed(10 + 37 rep + 1000 idx) (NI) and
# set.seed(20 + 41 rep + 1000 idx) (INT) (real-data-sims.R:404, 423); here the per-eps seed
# is the Philox key and the replicate index is the counter, so replicates are independent
# streams and any split over launches or GPUs reproduces them exactly.
SITE_NI_LAP_X, SITE_NI_LAP_Y, SITE_INT_LOCAL, SITE_INT_CENTRAL, SITE_MIX_Z, SITE_MIX_L = 11, 12, 13, 14, 15, 16
DRAW_LAPLACE, DRAW_NORMAL = 0, 1


def r_seeds(idx: int, reps, rep_begin: int = 0):
    """The reference's per-run seeds at eps index idx (1-based, which(eps_grid == eps)) for
    runs rep = rep_begin+1 .. rep_begin+reps: set.seed(10 + 37 rep + 1000 idx) before
    run_NI_once and set.seed(20 + 41 rep + 1000 idx) before run_INT_once
    (real-data-sims.R:404, 423)."""
    rep = np.arange(rep_begin + 1, rep_begin + reps + 1, dtype=np.int64)
    return ((10 + 37 * rep + 1000 * idx).astype(np.int32), (20 + 41 * rep + 1000 * idx).astype(np.int32))


def _philox_draws(seed_ni, seed_int, rb, nr, n, k, m, nsim, bufs, sp):
    """The Philox unit-noise arrays of runs rb .. rb+nr-1 into bufs (perm, lap_x, lap_y,
    lap_local, lap_central, mix_z, mix_l), enqueued on stream sp."""
    import ctypes as C

    from . import _lib
    P = lambda t: C.c_void_p(t.data_ptr())
    perm, lx, ly, ll, lc, mz, ml = bufs
    chk = _lib.check
    chk(_lib.lib.dcor_perm_launch(seed_ni, _lib.SITE_PERM, rb, nr, n, k * m, P(perm), sp))
    chk(_lib.lib.dcor_draws_launch(DRAW_LAPLACE, seed_ni, SITE_NI_LAP_X, rb, nr, k, P(lx), sp))
    chk(_lib.lib.dcor_draws_launch(DRAW_LAPLACE, seed_ni, SITE_NI_LAP_Y, rb, nr, k, P(ly), sp))
    chk(_lib.lib.dcor_draws_launch(DRAW_LAPLACE, seed_int, SITE_INT_LOCAL, rb, nr, n, P(ll), sp))
    chk(_lib.lib.dcor_draws_launch(DRAW_LAPLACE, seed_int, SITE_INT_CENTRAL, rb, nr, 1, P(lc), sp))
    chk(_lib.lib.dcor_draws_launch(DRAW_NORMAL, seed_int, SITE_MIX_Z, rb, nr, nsim, P(mz), sp))
    chk(_lib.lib.dcor_draws_launch(DRAW_LAPLACE, seed_int, SITE_MIX_L, rb, nr, nsim, P(ml), sp))


def _premat_launch(X, Y, pn, n, nr, eps, lam_age, lam_bmi, lam_r, delta, nsim, alpha, bufs, out, sp):
    """One pre-materialised HRS launch over the panel pn: nr runs from the noise in bufs into
    out[:nr] (dcor_premat_subg_panel_launch), enqueued on stream sp."""
    import ctypes as C

    from . import _lib
    perm, lx, ly, ll, lc, mz, ml = bufs
    d = _lib.PrematSubg(n=n, reps=nr, eps1=eps, eps2=eps, eta1=1.0, eta2=1.0, alpha=alpha, hrs=1,
                        lam_x=lam_age, lam_y=lam_bmi, lam_s=lam_age, lam_o=lam_bmi, lam_r=lam_r,
                        delta=delta, nsim=nsim, X=X.data_ptr(), Y=Y.data_ptr(), xy_stride=0,
                        perm=perm.data_ptr(), lap_ni_x=lx.data_ptr(), lap_ni_y=ly.data_ptr(),
                        lap_local=ll.data_ptr(), lap_central=lc.data_ptr(), mix_z=mz.data_ptr(),
                        mix_l=ml.data_ptr())
    _lib.check(_lib.lib.dcor_premat_subg_panel_launch(C.byref(d), pn, C.c_void_p(out.data_ptr()), sp))


def hrs_replicates(age_z, bmi_z, lam_age, lam_bmi, eps, reps, seed_ni=NI_SEED, seed_int=INT_SEED,
                   nsim=2000, rep_begin=0, chunk=8192, alpha=0.05, keep_noise=False, rng="philox",
                   eps_idx=None, mode="premat"):
    """`reps` NI + INT replicates of the HRS estimators on one standardised panel at one eps:
    correlation_NI_subG(lambda_X = lam_age, lambda_Y = lam_bmi) and ci_INT_subG(AGE sends,
    lambda_receiver_from_noise, delta_clip = 1/n) (real-data-sims.R:357-400).  The panel is
    encoded once (dcor_panel_create); noise is generated in HBM per chunk and streamed by the
    pre-materialised kernel.  Returns float64 [reps, 6] (ni_hat, ni_lo, ni_hi, int_hat, int_lo,
    int_hi) and, with keep_noise, the host copies of every noise array.

    rng='R' replays the reference's own streams instead: run rep (1-based, rep_begin + 1 ..)
    draws its NI noise after set.seed(10 + 37 rep + 1000 eps_idx) and its INT noise after
    set.seed(20 + 41 rep + 1000 eps_idx) (dcor_rstream_hrs_draws), so every run is the
    reference's run for that seed; seed_ni / seed_int are then unused.

    mode='fused' (rng='philox' only) draws the same Philox noise inside the streaming kernel
    (dcor_hrs_fused_launch) instead of materialising it in HBM: the results equal the
    pre-materialised pipeline's to within its compensated sums' rounding.  Any panel: a
    dictionary-coded one (at most 256 distinct values per column) runs from LDS codes, a
    continuous one gathers its clipped values from L2 (n <= 65536) or is materialised per
    chunk (larger n)."""
    import ctypes as C

    import torch

    from . import _lib, api
    if rng not in ("philox", "R"):
        raise ValueError(f"rng must be 'philox' or 'R', not {rng!r}")
    if mode not in ("premat", "fused"):
        raise ValueError(f"mode must be 'premat' or 'fused', not {mode!r}")
    if mode == "fused" and (rng != "philox" or keep_noise):
        raise ValueError("mode='fused' draws Philox noise in the kernel: rng='philox', keep_noise=False")
    if rng == "R" and eps_idx is None:
        raise ValueError("rng='R' needs eps_idx (the 1-based position of eps in the sweep)")
    X = torch.as_tensor(np.ascontiguousarray(age_z, dtype=np.float64), device="cuda")
    Y = torch.as_tensor(np.ascontiguousarray(bmi_z, dtype=np.float64), device="cuda")
    n = int(X.shape[0])
    k, m = api.batch_geometry(n, eps, eps, "subG", hrs=True)
    delta = 1.0 / n
    lam_r = api.lambda_receiver_from_noise(lam_age, lam_bmi, eps, delta)
    P = lambda t: C.c_void_p(t.data_ptr())
    stream = torch.cuda.current_stream()
    sp = C.c_void_p(stream.cuda_stream)
    pn = C.c_void_p()
    _lib.check(_lib.lib.dcor_panel_create(P(X), P(Y), n, sp, C.byref(pn)))
    cr = min(chunk, max(1, reps))
    f64 = dict(dtype=torch.float64, device="cuda")
    if mode == "fused":
        out = torch.empty((reps, 6), **f64)
        try:
            for r0 in range(0, reps, cr):
                nr = min(cr, reps - r0)
                d = _lib.PrematSubg(n=n, reps=nr, eps1=eps, eps2=eps, eta1=1.0, eta2=1.0, alpha=alpha,
                                    hrs=1, lam_x=lam_age, lam_y=lam_bmi, lam_s=lam_age, lam_o=lam_bmi,
                                    lam_r=lam_r, delta=delta, nsim=nsim, X=X.data_ptr(), Y=Y.data_ptr(),
                                    xy_stride=0)
                _lib.check(_lib.lib.dcor_hrs_fused_launch(C.byref(d), pn, seed_ni, seed_int,
                                                          rep_begin + r0, P(out[r0:]), sp))
            return out.cpu().numpy()
        finally:
            _lib.lib.dcor_panel_destroy(pn)
    if rng == "philox" and not keep_noise:
        # the launch chain natively (dcor_hrs_sweep_launch), one segment per chunk of cr runs
        out = torch.empty((max(reps, 1), 6), **f64)
        try:
            _native_segments(X, Y, pn, lam_age, lam_bmi, nsim, alpha,
                             [(eps, seed_ni, seed_int, rep_begin + r0, min(cr, reps - r0), r0)
                              for r0 in range(0, reps, cr)], out, stream)
            return out[:reps].cpu().numpy()
        finally:
            _lib.lib.dcor_panel_destroy(pn)
    perm = torch.empty((cr, k * m), dtype=torch.int32, device="cuda")
    lx, ly = torch.empty((cr, k), **f64), torch.empty((cr, k), **f64)
    ll, lc = torch.empty((cr, n), **f64), torch.empty((cr,), **f64)
    mz, ml = torch.empty((cr, nsim), **f64), torch.empty((cr, nsim), **f64)
    out = torch.empty((reps, 6), **f64)
    noise = {key: [] for key in ("perm", "lap_x", "lap_y", "lap_local", "lap_central", "mix_z", "mix_l")}
    try:
        for r0 in range(0, reps, cr):
            nr = min(cr, reps - r0)
            rb = rep_begin + r0
            chk = _lib.check
            if rng == "R":
                sn, si = r_seeds(eps_idx, nr, rb)
                I32 = C.POINTER(C.c_int32)
                chk(_lib.lib.dcor_rstream_hrs_draws(n, k, m, nsim, nr, sn.ctypes.data_as(I32),
                                                    si.ctypes.data_as(I32), P(perm), P(lx), P(ly),
                                                    P(ll), P(lc), P(mz), P(ml), sp))
            else:
                _philox_draws(seed_ni, seed_int, rb, nr, n, k, m, nsim, (perm, lx, ly, ll, lc, mz, ml), sp)
            _premat_launch(X, Y, pn, n, nr, eps, lam_age, lam_bmi, lam_r, delta, nsim, alpha,
                           (perm, lx, ly, ll, lc, mz, ml), out[r0:], sp)
            if keep_noise:
                for key, t in (("perm", perm), ("lap_x", lx), ("lap_y", ly), ("lap_local", ll),
                               ("lap_central", lc), ("mix_z", mz), ("mix_l", ml)):
                    noise[key].append(t[:nr].cpu().numpy().copy())
        res = out.cpu().numpy()
    finally:
        _lib.lib.dcor_panel_destroy(pn)
    if keep_noise:
        return res, {key: np.concatenate(v) for key, v in noise.items()}, {"k": k, "m": m, "lam_r": lam_r,
                                                                           "delta": delta}
    return res


def _summ(method, eps, hat, lo, hi) -> dict:
    """real-data-sims.R:408-418 / 427-437: means and type-7 quantiles (NA propagates)."""
    def q(v, p):
        return float("nan") if np.isnan(v).any() else float(np.quantile(v, p))
    return {"method": method, "eps_corr": eps, "rho_hat_mean": float(np.mean(hat)),
            "ci_low_mean": float(np.mean(lo)), "ci_high_mean": float(np.mean(hi)),
            "ci_low_q10": q(lo, 0.10), "ci_high_q90": q(hi, 0.90)}


def _native_segments(X, Y, pn, lam_age, lam_bmi, nsim, alpha, rowsegs, out, stream, mode="premat"):
    """Enqueue (eps, seed_ni, seed_int, first run, count, output row) segments on `stream` with one
    dcor_hrs_sweep_launch: per segment the seven Philox noise arrays in one launch, then the
    pre-materialised panel kernels, records to out[row ..].  mode='fused': one
    dcor_hrs_fused_sweep_launch instead -- every segment in one launch of the in-kernel-noise
    kernels, no noise arrays."""
    import ctypes as C

    from . import _lib
    if not rowsegs:
        return
    n = int(X.shape[0])
    base = _lib.PrematSubg(n=n, reps=0, eps1=1.0, eps2=1.0, eta1=1.0, eta2=1.0, alpha=alpha, hrs=1,
                           lam_x=lam_age, lam_y=lam_bmi, lam_s=lam_age, lam_o=lam_bmi, lam_r=float("nan"),
                           delta=1.0 / n, nsim=nsim, X=X.data_ptr(), Y=Y.data_ptr(), xy_stride=0)
    arr = (_lib.HrsSegment * len(rowsegs))(*[
        _lib.HrsSegment(eps=e, seed_ni=sn, seed_int=si, rep_begin=r0, reps=c, out_row=row)
        for e, sn, si, r0, c, row in rowsegs])
    launch = _lib.lib.dcor_hrs_fused_sweep_launch if mode == "fused" else _lib.lib.dcor_hrs_sweep_launch
    _lib.check(launch(C.byref(base), pn, arr, len(rowsegs), C.c_void_p(out.data_ptr()),
                      C.c_void_p(stream.cuda_stream)))


_SIDE = {}


def _side_streams(ns):
    """ns HIP streams of the current device, created once per process (stream creation and
    destruction cost more than a sweep's launches)."""
    import torch
    dev = torch.cuda.current_device()
    pool = _SIDE.setdefault(dev, [])
    while len(pool) < ns:
        pool.append(torch.cuda.Stream(device=dev))
    return pool[:ns]


def _check_sweep_mode(mode, rng, streams):
    """The sweeps' mode argument, checked before any device work (as hrs_replicates checks its own)."""
    if mode not in ("premat", "fused"):
        raise ValueError(f"mode must be 'premat' or 'fused', not {mode!r}")
    if mode == "fused" and rng != "philox":
        raise ValueError("mode='fused' draws Philox noise in the kernel: rng='philox'")
    if mode == "fused" and streams > 1:
        raise ValueError("mode='fused' runs every segment in one launch: streams=1")


def sweep_segments(age_z, bmi_z, lam_age, lam_bmi, eps_grid, segs, nsim=2000, alpha=0.05, streams=1,
                   mode="premat"):
    """Philox pre-materialised runs of several (eps index 0-based, first run, count) segments of
    an eps sweep on one shared panel -> [sum(count), 6] float64 in segment order.  Each segment's
    runs equal hrs_replicates(eps_grid[e], count, seed_ni=10 + 1000 idx, seed_int=20 + 1000 idx,
    rep_begin=first) byte for byte (idx = e + 1; the same draws and kernels), but the panel is
    uploaded and encoded once and the per-eps launch chains run from one native call
    (dcor_hrs_sweep_launch) instead of eight launches from Python per eps; with streams > 1 the
    segments are dealt round-robin over that many HIP streams, one native call each.  The host
    waits once, at the end.

    mode='fused' (streams = 1 only) draws the same Philox noise inside the kernels
    (dcor_hrs_fused_sweep_launch): one streaming launch and one epilogue launch cover every
    segment, whatever its eps, and no noise array is allocated.  Each segment's runs then equal
    hrs_replicates(..., mode='fused') with the same keys and rep_begin byte for byte."""
    _check_sweep_mode(mode, "philox", streams)
    import ctypes as C

    import torch

    from . import _lib
    X = torch.as_tensor(np.ascontiguousarray(age_z, dtype=np.float64), device="cuda")
    Y = torch.as_tensor(np.ascontiguousarray(bmi_z, dtype=np.float64), device="cuda")
    n = int(X.shape[0])
    rows = np.cumsum([0] + [c for _, _, c in segs])
    total = int(rows[-1])
    main = torch.cuda.current_stream()
    pn = C.c_void_p()
    _lib.check(_lib.lib.dcor_panel_create(C.c_void_p(X.data_ptr()), C.c_void_p(Y.data_ptr()), n,
                                          C.c_void_p(main.cuda_stream), C.byref(pn)))
    out = torch.empty((max(total, 1), 6), dtype=torch.float64, device="cuda")
    rowsegs = [(eps_grid[e], 10 + 1000 * (e + 1), 20 + 1000 * (e + 1), r0, c, int(rows[j]))
               for j, (e, r0, c) in enumerate(segs)]
    ns = max(1, min(streams, len(segs)))
    side = _side_streams(ns) if ns > 1 else [main]
    try:
        for j, s in enumerate(side):
            if s is not main:
                s.wait_stream(main)              # X, Y, the panel and out exist before any launch
            _native_segments(X, Y, pn, lam_age, lam_bmi, nsim, alpha, rowsegs[j::ns], out, s, mode)
        for s in side:
            if s is not main:
                main.wait_stream(s)
        res = out[:total].cpu().numpy()
    finally:
        for s in side:
            s.synchronize()
        _lib.lib.dcor_panel_destroy(pn)
    return res


def eps_sweep(age_z, bmi_z, lam_age, lam_bmi, eps_grid=EPS_GRID, reps=R_PER_EPS, nsim=2000,
              rng="philox", streams=1, mode="premat"):
    """The replicate sweep of real-data-sims.R:345-448: for every eps in seq(.25, 2.5, .1),
    `reps` NI and INT runs (Philox keys 10 + 1000 idx and 20 + 1000 idx, idx 1-based as
    which(eps_grid == eps); rng='R': the reference's own per-run set.seed streams) and the
    per-eps summaries ni_mean / int_mean.  rng='philox' runs every eps on one encoded panel from
    one native call per HIP stream (sweep_segments); the runs equal one hrs_replicates call per eps.
    mode='fused' (rng='philox', streams=1): the whole sweep in one launch of the in-kernel-noise
    kernels; the runs equal one hrs_replicates(mode='fused') call per eps."""
    _check_sweep_mode(mode, rng, streams)
    if rng == "philox":
        segs = [(e, 0, reps) for e in range(len(eps_grid))]
        runs = sweep_segments(age_z, bmi_z, lam_age, lam_bmi, eps_grid, segs, nsim=nsim, streams=streams,
                              mode=mode)
        return sweep_summaries(eps_grid, runs.reshape(len(eps_grid), reps, 6))
    runs = [hrs_replicates(age_z, bmi_z, lam_age, lam_bmi, eps, reps, seed_ni=10 + 1000 * idx,
                           seed_int=20 + 1000 * idx, nsim=nsim, rng=rng, eps_idx=idx)
            for idx, eps in enumerate(eps_grid, start=1)]
    return sweep_summaries(eps_grid, np.stack(runs))


def sweep_summaries(eps_grid, runs) -> dict:
    """The sweep's per-eps summaries from its runs [n_eps, reps, 6] (real-data-sims.R:408-437);
    dcor.dist.eps_sweep_distributed builds the same from the ranks' gathered runs.  Vectorised over
    eps; every value equals _summ's per-eps one (same reductions along contiguous rows)."""
    runs = np.asarray(runs, dtype=np.float64)
    cols = [np.ascontiguousarray(runs[:, :, j]) for j in range(6)]     # [n_eps, reps] each
    mean = [c.mean(axis=1) for c in cols]

    def q(c, p):                                                       # type 7; a NaN row -> NaN
        v = np.quantile(c, p, axis=1) if c.shape[1] else np.full(c.shape[0], np.nan)
        return np.where(np.isnan(c).any(axis=1), np.nan, v)
    lo_q = {1: q(cols[1], 0.10), 4: q(cols[4], 0.10)}
    hi_q = {2: q(cols[2], 0.90), 5: q(cols[5], 0.90)}

    def summ(method, j, i, eps):
        return {"method": method, "eps_corr": eps, "rho_hat_mean": float(mean[j][i]),
                "ci_low_mean": float(mean[j + 1][i]), "ci_high_mean": float(mean[j + 2][i]),
                "ci_low_q10": float(lo_q[j + 1][i]), "ci_high_q90": float(hi_q[j + 2][i])}
    ni_mean = [summ("NI", 0, i, eps) for i, eps in enumerate(eps_grid)]
    int_mean = [summ("INT", 3, i, eps) for i, eps in enumerate(eps_grid)]
    return {"eps": list(eps_grid), "runs": runs, "ni_mean": ni_mean, "int_mean": int_mean}


# ------------------------------------------------ every column pair of a shared table
def standardize_table(raw, bounds, lap=None, rng=None, na="listwise"):
    """standardize_panel for the p columns of the (n, p) array raw with per-column clip intervals
    bounds[c] = (lo, hi): dp_sd, standardize_dp and lambda_from_priv per column
    (real-data-sims.R:273-287), then the rows with any NaN dropped (drop_na, :282).  lap: optional
    unit Laplace draws, [mean, m2] of column 0, of column 1, ...  Returns {"Z": (n', p) column-major,
    "lam": [p], "priv": [p] {'mean', 'sd'}}.  na='pairwise' keeps every row, NaN where a column has a
    gap (dp_sd drops a column's own NA): the table of corr_matrix_pairwise, which drops per pair as
    the estimators do (real-data-sims.R:119-120, 187-189)."""
    from . import api
    if na not in ("listwise", "pairwise"):
        raise ValueError("na must be 'listwise' or 'pairwise'")
    raw = np.asarray(raw, dtype=np.float64)
    if raw.ndim != 2 or raw.shape[1] < 1 or len(bounds) != raw.shape[1]:
        raise ValueError("raw must be an (n, p) array and bounds p (lo, hi) pairs")
    p = raw.shape[1]
    lap = np.asarray(api.unit_laplace(2 * p, rng) if lap is None else lap, dtype=np.float64)
    if lap.shape != (2 * p,):
        raise ValueError("lap must hold 2 p unit Laplace draws")
    priv, cols = [], []
    for c, (lo, hi) in enumerate(bounds):
        col = np.ascontiguousarray(raw[:, c])
        priv.append(api.dp_sd(col, lo, hi, EPS_MEAN, EPS_M2, lap=lap[2 * c:2 * c + 2]))
        cols.append(api.standardize_dp(col, priv[c], lo, hi))
    Z = np.stack(cols, axis=1)
    ok = ~np.isnan(Z).any(axis=1) if na == "listwise" else np.ones(len(Z), dtype=bool)
    lam = np.array([api.lambda_from_priv(lo, hi, pv) for (lo, hi), pv in zip(bounds, priv)], dtype=np.float64)
    return {"Z": np.asfortranarray(Z[ok]), "lam": lam, "priv": priv}


def table_segments(Z, lam, segs, nsim=2000, alpha=0.05, delta=None, stream=None):
    """The HRS replicates of several (col_x, col_y, eps, seed_ni, seed_int, rep_begin, reps) segments
    on the columns of one shared (n, p) table of standardised variables, column c clipped at
    +-lam[c], in one native call (dcor_hrs_table_launch): one upload (a column-major Z is not
    copied), one preparation launch, every pair and eps in one streaming launch -> float64
    [sum(reps), 6] in segment order.  Each segment's records equal hrs_replicates(Z[:, col_x],
    Z[:, col_y], lam[col_x], lam[col_y], eps, reps, seed_ni, seed_int, rep_begin=rep_begin,
    mode='fused') byte for byte; X (col_x) is the sender, so (a, b) and (b, a) are different
    segments.  delta: delta_clip, 1 / n by default (real-data-sims.R:199)."""
    import ctypes as C

    from . import _lib
    from ._segcall import pack_segments, run_segment_call
    from .signpanel import _table
    segs = list(segs)
    F, n, p = _table(Z)
    lam = np.ascontiguousarray(lam, dtype=np.float64)
    if lam.shape != (p,):
        raise ValueError(f"lam must hold one clip bound per column ({p})")
    for a, b, *_ in segs:
        if not (0 <= int(a) < p and 0 <= int(b) < p):
            raise ValueError(f"columns ({a}, {b}) outside [0, {p})")
    arr, total = pack_segments(_lib.HrsPairSegment, segs, 6)
    import torch
    Dd = torch.as_tensor(F.reshape(-1, order="F"), device="cuda")   # the one upload
    desc = _lib.HrsTableDesc(n=n, p=p, ld=n, D=Dd.data_ptr(), lam=lam.ctypes.data_as(C.POINTER(C.c_double)),
                             alpha=float(alpha), delta=1.0 / n if delta is None else float(delta),
                             nsim=int(nsim))
    return run_segment_call(_lib.lib.dcor_hrs_table_launch, desc, arr, len(segs), total, stream)


def _pairs_of(Z, pairs):
    from .signpanel import _table, all_pairs
    _, _, p = _table(Z)
    return p, all_pairs(p) if pairs is None else [(int(a), int(b)) for a, b in pairs]


def _corr_matrix(run, Z, eps, reps, pairs):
    """corr_matrix / corr_matrix_pairwise: run(segs) -> [sum(reps), 6] is the table call."""
    from .signpanel import _pair_matrices
    p, pairs = _pairs_of(Z, pairs)
    segs = [(a, b, eps, 10 + 1000 * (j + 1), 20 + 1000 * (j + 1), 0, reps) for j, (a, b) in enumerate(pairs)]
    runs = run(segs).reshape(len(pairs), reps, 6)
    return {"pairs": pairs, "runs": runs, **_pair_matrices(p, pairs, runs)}


def _corr_matrix_sweep(run, Z, eps_grid, reps, pairs):
    """corr_matrix_sweep / corr_matrix_sweep_pairwise: run(segs) -> [sum(reps), 6] is the table call."""
    eps_grid = list(eps_grid)
    _, pairs = _pairs_of(Z, pairs)
    ne = len(eps_grid)
    segs = [(a, b, e, 10 + 1000 * (j * ne + idx), 20 + 1000 * (j * ne + idx), 0, reps)
            for j, (a, b) in enumerate(pairs) for idx, e in enumerate(eps_grid, start=1)]
    runs = run(segs).reshape(len(pairs), ne, reps, 6)
    return {"pairs": pairs, "eps": eps_grid, "runs": runs,
            "summaries": [sweep_summaries(eps_grid, runs[j]) for j in range(len(pairs))]}


def corr_matrix(Z, lam, eps, reps, pairs=None, nsim=2000, alpha=0.05, delta=None, stream=None):
    """The private correlation of every column pair of the standardised (n, p) table Z under the
    study's estimators at one eps: `reps` runs per pair in one native call.  pairs: every a < b in
    row-major order by default; pair j runs under the keys of corr_matrix_sweep with a one-eps grid,
    10 + 1000 (j + 1) and 20 + 1000 (j + 1).  Returns what dcor.signpanel.corr_matrix returns:
    {"pairs", "runs" [npairs, reps, 6], "ni", "int"}."""
    return _corr_matrix(lambda segs: table_segments(Z, lam, segs, nsim=nsim, alpha=alpha, delta=delta,
                                                    stream=stream), Z, eps, reps, pairs)


def corr_matrix_sweep(Z, lam, eps_grid=EPS_GRID, reps=R_PER_EPS, pairs=None, nsim=2000, alpha=0.05,
                      delta=None, stream=None):
    """The replicate sweep of real-data-sims.R:345-448 for every pair and every eps of eps_grid,
    pairs x eps in one native call.  Pair j at eps index idx (1-based) runs under Philox keys
    10 + 1000 (j n_eps + idx) and 20 + 1000 (j n_eps + idx), so pair 0's part equals
    eps_sweep(mode='fused') on its columns.  Returns what dcor.signpanel.corr_matrix_sweep returns:
    {"pairs", "eps", "runs" [npairs, n_eps, reps, 6], "summaries"}."""
    return _corr_matrix_sweep(lambda segs: table_segments(Z, lam, segs, nsim=nsim, alpha=alpha, delta=delta,
                                                          stream=stream), Z, eps_grid, reps, pairs)


# ------------------- the same on raw columns, the private standardisation drawn per replicate
STD_SEED = 433                                                   # the default key of the site-17 draws


def _bounds(bounds, p):
    b = np.asarray(bounds, dtype=np.float64)
    if b.shape != (p, 2):
        raise ValueError(f"bounds must hold one (lo, hi) pair per column ({p})")
    return np.ascontiguousarray(b[:, 0]), np.ascontiguousarray(b[:, 1])


def private_segments(raw, bounds, segs, eps_mean=EPS_MEAN, eps_m2=EPS_M2, seed_std=STD_SEED, nsim=2000,
                     alpha=0.05, delta=None, return_priv=False, stream=None):
    """table_segments on the RAW (n, p) table with the private standardisation of
    real-data-sims.R:273-287 drawn anew in every replicate, in one native call
    (dcor_hrs_private_table_launch): replicate r of a segment standardises column c with the dp_sd
    release from the unit Laplace pair dcor_draws_launch(0, seed_std, 17, r, 1, 2 p)[2 c : 2 c + 2]
    (budgets eps_mean, eps_m2 per column; bounds[c] = (lo, hi)) and runs the estimators on the result
    under lam = lambda_from_priv of that release.  Its records equal table_segments(Z_r, lam_r, [the
    segment at rep_begin = r, reps = 1]) byte for byte, (Z_r, lam_r) = standardize_table(raw, bounds,
    lap = those draws); a column's release at r is the same for every pair and eps.  -> float64
    [sum(reps), 6] in segment order, and with return_priv also [sum(reps), 6] (mean_x, sd_x, lam_x,
    mean_y, sd_y, lam_y).  A NaN in raw raises: standardize_table(na="pairwise") +
    corr_matrix_pairwise run tables with gaps."""
    import ctypes as C

    from . import _lib
    from ._segcall import pack_segments, run_segment_call
    from .signpanel import _table
    segs = list(segs)
    F, n, p = _table(raw)
    if np.isnan(F).any():
        raise ValueError("raw holds a NaN: a gap makes every record of its column's pairs NaN here; "
                         "standardize_table(na=\"pairwise\") + corr_matrix_pairwise run a table with gaps")
    lo, hi = _bounds(bounds, p)
    for a, b, *_ in segs:
        if not (0 <= int(a) < p and 0 <= int(b) < p):
            raise ValueError(f"columns ({a}, {b}) outside [0, {p})")
    arr, total = pack_segments(_lib.HrsPairSegment, segs, 6)
    import torch
    Dd = torch.as_tensor(F.reshape(-1, order="F"), device="cuda")   # the one upload
    D = C.POINTER(C.c_double)
    desc = _lib.HrsPrivateDesc(n=n, p=p, ld=n, D=Dd.data_ptr(), lo=lo.ctypes.data_as(D), hi=hi.ctypes.data_as(D),
                               eps_mean=float(eps_mean), eps_m2=float(eps_m2), seed_std=int(seed_std),
                               alpha=float(alpha), delta=1.0 / n if delta is None else float(delta),
                               nsim=int(nsim))
    if not return_priv:
        launch = lambda d, a, k, out, sp: _lib.lib.dcor_hrs_private_table_launch(d, a, k, out, None, sp)
        return run_segment_call(launch, desc, arr, len(segs), total, stream)
    st = torch.cuda.current_stream() if stream is None else stream
    with torch.cuda.stream(st):
        priv = torch.empty((max(total, 1), 6), dtype=torch.float64, device="cuda")
        launch = lambda d, a, k, out, sp: _lib.lib.dcor_hrs_private_table_launch(
            d, a, k, out, C.c_void_p(priv.data_ptr()), sp)
        res = run_segment_call(launch, desc, arr, len(segs), total, st)   # waits for the stream
        return res, priv[:total].cpu().numpy()


def corr_matrix_private(raw, bounds, eps, reps, pairs=None, eps_mean=EPS_MEAN, eps_m2=EPS_M2, seed_std=STD_SEED,
                        nsim=2000, alpha=0.05, delta=None, stream=None):
    """corr_matrix on the raw table with the standardisation drawn per replicate (private_segments):
    the same pairs, keys and result; run r of every pair uses release r of its columns."""
    run = lambda segs: private_segments(raw, bounds, segs, eps_mean=eps_mean, eps_m2=eps_m2, seed_std=seed_std,
                                        nsim=nsim, alpha=alpha, delta=delta, stream=stream)
    return _corr_matrix(run, raw, eps, reps, pairs)


def corr_matrix_sweep_private(raw, bounds, eps_grid=EPS_GRID, reps=R_PER_EPS, pairs=None, eps_mean=EPS_MEAN,
                              eps_m2=EPS_M2, seed_std=STD_SEED, nsim=2000, alpha=0.05, delta=None, stream=None):
    """corr_matrix_sweep on the raw table with the standardisation drawn per replicate
    (private_segments): the same pairs, keys and result."""
    run = lambda segs: private_segments(raw, bounds, segs, eps_mean=eps_mean, eps_m2=eps_m2, seed_std=seed_std,
                                        nsim=nsim, alpha=alpha, delta=delta, stream=stream)
    return _corr_matrix_sweep(run, raw, eps_grid, reps, pairs)


# ------------------------------- the same on pairwise-complete cases of a table with gaps
def valid_mask(Z):
    """The presence masks of the (n, p) table Z as dcor_hrs_table_pairwise_launch takes them: uint64
    [p, ceil(n / 64)], bit (i & 63) of word [c, i >> 6] set when Z[i, c] is not NaN (little-endian
    bit order); the last word's bits at i >= n are zero."""
    Z = np.asarray(Z, dtype=np.float64)
    if Z.ndim != 2 or Z.shape[0] < 1 or Z.shape[1] < 1:
        raise ValueError("Z must be an (n, p) array with n, p >= 1")
    n, p = Z.shape
    bits = np.zeros((p, 64 * ((n + 63) // 64)), dtype=np.uint8)
    bits[:, :n] = ~np.isnan(Z.T)
    return np.packbits(bits, axis=1, bitorder="little").view("<u8").astype(np.uint64).reshape(p, -1)


def _mask_rows(valid, n):
    """valid [p, nw] -> bool [p, n]: the rows each column has."""
    by = np.ascontiguousarray(valid).astype("<u8").view(np.uint8)
    return np.unpackbits(by, axis=1, bitorder="little")[:, :n].astype(bool)


def pairwise_segments(Z, lam, segs, nsim=2000, alpha=0.05, delta=None, valid=None, stream=None):
    """table_segments on the pairwise-complete cases of a table with gaps, in one native call
    (dcor_hrs_table_pairwise_launch): a segment on (col_x, col_y) runs on the n_ab rows present in
    both columns, as the reference's estimators drop NA per pair (real-data-sims.R:119-120, 187-189).
    Its records equal hrs_replicates(Z[ok, col_x], Z[ok, col_y], lam[col_x], lam[col_y], eps, reps,
    seed_ni, seed_int, rep_begin=rep_begin, mode='fused') byte for byte, with the geometry and
    delta_clip = 1 / n_ab (delta=None; :199) of that pair.  valid: the masks of valid_mask(Z) by
    default (present = not NaN); the value of Z at a row its column's mask leaves out is never used.
    Every named pair needs 2 <= n_ab <= 65536; n itself may be larger."""
    import ctypes as C

    from . import _lib
    from ._segcall import pack_segments, run_segment_call
    from .signpanel import _table
    segs = list(segs)
    F, n, p = _table(Z)
    lam = np.ascontiguousarray(lam, dtype=np.float64)
    if lam.shape != (p,):
        raise ValueError(f"lam must hold one clip bound per column ({p})")
    valid = valid_mask(F) if valid is None else np.ascontiguousarray(valid, dtype=np.uint64)
    if valid.shape != (p, (n + 63) // 64):
        raise ValueError(f"valid must be uint64 [{p}, {(n + 63) // 64}]")
    for a, b, *_ in segs:
        if not (0 <= int(a) < p and 0 <= int(b) < p):
            raise ValueError(f"columns ({a}, {b}) outside [0, {p})")
    arr, total = pack_segments(_lib.HrsPairSegment, segs, 6)
    import torch
    Dd = torch.as_tensor(F.reshape(-1, order="F"), device="cuda")   # the one upload
    desc = _lib.HrsTableNaDesc(n=n, p=p, ld=n, D=Dd.data_ptr(), lam=lam.ctypes.data_as(C.POINTER(C.c_double)),
                               valid=valid.ctypes.data_as(C.POINTER(C.c_uint64)), alpha=float(alpha),
                               delta=float("nan") if delta is None else float(delta), nsim=int(nsim))
    return run_segment_call(_lib.lib.dcor_hrs_table_pairwise_launch, desc, arr, len(segs), total, stream)


def _n_pair(Z, valid):
    """[p, p] int64: the rows present in both columns (the diagonal: in the column itself)."""
    Z = np.asarray(Z)
    V = _mask_rows(valid_mask(Z) if valid is None else valid, Z.shape[0]).astype(np.int64)
    return V @ V.T


def corr_matrix_pairwise(Z, lam, eps, reps, pairs=None, nsim=2000, alpha=0.05, delta=None, valid=None,
                         stream=None):
    """corr_matrix with every pair on its own pairwise-complete rows (pairwise_segments): the same
    pairs, keys and result, and "n_pair", the [p, p] integer matrix of the pairs' counts n_ab."""
    run = lambda segs: pairwise_segments(Z, lam, segs, nsim=nsim, alpha=alpha, delta=delta, valid=valid,
                                         stream=stream)
    return {**_corr_matrix(run, Z, eps, reps, pairs), "n_pair": _n_pair(Z, valid)}


def corr_matrix_sweep_pairwise(Z, lam, eps_grid=EPS_GRID, reps=R_PER_EPS, pairs=None, nsim=2000, alpha=0.05,
                               delta=None, valid=None, stream=None):
    """corr_matrix_sweep with every pair on its own pairwise-complete rows (pairwise_segments): the
    same pairs, keys and result, and "n_pair", the [p, p] integer matrix of the pairs' counts n_ab."""
    run = lambda segs: pairwise_segments(Z, lam, segs, nsim=nsim, alpha=alpha, delta=delta, valid=valid,
                                         stream=stream)
    return {**_corr_matrix_sweep(run, Z, eps_grid, reps, pairs), "n_pair": _n_pair(Z, valid)}


# ------------- raw columns with gaps: the private standardisation per replicate, every pair on its own rows
def private_pairwise_segments(raw, bounds, segs, eps_mean=EPS_MEAN, eps_m2=EPS_M2, seed_std=STD_SEED, nsim=2000,
                              alpha=0.05, delta=None, valid=None, return_priv=False, stream=None):
    """private_segments on a RAW (n, p) table with gaps, in one native call
    (dcor_hrs_private_pairwise_launch): the reference's real-data pipeline, replicated.  In replicate r
    column c is released by dp_sd from its own present rows (count n_c; real-data-sims.R:74) with the
    unit Laplace pair dcor_draws_launch(0, seed_std, 17, r, 1, 2 p)[2 c : 2 c + 2], and a segment on
    (col_x, col_y) runs on the n_ab rows present in both columns (:119-120, 187-189) with the geometry
    and delta_clip = 1 / n_ab (delta=None) of that pair.  Its records equal pairwise_segments(Z_r, lam_r,
    [the segment at rep_begin = r, reps = 1], valid=valid) byte for byte, (Z_r, lam_r) =
    standardize_table(raw, bounds, lap = those draws, na="pairwise").  valid: the masks of
    valid_mask(raw) by default (present = not NaN); the value of raw at a row its column's mask leaves
    out is never used.  Every named pair needs 2 <= n_ab <= 65536.  -> float64 [sum(reps), 6] in segment
    order, and with return_priv also [sum(reps), 6] (mean_x, sd_x, lam_x, mean_y, sd_y, lam_y)."""
    import ctypes as C

    from . import _lib
    from ._segcall import pack_segments, run_segment_call
    from .signpanel import _table
    segs = list(segs)
    F, n, p = _table(raw)
    lo, hi = _bounds(bounds, p)
    valid = valid_mask(F) if valid is None else np.ascontiguousarray(valid, dtype=np.uint64)
    if valid.shape != (p, (n + 63) // 64):
        raise ValueError(f"valid must be uint64 [{p}, {(n + 63) // 64}]")
    for a, b, *_ in segs:
        if not (0 <= int(a) < p and 0 <= int(b) < p):
            raise ValueError(f"columns ({a}, {b}) outside [0, {p})")
    arr, total = pack_segments(_lib.HrsPairSegment, segs, 6)
    import torch
    Dd = torch.as_tensor(F.reshape(-1, order="F"), device="cuda")   # the one upload
    D = C.POINTER(C.c_double)
    desc = _lib.HrsPrivateNaDesc(n=n, p=p, ld=n, D=Dd.data_ptr(), lo=lo.ctypes.data_as(D), hi=hi.ctypes.data_as(D),
                                 valid=valid.ctypes.data_as(C.POINTER(C.c_uint64)), eps_mean=float(eps_mean),
                                 eps_m2=float(eps_m2), seed_std=int(seed_std), alpha=float(alpha),
                                 delta=float("nan") if delta is None else float(delta), nsim=int(nsim))
    if not return_priv:
        launch = lambda d, a, k, out, sp: _lib.lib.dcor_hrs_private_pairwise_launch(d, a, k, out, None, sp)
        return run_segment_call(launch, desc, arr, len(segs), total, stream)
    st = torch.cuda.current_stream() if stream is None else stream
    with torch.cuda.stream(st):
        priv = torch.empty((max(total, 1), 6), dtype=torch.float64, device="cuda")
        launch = lambda d, a, k, out, sp: _lib.lib.dcor_hrs_private_pairwise_launch(
            d, a, k, out, C.c_void_p(priv.data_ptr()), sp)
        res = run_segment_call(launch, desc, arr, len(segs), total, st)   # waits for the stream
        return res, priv[:total].cpu().numpy()


def corr_matrix_private_pairwise(raw, bounds, eps, reps, pairs=None, eps_mean=EPS_MEAN, eps_m2=EPS_M2,
                                 seed_std=STD_SEED, nsim=2000, alpha=0.05, delta=None, valid=None, stream=None):
    """corr_matrix_private on a raw table with gaps (private_pairwise_segments): the same pairs, keys
    and result, and "n_pair", the [p, p] integer matrix of the pairs' counts n_ab (the diagonal: n_c)."""
    run = lambda segs: private_pairwise_segments(raw, bounds, segs, eps_mean=eps_mean, eps_m2=eps_m2,
                                                 seed_std=seed_std, nsim=nsim, alpha=alpha, delta=delta,
                                                 valid=valid, stream=stream)
    return {**_corr_matrix(run, raw, eps, reps, pairs), "n_pair": _n_pair(raw, valid)}


def corr_matrix_sweep_private_pairwise(raw, bounds, eps_grid=EPS_GRID, reps=R_PER_EPS, pairs=None,
                                       eps_mean=EPS_MEAN, eps_m2=EPS_M2, seed_std=STD_SEED, nsim=2000, alpha=0.05,
                                       delta=None, valid=None, stream=None):
    """corr_matrix_sweep_private on a raw table with gaps (private_pairwise_segments): the same pairs,
    keys and result, and "n_pair", the [p, p] integer matrix of the pairs' counts n_ab."""
    run = lambda segs: private_pairwise_segments(raw, bounds, segs, eps_mean=eps_mean, eps_m2=eps_m2,
                                                 seed_std=seed_std, nsim=nsim, alpha=alpha, delta=delta,
                                                 valid=valid, stream=stream)
    return {**_corr_matrix_sweep(run, raw, eps_grid, reps, pairs), "n_pair": _n_pair(raw, valid)}
