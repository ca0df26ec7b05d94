"""CPU tests of the four segment-list entries (dcor_hrs_sweep_launch, dcor_hrs_fused_sweep_launch,
dcor_sign_panel_launch, dcor_sign_table_launch): every call they reject, or finish, before the
device query -- its status code, the complete dcor_last_error() text and an unmoved
dcor_alloc_count().  EXPECTED was recorded from the library before the entries' host halves moved
into the planning unit (csrc/dcor_plan.cpp); the refactored entries have to give the same.

No case reaches a launch: each ends in a rejection, in DCOR_OK for a call without replicates, or
(NO_GPU cases, run only where no device is visible) in DCOR_ENODEV.  The pointers are fakes that
are never dereferenced; the panel is a block whose first three fields (X, Y, n) are all the HRS
entries read of a dcor_panel before the device query."""
import ctypes as C

import pytest

FAKE = 8            # a non-null pointer value that is never dereferenced
SENTINEL = "unknown implementation switch sentinel"
STATUS = {0: "OK", 1: "EINVAL", 2: "EKLT1", 3: "EHIP", 4: "ENOMEM", 5: "ENODEV", 6: "EFORK"}
NAN, INF = float("nan"), float("inf")
R31 = 2**31 - 1
RB_MAX = 2**32 - 1


class FakePanel(C.Structure):
    _fields_ = [("X", C.c_void_p), ("Y", C.c_void_p), ("n", C.c_int64), ("rest", C.c_int64 * 29)]


def _hrs_call(name, base=None, panel=None, segs=(), nseg=None, out=FAKE, null=()):
    """base / panel: field overrides; segs: HrsSegment field dicts; null: arguments passed as NULL."""
    from dcor import _lib
    b = dict(n=10, eta1=1.0, eta2=1.0, alpha=0.05, hrs=1, lam_x=2.0, lam_y=2.0, lam_s=2.0, lam_o=2.0,
             delta=0.1, nsim=10, X=FAKE, Y=FAKE)
    b.update(base or {})
    pn = FakePanel(**{**dict(X=FAKE, Y=FAKE, n=10), **(panel or {})})
    base_s = _lib.PrematSubg(**b)
    arr = (_lib.HrsSegment * max(1, len(segs)))(
        *[_lib.HrsSegment(**{**dict(eps=1.0, seed_ni=1, seed_int=2, reps=1), **s}) for s in segs])
    return getattr(_lib.lib, name)(
        None if "base" in null else C.byref(base_s), None if "panel" in null else C.byref(pn),
        None if "segs" in null else arr, len(segs) if nseg is None else nseg,
        None if "out" in null else C.c_void_p(out), None)


def _sign_call(name, desc=None, segs=(), nseg=None, out=FAKE, null=()):
    from dcor import _lib
    table = name == "dcor_sign_table_launch"
    if table:
        d = dict(n=100, p=3, ld=100, D=FAKE, alpha=0.05, normalise=1, ci_mode=0, nsim=1000)
        seg_t, seg0 = _lib.SignPairSegment, dict(eps1=1.0, eps2=1.0, seed=1, reps=1, col_x=0, col_y=1)
    else:
        d = dict(n=100, X=FAKE, Y=FAKE, alpha=0.05, normalise=1, ci_mode=0, nsim=1000)
        seg_t, seg0 = _lib.SignSegment, dict(eps1=1.0, eps2=1.0, seed=1, reps=1)
    d.update(desc or {})
    desc_s = (_lib.SignTableDesc if table else _lib.SignPanelDesc)(**d)
    arr = (seg_t * max(1, len(segs)))(*[seg_t(**{**seg0, **s}) for s in segs])
    return getattr(_lib.lib, name)(
        None if "desc" in null else C.byref(desc_s), None if "segs" in null else arr,
        len(segs) if nseg is None else nseg, None if "out" in null else C.c_void_p(out), None)


HRS = {"hrs_sweep": "dcor_hrs_sweep_launch", "hrs_fused_sweep": "dcor_hrs_fused_sweep_launch"}
SIGN = {"sign_panel": "dcor_sign_panel_launch", "sign_table": "dcor_sign_table_launch"}
NO_GPU = set()      # ids of the valid calls that reach the device query


def _cases():
    """id -> zero-argument call.  Ids start with the entry's short name."""
    cases = {}

    def add(key, fn, *a, no_gpu=False, **kw):
        assert key not in cases, key
        cases[key] = lambda: fn(*a, **kw)
        if no_gpu:
            NO_GPU.add(key)

    for short, name in HRS.items():
        def h(key, **kw):
            add(f"{short}/{key}", _hrs_call, name, no_gpu=kw.pop("no_gpu", False), **kw)
        one = [{}]
        for arg in ("base", "panel", "segs", "out"):
            h(f"null_{arg}", segs=one, null=(arg,))
        h("nseg_negative", segs=one, nseg=-1)
        h("nseg_zero", nseg=0, null=("segs", "out"))
        h("nseg_zero_panel_mismatch", nseg=0, panel=dict(n=11), null=("segs", "out"))
        for fld, val in (("eps", 0.0), ("eps", NAN), ("eps", -1.0), ("reps", -1), ("rep_begin", -1), ("out_row", -1)):
            h(f"seg0_{fld}_{val}", segs=[{fld: val}, {}, {}])
            h(f"last_{fld}_{val}", segs=[{}, {}, {fld: val}])
        h("rep_begin_max_reps0", segs=[dict(rep_begin=RB_MAX, reps=0)])
        h("rep_begin_max_reps0_then_valid", segs=[dict(rep_begin=RB_MAX, reps=0), {}], no_gpu=True)
        h("rep_begin_max_reps1", segs=[dict(rep_begin=RB_MAX, reps=1)])
        h("rep_begin_max_reps1_last", segs=[{}, dict(rep_begin=RB_MAX, reps=1)])
        h("rep_range_int64", segs=[{}, dict(rep_begin=2**63 - 2, reps=2)])
        # the running total: 2^31 - 1 passes the cap (the next check to fail is the bad third segment),
        # 2^31 does not -- except in the materialised sweep, which has no cap
        h("total_r31_then_bad", segs=[dict(reps=R31 - 5), dict(reps=5), dict(reps=-1)])
        h("total_r31_plus1_then_bad", segs=[dict(reps=R31 - 5), dict(reps=6), dict(reps=-1)])
        h("total_r31", segs=[dict(reps=R31 - 5), dict(reps=5)], no_gpu=True)
        h("total_r31_plus1", segs=[dict(reps=R31 - 5), dict(reps=6)], no_gpu=True)
        for fld, val in (("X", 16), ("Y", 16), ("n", 11)):
            h(f"panel_mismatch_{fld}", segs=one, panel={fld: val})
        h("xy_stride", segs=one, base=dict(xy_stride=10))
        h("hrs0", segs=one, base=dict(hrs=0))
        for val in (0.0, -1.0, NAN):
            h(f"delta_{val}", segs=one, base=dict(delta=val))
        # launch constants: make_subg's checks, also for a segment without replicates
        h("const_eps_inf", segs=[{}, dict(eps=INF)])
        h("const_eps_inf_reps0", segs=[{}, dict(eps=INF, reps=0)])
        h("const_alpha", segs=one, base=dict(alpha=2.0))
        h("const_nsim0_all_reps0", segs=[dict(reps=0)], base=dict(nsim=0))
        h("const_nsim_2049", segs=one, base=dict(nsim=2049))
        h("const_n1", segs=one, base=dict(n=1), panel=dict(n=1))
        h("const_misaligned", segs=one, base=dict(X=12), panel=dict(X=12))
        h("all_reps0", segs=[dict(reps=0), dict(reps=0, eps=2.0)])
        # two violations at once: which one is reported
        h("order_bad_segment_and_panel", segs=[dict(reps=-1)], panel=dict(n=11))
        h("order_bad_segment_and_hrs0", segs=[dict(reps=-1)], base=dict(hrs=0))
        h("order_bad_segment_and_delta", segs=[dict(reps=-1)], base=dict(delta=0.0))
        h("order_seg0_const_and_seg1_field", segs=[dict(eps=INF), dict(reps=-1)])
        h("order_seg0_const_and_seg1_range", segs=[dict(eps=INF), dict(rep_begin=RB_MAX)])
        h("order_cap_and_panel", segs=[dict(reps=R31), dict(reps=1)], panel=dict(n=11))
        h("order_hrs0_and_delta", segs=one, base=dict(hrs=0, delta=0.0))

    for short, name in SIGN.items():
        table = short == "sign_table"

        def s(key, **kw):
            add(f"{short}/{key}", _sign_call, name, no_gpu=kw.pop("no_gpu", False), **kw)
        one = [{}]
        for arg in ("desc", "segs", "out"):
            s(f"null_{arg}", segs=one, null=(arg,))
        s("nseg_negative", segs=one, nseg=-1)
        s("nseg_zero", nseg=0, null=("segs", "out"))
        if table:
            s("null_D", segs=one, desc=dict(D=0))
            s("nseg_zero_null_D", nseg=0, desc=dict(D=0), null=("segs", "out"))
        else:
            s("null_X", segs=one, desc=dict(X=0))
            s("null_Y", segs=one, desc=dict(Y=0))
            s("nseg_zero_null_X", nseg=0, desc=dict(X=0), null=("segs", "out"))
        for fld, val in (("eps1", 0.0), ("eps2", 0.0), ("eps1", NAN), ("eps2", -1.0), ("reps", -1),
                         ("rep_begin", -1), ("out_row", -1)):
            s(f"seg0_{fld}_{val}", segs=[{fld: val}, {}, {}])
            s(f"last_{fld}_{val}", segs=[{}, {}, {fld: val}])
        s("rep_begin_max_reps0", segs=[dict(rep_begin=RB_MAX, reps=0)])
        s("rep_begin_max_reps0_then_valid", segs=[dict(rep_begin=RB_MAX, reps=0), {}], no_gpu=True)
        s("rep_begin_max_reps1", segs=[dict(rep_begin=RB_MAX, reps=1)])
        s("rep_begin_max_reps1_last", segs=[{}, dict(rep_begin=RB_MAX, reps=1)])
        s("rep_range_int64", segs=[{}, dict(rep_begin=2**63 - 2, reps=2)])
        s("total_r31_then_bad", segs=[dict(reps=R31 - 5), dict(reps=5), dict(reps=-1)])
        s("total_r31_plus1_then_bad", segs=[dict(reps=R31 - 5), dict(reps=6), dict(reps=-1)])
        s("total_r31", segs=[dict(reps=R31 - 5), dict(reps=5)], no_gpu=True)
        s("total_r31_plus1", segs=[dict(reps=R31 - 5), dict(reps=6)], no_gpu=True)
        # launch constants: make_sign's checks, also for a segment without replicates
        s("const_klt1", segs=[{}, dict(eps1=0.2, eps2=0.2)])
        s("const_klt1_reps0", segs=[{}, dict(eps1=0.2, eps2=0.2, reps=0)])
        s("const_eps_inf_reps0", segs=[dict(reps=0), dict(eps2=INF, reps=0)])
        s("const_n0", segs=one, desc=dict(n=0, ld=0) if table else dict(n=0))
        s("const_n_2p31", segs=one, desc=dict(n=2**31, ld=2**31) if table else dict(n=2**31))
        s("const_alpha", segs=one, desc=dict(alpha=2.0))
        s("const_ci_mode", segs=one, desc=dict(ci_mode=7))
        s("const_nsim0_all_reps0", segs=[dict(reps=0)], desc=dict(nsim=0))
        s("const_nsim_2049", segs=one, desc=dict(nsim=2049))
        s("all_reps0", segs=[dict(reps=0), dict(reps=0, eps1=2.0)])
        s("order_seg0_const_and_seg1_field", segs=[dict(eps1=0.2, eps2=0.2), dict(reps=-1)])
        s("order_cap_and_const", segs=[dict(reps=R31, eps1=0.2, eps2=0.2), dict(reps=1)])
        if table:
            for p in (0, -3, 2**31):
                s(f"p_{p}", segs=one, desc=dict(p=p))
            s("ld_lt_n", segs=one, desc=dict(ld=99))
            for fld, val in (("col_x", 3), ("col_y", 3), ("col_x", -1), ("col_y", 2**31 - 1)):
                s(f"seg0_{fld}_{val}", segs=[{fld: val}, {}, {}])
                s(f"last_{fld}_{val}", segs=[{}, {}, {fld: val}])
            s("col_reps0", segs=[{}, dict(col_y=3, reps=0)])
            s("layout_overflow", segs=one, desc=dict(n=R31, p=R31, ld=R31))
            s("layout_overflow_all_reps0", segs=[dict(reps=0)], desc=dict(n=R31, p=R31, ld=R31))
            s("order_bad_segment_and_ld", segs=[dict(reps=-1)], desc=dict(ld=99))
            s("order_bad_segment_and_p", segs=[dict(reps=-1)], desc=dict(p=0))
            s("order_p_and_ld", segs=one, desc=dict(p=0, ld=99))
            s("order_null_D_and_p", segs=one, desc=dict(D=0, p=0))
            s("order_field_column_range", segs=[dict(out_row=-1, col_x=3, rep_begin=RB_MAX)])
            s("order_column_range", segs=[dict(col_x=3, rep_begin=RB_MAX)])
            s("order_seg0_range_and_seg1_column", segs=[dict(rep_begin=RB_MAX), dict(col_x=3)])
            s("order_const_and_layout", segs=one, desc=dict(n=R31, p=R31, ld=R31, alpha=2.0))
        else:
            s("order_bad_segment_and_null_X", segs=[dict(reps=-1)], desc=dict(X=0))
    return cases


CASES = _cases()

# (status, dcor_last_error() after the call); SENTINEL: the call left the last error alone
EXPECTED = {
    'hrs_sweep/null_base': ('EINVAL', 'hrs_sweep: null argument'),
    'hrs_sweep/null_panel': ('EINVAL', 'hrs_sweep: null argument'),
    'hrs_sweep/null_segs': ('EINVAL', 'hrs_sweep: null argument'),
    'hrs_sweep/null_out': ('EINVAL', 'hrs_sweep: null argument'),
    'hrs_sweep/nseg_negative': ('EINVAL', 'hrs_sweep: null argument'),
    'hrs_sweep/nseg_zero': ('OK', SENTINEL),
    'hrs_sweep/nseg_zero_panel_mismatch': ('EINVAL', "hrs_sweep: X, Y, n must be the panel's and xy_stride 0"),
    'hrs_sweep/seg0_eps_0.0': ('EINVAL', 'hrs_sweep: segment 0: need eps > 0, reps, rep_begin, out_row >= 0'),
    'hrs_sweep/last_eps_0.0': ('EINVAL', 'hrs_sweep: segment 2: need eps > 0, reps, rep_begin, out_row >= 0'),
    'hrs_sweep/seg0_eps_nan': ('EINVAL', 'hrs_sweep: segment 0: need eps > 0, reps, rep_begin, out_row >= 0'),
    'hrs_sweep/last_eps_nan': ('EINVAL', 'hrs_sweep: segment 2: need eps > 0, reps, rep_begin, out_row >= 0'),
    'hrs_sweep/seg0_eps_-1.0': ('EINVAL', 'hrs_sweep: segment 0: need eps > 0, reps, rep_begin, out_row >= 0'),
    'hrs_sweep/last_eps_-1.0': ('EINVAL', 'hrs_sweep: segment 2: need eps > 0, reps, rep_begin, out_row >= 0'),
    'hrs_sweep/seg0_reps_-1': ('EINVAL', 'hrs_sweep: segment 0: need eps > 0, reps, rep_begin, out_row >= 0'),
    'hrs_sweep/last_reps_-1': ('EINVAL', 'hrs_sweep: segment 2: need eps > 0, reps, rep_begin, out_row >= 0'),
    'hrs_sweep/seg0_rep_begin_-1': ('EINVAL', 'hrs_sweep: segment 0: need eps > 0, reps, rep_begin, out_row >= 0'),
    'hrs_sweep/last_rep_begin_-1': ('EINVAL', 'hrs_sweep: segment 2: need eps > 0, reps, rep_begin, out_row >= 0'),
    'hrs_sweep/seg0_out_row_-1': ('EINVAL', 'hrs_sweep: segment 0: need eps > 0, reps, rep_begin, out_row >= 0'),
    'hrs_sweep/last_out_row_-1': ('EINVAL', 'hrs_sweep: segment 2: need eps > 0, reps, rep_begin, out_row >= 0'),
    'hrs_sweep/rep_begin_max_reps0': ('OK', SENTINEL),
    'hrs_sweep/rep_begin_max_reps0_then_valid': ('ENODEV', 'no HIP device visible: the dcor engine has no CPU path'),
    'hrs_sweep/rep_begin_max_reps1': ('EINVAL', 'hrs_sweep: segment 0: replicate range exceeds 2^32'),
    'hrs_sweep/rep_begin_max_reps1_last': ('EINVAL', 'hrs_sweep: segment 1: replicate range exceeds 2^32'),
    'hrs_sweep/rep_range_int64': ('EINVAL', 'hrs_sweep: segment 1: replicate range exceeds 2^32'),
    'hrs_sweep/total_r31_then_bad': ('EINVAL', 'hrs_sweep: segment 2: need eps > 0, reps, rep_begin, out_row >= 0'),
    'hrs_sweep/total_r31_plus1_then_bad': ('EINVAL', 'hrs_sweep: segment 2: need eps > 0, reps, rep_begin, out_row >= 0'),
    'hrs_sweep/total_r31': ('ENODEV', 'no HIP device visible: the dcor engine has no CPU path'),
    'hrs_sweep/total_r31_plus1': ('ENODEV', 'no HIP device visible: the dcor engine has no CPU path'),
    'hrs_sweep/panel_mismatch_X': ('EINVAL', "hrs_sweep: X, Y, n must be the panel's and xy_stride 0"),
    'hrs_sweep/panel_mismatch_Y': ('EINVAL', "hrs_sweep: X, Y, n must be the panel's and xy_stride 0"),
    'hrs_sweep/panel_mismatch_n': ('EINVAL', "hrs_sweep: X, Y, n must be the panel's and xy_stride 0"),
    'hrs_sweep/xy_stride': ('EINVAL', "hrs_sweep: X, Y, n must be the panel's and xy_stride 0"),
    'hrs_sweep/hrs0': ('EINVAL', 'hrs_sweep: the HRS variant only (hrs = 1)'),
    'hrs_sweep/delta_0.0': ('EINVAL', 'hrs_sweep: delta must be positive'),
    'hrs_sweep/delta_-1.0': ('EINVAL', 'hrs_sweep: delta must be positive'),
    'hrs_sweep/delta_nan': ('EINVAL', 'hrs_sweep: delta must be positive'),
    'hrs_sweep/const_eps_inf': ('EINVAL', 'eps1 > 0 and eps2 > 0 required (vert-cor.R:264)'),
    'hrs_sweep/const_eps_inf_reps0': ('EINVAL', 'eps1 > 0 and eps2 > 0 required (vert-cor.R:264)'),
    'hrs_sweep/const_alpha': ('EINVAL', "alpha must be < 2 (R's mixquant index ceiling((1-alpha/2)*nsim) >= 1)"),
    'hrs_sweep/const_nsim0_all_reps0': ('EINVAL', 'nsim must be in [1, 2048] (got 0)'),
    'hrs_sweep/const_nsim_2049': ('EINVAL', 'nsim must be in [1, 2048] (got 2049)'),
    'hrs_sweep/const_n1': ('EINVAL', 'n >= 2 required (real-data-sims.R:121)'),
    'hrs_sweep/const_misaligned': ('EINVAL', 'premat_subg: arrays must be aligned to their element size'),
    'hrs_sweep/all_reps0': ('OK', SENTINEL),
    'hrs_sweep/order_bad_segment_and_panel': ('EINVAL', "hrs_sweep: X, Y, n must be the panel's and xy_stride 0"),
    'hrs_sweep/order_bad_segment_and_hrs0': ('EINVAL', 'hrs_sweep: the HRS variant only (hrs = 1)'),
    'hrs_sweep/order_bad_segment_and_delta': ('EINVAL', 'hrs_sweep: delta must be positive'),
    'hrs_sweep/order_seg0_const_and_seg1_field': ('EINVAL', 'eps1 > 0 and eps2 > 0 required (vert-cor.R:264)'),
    'hrs_sweep/order_seg0_const_and_seg1_range': ('EINVAL', 'eps1 > 0 and eps2 > 0 required (vert-cor.R:264)'),
    'hrs_sweep/order_cap_and_panel': ('EINVAL', "hrs_sweep: X, Y, n must be the panel's and xy_stride 0"),
    'hrs_sweep/order_hrs0_and_delta': ('EINVAL', 'hrs_sweep: the HRS variant only (hrs = 1)'),
    'hrs_fused_sweep/null_base': ('EINVAL', 'hrs_fused_sweep: null argument'),
    'hrs_fused_sweep/null_panel': ('EINVAL', 'hrs_fused_sweep: null argument'),
    'hrs_fused_sweep/null_segs': ('EINVAL', 'hrs_fused_sweep: null argument'),
    'hrs_fused_sweep/null_out': ('EINVAL', 'hrs_fused_sweep: null argument'),
    'hrs_fused_sweep/nseg_negative': ('EINVAL', 'hrs_fused_sweep: null argument'),
    'hrs_fused_sweep/nseg_zero': ('OK', SENTINEL),
    'hrs_fused_sweep/nseg_zero_panel_mismatch': ('OK', SENTINEL),
    'hrs_fused_sweep/seg0_eps_0.0': ('EINVAL', 'hrs_fused_sweep: segment 0: need eps > 0, reps, rep_begin, out_row >= 0'),
    'hrs_fused_sweep/last_eps_0.0': ('EINVAL', 'hrs_fused_sweep: segment 2: need eps > 0, reps, rep_begin, out_row >= 0'),
    'hrs_fused_sweep/seg0_eps_nan': ('EINVAL', 'hrs_fused_sweep: segment 0: need eps > 0, reps, rep_begin, out_row >= 0'),
    'hrs_fused_sweep/last_eps_nan': ('EINVAL', 'hrs_fused_sweep: segment 2: need eps > 0, reps, rep_begin, out_row >= 0'),
    'hrs_fused_sweep/seg0_eps_-1.0': ('EINVAL', 'hrs_fused_sweep: segment 0: need eps > 0, reps, rep_begin, out_row >= 0'),
    'hrs_fused_sweep/last_eps_-1.0': ('EINVAL', 'hrs_fused_sweep: segment 2: need eps > 0, reps, rep_begin, out_row >= 0'),
    'hrs_fused_sweep/seg0_reps_-1': ('EINVAL', 'hrs_fused_sweep: segment 0: need eps > 0, reps, rep_begin, out_row >= 0'),
    'hrs_fused_sweep/last_reps_-1': ('EINVAL', 'hrs_fused_sweep: segment 2: need eps > 0, reps, rep_begin, out_row >= 0'),
    'hrs_fused_sweep/seg0_rep_begin_-1': ('EINVAL', 'hrs_fused_sweep: segment 0: need eps > 0, reps, rep_begin, out_row >= 0'),
    'hrs_fused_sweep/last_rep_begin_-1': ('EINVAL', 'hrs_fused_sweep: segment 2: need eps > 0, reps, rep_begin, out_row >= 0'),
    'hrs_fused_sweep/seg0_out_row_-1': ('EINVAL', 'hrs_fused_sweep: segment 0: need eps > 0, reps, rep_begin, out_row >= 0'),
    'hrs_fused_sweep/last_out_row_-1': ('EINVAL', 'hrs_fused_sweep: segment 2: need eps > 0, reps, rep_begin, out_row >= 0'),
    'hrs_fused_sweep/rep_begin_max_reps0': ('OK', SENTINEL),
    'hrs_fused_sweep/rep_begin_max_reps0_then_valid': ('ENODEV', 'no HIP device visible: the dcor engine has no CPU path'),
    'hrs_fused_sweep/rep_begin_max_reps1': ('EINVAL', 'hrs_fused_sweep: segment 0: replicate range exceeds 2^32'),
    'hrs_fused_sweep/rep_begin_max_reps1_last': ('EINVAL', 'hrs_fused_sweep: segment 1: replicate range exceeds 2^32'),
    'hrs_fused_sweep/rep_range_int64': ('EINVAL', 'hrs_fused_sweep: segment 1: replicate range exceeds 2^32'),
    'hrs_fused_sweep/total_r31_then_bad': ('EINVAL', 'hrs_fused_sweep: segment 2: need eps > 0, reps, rep_begin, out_row >= 0'),
    'hrs_fused_sweep/total_r31_plus1_then_bad': ('EINVAL', 'hrs_fused_sweep: more than 2^31 - 1 replicates in one call'),
    'hrs_fused_sweep/total_r31': ('ENODEV', 'no HIP device visible: the dcor engine has no CPU path'),
    'hrs_fused_sweep/total_r31_plus1': ('EINVAL', 'hrs_fused_sweep: more than 2^31 - 1 replicates in one call'),
    'hrs_fused_sweep/panel_mismatch_X': ('EINVAL', "hrs_fused_sweep: X, Y, n must be the panel's and xy_stride 0"),
    'hrs_fused_sweep/panel_mismatch_Y': ('EINVAL', "hrs_fused_sweep: X, Y, n must be the panel's and xy_stride 0"),
    'hrs_fused_sweep/panel_mismatch_n': ('EINVAL', "hrs_fused_sweep: X, Y, n must be the panel's and xy_stride 0"),
    'hrs_fused_sweep/xy_stride': ('EINVAL', "hrs_fused_sweep: X, Y, n must be the panel's and xy_stride 0"),
    'hrs_fused_sweep/hrs0': ('EINVAL', 'hrs_fused_sweep: the HRS variant only (hrs = 1)'),
    'hrs_fused_sweep/delta_0.0': ('EINVAL', 'hrs_fused_sweep: delta must be positive'),
    'hrs_fused_sweep/delta_-1.0': ('EINVAL', 'hrs_fused_sweep: delta must be positive'),
    'hrs_fused_sweep/delta_nan': ('EINVAL', 'hrs_fused_sweep: delta must be positive'),
    'hrs_fused_sweep/const_eps_inf': ('EINVAL', 'eps1 > 0 and eps2 > 0 required (vert-cor.R:264)'),
    'hrs_fused_sweep/const_eps_inf_reps0': ('EINVAL', 'eps1 > 0 and eps2 > 0 required (vert-cor.R:264)'),
    'hrs_fused_sweep/const_alpha': ('EINVAL', "alpha must be < 2 (R's mixquant index ceiling((1-alpha/2)*nsim) >= 1)"),
    'hrs_fused_sweep/const_nsim0_all_reps0': ('EINVAL', 'nsim must be in [1, 2048] (got 0)'),
    'hrs_fused_sweep/const_nsim_2049': ('EINVAL', 'nsim must be in [1, 2048] (got 2049)'),
    'hrs_fused_sweep/const_n1': ('EINVAL', 'n >= 2 required (real-data-sims.R:121)'),
    'hrs_fused_sweep/const_misaligned': ('EINVAL', 'premat_subg: arrays must be aligned to their element size'),
    'hrs_fused_sweep/all_reps0': ('OK', SENTINEL),
    'hrs_fused_sweep/order_bad_segment_and_panel': ('EINVAL', 'hrs_fused_sweep: segment 0: need eps > 0, reps, rep_begin, out_row >= 0'),
    'hrs_fused_sweep/order_bad_segment_and_hrs0': ('EINVAL', 'hrs_fused_sweep: segment 0: need eps > 0, reps, rep_begin, out_row >= 0'),
    'hrs_fused_sweep/order_bad_segment_and_delta': ('EINVAL', 'hrs_fused_sweep: segment 0: need eps > 0, reps, rep_begin, out_row >= 0'),
    'hrs_fused_sweep/order_seg0_const_and_seg1_field': ('EINVAL', 'hrs_fused_sweep: segment 1: need eps > 0, reps, rep_begin, out_row >= 0'),
    'hrs_fused_sweep/order_seg0_const_and_seg1_range': ('EINVAL', 'hrs_fused_sweep: segment 1: replicate range exceeds 2^32'),
    'hrs_fused_sweep/order_cap_and_panel': ('EINVAL', 'hrs_fused_sweep: more than 2^31 - 1 replicates in one call'),
    'hrs_fused_sweep/order_hrs0_and_delta': ('EINVAL', 'hrs_fused_sweep: the HRS variant only (hrs = 1)'),
    'sign_panel/null_desc': ('EINVAL', 'sign_panel: null argument'),
    'sign_panel/null_segs': ('EINVAL', 'sign_panel: null argument'),
    'sign_panel/null_out': ('EINVAL', 'sign_panel: null argument'),
    'sign_panel/nseg_negative': ('EINVAL', 'sign_panel: null argument'),
    'sign_panel/nseg_zero': ('OK', SENTINEL),
    'sign_panel/null_X': ('EINVAL', 'sign_panel: null argument (X, Y)'),
    'sign_panel/null_Y': ('EINVAL', 'sign_panel: null argument (X, Y)'),
    'sign_panel/nseg_zero_null_X': ('OK', SENTINEL),
    'sign_panel/seg0_eps1_0.0': ('EINVAL', 'sign_panel: segment 0: need eps1, eps2 > 0, reps, rep_begin, out_row >= 0'),
    'sign_panel/last_eps1_0.0': ('EINVAL', 'sign_panel: segment 2: need eps1, eps2 > 0, reps, rep_begin, out_row >= 0'),
    'sign_panel/seg0_eps2_0.0': ('EINVAL', 'sign_panel: segment 0: need eps1, eps2 > 0, reps, rep_begin, out_row >= 0'),
    'sign_panel/last_eps2_0.0': ('EINVAL', 'sign_panel: segment 2: need eps1, eps2 > 0, reps, rep_begin, out_row >= 0'),
    'sign_panel/seg0_eps1_nan': ('EINVAL', 'sign_panel: segment 0: need eps1, eps2 > 0, reps, rep_begin, out_row >= 0'),
    'sign_panel/last_eps1_nan': ('EINVAL', 'sign_panel: segment 2: need eps1, eps2 > 0, reps, rep_begin, out_row >= 0'),
    'sign_panel/seg0_eps2_-1.0': ('EINVAL', 'sign_panel: segment 0: need eps1, eps2 > 0, reps, rep_begin, out_row >= 0'),
    'sign_panel/last_eps2_-1.0': ('EINVAL', 'sign_panel: segment 2: need eps1, eps2 > 0, reps, rep_begin, out_row >= 0'),
    'sign_panel/seg0_reps_-1': ('EINVAL', 'sign_panel: segment 0: need eps1, eps2 > 0, reps, rep_begin, out_row >= 0'),
    'sign_panel/last_reps_-1': ('EINVAL', 'sign_panel: segment 2: need eps1, eps2 > 0, reps, rep_begin, out_row >= 0'),
    'sign_panel/seg0_rep_begin_-1': ('EINVAL', 'sign_panel: segment 0: need eps1, eps2 > 0, reps, rep_begin, out_row >= 0'),
    'sign_panel/last_rep_begin_-1': ('EINVAL', 'sign_panel: segment 2: need eps1, eps2 > 0, reps, rep_begin, out_row >= 0'),
    'sign_panel/seg0_out_row_-1': ('EINVAL', 'sign_panel: segment 0: need eps1, eps2 > 0, reps, rep_begin, out_row >= 0'),
    'sign_panel/last_out_row_-1': ('EINVAL', 'sign_panel: segment 2: need eps1, eps2 > 0, reps, rep_begin, out_row >= 0'),
    'sign_panel/rep_begin_max_reps0': ('OK', SENTINEL),
    'sign_panel/rep_begin_max_reps0_then_valid': ('ENODEV', 'no HIP device visible: the dcor engine has no CPU path'),
    'sign_panel/rep_begin_max_reps1': ('EINVAL', 'sign_panel: segment 0: replicate range exceeds 2^32'),
    'sign_panel/rep_begin_max_reps1_last': ('EINVAL', 'sign_panel: segment 1: replicate range exceeds 2^32'),
    'sign_panel/rep_range_int64': ('EINVAL', 'sign_panel: segment 1: replicate range exceeds 2^32'),
    'sign_panel/total_r31_then_bad': ('EINVAL', 'sign_panel: segment 2: need eps1, eps2 > 0, reps, rep_begin, out_row >= 0'),
    'sign_panel/total_r31_plus1_then_bad': ('EINVAL', 'sign_panel: more than 2^31 - 1 replicates in one call'),
    'sign_panel/total_r31': ('ENODEV', 'no HIP device visible: the dcor engine has no CPU path'),
    'sign_panel/total_r31_plus1': ('EINVAL', 'sign_panel: more than 2^31 - 1 replicates in one call'),
    'sign_panel/const_klt1': ('EKLT1', 'ci_NI_signbatch: k = floor(n/m) = 0 < 1 (n=100, m=200; vert-cor.R:209)'),
    'sign_panel/const_klt1_reps0': ('EKLT1', 'ci_NI_signbatch: k = floor(n/m) = 0 < 1 (n=100, m=200; vert-cor.R:209)'),
    'sign_panel/const_eps_inf_reps0': ('EINVAL', 'eps1 > 0 and eps2 > 0 required (vert-cor.R:264)'),
    'sign_panel/const_n0': ('EINVAL', 'n must be in [1, 2^31) (got 0)'),
    'sign_panel/const_n_2p31': ('EINVAL', 'n must be in [1, 2^31) (got 2147483648)'),
    'sign_panel/const_alpha': ('EINVAL', "alpha must be < 2 (R's mixquant index ceiling((1-alpha/2)*nsim) >= 1)"),
    'sign_panel/const_ci_mode': ('EINVAL', 'ci_mode must be auto/normal/laplace'),
    'sign_panel/const_nsim0_all_reps0': ('EINVAL', 'nsim must be in [1, 2048] (got 0)'),
    'sign_panel/const_nsim_2049': ('EINVAL', 'nsim must be in [1, 2048] (got 2049)'),
    'sign_panel/all_reps0': ('OK', SENTINEL),
    'sign_panel/order_seg0_const_and_seg1_field': ('EINVAL', 'sign_panel: segment 1: need eps1, eps2 > 0, reps, rep_begin, out_row >= 0'),
    'sign_panel/order_cap_and_const': ('EINVAL', 'sign_panel: more than 2^31 - 1 replicates in one call'),
    'sign_panel/order_bad_segment_and_null_X': ('EINVAL', 'sign_panel: null argument (X, Y)'),
    'sign_table/null_desc': ('EINVAL', 'sign_table: null argument'),
    'sign_table/null_segs': ('EINVAL', 'sign_table: null argument'),
    'sign_table/null_out': ('EINVAL', 'sign_table: null argument'),
    'sign_table/nseg_negative': ('EINVAL', 'sign_table: null argument'),
    'sign_table/nseg_zero': ('OK', SENTINEL),
    'sign_table/null_D': ('EINVAL', 'sign_table: null argument (D)'),
    'sign_table/nseg_zero_null_D': ('OK', SENTINEL),
    'sign_table/seg0_eps1_0.0': ('EINVAL', 'sign_table: segment 0: need eps1, eps2 > 0, reps, rep_begin, out_row >= 0'),
    'sign_table/last_eps1_0.0': ('EINVAL', 'sign_table: segment 2: need eps1, eps2 > 0, reps, rep_begin, out_row >= 0'),
    'sign_table/seg0_eps2_0.0': ('EINVAL', 'sign_table: segment 0: need eps1, eps2 > 0, reps, rep_begin, out_row >= 0'),
    'sign_table/last_eps2_0.0': ('EINVAL', 'sign_table: segment 2: need eps1, eps2 > 0, reps, rep_begin, out_row >= 0'),
    'sign_table/seg0_eps1_nan': ('EINVAL', 'sign_table: segment 0: need eps1, eps2 > 0, reps, rep_begin, out_row >= 0'),
    'sign_table/last_eps1_nan': ('EINVAL', 'sign_table: segment 2: need eps1, eps2 > 0, reps, rep_begin, out_row >= 0'),
    'sign_table/seg0_eps2_-1.0': ('EINVAL', 'sign_table: segment 0: need eps1, eps2 > 0, reps, rep_begin, out_row >= 0'),
    'sign_table/last_eps2_-1.0': ('EINVAL', 'sign_table: segment 2: need eps1, eps2 > 0, reps, rep_begin, out_row >= 0'),
    'sign_table/seg0_reps_-1': ('EINVAL', 'sign_table: segment 0: need eps1, eps2 > 0, reps, rep_begin, out_row >= 0'),
    'sign_table/last_reps_-1': ('EINVAL', 'sign_table: segment 2: need eps1, eps2 > 0, reps, rep_begin, out_row >= 0'),
    'sign_table/seg0_rep_begin_-1': ('EINVAL', 'sign_table: segment 0: need eps1, eps2 > 0, reps, rep_begin, out_row >= 0'),
    'sign_table/last_rep_begin_-1': ('EINVAL', 'sign_table: segment 2: need eps1, eps2 > 0, reps, rep_begin, out_row >= 0'),
    'sign_table/seg0_out_row_-1': ('EINVAL', 'sign_table: segment 0: need eps1, eps2 > 0, reps, rep_begin, out_row >= 0'),
    'sign_table/last_out_row_-1': ('EINVAL', 'sign_table: segment 2: need eps1, eps2 > 0, reps, rep_begin, out_row >= 0'),
    'sign_table/rep_begin_max_reps0': ('OK', SENTINEL),
    'sign_table/rep_begin_max_reps0_then_valid': ('ENODEV', 'no HIP device visible: the dcor engine has no CPU path'),
    'sign_table/rep_begin_max_reps1': ('EINVAL', 'sign_table: segment 0: replicate range exceeds 2^32'),
    'sign_table/rep_begin_max_reps1_last': ('EINVAL', 'sign_table: segment 1: replicate range exceeds 2^32'),
    'sign_table/rep_range_int64': ('EINVAL', 'sign_table: segment 1: replicate range exceeds 2^32'),
    'sign_table/total_r31_then_bad': ('EINVAL', 'sign_table: segment 2: need eps1, eps2 > 0, reps, rep_begin, out_row >= 0'),
    'sign_table/total_r31_plus1_then_bad': ('EINVAL', 'sign_table: more than 2^31 - 1 replicates in one call'),
    'sign_table/total_r31': ('ENODEV', 'no HIP device visible: the dcor engine has no CPU path'),
    'sign_table/total_r31_plus1': ('EINVAL', 'sign_table: more than 2^31 - 1 replicates in one call'),
    'sign_table/const_klt1': ('EKLT1', 'ci_NI_signbatch: k = floor(n/m) = 0 < 1 (n=100, m=200; vert-cor.R:209)'),
    'sign_table/const_klt1_reps0': ('EKLT1', 'ci_NI_signbatch: k = floor(n/m) = 0 < 1 (n=100, m=200; vert-cor.R:209)'),
    'sign_table/const_eps_inf_reps0': ('EINVAL', 'eps1 > 0 and eps2 > 0 required (vert-cor.R:264)'),
    'sign_table/const_n0': ('EINVAL', 'n must be in [1, 2^31) (got 0)'),
    'sign_table/const_n_2p31': ('EINVAL', 'n must be in [1, 2^31) (got 2147483648)'),
    'sign_table/const_alpha': ('EINVAL', "alpha must be < 2 (R's mixquant index ceiling((1-alpha/2)*nsim) >= 1)"),
    'sign_table/const_ci_mode': ('EINVAL', 'ci_mode must be auto/normal/laplace'),
    'sign_table/const_nsim0_all_reps0': ('EINVAL', 'nsim must be in [1, 2048] (got 0)'),
    'sign_table/const_nsim_2049': ('EINVAL', 'nsim must be in [1, 2048] (got 2049)'),
    'sign_table/all_reps0': ('OK', SENTINEL),
    'sign_table/order_seg0_const_and_seg1_field': ('EINVAL', 'sign_table: segment 1: need eps1, eps2 > 0, reps, rep_begin, out_row >= 0'),
    'sign_table/order_cap_and_const': ('EINVAL', 'sign_table: more than 2^31 - 1 replicates in one call'),
    'sign_table/p_0': ('EINVAL', 'sign_table: p must be in [1, 2^31) (got 0)'),
    'sign_table/p_-3': ('EINVAL', 'sign_table: p must be in [1, 2^31) (got -3)'),
    'sign_table/p_2147483648': ('EINVAL', 'sign_table: p must be in [1, 2^31) (got 2147483648)'),
    'sign_table/ld_lt_n': ('EINVAL', 'sign_table: ld = 99 < n = 100'),
    'sign_table/seg0_col_x_3': ('EINVAL', 'sign_table: segment 0: columns (3, 1) outside [0, 3)'),
    'sign_table/last_col_x_3': ('EINVAL', 'sign_table: segment 2: columns (3, 1) outside [0, 3)'),
    'sign_table/seg0_col_y_3': ('EINVAL', 'sign_table: segment 0: columns (0, 3) outside [0, 3)'),
    'sign_table/last_col_y_3': ('EINVAL', 'sign_table: segment 2: columns (0, 3) outside [0, 3)'),
    'sign_table/seg0_col_x_-1': ('EINVAL', 'sign_table: segment 0: columns (-1, 1) outside [0, 3)'),
    'sign_table/last_col_x_-1': ('EINVAL', 'sign_table: segment 2: columns (-1, 1) outside [0, 3)'),
    'sign_table/seg0_col_y_2147483647': ('EINVAL', 'sign_table: segment 0: columns (0, 2147483647) outside [0, 3)'),
    'sign_table/last_col_y_2147483647': ('EINVAL', 'sign_table: segment 2: columns (0, 2147483647) outside [0, 3)'),
    'sign_table/col_reps0': ('EINVAL', 'sign_table: segment 1: columns (0, 3) outside [0, 3)'),
    'sign_table/layout_overflow': ('EINVAL', 'sign_table: p * npad * 8 scratch bytes overflow (p = 2147483647, n = 2147483647)'),
    'sign_table/layout_overflow_all_reps0': ('EINVAL', 'sign_table: p * npad * 8 scratch bytes overflow (p = 2147483647, n = 2147483647)'),
    'sign_table/order_bad_segment_and_ld': ('EINVAL', 'sign_table: ld = 99 < n = 100'),
    'sign_table/order_bad_segment_and_p': ('EINVAL', 'sign_table: p must be in [1, 2^31) (got 0)'),
    'sign_table/order_p_and_ld': ('EINVAL', 'sign_table: p must be in [1, 2^31) (got 0)'),
    'sign_table/order_null_D_and_p': ('EINVAL', 'sign_table: null argument (D)'),
    'sign_table/order_field_column_range': ('EINVAL', 'sign_table: segment 0: need eps1, eps2 > 0, reps, rep_begin, out_row >= 0'),
    'sign_table/order_column_range': ('EINVAL', 'sign_table: segment 0: columns (3, 1) outside [0, 3)'),
    'sign_table/order_seg0_range_and_seg1_column': ('EINVAL', 'sign_table: segment 0: replicate range exceeds 2^32'),
    'sign_table/order_const_and_layout': ('EINVAL', "alpha must be < 2 (R's mixquant index ceiling((1-alpha/2)*nsim) >= 1)"),
}


def _run(key):
    from dcor import _lib
    assert _lib.lib.dcor_get_variant(b"sentinel", None, 0) == -1 and _lib.last_error() == SENTINEL
    allocs = _lib.lib.dcor_alloc_count()
    st = CASES[key]()
    return STATUS[st], _lib.last_error(), _lib.lib.dcor_alloc_count() - allocs


def test_every_case_has_an_expectation():
    assert sorted(CASES) == sorted(EXPECTED)
    for short in list(HRS) + list(SIGN):
        assert sum(k.startswith(short + "/") for k in CASES) >= 40, short


@pytest.mark.parametrize("entry", list(HRS) + list(SIGN))
def test_rejections_and_empty_calls(entry):
    """Status, full message and no allocation, for every case of one entry that cannot reach a
    launch whether or not a device is present."""
    for key in sorted(CASES):
        if key.startswith(entry + "/") and key not in NO_GPU:
            st, msg, allocs = _run(key)
            assert (st, msg) == EXPECTED[key], key
            assert st != "ENODEV" and (st == "OK") == (msg == SENTINEL), key
            assert allocs == 0, key


@pytest.mark.parametrize("entry", list(HRS) + list(SIGN))
def test_valid_calls_reach_the_device_query(entry):
    """The accepted ends of the range and cap checks pass every host check: DCOR_ENODEV on a host
    without a device (with one the fake pointers must not be launched on)."""
    from dcor import _lib
    if _lib.lib.dcor_device_count() > 0:
        return
    for key in sorted(NO_GPU):
        if key.startswith(entry + "/"):
            st, msg, allocs = _run(key)
            assert (st, msg) == EXPECTED[key], key
            assert allocs == 0, key
