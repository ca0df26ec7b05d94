"""CPU tests of the private pairwise HRS-table boundary (dcor_hrs_private_pairwise_launch): the
descriptor's layout against the header, the entry declared / exported / bound, and every argument
check happening before any device access, with the code, the message dcor_last_error keeps and both
output buffers left at a sentinel.  D is a fake pointer; lo, hi and valid are real host arrays (the
entry reads them); the records and d_priv are real host buffers no check may write."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "dcor.h")
NAME = "dcor_hrs_private_pairwise_launch"
FAKE = 8   # a non-null pointer value that is never dereferenced
LO, HI = (45.0, 15.0, -3.0), (90.0, 35.0, 3.0)
SENTINEL = -7.25
_KEEP = []  # the host arrays the descriptors point into


def _arr(v):
    if v is None:
        return None
    a = (C.c_double * len(v))(*v)
    _KEEP.append(a)
    return C.cast(a, C.POINTER(C.c_double))


def _full(n, p):
    """Every row of every column present (the last word's bits at i >= n set too: they are ignored)."""
    return np.full((p, (n + 63) // 64), 2**64 - 1, dtype=np.uint64)


def _desc(lo=LO, hi=HI, valid="full", **kw):
    from dcor import _lib
    d = dict(n=100, p=3, ld=100, D=FAKE, eps_mean=0.1, eps_m2=0.1, seed_std=2**40 + 5, alpha=0.05,
             delta=float("nan"), nsim=1000)
    d.update(kw)
    if isinstance(valid, str):
        valid = _full(max(int(d["n"]), 1) if d["n"] < 2**20 else 64, max(int(d["p"]), 1) if d["p"] < 2**20 else 1)
    vp = None
    if valid is not None:
        valid = np.ascontiguousarray(valid, dtype=np.uint64)
        _KEEP.append(valid)
        vp = valid.ctypes.data_as(C.POINTER(C.c_uint64))
    return _lib.HrsPrivateNaDesc(lo=_arr(lo), hi=_arr(hi), valid=vp, **d)


def _segs(*kws):
    from dcor import _lib
    base = dict(eps=1.0, seed_ni=1, seed_int=2, reps=1, col_x=0, col_y=1)
    return (_lib.HrsPairSegment * len(kws))(*[_lib.HrsPairSegment(**{**base, **k}) for k in kws])


def _call(desc, segs, nseg=None, out=True, priv=True):
    """-> the status; the record and d_priv buffers (host memory: a check that wrote them would show)
    must still hold the sentinel."""
    from dcor import _lib
    rec = np.full((8, 6), SENTINEL)
    pv = np.full((8, 6), SENTINEL)
    st = _lib.lib.dcor_hrs_private_pairwise_launch(
        None if desc is None else C.byref(desc), segs,
        (0 if segs is None else len(segs)) if nseg is None else nseg,
        C.c_void_p(rec.ctypes.data) if out else None, C.c_void_p(pv.ctypes.data) if priv else None, None)
    assert np.all(rec == SENTINEL) and np.all(pv == SENTINEL)
    return st


def _rejected(desc, segs, *needles, **kw):
    from dcor import _lib
    assert _call(desc, segs, **kw) == _lib.DCOR_EINVAL
    msg = _lib.last_error()
    for s in needles:
        assert s in msg, msg


def _valid(desc, segs, **kw):
    """A call that passes every host check reaches the device query: DCOR_ENODEV on a host without a
    device.  With one the host buffers must not be launched on, so nothing is called."""
    from dcor import _lib
    if _lib.lib.dcor_device_count() > 0:
        return
    assert _call(desc, segs, **kw) == _lib.DCOR_ENODEV, _lib.last_error()


def test_entry_declared_exported_and_bound():
    from dcor import _lib
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"\bint\s+" + NAME + r"\s*\(", txt), "not declared in include/dcor.h"
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    assert re.search(r"\bT " + NAME + r"$", out, flags=re.M), "not an exported C symbol"
    assert NAME in _lib.SIGNATURES
    assert "plan_hrs_private_pairwise" not in out     # the planner stays out of the dynamic symbols


def test_struct_layout_matches_header():
    from dcor import _lib
    cname, py = "dcor_hrs_private_na_desc", _lib.HrsPrivateNaDesc
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void){",
             f'printf("{cname} %zu\\n", sizeof({cname}));']
    for fname, _ in py._fields_:
        lines.append(f'printf("{cname}.{fname} %zu\\n", offsetof({cname}, {fname}));')
    lines.append("return 0;}")
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "l.c"), os.path.join(d, "l")
        open(src, "w").write("\n".join(lines))
        subprocess.run(["gcc", "-o", exe, src], check=True)
        out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout
    got = dict(line.rsplit(" ", 1) for line in out.strip().splitlines())
    assert int(got[cname]) == C.sizeof(py) == 104
    for fname, _ in py._fields_:
        assert int(got[f"{cname}.{fname}"]) == getattr(py, fname).offset, fname
    assert [f for f, _ in py._fields_] == ["n", "p", "ld", "D", "lo", "hi", "valid", "eps_mean", "eps_m2",
                                           "seed_std", "alpha", "delta", "nsim"]


def test_null_arguments_rejected_without_gpu():
    from dcor import _lib
    seg = _segs({})
    assert _call(None, seg) == _lib.DCOR_EINVAL
    assert _call(_desc(), None, nseg=1) == _lib.DCOR_EINVAL
    assert _call(_desc(), seg, out=False) == _lib.DCOR_EINVAL
    assert _call(_desc(), seg, nseg=-1) == _lib.DCOR_EINVAL
    for bad in (dict(D=0), dict(lo=None), dict(hi=None), dict(valid=None)):
        _rejected(_desc(**bad), seg, "null argument (D, lo, hi, valid)")
    _valid(_desc(), seg, priv=False)                   # d_priv is optional
    _valid(_desc(), seg)


def test_table_geometry_intervals_budgets_delta_and_columns_rejected_without_gpu():
    """The union of the two parents' checks: n outside [2, 2^31), p < 1, ld < n, D misaligned, an
    interval that is not finite with lo < hi (the message names the column), a budget that is not
    finite and positive, delta <= 0 (NaN is 1 / n_ab), a column outside [0, p) (the message names the
    segment): DCOR_EINVAL, no device needed, no allocation made."""
    from dcor import _lib
    allocs = _lib.lib.dcor_alloc_count()
    for n in (1, 0, -4, 2**31, 2**40):
        _rejected(_desc(n=n, ld=max(n, 1)), _segs({}), "n must be in [2, 2^31)")
    for n in (2, 100, 65536):
        _valid(_desc(n=n, ld=n), _segs({}))
    for p in (0, -3, 2**31):
        _rejected(_desc(p=p), _segs({}), "p must be in [1, 2^31)")
    _rejected(_desc(ld=99), _segs({}), "ld = 99 < n = 100")
    _valid(_desc(ld=2**40), _segs({}))
    _rejected(_desc(D=12), _segs({}), "aligned to 8 bytes")
    inf, nan = float("inf"), float("nan")
    for col in range(3):
        # the interval of a column no segment names is checked too
        for lo_c, hi_c in ((nan, HI[col]), (-inf, HI[col]), (LO[col], nan), (LO[col], inf),
                           (HI[col], HI[col]), (HI[col], LO[col])):
            lo, hi = list(LO), list(HI)
            lo[col], hi[col] = lo_c, hi_c
            _rejected(_desc(lo=lo, hi=hi), _segs(dict(col_x=(col + 1) % 3, col_y=(col + 1) % 3)),
                      f"column {col}: need finite lo < hi")
    for field in ("eps_mean", "eps_m2"):
        for bad in (0.0, -0.1, inf, nan):
            _rejected(_desc(**{field: bad}), _segs({}), "eps_mean, eps_m2 must be finite and > 0")
    for delta in (0.0, -0.5, -inf):
        _rejected(_desc(delta=delta), _segs({}), "delta must be positive, or NaN")
    for delta in (nan, 0.01, 1.0 / 100):
        _valid(_desc(delta=delta), _segs({}))
    for bad in (dict(col_x=3), dict(col_y=3), dict(col_x=-1), dict(col_y=-1), dict(col_x=2**31 - 1)):
        _rejected(_desc(), _segs({}, dict(col_x=2, col_y=2), bad), "segment 2: columns", "outside [0, 3)")
    _rejected(_desc(), _segs({}, dict(col_y=3, reps=0)), "segment 1: columns (0, 3)")
    _valid(_desc(), _segs(dict(col_x=2, col_y=2), dict(col_x=2, col_y=0)))
    assert _lib.lib.dcor_alloc_count() == allocs


def test_invalid_segments_and_descriptor_rejected_without_gpu():
    """The segment and replicate-range checks of dcor_hrs_table_launch."""
    from dcor import _lib
    allocs = _lib.lib.dcor_alloc_count()
    for bad in (dict(eps=0.0), dict(eps=-1.0), dict(eps=float("nan")), dict(eps=float("inf")),
                dict(reps=-1), dict(rep_begin=-1), dict(out_row=-1)):
        assert _call(_desc(), _segs({}, {}, bad)) == _lib.DCOR_EINVAL, bad
        if "eps" not in bad or bad["eps"] != float("inf"):
            assert "segment 2: need eps > 0" in _lib.last_error(), bad
    for rb, reps in ((2**63 - 2, 2), (2**32 - 2, 4), (0xfffffffe, 3), (2**32 - 3, 3), (2**32 - 1, 1)):
        _rejected(_desc(), _segs({}, dict(rep_begin=rb, reps=reps)), "segment 1: replicate range exceeds 2^32")
    _valid(_desc(), _segs(dict(rep_begin=0xfffffffd, reps=2)))
    _valid(_desc(), _segs(dict(rep_begin=2**32 - 4, reps=3)))
    _rejected(_desc(), _segs(dict(reps=2**30), dict(reps=2**30)), "2^31 - 1")
    for bad in (dict(nsim=0), dict(nsim=2049), dict(alpha=2.0), dict(alpha=float("nan"))):
        assert _call(_desc(**bad), _segs({})) == _lib.DCOR_EINVAL, bad
    assert _lib.lib.dcor_alloc_count() == allocs


def test_pair_counts_rejected_without_gpu():
    """Every named pair needs 2 <= n_ab <= 65536: n = 70000 with full masks, a pair with n_ab = 1 and
    one with n_ab = 0; the message names the segment and n_ab.  A pair no segment names may have any
    count, and n itself may exceed 65536 when the named pairs' counts do not."""
    from dcor import _lib
    allocs = _lib.lib.dcor_alloc_count()
    big = 70000
    _rejected(_desc(n=big, ld=big, valid=_full(big, 3)), _segs({}, dict(col_x=2, col_y=2)),
              "segment 0: columns (0, 1) have n_ab = 70000 ", "must be in [2, 65536]")
    sparse = _full(big, 3)
    sparse[1, 100:] = 0                                  # column 1: rows 0 .. 6399
    _rejected(_desc(n=big, ld=big, valid=sparse), _segs({}, dict(col_x=1, col_y=1), dict(col_x=2, col_y=1),
                                                        dict(col_x=0, col_y=2)),
              "segment 3: columns (0, 2) have n_ab = 70000 ")
    _valid(_desc(n=big, ld=big, valid=sparse), _segs({}, dict(col_x=1, col_y=1), dict(col_x=2, col_y=1)))
    v = _full(100, 3)
    v[1] = 0
    v[1, 1] = 1 << 5                                     # column 1: row 69 only
    v[2] = 0
    v[2, 0] = 0b101                                      # column 2: rows 0 and 2
    _rejected(_desc(valid=v), _segs(dict(col_x=0, col_y=2), {}), "segment 1: columns (0, 1) have n_ab = 1 ")
    _rejected(_desc(valid=v), _segs(dict(col_x=0, col_y=2), dict(col_x=1, col_y=1, reps=0)),
              "segment 1: columns (1, 1) have n_ab = 1 ")
    _rejected(_desc(valid=v), _segs(dict(col_x=2, col_y=1)), "segment 0: columns (2, 1) have n_ab = 0 ")
    _valid(_desc(valid=v), _segs(dict(col_x=0, col_y=2), dict(col_x=2, col_y=0), dict(col_x=0, col_y=0)))
    # the last word's bits at i >= n never count: row 100 .. 127 of column 1 set, rows below clear
    v[1] = 0
    v[1, 1] = ((1 << 28) - 1) << 36
    _rejected(_desc(valid=v), _segs({}), "segment 0: columns (0, 1) have n_ab = 0 ")
    assert _lib.lib.dcor_alloc_count() == allocs


def test_empty_calls_are_ok_without_gpu():
    """nseg = 0, and segments with no replicates at all, return DCOR_OK: no device work."""
    from dcor import _lib
    assert _call(_desc(), None, nseg=0, out=False, priv=False) == _lib.DCOR_OK
    assert _call(_desc(), _segs(dict(reps=0), dict(reps=0, eps=2.0, col_x=2))) == _lib.DCOR_OK


def test_python_surface_checks_before_device_work():
    from dcor import hrs
    from dcor.dist import hrs_private_pairwise_distributed
    raw = np.zeros((16, 3))
    raw[5, 2] = np.nan
    b3 = [(0.0, 1.0)] * 3
    with pytest.raises(ValueError, match="outside"):
        hrs.private_pairwise_segments(raw, b3, [(0, 3, 1.0, 1, 2, 0, 1)])
    with pytest.raises(ValueError, match=r"one \(lo, hi\) pair per column"):
        hrs.private_pairwise_segments(raw, b3[:2], [(0, 1, 1.0, 1, 2, 0, 1)])
    with pytest.raises(ValueError, match=r"\(n, p\)"):
        hrs.private_pairwise_segments(np.zeros(16), [(0.0, 1.0)], [])
    with pytest.raises(ValueError, match="valid must be uint64"):
        hrs.private_pairwise_segments(raw, b3, [(0, 1, 1.0, 1, 2, 0, 1)], valid=np.zeros((3, 2), dtype=np.uint64))
    with pytest.raises(ValueError, match="return_priv"):
        hrs_private_pairwise_distributed(raw, b3, [(0, 1, 1.0, 1, 2, 0, 1)], return_priv=True)
    # the private entry still refuses a gap, with its own message
    with pytest.raises(ValueError, match="corr_matrix_pairwise"):
        hrs.private_segments(raw, b3, [(0, 1, 1.0, 1, 2, 0, 1)])
