"""CPU tests of the private HRS-table boundary (dcor_hrs_private_table_launch): the descriptor's
layout against the header, the entry and the draw site declared / exported / bound, and every
argument check happening before any device access, with the message dcor_last_error keeps.  D, the
records and d_priv are fake pointers; lo and hi are real host arrays (the entry reads them)."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "dcor.h")
NAME = "dcor_hrs_private_table_launch"
FAKE = 8   # a non-null pointer value that is never dereferenced
LO, HI = (45.0, 15.0, -3.0), (90.0, 35.0, 3.0)
_KEEP = []  # the lo / hi arrays the descriptors point into


def _arr(v):
    if v is None:
        return None
    a = (C.c_double * len(v))(*v)
    _KEEP.append(a)
    return C.cast(a, C.POINTER(C.c_double))


def _desc(lo=LO, hi=HI, **kw):
    from dcor import _lib
    d = dict(n=100, p=3, ld=100, D=FAKE, eps_mean=0.1, eps_m2=0.1, seed_std=2**40 + 5, alpha=0.05, delta=0.01,
             nsim=1000)
    d.update(kw)
    return _lib.HrsPrivateDesc(lo=_arr(lo), hi=_arr(hi), **d)


def _segs(*kws):
    from dcor import _lib
    base = dict(eps=1.0, seed_ni=1, seed_int=2, reps=1, col_x=0, col_y=1)
    return (_lib.HrsPairSegment * len(kws))(*[_lib.HrsPairSegment(**{**base, **k}) for k in kws])


def _call(desc, segs, nseg=None, out=FAKE, priv=FAKE):
    from dcor import _lib
    return _lib.lib.dcor_hrs_private_table_launch(None if desc is None else C.byref(desc), segs,
                                                  (0 if segs is None else len(segs)) if nseg is None else nseg,
                                                  None if out is None else C.c_void_p(out),
                                                  None if priv is None else C.c_void_p(priv), None)


def _valid(desc, segs, **kw):
    """A call that passes every host check reaches the device query: DCOR_ENODEV on a host without a
    device.  With one the fake pointers must not be launched on, so nothing is called."""
    from dcor import _lib
    if _lib.lib.dcor_device_count() > 0:
        return
    assert _call(desc, segs, **kw) == _lib.DCOR_ENODEV, _lib.last_error()


def test_entry_and_site_declared_exported_and_bound():
    from dcor import _lib
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"\bint\s+" + NAME + r"\s*\(", txt), "not declared in include/dcor.h"
    assert re.search(r"\bDCOR_SITE_STD\s*=\s*17\b", txt), "DCOR_SITE_STD = 17 not in the site enum"
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    assert re.search(r"\bT " + NAME + r"$", out, flags=re.M), "not an exported C symbol"
    assert NAME in _lib.SIGNATURES and _lib.SITE_STD == 17
    # the planner stays out of the dynamic symbols
    assert "plan_hrs_private" not in out


def test_struct_layout_matches_header():
    from dcor import _lib
    cname, py = "dcor_hrs_private_desc", _lib.HrsPrivateDesc
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void){",
             f'printf("{cname} %zu\\n", sizeof({cname}));']
    for fname, _ in py._fields_:
        lines.append(f'printf("{cname}.{fname} %zu\\n", offsetof({cname}, {fname}));')
    lines.append('printf("site %d\\n", (int)DCOR_SITE_STD);')
    lines.append("return 0;}")
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "l.c"), os.path.join(d, "l")
        open(src, "w").write("\n".join(lines))
        subprocess.run(["gcc", "-o", exe, src], check=True)
        out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout
    got = dict(line.rsplit(" ", 1) for line in out.strip().splitlines())
    assert int(got[cname]) == C.sizeof(py) == 96
    for fname, _ in py._fields_:
        assert int(got[f"{cname}.{fname}"]) == getattr(py, fname).offset, fname
    assert int(got["site"]) == 17


def test_null_arguments_rejected_without_gpu():
    from dcor import _lib
    seg = _segs({})
    assert _call(None, seg) == _lib.DCOR_EINVAL
    assert _call(_desc(), None, nseg=1) == _lib.DCOR_EINVAL
    assert _call(_desc(), seg, out=None) == _lib.DCOR_EINVAL
    assert _call(_desc(), seg, nseg=-1) == _lib.DCOR_EINVAL
    for bad in (dict(D=0), dict(lo=None), dict(hi=None)):
        assert _call(_desc(**bad), seg) == _lib.DCOR_EINVAL, bad
        assert "null argument (D, lo, hi)" in _lib.last_error()
    # d_priv is optional
    _valid(_desc(), seg, priv=None)
    _valid(_desc(), seg)


def test_table_geometry_intervals_budgets_and_columns_rejected_without_gpu():
    """n outside [2, 65536], p < 1, ld < n, an interval that is not finite with lo < hi (the message
    names the column), a budget that is not finite and positive, delta <= 0 and a column outside
    [0, p) (the message names the segment): DCOR_EINVAL, no device needed, no allocation made."""
    from dcor import _lib
    allocs = _lib.lib.dcor_alloc_count()
    for n in (1, 0, -4, 65537, 2**31):
        assert _call(_desc(n=n, ld=max(n, 1)), _segs({})) == _lib.DCOR_EINVAL, n
        msg = _lib.last_error()
        assert "n must be in [2, 65536]" in msg and "no fallback" in msg, msg
    for n in (2, 65536):
        _valid(_desc(n=n, ld=n), _segs({}))
    for p in (0, -3, 2**31):
        assert _call(_desc(p=p), _segs({})) == _lib.DCOR_EINVAL, p
        assert "p must be in [1, 2^31)" in _lib.last_error()
    assert _call(_desc(ld=99), _segs({})) == _lib.DCOR_EINVAL
    assert "ld = 99 < n = 100" in _lib.last_error()
    _valid(_desc(ld=2**40), _segs({}))
    assert _call(_desc(D=12), _segs({})) == _lib.DCOR_EINVAL
    assert "aligned to 8 bytes" in _lib.last_error()
    inf, nan = float("inf"), float("nan")
    for col in range(3):
        # the interval of a column no segment names is checked too
        for lo_c, hi_c in ((nan, HI[col]), (-inf, HI[col]), (LO[col], nan), (LO[col], inf),
                           (HI[col], HI[col]), (HI[col], LO[col])):
            lo, hi = list(LO), list(HI)
            lo[col], hi[col] = lo_c, hi_c
            assert _call(_desc(lo=lo, hi=hi), _segs(dict(col_x=(col + 1) % 3, col_y=(col + 1) % 3))) == \
                _lib.DCOR_EINVAL, (col, lo_c, hi_c)
            msg = _lib.last_error()
            assert f"column {col}: need finite lo < hi" in msg, msg
    for field in ("eps_mean", "eps_m2"):
        for bad in (0.0, -0.1, inf, nan):
            assert _call(_desc(**{field: bad}), _segs({})) == _lib.DCOR_EINVAL, (field, bad)
            assert "eps_mean, eps_m2 must be finite and > 0" in _lib.last_error()
    for delta in (0.0, -0.5, nan):
        assert _call(_desc(delta=delta), _segs({})) == _lib.DCOR_EINVAL, delta
        assert "delta must be positive" in _lib.last_error()
    for bad in (dict(col_x=3), dict(col_y=3), dict(col_x=-1), dict(col_y=-1), dict(col_x=2**31 - 1)):
        assert _call(_desc(), _segs({}, dict(col_x=2, col_y=2), bad)) == _lib.DCOR_EINVAL, bad
        msg = _lib.last_error()
        assert "segment 2: columns" in msg and "outside [0, 3)" in msg, msg
    assert _call(_desc(), _segs({}, dict(col_y=3, reps=0))) == _lib.DCOR_EINVAL
    assert "segment 1: columns (0, 3)" in _lib.last_error()
    _valid(_desc(), _segs(dict(col_x=2, col_y=2), dict(col_x=2, col_y=0)))
    assert _lib.lib.dcor_alloc_count() == allocs


def test_invalid_segments_and_descriptor_rejected_without_gpu():
    from dcor import _lib
    allocs = _lib.lib.dcor_alloc_count()
    for bad in (dict(eps=0.0), dict(eps=-1.0), dict(eps=float("nan")), dict(eps=float("inf")),
                dict(reps=-1), dict(rep_begin=-1), dict(out_row=-1)):
        assert _call(_desc(), _segs({}, {}, bad)) == _lib.DCOR_EINVAL, bad
        if "eps" not in bad or bad["eps"] != float("inf"):
            assert "segment 2: need eps > 0" in _lib.last_error(), bad
    # replicate 2^32 - 1 is no segment entry's to run (rep_begin + reps <= 2^32 - 1, as dcor_hrs_table_launch)
    for rb, reps in ((2**63 - 2, 2), (2**32 - 2, 4), (0xfffffffe, 3), (2**32 - 3, 3), (2**32 - 1, 1)):
        assert _call(_desc(), _segs({}, dict(rep_begin=rb, reps=reps))) == _lib.DCOR_EINVAL, (rb, reps)
        assert "segment 1: replicate range exceeds 2^32" in _lib.last_error()
    _valid(_desc(), _segs(dict(rep_begin=0xfffffffd, reps=2)))
    _valid(_desc(), _segs(dict(rep_begin=2**32 - 4, reps=3)))
    assert _call(_desc(), _segs(dict(reps=2**30), dict(reps=2**30))) == _lib.DCOR_EINVAL
    assert "2^31 - 1" in _lib.last_error()
    for bad in (dict(nsim=0), dict(nsim=2049), dict(alpha=2.0), dict(alpha=float("nan"))):
        assert _call(_desc(**bad), _segs({})) == _lib.DCOR_EINVAL, bad
    # the HRS geometry has no k < 1: n = 100 at eps = 0.1 (m = 800 > n) runs with k = 2, m = 50
    _valid(_desc(), _segs(dict(eps=0.1)))
    assert _lib.lib.dcor_alloc_count() == allocs


def test_empty_calls_are_ok_without_gpu():
    """nseg = 0, and segments with no replicates at all, return DCOR_OK: no device work."""
    from dcor import _lib
    assert _call(_desc(), None, nseg=0, out=None, priv=None) == _lib.DCOR_OK
    assert _call(_desc(), _segs(dict(reps=0), dict(reps=0, eps=2.0, col_x=2))) == _lib.DCOR_OK


def test_valid_calls_fail_loudly_without_gpu():
    """The shapes of the GPU tests pass every check and reach the device query (DCOR_ENODEV here)."""
    from dcor import _lib
    if _lib.lib.dcor_device_count() > 0:
        return   # with a device the fake pointers must not be launched on
    pairs = [(0, 1), (1, 0), (2, 3), (1, 1)]
    segs = [dict(col_x=a, col_y=b, eps=e, seed_ni=2**33 + j, seed_int=2**34 + j,
                 rep_begin=(0, 1001, 2**32 - 4)[j % 3], reps=3, out_row=4 * j)
            for j, ((a, b), e) in enumerate((pr, e) for pr in pairs for e in (0.1, 1.0, 2.0, 2.45))]
    for n in (1001, 1000):
        d = _desc(lo=(45.0, 15.0, 0.0, -1.0), hi=(90.0, 35.0, 8.0, 1.0), n=n, p=4, ld=n + 3)
        assert _call(d, _segs(*segs)) == _lib.DCOR_ENODEV, _lib.last_error()


def test_python_surface_checks_before_device_work():
    from dcor import hrs
    raw = np.zeros((16, 3))
    b3 = [(0.0, 1.0)] * 3
    with pytest.raises(ValueError, match="outside"):
        hrs.private_segments(raw, b3, [(0, 3, 1.0, 1, 2, 0, 1)])
    with pytest.raises(ValueError, match=r"one \(lo, hi\) pair per column"):
        hrs.private_segments(raw, b3[:2], [(0, 1, 1.0, 1, 2, 0, 1)])
    with pytest.raises(ValueError, match=r"\(n, p\)"):
        hrs.private_segments(np.zeros(16), [(0.0, 1.0)], [])
    gap = raw.copy()
    gap[5, 2] = np.nan
    with pytest.raises(ValueError, match="corr_matrix_pairwise"):
        hrs.private_segments(gap, b3, [(0, 1, 1.0, 1, 2, 0, 1)])
    with pytest.raises(ValueError, match="corr_matrix_pairwise"):
        hrs.corr_matrix_private(gap, b3, 1.0, 2)
