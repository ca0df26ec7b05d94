"""CPU tests of the HRS-table boundary (dcor_hrs_table_launch): the structs' layout against the
header, the entry declared / exported / bound, and every argument check happening before any
device access, with the message dcor_last_error keeps.  D and the output are fake pointers; lam is a
real host array (the entry reads it)."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "dcor.h")
NAME = "dcor_hrs_table_launch"
FAKE = 8   # a non-null pointer value that is never dereferenced
_KEEP = []  # the lam arrays the descriptors point into


def _desc(lam=(1.5, 2.0, 2.5), **kw):
    from dcor import _lib
    d = dict(n=100, p=3, ld=100, D=FAKE, alpha=0.05, delta=0.01, nsim=1000)
    d.update(kw)
    if lam is None:
        ptr = None
    else:
        arr = (C.c_double * len(lam))(*lam)
        _KEEP.append(arr)
        ptr = C.cast(arr, C.POINTER(C.c_double))
    return _lib.HrsTableDesc(lam=ptr, **d)


def _segs(*kws):
    from dcor import _lib
    base = dict(eps=1.0, seed_ni=1, seed_int=2, reps=1, col_x=0, col_y=1)
    return (_lib.HrsPairSegment * len(kws))(*[_lib.HrsPairSegment(**{**base, **k}) for k in kws])


def _call(desc, segs, nseg=None, out=FAKE):
    from dcor import _lib
    return _lib.lib.dcor_hrs_table_launch(None if desc is None else C.byref(desc), segs,
                                          (0 if segs is None else len(segs)) if nseg is None else nseg,
                                          None if out is None else C.c_void_p(out), None)


def _valid(desc, segs):
    """A call that passes every host check reaches the device query: DCOR_ENODEV on a host without a
    device.  With one the fake pointers must not be launched on, so nothing is called."""
    from dcor import _lib
    if _lib.lib.dcor_device_count() > 0:
        return
    assert _call(desc, segs) == _lib.DCOR_ENODEV, _lib.last_error()


def test_entry_declared_exported_and_bound():
    from dcor import _lib
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"\bint\s+" + NAME + r"\s*\(", txt), "not declared in include/dcor.h"
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    assert re.search(r"\bT " + NAME + r"$", out, flags=re.M), "not an exported C symbol"
    assert NAME in _lib.SIGNATURES


def test_struct_layout_matches_header():
    """sizeof / offsetof of both structs from a C program compiled against include/dcor.h; the pair
    segment starts with dcor_hrs_segment's fields at dcor_hrs_segment's offsets."""
    from dcor import _lib
    structs = {"dcor_hrs_table_desc": _lib.HrsTableDesc, "dcor_hrs_pair_segment": _lib.HrsPairSegment}
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void){"]
    for cname, py in structs.items():
        lines.append(f'printf("{cname} %zu\\n", sizeof({cname}));')
        for fname, _ in py._fields_:
            lines.append(f'printf("{cname}.{fname} %zu\\n", offsetof({cname}, {fname}));')
    lines.append("return 0;}")
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "l.c"), os.path.join(d, "l")
        open(src, "w").write("\n".join(lines))
        subprocess.run(["gcc", "-o", exe, src], check=True)
        out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout
    got = dict(line.rsplit(" ", 1) for line in out.strip().splitlines())
    for cname, py in structs.items():
        assert int(got[cname]) == C.sizeof(py), cname
        for fname, _ in py._fields_:
            assert int(got[f"{cname}.{fname}"]) == getattr(py, fname).offset, f"{cname}.{fname}"
    assert C.sizeof(_lib.HrsTableDesc) == 64 and C.sizeof(_lib.HrsPairSegment) == 56
    for fname, _ in _lib.HrsSegment._fields_:
        assert getattr(_lib.HrsPairSegment, fname).offset == getattr(_lib.HrsSegment, fname).offset, fname
    assert _lib.HrsPairSegment.col_x.offset == 48 and _lib.HrsPairSegment.col_y.offset == 52


def test_null_arguments_rejected_without_gpu():
    from dcor import _lib
    seg = _segs({})
    assert _call(None, seg) == _lib.DCOR_EINVAL
    assert _call(_desc(), None, nseg=1) == _lib.DCOR_EINVAL
    assert _call(_desc(), seg, out=None) == _lib.DCOR_EINVAL
    assert _call(_desc(), seg, nseg=-1) == _lib.DCOR_EINVAL
    assert _call(_desc(D=0), seg) == _lib.DCOR_EINVAL
    assert "null argument" in _lib.last_error()
    assert _call(_desc(lam=None), seg) == _lib.DCOR_EINVAL
    assert "null argument" in _lib.last_error()


def test_table_geometry_clips_and_columns_rejected_without_gpu():
    """n outside [2, 65536], p < 1, ld < n, a clip bound that is not finite and positive (the message
    names the column), delta <= 0 and a column outside [0, p) (the message names the segment):
    DCOR_EINVAL, no device needed, no allocation made."""
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
    _valid(_desc(ld=100), _segs({}))
    _valid(_desc(ld=2**40), _segs({}))
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        for col in range(3):
            lam = [1.5, 2.0, 2.5]
            lam[col] = bad
            # the clip bound of a column no segment names is checked too
            assert _call(_desc(lam=lam), _segs(dict(col_x=0, col_y=0))) == _lib.DCOR_EINVAL, (bad, col)
            msg = _lib.last_error()
            assert f"column {col}: lam must be finite and > 0" in msg, msg
    for delta in (0.0, -0.5, float("nan")):
        assert _call(_desc(delta=delta), _segs({})) == _lib.DCOR_EINVAL, delta
        assert "delta must be positive" in _lib.last_error()
    for bad in (dict(col_x=3), dict(col_y=3), dict(col_x=-1), dict(col_y=-1), dict(col_x=2**31 - 1)):
        assert _call(_desc(), _segs({}, dict(col_x=2, col_y=2), bad)) == _lib.DCOR_EINVAL, bad
        msg = _lib.last_error()
        assert "segment 2: columns" in msg and "outside [0, 3)" in msg, msg
    # a bad column in a zero-replicate segment is refused too
    assert _call(_desc(), _segs({}, dict(col_y=3, reps=0))) == _lib.DCOR_EINVAL
    assert "segment 1: columns (0, 3)" in _lib.last_error()
    # (a, a) and (b, a) are valid
    _valid(_desc(), _segs(dict(col_x=2, col_y=2), dict(col_x=2, col_y=0)))
    assert _lib.lib.dcor_alloc_count() == allocs


def test_invalid_segments_and_descriptor_rejected_without_gpu():
    """The sweep entry's segment checks carried over: each returns its code with no device present;
    a bad LAST segment is caught although the earlier ones are valid."""
    from dcor import _lib
    allocs = _lib.lib.dcor_alloc_count()
    for bad in (dict(eps=0.0), dict(eps=-1.0), dict(eps=float("nan")), dict(eps=float("inf")),
                dict(reps=-1), dict(rep_begin=-1), dict(out_row=-1)):
        assert _call(_desc(), _segs({}, {}, bad)) == _lib.DCOR_EINVAL, bad
        if "eps" not in bad or bad["eps"] != float("inf"):
            assert "segment 2: need eps > 0" in _lib.last_error(), bad
    for rb, reps in ((2**63 - 2, 2), (2**32 - 2, 4), (0xfffffffe, 3)):
        assert _call(_desc(), _segs({}, dict(rep_begin=rb, reps=reps))) == _lib.DCOR_EINVAL, (rb, reps)
        assert "segment 1: replicate range exceeds 2^32" in _lib.last_error()
    _valid(_desc(), _segs(dict(rep_begin=0xfffffffd, reps=2)))
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
    assert _call(_desc(), None, nseg=0, out=None) == _lib.DCOR_OK
    assert _call(_desc(), _segs(dict(reps=0), dict(reps=0, eps=2.0, col_x=2))) == _lib.DCOR_OK


def test_valid_calls_fail_loudly_without_gpu():
    """The shapes of the GPU tests pass every check and reach the device query (DCOR_ENODEV here)."""
    from dcor import _lib
    if _lib.lib.dcor_device_count() > 0:
        return   # with a device the fake pointers must not be launched on
    assert _call(_desc(), _segs({})) == _lib.DCOR_ENODEV
    pairs = [(0, 1), (1, 0), (2, 3), (0, 2), (1, 1)]
    segs = [dict(col_x=a, col_y=b, eps=e, seed_ni=2**33 + j, seed_int=2**34 + j,
                 rep_begin=(0, 1001, 2**32 - 6)[j % 3], reps=3, out_row=3 * j)
            for j, ((a, b), e) in enumerate((pr, e) for pr in pairs for e in (0.1, 0.25, 1.0, 2.0, 2.45))]
    for n in (1001, 1000):
        assert _call(_desc(lam=(1.5, 2.0, 2.5, 3.0), n=n, p=4, ld=n + 8), _segs(*segs)) == _lib.DCOR_ENODEV


def test_python_surface_checks_before_device_work():
    from dcor import hrs
    Z = np.zeros((16, 3))
    with pytest.raises(ValueError, match="outside"):
        hrs.table_segments(Z, [1.0, 1.0, 1.0], [(0, 3, 1.0, 1, 2, 0, 1)])
    with pytest.raises(ValueError, match="one clip bound per column"):
        hrs.table_segments(Z, [1.0, 1.0], [(0, 1, 1.0, 1, 2, 0, 1)])
    with pytest.raises(ValueError, match=r"\(n, p\)"):
        hrs.table_segments(np.zeros(16), [1.0], [])
    with pytest.raises(ValueError, match="bounds"):
        hrs.standardize_table(np.zeros((16, 3)), [(0.0, 1.0)] * 2)
