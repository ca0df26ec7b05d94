"""CPU tests of the pairwise HRS-table boundary (dcor_hrs_table_pairwise_launch): the descriptor's
layout against the header, the entry declared / exported / bound, and every argument check happening
on the host before any device access, with the message dcor_last_error keeps.  D is a fake pointer;
lam and the masks are real host arrays (the entry reads them); the output is a real host buffer
filled with a sentinel, which no refused call may touch."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "dcor.h")
NAME = "dcor_hrs_table_pairwise_launch"
FAKE = 8   # a non-null pointer value that is never dereferenced
SENTINEL = -7.25
_KEEP = []  # the host arrays the descriptors point into


def _masks(rows, n, junk=True):
    """rows: per column a boolean [n] array -> uint64 [p, nw], little-endian bit order; junk: the last
    word's bits at i >= n set, which must never count."""
    p, nw = len(rows), (n + 63) // 64
    bits = np.zeros((p, 64 * nw), dtype=np.uint8)
    bits[:, :n] = np.asarray(rows, dtype=bool)
    if junk:
        bits[:, n:] = 1
    return np.packbits(bits, axis=1, bitorder="little").view("<u8").astype(np.uint64).reshape(p, nw)


def _desc(lam=(1.5, 2.0, 2.5), valid="full", **kw):
    from dcor import _lib
    d = dict(n=100, p=3, ld=100, D=FAKE, alpha=0.05, delta=float("nan"), nsim=1000)
    d.update(kw)
    larr = (C.c_double * len(lam))(*lam)
    _KEEP.append(larr)
    if isinstance(valid, str):   # every row present; an n or p the entry refuses first gets a dummy word
        n, p = (d["n"], d["p"]) if 1 <= d["n"] <= 10**6 and 1 <= d["p"] <= 64 else (64, 1)
        valid = _masks(np.ones((p, n), dtype=bool), n)
    vptr = None
    if valid is not None:
        valid = np.ascontiguousarray(valid, dtype=np.uint64)
        _KEEP.append(valid)
        vptr = valid.ctypes.data_as(C.POINTER(C.c_uint64))
    return _lib.HrsTableNaDesc(lam=C.cast(larr, C.POINTER(C.c_double)), valid=vptr, **d)


def _segs(*kws):
    from dcor import _lib
    base = dict(eps=1.0, seed_ni=1, seed_int=2, reps=1, col_x=0, col_y=1)
    return (_lib.HrsPairSegment * len(kws))(*[_lib.HrsPairSegment(**{**base, **k}) for k in kws])


def _call(desc, segs, nseg=None, rows=4):
    """The call on a host record buffer of `rows` sentinel records -> (status, records untouched)."""
    from dcor import _lib
    out = np.full((rows, 6), SENTINEL)
    st = _lib.lib.dcor_hrs_table_pairwise_launch(None if desc is None else C.byref(desc), segs,
                                                 (0 if segs is None else len(segs)) if nseg is None else nseg,
                                                 C.c_void_p(out.ctypes.data), None)
    return st, bool(np.all(out == SENTINEL))


def _refused(desc, segs, msg, **kw):
    from dcor import _lib
    st, clean = _call(desc, segs, **kw)
    assert st == _lib.DCOR_EINVAL and clean, (st, _lib.last_error())
    assert msg in _lib.last_error(), _lib.last_error()


def _valid(desc, segs):
    """A call that passes every host check reaches the device query: DCOR_ENODEV on a host without a
    device.  With one the fake table pointer must not be launched on, so nothing is called."""
    from dcor import _lib
    if _lib.lib.dcor_device_count() > 0:
        return
    st, clean = _call(desc, segs)
    assert st == _lib.DCOR_ENODEV and clean, _lib.last_error()


def test_entry_declared_exported_and_bound():
    from dcor import _lib
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"\bint\s+" + NAME + r"\s*\(", txt), "not declared in include/dcor.h"
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    assert re.search(r"\bT " + NAME + r"$", out, flags=re.M), "not an exported C symbol"
    assert NAME in _lib.SIGNATURES


def test_struct_layout_matches_header():
    """sizeof / offsetof of the descriptor from a C program compiled against include/dcor.h; it is
    dcor_hrs_table_desc with `valid` after `lam`."""
    from dcor import _lib
    cname, py = "dcor_hrs_table_na_desc", _lib.HrsTableNaDesc
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
    assert int(got[cname]) == C.sizeof(py) == 72
    for fname, _ in py._fields_:
        assert int(got[f"{cname}.{fname}"]) == getattr(py, fname).offset, fname
    assert [f for f, _ in py._fields_] == ["n", "p", "ld", "D", "lam", "valid", "alpha", "delta", "nsim"]


def test_null_arguments_rejected_without_gpu():
    from dcor import _lib
    seg = _segs({})
    assert _call(None, seg)[0] == _lib.DCOR_EINVAL
    assert _call(_desc(), None, nseg=1)[0] == _lib.DCOR_EINVAL
    assert _call(_desc(), seg, nseg=-1)[0] == _lib.DCOR_EINVAL
    _refused(_desc(D=0), seg, "null argument")
    _refused(_desc(valid=None), seg, "null argument (D, lam, valid)")


def test_pair_counts_rejected_without_gpu():
    """n_ab = 1, n_ab = 0 and n_ab = 65537: DCOR_EINVAL, the message names the segment and the count;
    the bits at i >= n never count."""
    from dcor import _lib
    allocs = _lib.lib.dcor_alloc_count()
    n = 100
    rows = np.ones((3, n), dtype=bool)
    rows[1] = False
    rows[1, 37] = True                     # (0, 1): one row in common
    rows[2] = ~rows[1]                     # (1, 2): none
    d = _desc(valid=_masks(rows, n))
    _refused(d, _segs(dict(col_x=0, col_y=2), dict(col_x=0, col_y=1)),
             "segment 1: columns (0, 1) have n_ab = 1 ")
    _refused(d, _segs(dict(col_x=0, col_y=2), {}, dict(col_x=1, col_y=2)), "segment 1: columns (0, 1) have n_ab = 1 ")
    _refused(d, _segs(dict(col_x=2, col_y=1)), "segment 0: columns (2, 1) have n_ab = 0 ")
    # a pair without replicates is checked too
    _refused(d, _segs(dict(col_x=0, col_y=2), dict(col_x=1, col_y=1, reps=0)), "segment 1: columns (1, 1) have n_ab = 1 ")
    _valid(d, _segs(dict(col_x=0, col_y=2), dict(col_x=2, col_y=2)))
    # n = 65: row 64 is the only one both columns have; the 63 junk bits of the last word would
    # lift n_ab to 64
    n = 65
    rows = np.ones((2, n), dtype=bool)
    rows[1, :64] = False
    _refused(_desc(lam=(1.5, 2.0), n=n, p=2, ld=n, valid=_masks(rows, n, junk=True)), _segs({}),
             "segment 0: columns (0, 1) have n_ab = 1 ")
    # n = 70000 rows is legal; 65537 of them in a pair is not, 65536 is
    n = 70000
    rows = np.ones((3, n), dtype=bool)
    rows[1, 65536:] = False
    d = _desc(n=n, ld=n, valid=_masks(rows, n))
    _refused(d, _segs(dict(col_x=0, col_y=2)), "segment 0: columns (0, 2) have n_ab = 70000 ")
    rows[1, 65536] = True
    _refused(_desc(n=n, ld=n, valid=_masks(rows, n)), _segs({}), "have n_ab = 65537 ")
    assert "[2, 65536]" in _lib.last_error()
    _valid(d, _segs({}))
    assert _lib.lib.dcor_alloc_count() == allocs


def test_delta_and_table_fields_rejected_without_gpu():
    from dcor import _lib
    for delta in (0.0, -0.5, float("-inf")):
        _refused(_desc(delta=delta), _segs({}), "delta must be positive")
    for delta in (float("nan"), 0.01, 1.0):
        _valid(_desc(delta=delta), _segs({}))
    for n in (1, 0, -4, 2**31):
        _refused(_desc(n=n, ld=max(n, 1)), _segs({}), "n must be in [2, 2^31)")
    for p in (0, -3, 2**31):
        _refused(_desc(p=p), _segs({}), "p must be in [1, 2^31)")
    _refused(_desc(ld=99), _segs({}), "ld = 99 < n = 100")
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        for col in range(3):
            lam = [1.5, 2.0, 2.5]
            lam[col] = bad
            _refused(_desc(lam=lam), _segs(dict(col_x=0, col_y=0)), f"column {col}: lam must be finite and > 0")
    for bad in (dict(col_x=3), dict(col_y=3), dict(col_x=-1), dict(col_y=-1)):
        _refused(_desc(), _segs({}, dict(col_x=2, col_y=2), bad), "segment 2: columns")
    for bad in (dict(eps=0.0), dict(eps=float("nan")), dict(reps=-1), dict(rep_begin=-1), dict(out_row=-1)):
        _refused(_desc(), _segs({}, {}, bad), "segment 2: need eps > 0")
    _refused(_desc(), _segs({}, dict(rep_begin=2**32 - 2, reps=4)), "segment 1: replicate range exceeds 2^32")
    for bad in (dict(nsim=0), dict(nsim=2049), dict(alpha=2.0), dict(alpha=float("nan"))):
        assert _call(_desc(**bad), _segs({})) == (_lib.DCOR_EINVAL, True), bad


def test_empty_calls_are_ok_without_gpu():
    """nseg = 0, and segments with no replicates at all, return DCOR_OK: no device work."""
    from dcor import _lib
    assert _call(_desc(), None, nseg=0) == (_lib.DCOR_OK, True)
    assert _call(_desc(), _segs(dict(reps=0), dict(reps=0, eps=2.0, col_x=2))) == (_lib.DCOR_OK, True)


def test_python_surface_checks_before_device_work():
    import pytest

    from dcor import hrs
    Z = np.zeros((16, 3))
    with pytest.raises(ValueError, match="outside"):
        hrs.pairwise_segments(Z, [1.0, 1.0, 1.0], [(0, 3, 1.0, 1, 2, 0, 1)])
    with pytest.raises(ValueError, match="one clip bound per column"):
        hrs.pairwise_segments(Z, [1.0, 1.0], [(0, 1, 1.0, 1, 2, 0, 1)])
    with pytest.raises(ValueError, match="valid must be uint64"):
        hrs.pairwise_segments(Z, [1.0, 1.0, 1.0], [(0, 1, 1.0, 1, 2, 0, 1)], valid=np.zeros((3, 2), dtype=np.uint64))
