"""CPU tests of the sign-table boundary (dcor_sign_table_launch): the structs' layout against the
header, the entry declared / exported / bound, and every argument check happening before any
device access, with the message dcor_last_error keeps."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "dcor.h")
NAME = "dcor_sign_table_launch"
FAKE = 8   # a non-null pointer value that is never dereferenced


def _desc(**kw):
    from dcor import _lib
    d = dict(n=100, p=3, ld=100, D=FAKE, alpha=0.05, normalise=1, ci_mode=0, nsim=1000)
    d.update(kw)
    return _lib.SignTableDesc(**d)


def _segs(*kws):
    from dcor import _lib
    base = dict(eps1=1.0, eps2=1.0, seed=1, reps=1, col_x=0, col_y=1)
    return (_lib.SignPairSegment * len(kws))(*[_lib.SignPairSegment(**{**base, **k}) for k in kws])


def _call(desc, segs, nseg=None, out=FAKE):
    from dcor import _lib
    return _lib.lib.dcor_sign_table_launch(None if desc is None else C.byref(desc), segs,
                                           (0 if segs is None else len(segs)) if nseg is None else nseg,
                                           None if out is None else C.c_void_p(out), None)


def test_entry_declared_exported_and_bound():
    from dcor import _lib
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"\bint\s+" + NAME + r"\s*\(", txt), "not declared in include/dcor.h"
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    assert re.search(r"\bT " + NAME + r"$", out, flags=re.M), "not an exported C symbol"
    assert NAME in _lib.SIGNATURES


def test_struct_layout_matches_header():
    """sizeof / offsetof of both structs from a C program compiled against include/dcor.h; the pair
    segment starts with dcor_sign_segment's fields at dcor_sign_segment's offsets."""
    from dcor import _lib
    structs = {"dcor_sign_table_desc": _lib.SignTableDesc, "dcor_sign_pair_segment": _lib.SignPairSegment}
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
    assert C.sizeof(_lib.SignTableDesc) == 56 and C.sizeof(_lib.SignPairSegment) == 56
    for fname, _ in _lib.SignSegment._fields_:
        assert getattr(_lib.SignPairSegment, fname).offset == getattr(_lib.SignSegment, fname).offset, fname
    assert _lib.SignPairSegment.col_x.offset == 48 and _lib.SignPairSegment.col_y.offset == 52


def test_null_arguments_rejected_without_gpu():
    from dcor import _lib
    seg = _segs({})
    assert _call(None, seg) == _lib.DCOR_EINVAL
    assert _call(_desc(), None, nseg=1) == _lib.DCOR_EINVAL
    assert _call(_desc(), seg, out=None) == _lib.DCOR_EINVAL
    assert _call(_desc(), seg, nseg=-1) == _lib.DCOR_EINVAL
    assert _call(_desc(D=0), seg) == _lib.DCOR_EINVAL
    assert "null argument" in _lib.last_error()


def test_table_geometry_and_columns_rejected_without_gpu():
    """p < 1, ld < n, a column outside [0, p) (the message names the segment) and a scratch size that
    does not fit: DCOR_EINVAL, no device needed, no allocation made."""
    from dcor import _lib
    allocs = _lib.lib.dcor_alloc_count()
    for p in (0, -3, 2**31):
        assert _call(_desc(p=p), _segs({})) == _lib.DCOR_EINVAL, p
        assert "p must be in [1, 2^31)" in _lib.last_error()
    assert _call(_desc(ld=99), _segs({})) == _lib.DCOR_EINVAL
    assert "ld = 99 < n = 100" in _lib.last_error()
    assert _call(_desc(ld=100), _segs({})) != _lib.DCOR_EINVAL
    assert _call(_desc(ld=2**40), _segs({})) != _lib.DCOR_EINVAL
    for bad in (dict(col_x=3), dict(col_y=3), dict(col_x=-1), dict(col_y=-1), dict(col_x=2**31 - 1)):
        assert _call(_desc(), _segs({}, dict(col_x=2, col_y=2), bad)) == _lib.DCOR_EINVAL, bad
        msg = _lib.last_error()
        assert "segment 2: columns" in msg and "outside [0, 3)" in msg, msg
    # a bad column in a zero-replicate segment is refused too
    assert _call(_desc(), _segs({}, dict(col_y=3, reps=0))) == _lib.DCOR_EINVAL
    assert "segment 1: columns (0, 3)" in _lib.last_error()
    # (a, a) and (b, a) are valid
    assert _call(_desc(), _segs(dict(col_x=2, col_y=2), dict(col_x=2, col_y=0))) != _lib.DCOR_EINVAL
    # p * npad * 8 bytes: (2^31 - 1) columns of 2^31 padded samples do not fit 2^63 bytes
    big = 2**31 - 1
    assert _call(_desc(n=big, p=big, ld=big), _segs({})) == _lib.DCOR_EINVAL
    assert "scratch bytes overflow" in _lib.last_error()
    assert _lib.lib.dcor_alloc_count() == allocs


def test_invalid_segments_and_descriptor_rejected_without_gpu():
    """The panel entry's checks carried over: each returns its code with no device present; a bad
    LAST segment is caught although the earlier ones are valid."""
    from dcor import _lib
    allocs = _lib.lib.dcor_alloc_count()
    for bad in (dict(eps1=0.0), dict(eps2=-1.0), dict(eps1=float("nan")), dict(eps2=float("inf")),
                dict(reps=-1), dict(rep_begin=-1), dict(out_row=-1)):
        assert _call(_desc(), _segs({}, {}, bad)) == _lib.DCOR_EINVAL, bad
    for rb, reps in ((2**63 - 2, 2), (2**32 - 2, 4), (0xfffffffe, 3)):
        assert _call(_desc(), _segs({}, dict(rep_begin=rb, reps=reps))) == _lib.DCOR_EINVAL, (rb, reps)
        assert "segment 1: replicate range exceeds 2^32" in _lib.last_error()
    assert _call(_desc(), _segs(dict(rep_begin=0xfffffffd, reps=2))) != _lib.DCOR_EINVAL
    assert _call(_desc(), _segs(dict(reps=2**30), dict(reps=2**30))) == _lib.DCOR_EINVAL
    assert "2^31 - 1" in _lib.last_error()
    # k = floor(n / m) < 1: n = 100 at eps = (.2, .2) has m = 200 (also in a zero-replicate segment)
    assert _call(_desc(), _segs({}, dict(eps1=0.2, eps2=0.2))) == _lib.DCOR_EKLT1
    assert _call(_desc(), _segs({}, dict(eps1=0.2, eps2=0.2, reps=0))) == _lib.DCOR_EKLT1
    assert _call(_desc(n=7, ld=7), _segs({})) == _lib.DCOR_EKLT1
    for bad in (dict(n=0, ld=0), dict(n=-5), dict(n=2**31, ld=2**31), dict(nsim=0), dict(nsim=2049),
                dict(ci_mode=7), dict(alpha=2.0), dict(alpha=float("nan"))):
        assert _call(_desc(**bad), _segs({})) == _lib.DCOR_EINVAL, bad
    assert _lib.lib.dcor_alloc_count() == allocs


def test_empty_calls_are_ok_without_gpu():
    """nseg = 0, and segments with no replicates at all, return DCOR_OK: no device work."""
    from dcor import _lib
    assert _call(_desc(), None, nseg=0, out=None) == _lib.DCOR_OK
    assert _call(_desc(), _segs(dict(reps=0), dict(reps=0, eps1=2.0, col_x=2))) == _lib.DCOR_OK


def test_valid_calls_fail_loudly_without_gpu():
    """The shapes of the GPU tests pass every check and reach the device query (DCOR_ENODEV here)."""
    from dcor import _lib
    if _lib.lib.dcor_device_count() > 0:
        return   # with a device the fake pointers must not be launched on
    assert _call(_desc(), _segs({})) == _lib.DCOR_ENODEV
    pairs = [(a, b) for a in range(4) for b in range(a + 1, 4)] + [(3, 1), (2, 2)]
    segs = [dict(col_x=a, col_y=b, eps1=e1, eps2=e2, seed=100 + j, rep_begin=(0, 7)[j % 2], reps=5, out_row=5 * j)
            for j, ((a, b), (e1, e2)) in enumerate((pr, e) for pr in pairs
                                                   for e in ((2.0, 2.0), (1.0, 1.0), (0.2, 0.2), (1.5, 0.7)))]
    assert _call(_desc(n=1003, p=4, ld=1011), _segs(*segs)) == _lib.DCOR_ENODEV
    assert _call(_desc(n=9001, p=2, ld=9001), _segs(dict(eps1=2.0, eps2=2.0, reps=3))) == _lib.DCOR_ENODEV
    assert _call(_desc(n=40001, p=2, ld=40001), _segs(dict(eps1=0.0156, eps2=0.0156, reps=3))) == _lib.DCOR_ENODEV


def test_python_surface_checks_before_device_work():
    from dcor import signpanel
    D = np.zeros((16, 3))
    with pytest.raises(ValueError, match="mode must be"):
        signpanel.table_segments(D, [(0, 1, 1.0, 1.0, 1, 0, 1)], mode="nope")
    with pytest.raises(ValueError, match="outside"):
        signpanel.table_segments(D, [(0, 3, 1.0, 1.0, 1, 0, 1)])
    with pytest.raises(ValueError, match=r"\(n, p\)"):
        signpanel.table_segments(np.zeros(16), [])
    assert signpanel.all_pairs(4) == [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]


def test_standin_table_shape_and_grid():
    """Column-major, equicorrelated, whole-number and one-decimal columns on the standard scale."""
    from dcor import signpanel
    from dcor.hrs import AGE_HI, AGE_LO, BMI_HI, BMI_LO
    D = signpanel.standin_table(5001, 4, 0.5, seed=3)
    assert D.shape == (5001, 4) and D.flags.f_contiguous and D.dtype == np.float64
    assert np.array_equal(D, signpanel.standin_table(5001, 4, 0.5, seed=3))
    r = np.corrcoef(D.T)
    assert np.all(np.abs(r[~np.eye(4, dtype=bool)] - 0.5) < 0.05)
    age = D[:, 0] * 0.25 * (AGE_HI - AGE_LO) + 0.5 * (AGE_LO + AGE_HI)
    bmi = D[:, 1] * 0.25 * (BMI_HI - BMI_LO) + 0.5 * (BMI_LO + BMI_HI)
    assert np.allclose(age, np.round(age), atol=1e-9) and np.allclose(bmi, np.round(bmi, 1), atol=1e-9)


def test_segment_shard_covers_the_flattened_space():
    """dcor.dist.segment_shard: the ranks' pieces, in rank order, are the (segment, replicate) space
    once and in order; on equal segments it is sweep_shard; fewer items than ranks leaves ranks empty."""
    from dcor.dist import segment_shard, sweep_shard
    for reps in ([5, 5, 5, 5], [3, 0, 4, 1], [1], [0, 0, 2], [], [7, 1, 1, 1, 30]):
        flat = [(j, r) for j, c in enumerate(reps) for r in range(c)]
        for world in (1, 2, 3, 5):
            got = [(j, r0 + i) for rank in range(world) for j, r0, c in segment_shard(reps, rank, world)
                   for i in range(c)]
            assert got == flat, (reps, world)
            assert all(c > 0 for rank in range(world) for _, _, c in segment_shard(reps, rank, world))
    for world in (1, 2, 3, 7):
        for rank in range(world):
            assert segment_shard([5] * 4, rank, world) == sweep_shard(4, 5, rank, world)
    assert segment_shard([1], 0, 2) == [] and segment_shard([1], 1, 2) == [(0, 0, 1)]
