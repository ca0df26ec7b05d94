"""CPU tests of the sub-G table boundary (dcor_subg_table_launch): the structs' layout against the
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
NAME = "dcor_subg_table_launch"
FAKE = 8   # a non-null, 8-byte aligned pointer value that is never dereferenced


def _desc(eta=(1.0, 0.5, 0.8), **kw):
    """The descriptor and the host eta array it points to (kept alive by the caller)."""
    from dcor import _lib
    d = dict(n=100, p=3, ld=100, D=FAKE, alpha=0.05, nsim=1000)
    d.update(kw)
    arr = None if eta is None else (C.c_double * len(eta))(*eta)
    desc = _lib.SubgTableDesc(eta=arr, **d)
    desc._keep = arr
    return desc


def _segs(*kws):
    from dcor import _lib
    base = dict(eps1=1.0, eps2=1.0, seed=1, reps=1, col_x=0, col_y=1)
    return (_lib.SubgPairSegment * len(kws))(*[_lib.SubgPairSegment(**{**base, **k}) for k in kws])


def _call(desc, segs, nseg=None, out=FAKE):
    from dcor import _lib
    return _lib.lib.dcor_subg_table_launch(None if desc is None else C.byref(desc), segs,
                                           (0 if segs is None else len(segs)) if nseg is None else nseg,
                                           None if out is None else C.c_void_p(out), None)


def _refused(desc, segs, *needles):
    from dcor import _lib
    assert _call(desc, segs) == _lib.DCOR_EINVAL, needles
    msg = _lib.last_error()
    for s in ("subg_table",) + needles:
        assert s in msg, (s, msg)


def _accepted(desc, segs):
    """A valid call passes every check and gets as far as the device query -- asserted only where
    there is no device: with one the fake pointers must not be launched on."""
    from dcor import _lib
    if _lib.lib.dcor_device_count() == 0:
        assert _call(desc, segs) == _lib.DCOR_ENODEV, _lib.last_error()


def test_entry_declared_exported_and_bound():
    from dcor import _lib
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"\bint\s+" + NAME + r"\s*\(", txt), "not declared in include/dcor.h"
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    assert re.search(r"\bT " + NAME + r"$", out, flags=re.M), "not an exported C symbol"
    assert NAME in _lib.SIGNATURES
    # the planner stays out of the dynamic symbols
    assert "plan_subg_table" not in out


def test_struct_layout_matches_header():
    """sizeof / offsetof of both structs from a C program compiled against include/dcor.h; the pair
    segment starts with dcor_subg_segment's fields at dcor_subg_segment's offsets."""
    from dcor import _lib
    structs = {"dcor_subg_table_desc": _lib.SubgTableDesc, "dcor_subg_pair_segment": _lib.SubgPairSegment,
               "dcor_subg_segment": _lib.SubgSegment}
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
    assert int(got["dcor_subg_table_desc"]) == 56 and int(got["dcor_subg_pair_segment"]) == 56
    for fname, _ in _lib.SubgSegment._fields_:   # the C offsets, not only the bindings'
        assert got[f"dcor_subg_pair_segment.{fname}"] == got[f"dcor_subg_segment.{fname}"], fname
    assert int(got["dcor_subg_pair_segment.col_x"]) == 48 and int(got["dcor_subg_pair_segment.col_y"]) == 52


def test_null_and_misaligned_arguments_rejected_without_gpu():
    from dcor import _lib
    seg = _segs({})
    assert _call(None, seg) == _lib.DCOR_EINVAL
    assert _call(_desc(), None, nseg=1) == _lib.DCOR_EINVAL
    assert _call(_desc(), seg, out=None) == _lib.DCOR_EINVAL
    assert _call(_desc(), seg, nseg=-1) == _lib.DCOR_EINVAL
    _refused(_desc(D=0), seg, "null argument")
    _refused(_desc(eta=None), seg, "null argument", "eta")
    _refused(_desc(D=12), seg, "D must be aligned to 8 bytes")


def test_table_geometry_eta_and_columns_rejected_without_gpu():
    """n, p, ld, the columns' scratch, every eta[c] (the message names the column) and a column
    outside [0, p) (the message names the segment): DCOR_EINVAL, no device needed, no allocation."""
    from dcor import _lib
    allocs = _lib.lib.dcor_alloc_count()
    for n in (0, -5, 2**31):
        _refused(_desc(n=n, ld=max(n, 1)), _segs({}), "n must be in [1, 2^31)")
    for p in (0, -3, 2**31):
        _refused(_desc(p=p), _segs({}), "p must be in [1, 2^31)")
    _refused(_desc(ld=99), _segs({}), "ld = 99 < n = 100")
    _accepted(_desc(ld=2**40), _segs({}))
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        _refused(_desc(eta=(1.0, 0.5, bad)), _segs({}), "column 2: eta must be finite and > 0")
    _refused(_desc(eta=(0.0, 0.5, 0.0)), _segs({}), "column 0:")
    for bad in (dict(col_y=3), dict(col_x=3), dict(col_x=-1), dict(col_y=-1), dict(col_x=2**31 - 1)):
        _refused(_desc(), _segs({}, dict(col_x=2, col_y=2), bad), "segment 2: columns", "outside [0, 3)")
    # a bad column in a zero-replicate segment is refused too
    _refused(_desc(), _segs({}, dict(col_y=3, reps=0)), "segment 1: columns (0, 3)")
    # (a, a) and (b, a) are valid
    _accepted(_desc(), _segs(dict(col_x=2, col_y=2), dict(col_x=2, col_y=0)))
    # p * npad * 8 bytes: (2^31 - 1) columns of 2^31 padded samples do not fit; refused before eta
    # (three entries here) is read
    big = 2**31 - 1
    _refused(_desc(n=big, p=big, ld=big), _segs({}), "scratch bytes overflow")
    assert _lib.lib.dcor_alloc_count() == allocs


def test_invalid_segments_and_descriptor_rejected_without_gpu():
    """The panel entry's checks carried over: each returns its code with no device present; a bad
    LAST segment is caught although the earlier ones are valid, and the message names it."""
    from dcor import _lib
    allocs = _lib.lib.dcor_alloc_count()
    for bad in (dict(eps1=0.0), dict(eps2=-1.0), dict(eps1=float("nan")), dict(eps2=float("inf")),
                dict(eps1=float("inf")), dict(reps=-1), dict(rep_begin=-1), dict(out_row=-1)):
        _refused(_desc(), _segs({}, {}, bad), "segment 2:")
        # a segment without replicates is checked too
        _refused(_desc(), _segs({}, {**bad, **({} if "reps" in bad else dict(reps=0))}), "segment 1:")
    for rb, reps in ((2**32 - 6, 7), (2**63 - 2, 2), (2**32 - 2, 4), (0xfffffffe, 3)):   # the first: 2^32 + 1
        _refused(_desc(), _segs({}, dict(rep_begin=rb, reps=reps)), "segment 1: replicate range exceeds 2^32")
    _accepted(_desc(), _segs(dict(rep_begin=0xfffffffd, reps=2)))
    _refused(_desc(), _segs(dict(reps=2**30), dict(reps=2**30)), "2^31 - 1")
    for bad, needle in ((dict(nsim=0), "nsim"), (dict(nsim=2049), "nsim must be in [1, 2048]"),
                        (dict(alpha=2.0), "alpha must be < 2"), (dict(alpha=float("nan")), "alpha")):
        assert _call(_desc(**bad), _segs({})) == _lib.DCOR_EINVAL, bad
        assert needle in _lib.last_error(), (bad, _lib.last_error())
    # the header's order: D's alignment, n, p, ld, eta, alpha, nsim, then the segments
    worst = dict(eps1=0.0, col_x=9)
    for kw, needle in ((dict(nsim=0), "nsim"), (dict(nsim=0, alpha=3.0), "alpha"),
                       (dict(nsim=0, alpha=3.0, eta=(1.0, -1.0, 1.0)), "column 1"),
                       (dict(nsim=0, eta=(1.0, -1.0, 1.0), ld=5), "ld = 5"),
                       (dict(eta=(1.0, -1.0, 1.0), ld=5, p=0), "p must be"),
                       (dict(ld=5, p=0, n=0), "n must be"), (dict(p=0, n=0, D=20), "aligned")):
        assert _call(_desc(**kw), _segs(worst)) == _lib.DCOR_EINVAL, kw
        assert needle in _lib.last_error(), (kw, _lib.last_error())
    # eps before the columns within a segment, an earlier segment before a later one
    _refused(_desc(), _segs(dict(col_x=9), dict(eps1=0.0)), "segment 0: columns")
    _refused(_desc(), _segs(worst), "segment 0: need finite eps1, eps2 > 0")
    assert _lib.lib.dcor_alloc_count() == allocs


def test_small_n_and_empty_calls_are_ok_without_gpu():
    """m > n gives m = n, k = 1 (never DCOR_EKLT1); nseg = 0 and segments with no replicates at all
    return DCOR_OK: no device work."""
    from dcor import _lib
    for n, e in ((1, 1.0), (5, 1.0), (100, 0.2)):
        assert _call(_desc(n=n, ld=n), _segs(dict(eps1=e, eps2=e, reps=0))) == _lib.DCOR_OK, (n, e)
    assert _call(_desc(), None, nseg=0, out=None) == _lib.DCOR_OK
    assert _call(_desc(), _segs(dict(reps=0), dict(reps=0, eps1=2.0, col_x=2))) == _lib.DCOR_OK


def test_valid_calls_fail_loudly_without_gpu():
    """The shapes of the GPU tests pass every check and reach the device query (DCOR_ENODEV here)."""
    from dcor import _lib
    if _lib.lib.dcor_device_count() > 0:
        return   # with a device the fake pointers must not be launched on
    assert _call(_desc(), _segs({})) == _lib.DCOR_ENODEV
    pairs = [(0, 1), (1, 0), (2, 2), (3, 1), (0, 3)]
    eps = [(1.0, 1.0), (2.0, 0.5), (0.2, 0.2), (0.5, 1.5), (1.5, 0.5)]
    segs = [dict(col_x=a, col_y=b, eps1=e1, eps2=e2, seed=(j << 32) + 5, rep_begin=(0, 2**32 - 6)[j % 2], reps=5,
                 out_row=5 * j) for j, ((a, b), (e1, e2)) in enumerate(zip(pairs, eps))]
    for n in (5, 12, 37, 1001, 16384, 16385):
        assert _call(_desc(eta=(1.0, 0.5, 0.8, 1.3), n=n, p=4, ld=n + 1), _segs(*segs)) == _lib.DCOR_ENODEV, n


def test_python_surface_checks_before_device_work():
    from dcor import subgpanel
    D = np.zeros((16, 3))
    with pytest.raises(ValueError, match="outside"):
        subgpanel.table_segments(D, [(0, 3, 1.0, 1.0, 1, 0, 1)])
    with pytest.raises(ValueError, match=r"\(n, p\)"):
        subgpanel.table_segments(np.zeros(16), [])
    with pytest.raises(ValueError, match="eta must be"):
        subgpanel.table_segments(D, [(0, 1, 1.0, 1.0, 1, 0, 1)], eta=[1.0, 2.0])
    assert subgpanel.all_pairs is __import__("dcor").signpanel.all_pairs
    assert subgpanel._eps_pairs([0.5, (1.5, 0.5)]) == [(0.5, 0.5), (1.5, 0.5)]
