"""CPU tests of the sign-panel boundary (dcor_sign_panel_launch): the structs' layout against the
header, the entry declared / exported / bound, and every argument check happening before any
device access.  Also pins the tests' own numpy Philox and the oracle side of the GPU law check."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np

import sign_panel_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "dcor.h")
NAME = "dcor_sign_panel_launch"
FAKE = 8   # a non-null pointer value that is never dereferenced


def _desc(**kw):
    from dcor import _lib
    d = dict(n=100, X=FAKE, Y=FAKE, alpha=0.05, normalise=1, ci_mode=0, nsim=1000)
    d.update(kw)
    return _lib.SignPanelDesc(**d)


def _segs(*kws):
    from dcor import _lib
    return (_lib.SignSegment * len(kws))(*[_lib.SignSegment(**{**dict(eps1=1.0, eps2=1.0, seed=1, reps=1), **k})
                                           for k in kws])


def _call(desc, segs, nseg=None, out=FAKE):
    from dcor import _lib
    return _lib.lib.dcor_sign_panel_launch(None if desc is None else C.byref(desc), segs,
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
    """sizeof / offsetof of both structs from a C program compiled against include/dcor.h."""
    from dcor import _lib
    structs = {"dcor_sign_panel_desc": _lib.SignPanelDesc, "dcor_sign_segment": _lib.SignSegment}
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
    assert C.sizeof(_lib.SignPanelDesc) == 48 and C.sizeof(_lib.SignSegment) == 48


def test_null_arguments_rejected_without_gpu():
    from dcor import _lib
    seg = _segs({})
    assert _call(None, seg) == _lib.DCOR_EINVAL
    assert _call(_desc(), None, nseg=1) == _lib.DCOR_EINVAL
    assert _call(_desc(), seg, out=None) == _lib.DCOR_EINVAL
    assert _call(_desc(), seg, nseg=-1) == _lib.DCOR_EINVAL
    assert _call(_desc(X=0), seg) == _lib.DCOR_EINVAL
    assert _call(_desc(Y=0), seg) == _lib.DCOR_EINVAL
    assert "null argument" in _lib.last_error()


def test_invalid_segments_and_descriptor_rejected_without_gpu():
    """Each invalid argument returns its code with no device present and no allocation made; a bad
    LAST segment is caught although the earlier ones are valid."""
    from dcor import _lib
    allocs = _lib.lib.dcor_alloc_count()
    for bad in (dict(eps1=0.0), dict(eps2=-1.0), dict(eps1=float("nan")), dict(eps2=float("inf")),
                dict(reps=-1), dict(rep_begin=-1), dict(out_row=-1)):
        assert _call(_desc(), _segs({}, {}, bad)) == _lib.DCOR_EINVAL, bad
    for rb, reps in ((2**63 - 2, 2), (2**32 - 2, 4), (0xfffffffe, 3)):
        assert _call(_desc(), _segs({}, dict(rep_begin=rb, reps=reps))) == _lib.DCOR_EINVAL, (rb, reps)
        assert "segment 1: replicate range exceeds 2^32" in _lib.last_error()
    # the last allowed range passes the checks: the call gets as far as the device
    assert _call(_desc(), _segs(dict(rep_begin=0xfffffffd, reps=2))) != _lib.DCOR_EINVAL
    # more than 2^31 - 1 replicates in one call
    assert _call(_desc(), _segs(dict(reps=2**30), dict(reps=2**30))) == _lib.DCOR_EINVAL
    assert "2^31 - 1" in _lib.last_error()
    # k = floor(n / m) < 1: n = 100 at eps = (.2, .2) has m = 200 (also in a zero-replicate segment)
    assert _call(_desc(), _segs({}, dict(eps1=0.2, eps2=0.2))) == _lib.DCOR_EKLT1
    assert _call(_desc(), _segs({}, dict(eps1=0.2, eps2=0.2, reps=0))) == _lib.DCOR_EKLT1
    assert _call(_desc(n=7), _segs({})) == _lib.DCOR_EKLT1
    for bad in (dict(n=0), dict(n=-5), dict(n=2**31), dict(nsim=0), dict(nsim=2049), dict(ci_mode=7),
                dict(alpha=2.0), dict(alpha=float("nan"))):
        assert _call(_desc(**bad), _segs({})) == _lib.DCOR_EINVAL, bad
    assert _lib.lib.dcor_alloc_count() == allocs


def test_empty_calls_are_ok_without_gpu():
    """nseg = 0, and segments with no replicates at all, return DCOR_OK: no device work."""
    from dcor import _lib
    assert _call(_desc(), None, nseg=0, out=None) == _lib.DCOR_OK
    assert _call(_desc(), _segs(dict(reps=0), dict(reps=0, eps1=2.0))) == _lib.DCOR_OK


def test_valid_call_fails_loudly_without_gpu():
    from dcor import _lib
    if _lib.lib.dcor_device_count() > 0:
        return   # with a device the fake pointers must not be launched on
    assert _call(_desc(), _segs({})) == _lib.DCOR_ENODEV


def test_python_surface_checks_before_device_work():
    import pytest
    from dcor import signpanel
    x = np.zeros(16)
    with pytest.raises(ValueError, match="mode must be"):
        signpanel.replicates(x, x, 1.0, 1.0, 1, seed=1, mode="nope")


def test_numpy_philox_is_the_oracles():
    import oracle.oracle as orc
    k0, k1 = 0x12345678, 0x9abcdef0
    idx = np.array([0, 1, 7, 2**31 + 5, 2**32 - 1], dtype=np.uint64)
    w = R.philox4x32_10(idx, 1001, 3, 0, k0, k1)
    for j, i in enumerate(idx):
        assert list(orc.philox((int(i), 1001, 3, 0), k0, k1)) == [int(v[j]) for v in w]


def test_law_check_oracle_side_is_well_defined():
    """No NaN among the oracle's records of the law check's input (a sample of its replicates; the
    GPU test asserts it again over all 2,000)."""
    import oracle.oracle as orc
    X, Y = R.law_panel()
    rec = R.oracle_records(orc, X, Y, 1.0, 1.0, 777, 0, 200)
    assert rec.shape == (200, 6) and not np.isnan(rec).any()
    assert np.all(rec[:, 1] <= rec[:, 0]) and np.all(rec[:, 0] <= rec[:, 2])
    assert np.all(rec[:, 4] <= rec[:, 5])
