"""CPU tests of the fused HRS sweep's boundary (dcor_hrs_fused_sweep_launch, mode='fused' of the
Python sweeps): the entry is declared, exported and bound, and every argument check that needs no
device happens before any device access."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "dcor.h")
NAME = "dcor_hrs_fused_sweep_launch"


def _base():
    from dcor import _lib
    return _lib.PrematSubg(n=10, eta1=1.0, eta2=1.0, alpha=0.05, hrs=1, lam_x=2.0, lam_y=2.0, lam_s=2.0,
                           lam_o=2.0, delta=0.1, nsim=10)


def test_entry_declared_exported_and_bound():
    from dcor import _lib
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"\bint\s+" + NAME + r"\s*\(", txt), "not declared in include/dcor.h"
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    assert re.search(r"\bT " + NAME + r"$", out, flags=re.M), "not an exported C symbol"
    assert NAME in _lib.SIGNATURES
    # the segment struct and the argument list are dcor_hrs_sweep_launch's
    assert _lib.SIGNATURES[NAME] == _lib.SIGNATURES["dcor_hrs_sweep_launch"]


def test_null_arguments_rejected_without_gpu():
    """Null base / panel / segs / d_out with nseg > 0: DCOR_EINVAL before any device access (the
    panel and output pointers below are never dereferenced)."""
    from dcor import _lib
    f = _lib.lib.dcor_hrs_fused_sweep_launch
    base = _base()
    seg = (_lib.HrsSegment * 1)(_lib.HrsSegment(eps=1.0, reps=1))
    fake, out = C.c_void_p(8), C.c_void_p(8)
    assert f(None, fake, seg, 1, out, None) == _lib.DCOR_EINVAL
    assert f(C.byref(base), None, seg, 1, out, None) == _lib.DCOR_EINVAL
    assert f(C.byref(base), fake, None, 1, out, None) == _lib.DCOR_EINVAL
    assert f(C.byref(base), fake, seg, 1, None, None) == _lib.DCOR_EINVAL
    assert f(C.byref(base), fake, seg, -1, out, None) == _lib.DCOR_EINVAL
    assert "null argument" in _lib.last_error()


def test_replicate_range_rejected_without_wrapping():
    """rep_begin = INT64_MAX - 1 with reps = 2: the range check does not form the sum.  The
    segments' own fields are checked before the panel is looked at, so no panel is needed."""
    from dcor import _lib
    f = _lib.lib.dcor_hrs_fused_sweep_launch
    base = _base()
    fake, out = C.c_void_p(8), C.c_void_p(8)
    allocs = _lib.lib.dcor_alloc_count()
    for rb, reps in ((2**63 - 2, 2), (2**32 - 2, 4), (0xfffffffe, 2)):
        seg = (_lib.HrsSegment * 2)(_lib.HrsSegment(eps=1.0, reps=0),
                                    _lib.HrsSegment(eps=2.0, seed_ni=1, seed_int=2, rep_begin=rb, reps=reps))
        assert f(C.byref(base), fake, seg, 2, out, None) == _lib.DCOR_EINVAL, (rb, reps)
        assert "segment 1: replicate range exceeds 2^32" in _lib.last_error()
    for bad in (dict(eps=0.0), dict(eps=float("nan")), dict(reps=-1), dict(rep_begin=-1), dict(out_row=-1)):
        seg = (_lib.HrsSegment * 1)(_lib.HrsSegment(**{**dict(eps=1.0, reps=1), **bad}))
        assert f(C.byref(base), fake, seg, 1, out, None) == _lib.DCOR_EINVAL, bad
    assert _lib.lib.dcor_alloc_count() == allocs


def test_empty_sweep_is_ok_without_gpu():
    """nseg = 0 returns DCOR_OK: no device work, so no device is needed."""
    from dcor import _lib
    base = _base()
    assert _lib.lib.dcor_hrs_fused_sweep_launch(C.byref(base), C.c_void_p(8), None, 0, None, None) == _lib.DCOR_OK


def test_mode_checks_come_before_device_work():
    """mode='fused' with rng='R' or streams > 1, and an unknown mode, raise ValueError before the
    functions import torch or touch a device: on a host without a GPU anything later would fail
    with another error."""
    import numpy as np
    from dcor import hrs
    x = np.zeros(4)
    with pytest.raises(ValueError, match="rng='philox'"):
        hrs.eps_sweep(x, x, 2.0, 2.0, mode="fused", rng="R")
    with pytest.raises(ValueError, match="streams=1"):
        hrs.eps_sweep(x, x, 2.0, 2.0, mode="fused", streams=2)
    with pytest.raises(ValueError, match="streams=1"):
        hrs.sweep_segments(x, x, 2.0, 2.0, (2.0,), [(0, 0, 1)], mode="fused", streams=2)
    for f, a in ((hrs.eps_sweep, ()), (hrs.sweep_segments, ((2.0,), [(0, 0, 1)]))):
        with pytest.raises(ValueError, match="mode must be"):
            f(x, x, 2.0, 2.0, *a, mode="nope")


def test_distributed_sweep_mode_checked():
    from dcor import hrs
    with pytest.raises(ValueError):
        hrs._check_sweep_mode("fused", "R", 1)
    with pytest.raises(ValueError):
        hrs._check_sweep_mode("fused", "philox", 2)
    with pytest.raises(ValueError):
        hrs._check_sweep_mode("other", "philox", 1)
    hrs._check_sweep_mode("fused", "philox", 1)
    hrs._check_sweep_mode("premat", "R", 4)
