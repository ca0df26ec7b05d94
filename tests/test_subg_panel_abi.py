"""CPU tests of the sub-G panel boundary (dcor_subg_panel_launch): the structs' layout against the
header, the entry declared / exported / bound, and every argument check happening before any
device access.  Also pins the numpy restatement of the draw contract (tests/subg_panel_ref.py) to
the fused engine's oracle, and the law check's power on the CPU side."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np

import subg_panel_ref as R
from helpers import assert_close

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "dcor.h")
NAME = "dcor_subg_panel_launch"
FAKE = 8   # a non-null, 8-byte aligned pointer value that is never dereferenced


def _desc(**kw):
    from dcor import _lib
    d = dict(n=100, X=FAKE, Y=FAKE, eta1=1.0, eta2=1.0, alpha=0.05, nsim=1000)
    d.update(kw)
    return _lib.SubgPanelDesc(**d)


def _segs(*kws):
    from dcor import _lib
    return (_lib.SubgSegment * len(kws))(*[_lib.SubgSegment(**{**dict(eps1=1.0, eps2=1.0, seed=1, reps=1), **k})
                                           for k in kws])


def _call(desc, segs, nseg=None, out=FAKE):
    from dcor import _lib
    return _lib.lib.dcor_subg_panel_launch(None if desc is None else C.byref(desc), segs,
                                           (0 if segs is None else len(segs)) if nseg is None else nseg,
                                           None if out is None else C.c_void_p(out), None)


def test_entry_declared_exported_and_bound():
    from dcor import _lib
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"\bint\s+" + NAME + r"\s*\(", txt), "not declared in include/dcor.h"
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    assert re.search(r"\bT " + NAME + r"$", out, flags=re.M), "not an exported C symbol"
    assert NAME in _lib.SIGNATURES
    # the planner stays out of the dynamic symbols
    assert "plan_subg_panel" not in out


def test_struct_layout_matches_header():
    """sizeof / offsetof of both structs from a C program compiled against include/dcor.h."""
    from dcor import _lib
    structs = {"dcor_subg_panel_desc": _lib.SubgPanelDesc, "dcor_subg_segment": _lib.SubgSegment}
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
    assert C.sizeof(_lib.SubgPanelDesc) == 56 and C.sizeof(_lib.SubgSegment) == 48


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
    assert _call(_desc(X=12), seg) == _lib.DCOR_EINVAL
    assert "aligned" in _lib.last_error()


def test_invalid_segments_and_descriptor_rejected_without_gpu():
    """Each invalid argument returns its code with no device present and no allocation made; a bad
    LAST segment is caught although the earlier ones are valid, and the message names it."""
    from dcor import _lib
    allocs = _lib.lib.dcor_alloc_count()
    for bad in (dict(eps1=0.0), dict(eps2=-1.0), dict(eps1=float("nan")), dict(eps2=float("inf")),
                dict(eps1=float("inf")), dict(reps=-1), dict(rep_begin=-1), dict(out_row=-1)):
        assert _call(_desc(), _segs({}, {}, bad)) == _lib.DCOR_EINVAL, bad
        assert "segment 2:" in _lib.last_error(), (bad, _lib.last_error())
        # a segment without replicates is checked too
        assert _call(_desc(), _segs({}, {**bad, **({} if "reps" in bad else dict(reps=0))})) == _lib.DCOR_EINVAL, bad
    for rb, reps in ((2**63 - 2, 2), (2**32 - 2, 4), (0xfffffffe, 3)):
        assert _call(_desc(), _segs({}, dict(rep_begin=rb, reps=reps))) == _lib.DCOR_EINVAL, (rb, reps)
        assert "segment 1: replicate range exceeds 2^32" in _lib.last_error()
    # the last allowed range passes the checks: the call gets as far as the device (only where there
    # is none: with a device the fake pointers must not be launched on)
    if _lib.lib.dcor_device_count() == 0:
        assert _call(_desc(), _segs(dict(rep_begin=0xfffffffd, reps=2))) == _lib.DCOR_ENODEV
    assert _call(_desc(), _segs(dict(rep_begin=0xfffffffd, reps=2), dict(reps=-1))) == _lib.DCOR_EINVAL
    assert "segment 1:" in _lib.last_error()
    # more than 2^31 - 1 replicates in one call
    assert _call(_desc(), _segs(dict(reps=2**30), dict(reps=2**30))) == _lib.DCOR_EINVAL
    assert "2^31 - 1" in _lib.last_error()
    for bad in (dict(n=0), dict(n=-5), dict(n=2**31), dict(nsim=0), dict(nsim=2049), dict(alpha=2.0),
                dict(alpha=float("nan")), dict(eta1=0.0), dict(eta2=-1.0), dict(eta1=float("nan")),
                dict(eta2=float("inf"))):
        assert _call(_desc(**bad), _segs({})) == _lib.DCOR_EINVAL, bad
    # the header's order: the descriptor before the segments
    assert _call(_desc(n=0), _segs(dict(eps1=0.0))) == _lib.DCOR_EINVAL
    assert "n must be" in _lib.last_error()
    assert _call(_desc(eta1=0.0, nsim=0), _segs(dict(eps1=0.0))) == _lib.DCOR_EINVAL
    assert "eta1" in _lib.last_error()
    assert _lib.lib.dcor_alloc_count() == allocs


def test_small_n_is_valid_without_gpu():
    """m > n gives m = n, k = 1 (ver-cor-subG.R:37): never DCOR_EKLT1, unlike the sign family."""
    from dcor import _lib
    for n, e in ((1, 1.0), (5, 1.0), (100, 0.2)):
        assert _call(_desc(n=n), _segs(dict(eps1=e, eps2=e, reps=0))) == _lib.DCOR_OK, (n, e)


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


# ------------------------------------------------------------- the numpy restatement
def test_local_laplace_is_words_23_of_the_dgp_b_block():
    import oracle.oracle as orc
    for seed, rep, n in ((1_000_011, 0, 300), (2**40 + 5, 1001, 257)):
        a = R.local_laplace(orc, n, seed, rep)
        b = R.local_laplace_words(n, seed, rep)
        assert a.shape == b.shape == (n,)
        np.testing.assert_allclose(a, b, rtol=1e-14, atol=1e-300)


def test_restatement_equals_the_fused_oracle_on_its_own_samples():
    """The anchor of the draw contract: on oracle.gen_xy's samples of replicate r of a sub-G cell
    the restated record is oracle.sim_reps's record of that replicate (same draws at every site;
    the two differ only in the order of the sums)."""
    import oracle.oracle as orc
    from dcor.sim import CellSpec
    for kw in (dict(n=1000, eps1=1.0, eps2=1.0, dgp="bounded_factor", rho=0.3, seed=1_000_011),
               dict(n=1003, eps1=1.5, eps2=0.5, dgp="bounded_factor", rho=0.3, seed=2**40 + 7),
               dict(n=1003, eps1=0.5, eps2=1.5, dgp="gaussian", rho=0.5, seed=1_000_073, eta1=0.5, eta2=0.8),
               dict(n=401, eps1=0.2, eps2=0.2, dgp="gaussian", rho=0.5, seed=5, nsim=2000)):
        cell = CellSpec(family="subG", **kw)
        cs = cell.to_c()
        for rep in (0, 1, 1001):
            X, Y = orc.gen_xy(cs, rep)
            got = R.oracle_record(orc, X, Y, cell.eps1, cell.eps2, cell.seed, rep, eta1=cs.eta1, eta2=cs.eta2,
                                  alpha=cs.alpha, nsim=cs.nsim)
            assert_close(got, orc.sim_reps(cs, rep, rep + 1)[0], what=f"{kw} rep {rep}")


def test_law_check_is_well_defined_and_has_power():
    """The CPU side of the GPU law check (tests/test_gpu_subg_panel.py): the restatement's records
    on the law panel are finite with the INT interval inside (-1, 1) for most replicates, two
    independent runs of it pass the Welch test, and a restatement with the local noise scale halved
    fails it -- so the test would see a miscalibrated local Laplace."""
    import oracle.oracle as orc
    X, Y = R.law_panel()
    a = R.oracle_records(orc, X, Y, 1.0, 1.0, 777, 0, 2000)
    b = R.oracle_records(orc, X, Y, 1.0, 1.0, 424242, 0, 2000)
    h = R.oracle_records(orc, X, Y, 1.0, 1.0, 424242, 0, 2000, local_scale=0.5)
    assert a.shape == (2000, 6) and not np.isnan(a).any() and not np.isnan(h).any()
    assert np.mean((a[:, 4] > -1.0) & (a[:, 5] < 1.0)) > 0.9
    ts = [R.welch_t(u, v) for u, v in zip(R.law_stats(a), R.law_stats(b))]
    assert all(abs(t) < 5.0 for t in ts), ts
    th = [R.welch_t(u, v) for u, v in zip(R.law_stats(a), R.law_stats(h))]
    assert max(abs(t) for t in th) > 5.0, th
