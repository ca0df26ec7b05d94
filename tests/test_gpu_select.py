"""The four order-statistic selectors of csrc/dcor_device.h on adversarial keys, exactly.

dcor_diag_select runs value_select, reg_select, wave_select<16 / 32> and wave_select_lds<16 / 32> on
caller keys; every family of tests/select_ref.py (ties, NaN, infinities, range edges, the round-cap
ladder, radix digits, set sizes, and the benign draws the suite used before) must come back equal to
sort(keys without NaN)[pos] -- a selector returns one of its inputs, so there is no tolerance.  Sets of
one size and position share a launch (tens of sets each), and two launches mix families so that the
waves of one workgroup run different numbers of rounds.  The public glue (dcor_mixquant,
dcor_premat_subg_launch under both DCOR_EPILOGUE settings) gets a few of the same key sets as z
with l = 0, where z + c * 0 == z."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import numpy_ref
import select_ref as S
from helpers import assert_close, unit_laplace

pytestmark = pytest.mark.gpu

_D = C.POINTER(C.c_double)


def select(which, sets, pos):
    """One dcor_diag_select launch: sets [nsets][nkeys] -> [nsets]."""
    from dcor import _lib
    k = np.ascontiguousarray(sets, dtype=np.float64)
    out = np.full(k.shape[0], -12345.0)
    _lib.check(_lib.lib.dcor_diag_select(k.ctypes.data_as(_D), k.shape[1], k.shape[0], pos, which,
                                         out.ctypes.data_as(_D)))
    return out


@functools.lru_cache(maxsize=None)
def batches(family, n):
    """The family's (case, pos) pairs at set size n, grouped into launches by (set size, pos), each
    with its reference: computed once, shared by the six selectors."""
    groups = {}
    for c in S.family_cases(family, n):
        for p in c.pos:
            groups.setdefault((len(c.keys), p), []).append((c.name, c.keys, S.reference(c.keys, p)))
    return groups


@pytest.mark.parametrize("which", sorted(S.WHICH), ids=lambda w: S.WHICH[w])
@pytest.mark.parametrize("family", sorted(S.FAMILIES))
def test_selector_matches_sort(family, which):
    bad, nsets = [], 0
    for n in ((1000,) if family == "sizes" else (1000, 2000)):
        for (nkeys, pos), items in batches(family, n).items():
            if nkeys > S.max_keys(which):
                continue
            got = select(which, np.stack([k for _, k, _ in items]), pos)
            nsets += len(items)
            bad += [(name, nkeys, pos, g, r) for (name, _, r), g in zip(items, got) if not S.same(g, r)]
    assert nsets > 0
    assert not bad, f"{S.WHICH[which]}: {len(bad)} of {nsets} wrong (name, nkeys, pos, got, ref): {bad[:12]}"


@pytest.mark.parametrize("nsets", [5, 7])
@pytest.mark.parametrize("which", sorted(S.WHICH), ids=lambda w: S.WHICH[w])
def test_mixed_families_in_one_launch(which, nsets):
    """Sets of different families in one launch: with one wave per set the waves of a workgroup run
    1 to 12 rounds side by side (their scratch and wave_sync must not interact), and 5 or 7 sets
    leave the last workgroup part-filled."""
    n, pos = 1000, 99
    by = {c.name: c.keys for f in ("ladder", "baseline", "ties", "inf", "range", "nan", "radix") for c in S.FAMILIES[f](n)}
    names = ["ladder200", "normal+1.0lap-seed1", "all-equal", "inf-100-100", "subnormal-range", "nan-interleaved",
             "low-byte"][:nsets]
    sets = np.stack([by[x] for x in names])
    got = select(which, sets, pos)
    ref = [S.reference(k, pos) for k in sets]
    assert all(S.same(g, r) for g, r in zip(got, ref)), (names, got, ref)


GLUE = [("ties", "all-equal"), ("ties", "two-split974"), ("ties", "bin65tied"), ("ties", "bin257"),
        ("nan", "nan-one"), ("nan", "nan-all-but-one"), ("nan", "nan-all"), ("nan", "nan-interleaved"),
        ("inf", "inf-3-70"), ("inf", "inf-only"), ("inf", "inf-nan"), ("inf", "inf-one-finite"),
        ("ladder", "ladder80"), ("ladder", "ladder200"), ("ladder", "ladder200-mirror"), ("ladder", "ladder81-neg")]


def _glue_keys(n, scale=1.0):
    """The GLUE key sets at size n; `scale` (a power of two: exact) shrinks the ties and NaN families."""
    by = {(f, c.name): c.keys * (scale if f in ("ties", "nan") else 1.0)
          for f in ("ties", "nan", "inf", "ladder") for c in S.FAMILIES[f](n)}
    by["nan", "nan-one"] = by["nan", "nan-middle"]
    by["ties", "two-split974"] = by["ties", f"two-split{math.ceil(0.975 * n) - 1}"]
    return [(f"{name}@{n}", by[f, name]) for f, name in GLUE]


def test_mixquant_entry_on_adversarial_keys():
    """dcor_mixquant(z, l = 0, c, p) = sort(z without NaN)[ceiling(p nsim) - 1], NaN past the valid keys."""
    from dcor import _lib
    bad = []
    for n in (1000, 2000):
        zero = np.zeros(n)
        for name, z in _glue_keys(n):
            z = np.ascontiguousarray(z)
            for p in (0.025, 0.25, 0.975, 1.0):
                out = C.c_double(-12345.0)
                _lib.check(_lib.lib.dcor_mixquant(z.ctypes.data_as(_D), zero.ctypes.data_as(_D), n, 0.75, p, C.byref(out)))
                ref = S.reference(z, math.ceil(p * n) - 1)
                assert S.same(ref, numpy_ref.mixquant(z, zero, 0.75, p))
                if not S.same(out.value, ref):
                    bad.append((name, p, out.value, ref))
    assert not bad, bad


@pytest.mark.parametrize("alpha", [0.05, 1.9])
@pytest.mark.parametrize("nsim", [1000, 2000])
def test_premat_subg_epilogues_on_adversarial_keys(variant, nsim, alpha):
    """dcor_premat_subg_launch with caller mixquant keys (z = the key set, l = 0), one replicate per
    key set, under the workgroup epilogue (value_select) and the wave epilogue (wave_select): the INT
    triple equals numpy_ref.int_subg, and the two epilogues write identical records.  n = 2 is the
    smallest n with a sample variance (n = 1 passes the entry's checks, but its c* is NaN and so is
    every key).  alpha = 1.9 asks element ceiling(0.05 nsim), inside the ladders' crowd.  Samples and
    noise are kept small, so that no product is clipped (sd > 0, a finite c*) and rho stays inside
    (-1, 1), where a width of 0 -- the ladders' crowd -- shows as lo = hi = rho; the ties and NaN
    sets are scaled by 2^-10 to keep most of their widths inside the clip at +-1 too."""
    import torch
    from dcor import _lib
    sets = _glue_keys(nsim, scale=2.0 ** -10)
    R, n, eps1, eps2 = len(sets), 2, 1.0, 0.8
    g = np.random.default_rng(nsim)
    X, Y = g.uniform(-0.5, 0.5, (R, n)), g.uniform(-0.5, 0.5, (R, n))
    lx, ly = unit_laplace(g, (R, 1)), unit_laplace(g, (R, 1))       # m = min(ceil(8 / (eps1 eps2)), n) = 2, k = 1
    ll, lc = g.uniform(-0.2, 0.2, (R, n)), g.uniform(-0.05, 0.05, R)
    mz, ml = np.stack([k for _, k in sets]), np.zeros((R, nsim))
    T = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in
         dict(X=X, Y=Y, lx=lx, ly=ly, ll=ll, lc=lc, mz=mz, ml=ml).items()}
    d = _lib.PrematSubg(n=n, reps=R, eps1=eps1, eps2=eps2, eta1=1.0, eta2=1.0, alpha=alpha, hrs=0,
                        lam_x=math.nan, lam_y=math.nan, lam_s=math.nan, lam_o=math.nan, lam_r=math.nan,
                        delta=math.nan, nsim=nsim, X=T["X"].data_ptr(), Y=T["Y"].data_ptr(), xy_stride=n,
                        perm=None, lap_ni_x=T["lx"].data_ptr(), lap_ni_y=T["ly"].data_ptr(),
                        lap_local=T["ll"].data_ptr(), lap_central=T["lc"].data_ptr(),
                        mix_z=T["mz"].data_ptr(), mix_l=T["ml"].data_ptr())
    got = {}
    for epi in ("block", "wave"):
        variant("DCOR_EPILOGUE", epi)
        out = torch.full((R, 6), -7.0, dtype=torch.float64, device="cuda")
        _lib.check(_lib.lib.dcor_premat_subg_launch(C.byref(d), C.c_void_p(out.data_ptr()), None))
        got[epi] = out.cpu().numpy()
    for r, (name, z) in enumerate(sets):
        ref = numpy_ref.int_subg(X[r], Y[r], eps1, eps2, alpha=alpha, lap_local=ll[r], lap_central=lc[r],
                                 mix_z=z, mix_l=ml[r])
        for epi in got:
            assert_close(got[epi][r, 3:], ref, what=f"{name}, {epi} epilogue, INT triple")
    np.testing.assert_array_equal(got["wave"], got["block"])
