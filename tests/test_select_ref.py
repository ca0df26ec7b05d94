"""CPU checks of tests/select_ref.py (the key families test_gpu_select.py feeds the selectors):
the builders produce what they say, the reference is R's sort(x)[pos] with NaN dropped, and the numpy
restatement of the wave selectors' round loop shows why the round cap was replaced.  The argument
checks of dcor_diag_select run before any device access, so they are tested here too."""
import ctypes as C
import math

import numpy as np
import pytest

import select_ref as S

NS = (1000, 2000)


@pytest.fixture(scope="module")
def cases():
    return {(f, n): S.family_cases(f, n) for f in S.FAMILIES for n in NS}


def test_reference_hand_cases():
    nan, inf = math.nan, math.inf
    k = np.array([3.0, nan, -inf, 0.0, -0.0, inf, 2.0, nan])
    assert [S.reference(k, p) for p in range(6)] == [-inf, 0.0, 0.0, 2.0, 3.0, inf]
    assert math.isnan(S.reference(k, -1)) and math.isnan(S.reference(k, 6))
    assert math.isnan(S.reference(np.full(5, nan), 0))
    assert S.same(-0.0, 0.0) and S.same(nan, nan) and not S.same(nan, 0.0) and not S.same(1.0, np.nextafter(1.0, 2.0))
    assert S.positions(1000) == [-1, 0, 1, 500, 974, 999, 1000]
    assert S.positions(1) == [-1, 0, 1]


@pytest.mark.parametrize("n", NS)
def test_builders_sizes_and_valid(cases, n):
    for f in S.FAMILIES:
        cs = cases[f, n]
        assert len(cs) >= 4 * len(S.FAMILIES[f](n))          # as built + three arrangements
        for c in cs:
            assert c.keys.dtype == np.float64 and c.keys.ndim == 1
            assert len(c.keys) == (int(c.name.split("/")[0][4:]) if f == "sizes" else n), c.name
            v = S.valid_count(c.keys)
            # an arrangement keeps the multiset: same sorted valid keys (as bits) as the case it came from
            base = next(b for b in cs if b.name == c.name.split("/")[0])
            assert np.array_equal(np.sort(c.keys[~np.isnan(c.keys)].view(np.int64)),
                                  np.sort(base.keys[~np.isnan(base.keys)].view(np.int64))), c.name
            assert len(c.keys) - v == len(base.keys) - S.valid_count(base.keys)
        # every family asks in-range and out-of-range positions
        for c in S.FAMILIES[f](n):
            v = S.valid_count(c.keys)
            assert any(p < 0 or p >= v for p in c.pos), c.name
            assert v == 0 or any(0 <= p < v for p in c.pos), c.name
    assert sorted(len(c.keys) for c in S.fam_sizes()) == sorted(S.SIZES)


def test_builders_hand_values():
    n = 1000
    by = {c.name: c for f in S.FAMILIES for c in S.FAMILIES[f](n)}
    assert S.reference(by["all-equal"].keys, 500) == 2.5
    c = by["two-split499"]   # 499 copies of 1.0, then 2.0
    assert [S.reference(c.keys, p) for p in (498, 499, 500)] == [1.0, 2.0, 2.0]
    for x in (64, 65, 256, 257):   # exactly x keys in value_select's bin [100, 101) and the wave bins' [100, 102)
        for t in ("", "tied"):
            k = by[f"bin{x}{t}"].keys
            assert np.count_nonzero((k >= 100) & (k < 102)) == x and np.count_nonzero((k >= 99) & (k <= 103)) == x
            assert k.min() == 0.0 and k.max() == 256.0
            p = by[f"bin{x}{t}"].pos
            assert 100 <= S.reference(k, p[1]) < 101 and 100 <= S.reference(k, p[3]) < 101
            assert S.reference(k, p[0]) < 99 and S.reference(k, p[4]) > 103
    assert S.valid_count(by["nan-all"].keys) == 0 and S.valid_count(by["nan-all-but-one"].keys) == 1
    assert np.isnan(by["nan-slot0"].keys[:64]).all() and not np.isnan(by["nan-slot0"].keys[64:]).any()
    assert np.isnan(by["nan-tail-slot"].keys[960:]).all() and not np.isnan(by["nan-tail-slot"].keys[:960]).any()
    c = by["inf-3-70"]
    assert [S.reference(c.keys, p) for p in (2, 929, 930)][0::2] == [-math.inf, math.inf]
    assert math.isfinite(S.reference(c.keys, 3)) and math.isfinite(S.reference(c.keys, 929))
    assert S.reference(by["inf-one-finite"].keys, 333) == -2.75
    k = by["consecutive-from-tiny"].keys
    assert k[0] == S.TINY and k[-1] == n * S.TINY and np.all(np.diff(k.view(np.int64)) == 1)
    k = by["consecutive-straddle"].keys
    assert k[0] == -500 * S.TINY and k[500] == 0.0 and k[-1] == 499 * S.TINY
    k = by["consecutive-straddle-2zeros"].keys
    assert np.signbit(k[500]) and k[500] == 0.0 and not np.signbit(k[501]) and k[501] == 0.0
    assert by["subnormal-range"].keys.max() < 2.0 ** -1022 and by["subnormal-range"].keys.min() > 0
    assert set(by["tiny-over-zero"].keys) == {0.0, S.TINY}
    with np.errstate(over="ignore"):
        assert np.isinf(by["huge-range"].keys.max() - by["huge-range"].keys.min())   # hi - lo overflows
    k = by["ladder80"].keys
    assert np.count_nonzero(k == 0.0) == n - 80 and k[n - 80] == 2.0 ** -1000 and k[-1] == 2.0 ** (-1000 + 8 * 79)
    assert np.all(k[n - 79:] / k[n - 80:-1] == 256.0)
    k = by["low-byte"].keys.view(np.int64)
    assert len(set(k >> 8)) == 1 and len(set(k & 255)) == 256
    k = by["low-byte-unique-top"].keys.view(np.int64)
    assert np.count_nonzero(k == k.max()) == 1
    k = by["random-patterns"].keys
    assert np.isnan(k).any() and np.isinf(k).any() and (k < 0).any() and (k > 0).any()
    # the crowded cases' extra arrangements: the crowd in the fewest lanes / the fewest slots
    pl = {c.name: c for c in S.placed(by["ladder80"])}
    lanes, slots = pl["ladder80/lanes"].keys, pl["ladder80/slots"].keys
    assert np.all(slots[:920] == 0.0) and np.all(slots[920:] > 0.0)
    # n = 1000: lanes 0-39 hold 16 slots, lanes 40-63 hold 15; 920 = 40 * 16 + 18 * 15 + 10
    assert len(set(np.flatnonzero(lanes == 0.0) % 64)) == 59 and len(set(np.flatnonzero(slots == 0.0) % 64)) == 64
    b65 = {c.name: c for c in S.placed(by["bin65"])}["bin65/lanes"].keys
    assert len(set(np.flatnonzero((b65 >= 100) & (b65 < 101)) % 64)) == 5   # 65 keys, 16 slots a lane at n = 1000


def test_round_cap_history():
    """The loop before the fix (by-value rounds unless 128 / h overflows, 80 rounds): a ladder of 79
    rungs above more than 64 zeros is selected in 79 rounds, one of 80 or more returns NaN where
    sort(keys)[99] is 0.0 -- the defect the round-cap fix removed."""
    for j, want in ((79, 0.0), (80, math.nan), (81, math.nan), (200, math.nan)):
        k = S.ladder_keys(2000, j)
        assert S.reference(k, 99) == 0.0
        got, rounds = S.emulate_wave_select(k, 99, value_rounds=None, cap=80)
        assert S.same(got, want) and rounds == min(j, 80), (j, got, rounds)


def test_by_key_worst_case_uses_the_whole_round_budget():
    """ladder-bykey8 loses exactly 8 bits of the key range a round: four by-value rounds, eight by-key
    rounds and the all-equal return in round 13, the last the cap allows.  ladder-bykey7 is the same
    for a by-key map that kept 7 bits a round: such a map runs out of rounds on it (NaN), so the
    GPU test of this case fails for a shift of bits - 7 in the by-key map."""
    for n in NS:
        k = S.key_ladder_keys(n, 8)
        pos = int(np.count_nonzero(k == 2.0 ** -1022)) // 2
        assert S.emulate_wave_select(k, pos, value_rounds=4, cap=13) == (2.0 ** -1022, 12)
        k = S.key_ladder_keys(n, 7)
        assert S.emulate_wave_select(k, pos, value_rounds=4, cap=13)[0] == 2.0 ** -1022
        got, rounds = S.emulate_wave_select(k, pos, value_rounds=4, cap=13, key_bits=7)
        assert math.isnan(got) and rounds == 13


@pytest.mark.parametrize("n", NS)
def test_fixed_round_loop_selects_every_family(cases, n):
    """The loop now (by-key binning from round 4 on, 13 rounds): exact on every case, and no case
    comes near the cap."""
    worst = 0
    for f in S.FAMILIES:
        for c in cases[f, n]:
            for p in c.pos:
                got, rounds = S.emulate_wave_select(c.keys, p, value_rounds=4, cap=13)
                assert S.same(got, S.reference(c.keys, p)), (f, c.name, p, got)
                worst = max(worst, rounds)
    assert worst <= 13


def test_diag_select_argument_checks():
    """dcor_diag_select validates before any device access; an empty batch is DCOR_OK."""
    from dcor import _lib
    D = C.POINTER(C.c_double)
    k = np.zeros(4096)
    out = np.zeros(4)
    pk, po = k.ctypes.data_as(D), out.ctypes.data_as(D)
    f = _lib.lib.dcor_diag_select
    assert f(None, 10, 1, 0, 0, po) == _lib.DCOR_EINVAL
    assert f(pk, 10, 1, 0, 0, None) == _lib.DCOR_EINVAL
    for which in range(6):
        top = S.max_keys(which)
        assert f(pk, 0, 1, 0, which, po) == _lib.DCOR_EINVAL
        assert f(pk, top + 1, 1, 0, which, po) == _lib.DCOR_EINVAL
        assert f(pk, top, -1, 0, which, po) == _lib.DCOR_EINVAL
        assert f(pk, top, 0, 0, which, po) == _lib.DCOR_OK
    for which in (-1, 6):
        assert f(pk, 10, 1, 0, which, po) == _lib.DCOR_EINVAL
