"""GPU tests of the HRS replicate kernels at the top of their 16-bit index range.  Every HRS kernel
keeps a replicate's batch indices as uint16 in LDS, so n (or a pair's complete-case count n_ab) is
admitted up to 65,536; the other GPU tests stop at 19,433 (fused, sweep), 30,001 (premat), 1,001
(table, pairwise) and 20,000 (R's sample.int walk).  Between those sizes and 65,536 lie the dynamic
LDS above the 64-KB default, index 65,535 itself, the premat route's kernel switch at n < 65,536,
k_hrs_pair_pack's second and later trips (16,384 rows each), the Feistel split's change at 32,769
and the two 16-bit chunks R_unif_index takes once ceil(log2 n) reaches 16.

Three yardsticks, never the code under test:
  1. the CPU oracle's estimators fed the oracle's own restatement of the Philox streams, within
     helpers.assert_close (1e-12 relative, 1e-13 floor);
  2. bit equality with the panel entry hrs_replicates(mode='fused'), which yardstick 1 anchors in
     this module at these sizes, on the same or the host-compacted columns;
  3. exact integer equality with the oracle's restatement of R's sample.int.
Every geometry the cases rely on (k, m, each mask's n_ab, which n run the tiled kernel, R's bits,
"the permutation holds 65,535") is asserted on the CPU, at import or at the top of its test."""
import numpy as np
import pytest

from helpers import assert_close

pytestmark = pytest.mark.gpu

SN, SI, RB = 1010, 1020, 40     # the single-eps entry's keys and first replicate
SENTINEL = -7.25

# (n, eps) -> (k, m): eps = 2 gives m = 2 (k m = n, or n - 1 for odd n; k = 32,767 is odd, so the
# m == 2 loop's 2q + 1 < k tail runs), 0.25 gives m = 128, 0.55 m = 27, 1.05 m = 8
GEO = {(32768, 2.0): (16384, 2), (32769, 2.0): (16384, 2), (65535, 2.0): (32767, 2), (65536, 2.0): (32768, 2),
       (32768, 0.25): (256, 128), (32769, 0.25): (256, 128), (65535, 0.25): (511, 128), (65536, 0.25): (512, 128),
       (65535, 0.55): (2427, 27), (65536, 0.55): (2427, 27), (65536, 1.05): (8192, 8),
       (65532, 2.0): (32766, 2), (65533, 2.0): (32766, 2), (65534, 2.0): (32767, 2)}
# bits = ceil(log2 n): the Feistel domain (split 7 + 8 up to 32,768, 8 + 8 from 32,769) and the
# number of 16-bit chunks R_unif_index takes per candidate (one up to 15 bits, two at 16)
BITS = {32768: 15, 32769: 16, 65535: 16, 65536: 16}
PREMAT_N = (65532, 65533, 65534, 65535, 65536)
TILED_N = (65532, 65533)        # m == 2, k even, n < 65,536; the others run the L2-gather kernel


def _tiled(n):
    k, m = GEO[(n, 2.0)]
    return m == 2 and k % 2 == 0 and k >= 2 and n < 65536


def _check_geometry():
    from dcor import api
    for (n, eps), km in GEO.items():
        assert api.batch_geometry(n, eps, eps, "subG", hrs=True) == km, (n, eps)
    for n, b in BITS.items():
        assert (n - 1).bit_length() == b
    assert tuple(n for n in PREMAT_N if _tiled(n)) == TILED_N
    # the sweep's three segments fill the whole 65,536-entry index row
    assert all(GEO[(65536, e)][0] * GEO[(65536, e)][1] == 65536 for e in (0.25, 2.0, 1.05))


_check_geometry()

_WORST = {}


def _close(path, got, want, what):
    """assert_close, after recording and printing the largest relative error of the path."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    err = float(np.max(np.abs(got - want) / np.maximum(1e-300, np.maximum(np.abs(got), np.abs(want)))))
    _WORST[path] = max(_WORST.get(path, 0.0), err)
    print(f"[index ceiling] {path}: {what}: max rel err {err:.3e} (worst so far {_WORST[path]:.3e})")
    assert_close(got, want, what=what)


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


_PANELS = {}


def _panel_z(kind, n, seed=1):
    """'continuous': test_gpu_hrs._continuous (no dictionary: the L2-gather kernels); 'coded': the
    stand-in panel of test_hrs_fused_equals_premat (at most 256 distinct values per column)."""
    key = (kind, n, seed)
    if key not in _PANELS:
        if kind == "continuous":
            from test_gpu_hrs import _continuous
            z = _continuous(n, seed=seed)
            assert len(np.unique(z["age_z"])) == n and len(np.unique(z["bmi_z"])) == n
        else:
            from dcor import hrs
            age, bmi = hrs.standin_panel(n, -0.3, seed=5)
            z = hrs.standardize_panel(age, bmi, lap=np.array([0.3, -0.2, 0.1, 0.4]))
            assert len(z["age_z"]) == n
            assert len(np.unique(z["age_z"])) <= 256 and len(np.unique(z["bmi_z"])) <= 256
        for v in z.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _PANELS[key] = z
    return _PANELS[key]


def _args(z):
    return (z["age_z"], z["bmi_z"], z["lambda_age_z"], z["lambda_bmi_z"])


def _fused(z, eps, reps, rb=RB, sn=SN, si=SI):
    from dcor import hrs
    return hrs.hrs_replicates(*_args(z), eps, reps, seed_ni=sn, seed_int=si, rep_begin=rb, mode="fused")


_ORACLE = {}


def _oracle(kind, z, eps, rep, seed=1):
    """Yardstick 1: oracle.ni_subg / int_subg (hrs = 1) of replicate `rep` under the keys SN / SI, fed
    the oracle's own Philox restatement; computed once per case and left unchanged."""
    from dcor import api, hrs
    from oracle import oracle as orc
    n = len(z["age_z"])
    key = (kind, n, seed, eps, rep)
    if key not in _ORACLE:
        k, m = GEO[(n, eps)]
        delta = 1.0 / n
        lam_r = api.lambda_receiver_from_noise(z["lambda_age_z"], z["lambda_bmi_z"], eps, delta)
        st, ni, km = orc.ni_subg(z["age_z"], z["bmi_z"], eps, eps, hrs=1, lam_x=z["lambda_age_z"],
                                 lam_y=z["lambda_bmi_z"], perm=orc.perm(SN, 8, rep, n, k * m),
                                 lap_x=orc.gen_laplace(SN, rep, hrs.SITE_NI_LAP_X, k),
                                 lap_y=orc.gen_laplace(SN, rep, hrs.SITE_NI_LAP_Y, k))
        st2, it, _ = orc.int_subg(z["age_z"], z["bmi_z"], eps, eps, hrs=1, lam_s=z["lambda_age_z"],
                                  lam_o=z["lambda_bmi_z"], lam_r=lam_r, delta=delta,
                                  lap_local=orc.gen_laplace(SI, rep, hrs.SITE_INT_LOCAL, n),
                                  lap_central=orc.gen_laplace(SI, rep, hrs.SITE_INT_CENTRAL, 1)[0],
                                  mix_z=orc.gen_normals(SI, rep, hrs.SITE_MIX_Z, 2000),
                                  mix_l=orc.gen_laplace(SI, rep, hrs.SITE_MIX_L, 2000))
        assert st == 0 and st2 == 0 and list(km) == [k, m]
        _ORACLE[key] = np.concatenate([ni, it])
        _ORACLE[key].setflags(write=False)
    return _ORACLE[key]


def _assert_last_index_is_drawn(reps):
    """n = 65,536 at eps = 2: k m = n, so the batch indices of every replicate are a full permutation
    of [0, 65536) and hold 65,535 -- the case cannot pass without reading the last uint16 value."""
    from oracle import oracle as orc
    for rep in reps:
        p = orc.perm(SN, 8, rep, 65536, 65536)
        assert np.array_equal(np.sort(p), np.arange(65536)) and 65535 in p, rep


# ------------------------------------------------ 1. fused panel entry (k_hrs_fused_l2, k_hrs_fused)
@pytest.mark.parametrize("eps", [2.0, 0.25])
@pytest.mark.parametrize("n", [32768, 32769, 65535, 65536])
def test_fused_continuous_panel_matches_oracle(n, eps):
    """k_hrs_fused_l2: 1,280 + 2 k m bytes of dynamic LDS (132 KB at k m = 65,536, above the 64-KB
    default), the Feistel split on either side of 32,769, the odd-k tail of the m == 2 loop at 65,535;
    at 65,536 the four-waves-per-SIMD instantiation returns the same bits."""
    from dcor import _lib
    reps = 3
    if (n, eps) == (65536, 2.0):
        _assert_last_index_is_drawn(range(RB, RB + reps))
    z = _panel_z("continuous", n)
    fu = _fused(z, eps, reps)
    for r in range(reps):
        _close("k_hrs_fused_l2", fu[r], _oracle("continuous", z, eps, RB + r),
               f"fused continuous n={n} eps={eps} rep {RB + r}")
    if n == 65536:
        with _lib.variants(DCOR_HRS_WPE="4"):
            w4 = _fused(z, eps, reps)
        assert np.array_equal(_bits(w4), _bits(fu))


@pytest.mark.parametrize("eps", [2.0, 0.55])
@pytest.mark.parametrize("n", [65535, 65536])
def test_fused_coded_panel_matches_oracle(n, eps):
    """k_hrs_fused: 137 KB of dynamic LDS (dictionaries, reduction buffers, 2 n bytes of codes) and a
    k m scratch row of codes; at 65,536 the uncoded kernel on the same panel returns the same bits."""
    from dcor import _lib
    reps = 3
    if (n, eps) == (65536, 2.0):
        _assert_last_index_is_drawn(range(RB, RB + reps))
    z = _panel_z("coded", n)
    fu = _fused(z, eps, reps)
    for r in range(reps):
        _close("k_hrs_fused", fu[r], _oracle("coded", z, eps, RB + r), f"fused coded n={n} eps={eps} rep {RB + r}")
    if n == 65536:
        with _lib.variants(DCOR_HRS_FUSED_L2="1"):
            l2 = _fused(z, eps, reps)
        assert np.array_equal(_bits(l2), _bits(fu))


# ------------------------------------------------ 2. fused eps sweep (k_hrs_sweep_fused(_l2))
@pytest.mark.parametrize("kind", ["continuous", "coded"])
def test_fused_sweep_segments_equal_the_single_eps_entry_bitwise(kind):
    """One dcor_hrs_fused_sweep_launch, n = 65,536, eps = 0.25, 2.0, 1.05 (m = 128, 2, 8; every
    segment's k m is the whole 65,536-entry row), 2 replicates each from replicate 40: each segment
    bit-equal to the single-eps entry under the segment's keys (segment 0's are test 1's)."""
    from dcor import hrs
    n, grid, reps = 65536, (0.25, 2.0, 1.05), 2
    z = _panel_z(kind, n)
    got = hrs.sweep_segments(*_args(z), grid, [(e, RB, reps) for e in range(len(grid))], mode="fused")
    assert got.shape == (len(grid) * reps, 6) and np.isfinite(got).all()
    for e, eps in enumerate(grid):
        want = _fused(z, eps, reps, sn=10 + 1000 * (e + 1), si=20 + 1000 * (e + 1))
        assert np.array_equal(_bits(got[e * reps:(e + 1) * reps]), _bits(want)), (kind, eps)
    # segment 0 runs under test 1's keys: anchored to the oracle directly as well
    for r in range(reps):
        _close(f"k_hrs_sweep_fused{'_l2' if kind == 'continuous' else ''}", got[r],
               _oracle(kind, z, 0.25, RB + r), f"sweep {kind} n={n} eps=0.25 rep {RB + r}")


# ------------------------------------------------ 3. premat route across its kernel switch
@pytest.mark.parametrize("n", PREMAT_N)
def test_premat_route_across_the_kernel_switch(n):
    """hrs_replicates' default mode on a continuous panel at eps = 2: 65,532 and 65,533 (the odd one on
    the head-sample path) are the largest sizes of the tiled kernel, 65,534 and 65,535 have an odd k
    and 65,536 fails the n < 65,536 clause (the tiled kernel's 'no sample' mark is index 65,535), so
    those three run the L2-gather kernel.  The records are pinned on both sides of the switch; the
    choice itself shows in them only where the two kernels' compensated sums round differently, which
    they rarely do ('Next')."""
    from dcor import _lib, hrs
    eps, reps = 2.0, 2
    assert _tiled(n) == (n in TILED_N)
    z = _panel_z("continuous", n, seed=n)
    run = lambda: hrs.hrs_replicates(*_args(z), eps, reps, seed_ni=SN, seed_int=SI, rep_begin=RB)
    pm = run()
    fu = _fused(z, eps, reps)
    assert np.isfinite(pm).all()
    for r in range(reps):
        _close("premat vs fused", pm[r], fu[r], f"premat vs fused n={n} rep {RB + r}")
    if n in (65533, 65536):
        for r in range(reps):
            _close("premat tiled" if _tiled(n) else "premat L2-gather", pm[r],
                   _oracle("continuous", z, eps, RB + r, seed=n), f"premat n={n} rep {RB + r}")
    with _lib.variants(DCOR_TILED="0"):
        l2 = run()
    if _tiled(n):
        with _lib.variants(DCOR_TILED_VARIANT="0"):
            v0 = run()
        assert np.array_equal(_bits(v0), _bits(l2)), "512-thread tiled kernel vs L2-gather kernel"
        for r in range(reps):
            _close("premat tiled vs L2-gather", pm[r], l2[r], f"default vs L2 kernel n={n} rep {RB + r}")
    else:
        assert np.array_equal(_bits(pm), _bits(l2)), "the tiled kernel must not have been chosen"


# ------------------------------------------------ 4. table entry (k_hrs_table_prep, k_hrs_table)
TABLE_LAM = np.array([2.2, 2.6, 1.9])
TABLE_PAIRS = [(0, 1), (1, 0), (0, 2), (1, 1)]


def _table3(n):
    """Columns 0-1 continuous, column 2 of dcor.signpanel.standin_table (a coarse grid)."""
    from dcor import signpanel
    g = np.random.default_rng(23 + n)
    x = g.standard_normal(n)
    y = -0.3 * x + np.sqrt(1 - 0.09) * g.standard_normal(n)
    t = signpanel.standin_table(n, 4, 0.5, seed=23)[:, 2]
    assert len(np.unique(t)) <= 256 and len(np.unique(x)) == n and len(np.unique(y)) == n
    return np.asfortranarray(np.stack([x, y, t], axis=1))


@pytest.mark.parametrize("n", [65535, 65536])
def test_table_segments_equal_the_panel_entry_bitwise(n):
    """p = 3, columns at odd 8-B offsets (ld = n + 3), (a, b), (b, a), a mixed pair and (a, a) at m = 128
    and m = 2, keys above 2^32, one segment on the last replicate range the entry admits with two
    replicates (rep_begin = 2^32 - 3): every segment bit-equal to the panel entry on its two columns,
    unnamed rows untouched."""
    from test_gpu_hrs_table import _launch, _panel
    reps = 2
    Z = _table3(n)
    cells = [(a, b, e) for a, b in TABLE_PAIRS for e in (0.25, 2.0)]
    order = np.random.default_rng(4).permutation(len(cells))
    rbs = [RB, 2**32 - 3, 1001]
    segs = [(a, b, e, 2**33 + 1010 + 7 * j, 2**34 + 1020 + 11 * j, rbs[j % 3], reps, (reps + 1) * int(order[j]))
            for j, (a, b, e) in enumerate(cells)]
    assert any(s[5] == 2**32 - 3 and s[2] == 2.0 for s in segs)
    rows = (reps + 1) * len(segs)
    got = _launch(Z, TABLE_LAM, segs, rows, ld=n + 3)
    named = np.zeros(rows, dtype=bool)
    for seg in segs:
        sl = slice(seg[7], seg[7] + reps)
        named[sl] = True
        want = _panel(Z, TABLE_LAM, seg)
        assert np.isfinite(want).all()
        assert np.array_equal(_bits(got[sl]), _bits(want)), seg
    assert named.sum() == reps * len(segs) and np.all(got[~named] == SENTINEL)


# ------------------------------------------------ 5. pairwise entry: k_hrs_pair_pack over several trips
PAIR_N = 70000                   # 1,094 mask words: four full trips of 256 words and one of 70
TRIP = 16384                     # rows per trip
PAIR_LAM = np.array([2.2, 2.6, 1.9])


def _big_masks():
    """name -> (bool [PAIR_N] for column 1, its count); column 0 is complete."""
    n, i = PAIR_N, np.arange(PAIR_N)
    seams = np.ones(n, dtype=bool)
    seams[[16383, 16384, 32767, 32768, 49151, 49152, 65535, 65536]] = False
    seams[65544:] = False
    one_per_trip = np.zeros(n, dtype=bool)
    one_per_trip[[5, TRIP + 100, 3 * TRIP - 1, 3 * TRIP, n - 1]] = True
    m = {"cap": (i < 65536, 65536),                                  # the last rank is 65,535
         "cap-1": ((i >= 1) & (i < 65536), 65535),                   # odd: the zero pad at dst[65535]
         "seams": (seams, 65536),                                    # both rows of every trip seam
         "empty-trip": (((i < TRIP) | (i >= 2 * TRIP)) & (i < 69000), 52616),   # a trip total of 0
         "first-trip-empty": (i >= TRIP, 53616),
         "last-words-only": (i >= 65536, 4464),                      # every full trip is empty
         "two-rows-seam": ((i == TRIP - 1) | (i == TRIP), 2),
         "two-rows-ends": ((i == 0) | (i == n - 1), 2),
         "one-per-trip": (one_per_trip, 5),
         "random-half": (np.random.default_rng(77).random(n) >= 0.5, 34947)}
    return m


def _check_pair_geometry():
    from dcor import api
    assert (PAIR_N + 63) // 64 == 4 * 256 + 70
    for name, (mask, count) in _big_masks().items():
        assert int(mask.sum()) == count and 2 <= count <= 65536, (name, int(mask.sum()))
    assert sorted(np.flatnonzero(_big_masks()["one-per-trip"][0]) // TRIP) == [0, 1, 2, 3, 4]
    geo = lambda nab: [api.batch_geometry(nab, e, e, "subG", hrs=True) for e in (2.0, 0.25)]
    assert geo(2) == [(2, 1), (2, 1)] and geo(5) == [(2, 2), (2, 2)]          # the k < 2 guard
    assert geo(65536) == [(32768, 2), (512, 128)] and geo(65535) == [(32767, 2), (511, 128)]
    assert geo(4464) == [(2232, 2), (34, 128)] and geo(34947) == [(17473, 2), (273, 128)]
    for nn, words in ((16384, 256), (16385, 257), (16448, 257)):
        assert (nn + 63) // 64 == words


_check_pair_geometry()


def _pair_table(n):
    from test_gpu_hrs_pairwise import _table
    return _table(n)


def _check_pairs(Z, lam, V, pairs, eps_list, ld, what):
    """One pairwise call over pairs x eps_list, 2 replicates each with one unnamed row after each block:
    every segment bit-equal to the panel entry on the host-compacted columns."""
    from test_gpu_hrs_pairwise import REP_BEGIN, _launch, _panel
    reps = 2
    cells = [(a, b, e) for a, b in pairs for e in eps_list]
    segs = [(a, b, e, 2**33 + 5 + j, 2**34 + 9 + j, REP_BEGIN[j % 3], reps, (reps + 1) * (len(cells) - 1 - j))
            for j, (a, b, e) in enumerate(cells)]
    rows = (reps + 1) * len(segs)
    got = _launch(Z, lam, V, segs, rows, ld=ld)
    for seg in segs:
        want = _panel(Z, lam, V, seg)
        assert np.isfinite(want).all(), (what, seg)
        assert np.array_equal(_bits(got[seg[7]:seg[7] + reps]), _bits(want)), (what, seg[:3])
        assert np.all(got[seg[7] + reps] == SENTINEL)


@pytest.mark.parametrize("name", ["cap", "cap-1", "seams", "empty-trip", "first-trip-empty", "last-words-only",
                                  "two-rows-seam", "two-rows-ends", "one-per-trip", "random-half"])
def test_pair_pack_over_several_trips_equals_the_panel_entry_bitwise(name):
    """n = 70,000, column 0 complete, the mask on column 1, missing rows NaN; the pair and the reversed
    pair at eps = 2.0 and 0.25.  The running base across trips, a trip whose total is 0, the partial
    last trip, ranks up to 65,535 and the pad element after an odd count."""
    n = PAIR_N
    mask, count = _big_masks()[name]
    Z = _pair_table(n)[:, :2]
    V = np.stack([np.ones(n, dtype=bool), mask])
    assert int((V[0] & V[1]).sum()) == count
    _check_pairs(Z, PAIR_LAM[:2], V, [(0, 1), (1, 0)], (2.0, 0.25), n + 1, name)


@pytest.mark.parametrize("n", [16384, 16385, 16448])
def test_pair_pack_trip_edges_in_the_word_count(n):
    """Exactly 256 mask words (one trip), 256 words and one row, 257 words: every other row present, and
    every row."""
    Z = _pair_table(n)[:, :2]
    i = np.arange(n)
    for what, m1 in (("alternate", i % 2 == 0), ("full", np.ones(n, dtype=bool))):
        V = np.stack([np.ones(n, dtype=bool), m1])
        _check_pairs(Z, PAIR_LAM[:2], V, [(0, 1)], (2.0, 0.25), n + 1, (n, what))


def test_pair_full_masks_equal_the_table_entry_bitwise():
    """n = 40,000 (three trips), every mask bit set: the table entry's records byte for byte, with the
    bits past n in the last word set or clear."""
    from test_gpu_hrs_pairwise import LAM, _launch
    from test_gpu_hrs_table import _launch as table_launch
    n, reps = 40000, 2
    Z = _pair_table(n)
    cells = [(a, b, e) for a, b in ((0, 1), (2, 3), (1, 1)) for e in (2.0, 0.25)]
    segs = [(a, b, e, 2**33 + 1010 + 7 * j, 2**34 + 1020 + 11 * j, RB + j, reps, (reps + 1) * j)
            for j, (a, b, e) in enumerate(cells)]
    rows = (reps + 1) * len(segs)
    want = table_launch(Z, LAM, segs, rows, ld=n + 3)
    assert np.isfinite(want[want != SENTINEL]).all() and (want != SENTINEL).any(axis=1).sum() == reps * len(segs)
    full = np.ones((4, n), dtype=bool)
    assert np.array_equal(_bits(_launch(Z, LAM, full, segs, rows, ld=n + 3, delta=1.0 / n, junk=True)), _bits(want))
    assert np.array_equal(_bits(_launch(Z, LAM, full, segs, rows, ld=n, junk=False)), _bits(want))


def test_pair_slots_at_different_offsets_in_one_call():
    """p = 3, column 1 with 'cap-1' and column 2 with 'random-half': three slots of 65,535, 35,084 and
    32,859 rows, whose panels start at different 16-element offsets of one buffer."""
    n = PAIR_N
    masks = _big_masks()
    V = np.stack([np.ones(n, dtype=bool), masks["cap-1"][0], masks["random-half"][0]])
    counts = [int((V[a] & V[b]).sum()) for a, b in ((0, 1), (0, 2), (1, 2))]
    assert counts == [65535, 34947, 32762]
    _check_pairs(_pair_table(n)[:, :3], PAIR_LAM, V, [(0, 1), (0, 2), (1, 2)], (2.0,), n + 1, "slots")


# ------------------------------------------------ 6. R's sample.int with 16-bit `bits`
@pytest.mark.parametrize("n,k,m", [(32768, 16384, 2), (32769, 16384, 2), (65535, 32767, 2), (65536, 32768, 2),
                                   (65536, 512, 128)])
def test_r_sample_int_walk_with_two_chunks_per_candidate(n, k, m):
    """dcor_rstream_hrs_draws' permutation rows against the oracle's restatement of R's sample.int:
    from n = 32,769 on bits = ceil(log2 n) is 16 and R_unif_index takes two 16-bit chunks per
    candidate until the remaining count falls to 32,768."""
    import ctypes as C

    import torch
    from dcor import _lib
    from oracle import oracle as orc
    assert GEO[(n, 2.0 if m == 2 else 0.25)] == (k, m) and k * m <= n
    assert (n - 1).bit_length() == BITS[n] and (BITS[n] == 16) == (n > 32768)
    seeds = np.array([1, 42, 123], dtype=np.int32)
    runs = len(seeds)
    perm = torch.full((runs, k * m), -1, dtype=torch.int32, device="cuda")
    lx = torch.empty((runs, k), dtype=torch.float64, device="cuda")
    ly = torch.empty_like(lx)
    P = lambda t: C.c_void_p(t.data_ptr())
    _lib.check(_lib.lib.dcor_rstream_hrs_draws(n, k, m, 2000, runs, seeds.ctypes.data_as(C.POINTER(C.c_int32)),
                                               None, P(perm), P(lx), P(ly), None, None, None, None, None))
    got = perm.cpu().numpy()
    for r in range(runs):
        assert len(np.unique(got[r])) == k * m and got[r].min() >= 0 and got[r].max() < n
        np.testing.assert_array_equal(got[r], orc.rs_sample_int(int(seeds[r]), n, k * m))


def test_r_stream_replicates_at_the_ceiling_match_oracle():
    """rng='R' at n = 65,536, eps = 2 on the coded panel (the pre-materialised coded kernel with 137 KB
    of LDS codes): every draw bit-exact against the CPU restatement of R's streams, the estimates
    within the estimator tolerance."""
    from dcor import hrs
    from oracle import oracle as orc
    n, eps, idx, R, rb = 65536, 2.0, 18, 2, 6
    z = _panel_z("coded", n)
    k, m = GEO[(n, eps)]
    res, noise, geo = hrs.hrs_replicates(*_args(z), eps, R, rep_begin=rb, keep_noise=True, rng="R", eps_idx=idx)
    assert (geo["k"], geo["m"]) == (k, m)
    sn, si = hrs.r_seeds(idx, R, rb)
    for r in range(R):
        perm, lx, ly = orc.rs_hrs_ni_draws(int(sn[r]), n, k, m)
        assert np.array_equal(np.sort(perm), np.arange(n))
        np.testing.assert_array_equal(noise["perm"][r], perm)
        np.testing.assert_array_equal(noise["lap_x"][r], lx)
        np.testing.assert_array_equal(noise["lap_y"][r], ly)
        ll, lc, mz, ml = orc.rs_hrs_int_draws(int(si[r]), n, 2000)
        np.testing.assert_array_equal(noise["lap_local"][r], ll)
        assert noise["lap_central"][r] == lc
        np.testing.assert_array_equal(noise["mix_z"][r], mz)
        np.testing.assert_array_equal(noise["mix_l"][r], ml)
        st, ni, _ = orc.ni_subg(z["age_z"], z["bmi_z"], eps, eps, hrs=1, lam_x=z["lambda_age_z"],
                                lam_y=z["lambda_bmi_z"], perm=perm, lap_x=lx, lap_y=ly)
        st2, it, _ = orc.int_subg(z["age_z"], z["bmi_z"], eps, eps, hrs=1, lam_s=z["lambda_age_z"],
                                  lam_o=z["lambda_bmi_z"], lam_r=geo["lam_r"], delta=geo["delta"],
                                  lap_local=ll, lap_central=lc, mix_z=mz, mix_l=ml)
        assert st == 0 and st2 == 0
        _close("premat coded, R streams", res[r], np.concatenate([ni, it]), f"R-stream hrs n={n} run {rb + r + 1}")
