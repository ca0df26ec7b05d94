"""CPU checks of the fused sub-G edge-case table (subg_fused_cases.py): whether the GPU tests of
test_gpu_subg_fused_edges.py can fail at all.  Every case sits on the batch geometry and kernel form
it names, the table covers what it claims (every DGP in both kernel forms, eta (.5, 2) and (2, .5)
in both forms and under both senders), and the oracle's records of the replicates the GPU test
compares are informative: a CI bound clamped to -1 or +1 says nothing about se, sd or the order
statistic, so outside the named degenerate cases some replicate has both NI bounds, and some
replicate both INT bounds, strictly inside (-1, 1).  That is a condition on the inputs, not a
tolerance."""
import os
import re

import numpy as np
import pytest

import subg_fused_cases as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the issue's table (n, (eps1, eps2)); n = 20000 at eps (.5, .5) moved up to n = 64000 (see the table)
TABLE_ROWS = [(16384, (1, 1)), (16385, (1, 1)), (63, (4, 2)), (64, (4, 2)), (65, (4, 2)), (193, (2, 1.5)),
              (512, (1, 1)), (520, (1, 1)), (527, (1, 1)), (3001, (1.5, 0.5)), (3001, (0.5, 1.5)),
              (15, (1, 1)), (7, (1, 1)), (16385, (0.1, 0.1)), (204800, (0.1, 0.1)), (205605, (0.1, 0.1)),
              (64000, (0.5, 0.5))]


@pytest.fixture(scope="module")
def dc():
    import dcor
    return dcor


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle
    return oracle


def test_table_rows_present():
    have = {(c.n, c.eps) for c in T.CASES}
    for n, eps in TABLE_ROWS:
        assert (n, tuple(float(e) for e in eps)) in have, (n, eps)
    assert len(set(T.CASE_IDS)) == len(T.CASES)


def test_kernel_form_threshold_is_the_engine_headers():
    txt = open(os.path.join(ROOT, "distributed-correlation_amd", "csrc", "dcor_engine.h")).read()
    assert int(re.search(r"#define\s+SUBG_W_NMAX\s+(\d+)", txt).group(1)) == T.SUBG_W_NMAX
    ns = {c.n for c in T.CASES}
    assert T.SUBG_W_NMAX in ns and T.SUBG_W_NMAX + 1 in ns


@pytest.mark.parametrize("case", T.CASES, ids=T.CASE_IDS)
def test_case_geometry(dc, case):
    T.assert_geometry(case, dc.api.batch_geometry)
    assert case.k * case.m + case.tail == case.n and 0 <= case.tail < case.m
    assert case.k >= 1 and case.m <= case.n


def test_geometry_edges_covered():
    by = {c.id: c for c in T.CASES}
    wave = [c for c in T.CASES if c.form == "wave"]
    wg = [c for c in T.CASES if c.form == "wg"]
    assert {c.k for c in wave} >= {1, 63, 64, 65}                     # idle lane, full wave, lane wrap
    assert {c.k for c in wg} >= {20, 256, 257}                        # idle threads, full, thread wrap
    assert any(c.m == 1 for c in wave)                                # the pair loop never runs
    for form in (wave, wg):
        assert any(c.m % 2 == 1 and c.m > 1 and c.tail > 0 for c in form)      # pair loop + remainder + tail
        assert any(c.m & (c.m - 1) == 0 and c.m > 1 and c.tail == 0 for c in form)   # m = 2^e, no tail
        assert any(c.m & (c.m - 1) != 0 for c in form)                # sx / md instead of sx * inv_md
    assert by["n7-m-clipped"].m == by["n7-m-clipped"].n               # m clipped to n
    assert any(c.tail > T.WG_THREADS for c in wg)                     # the tail loop past one trip


def test_dgp_eta_sender_coverage():
    forms = ("wave", "wg")
    for form in forms:
        cases = [c for c in T.CASES if c.form == form]
        assert {c.spec["dgp"] for c in cases} == {"gaussian", "bernoulli", "bounded_factor", "mix_gaussian"}
        g = [c.spec for c in cases if c.spec["dgp"] == "gaussian"]
        assert any(all(m != 0 for m in s["mu"]) and all(v != 1 for v in s["sigma"]) for s in g)
        assert any(c.spec["rho"] > 0 for c in cases if c.spec["dgp"] == "bounded_factor")
        mix = [c.spec["pi_mix"] for c in cases if c.spec["dgp"] == "mix_gaussian"]
        assert any((p * 2 ** 20) % 1 != 0 for p in mix)               # a pi_mix that is no dyadic fraction
        for eta in ((0.5, 2.0), (2.0, 0.5)):
            for sender in ("X", "Y"):
                assert any(T.eta_of(c) == eta and T.sender_of(c) == sender for c in cases), (form, eta, sender)
    # eta1 != eta2 only tests the roles if it gives lambda1 != lambda2: 2 eta sqrt(log n) below the
    # cap 2 sqrt 3 on the eta = .5 side
    for c in T.CASES:
        if T.eta_of(c) in ((0.5, 2.0), (2.0, 0.5)):
            assert 2 * 0.5 * np.sqrt(np.log(c.n)) < 2 * np.sqrt(3.0), c.id


@pytest.mark.parametrize("case", T.CASES, ids=T.CASE_IDS)
def test_oracle_records_are_informative(orc, case):
    ref = orc.sim_reps(T.cell_of(case).to_c(), T.REP_BEGIN, T.REP_BEGIN + T.REPS)
    assert ref.shape == (T.REPS, 6)
    if case.k == 1:   # sd(T) of one batch is NA (ver-cor-subG.R:56): NI bounds NaN, everything else finite
        assert case.id in T.DEGENERATE
        assert np.all(np.isnan(ref[:, 1:3])) and np.all(np.isfinite(ref[:, [0, 3, 4, 5]]))
    else:
        assert np.all(np.isfinite(ref)), ref
    ni, it = T.unclamped(ref, 1, 2), T.unclamped(ref, 4, 5)
    print(f"{case.id}: k={case.k} m={case.m} tail={case.tail} {case.form}: replicates with both NI bounds "
          f"inside (-1, 1): {int(ni.sum())}/{T.REPS}, both INT bounds: {int(it.sum())}/{T.REPS}")
    if case.id not in T.DEGENERATE:
        assert ni.any(), f"{case.id}: every replicate has an NI bound clamped\n{ref}"
        assert it.any(), f"{case.id}: every replicate has an INT bound clamped\n{ref}"


def test_degenerate_list():
    assert len(T.DEGENERATE) <= 5
    by = {c.id: c for c in T.CASES}
    for cid, why in T.DEGENERATE.items():
        assert why and (by[cid].k == 1 or by[cid].n <= 65), cid
    assert {c.id for c in T.CASES if c.k == 1} <= set(T.DEGENERATE)


@pytest.mark.parametrize("form", ["wave", "wg"])
def test_key_count_cells(dc, orc, form):
    """The key-count runs: the cell is in the form it names, alpha reaches the first and the last
    order statistic, and the oracle's INT bounds are unclamped in every replicate of every run (the
    width is the order statistic times se_norm / sqrt(n))."""
    kw = T.KEY_CELLS[form]
    assert T.form_of(kw["n"]) == form and (kw["eps1"], kw["eps2"]) == (1.0, 1.0)
    assert {n for n, a in T.KEY_RUNS if a == 0.05} == {1, 2, 3, 1023, 1024, 1025, 2047, 2048}
    for nsim in (3, 1025, 2048):
        assert any(n == nsim and T.mix_pos(n, a) == 0 for n, a in T.KEY_ALPHA_EDGES)
        assert any(n == nsim and T.mix_pos(n, a) == n - 1 for n, a in T.KEY_ALPHA_EDGES)
    width = {}
    for nsim, alpha in T.KEY_RUNS:
        assert 0 <= T.mix_pos(nsim, alpha) < nsim
        ref = orc.sim_reps(dc.CellSpec(nsim=nsim, alpha=alpha, **kw).to_c(), 0, T.KEY_REPS)
        assert np.all(np.isfinite(ref)) and T.unclamped(ref, 4, 5).all(), (form, nsim, alpha, ref)
        width[nsim, alpha] = (ref[:, 5] - ref[:, 4]).tobytes()
    # the guards and positions are visible in the records: one, two and three keys give different
    # widths in some replicate, and so do the positions that alpha selects among the same keys
    for group in ([(1, 0.05), (2, 0.05), (3, 0.05), (3, 1.999)], [(1025, 0.05), (1025, 1.999), (1025, 1e-6)],
                  [(2048, 0.05), (2048, 1.999), (2048, 1.9995), (2048, 1e-6)], [(2047, 0.05), (2048, 1e-6)]):
        assert len({width[g] for g in group}) == len(group), group
    with pytest.raises(RuntimeError):
        orc.sim_reps(dc.CellSpec(nsim=2049, **kw).to_c(), 0, 1)
