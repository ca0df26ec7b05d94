"""The fused sub-G engine (subg_fused_core, csrc/dcor_fused.hip) against the CPU oracle at the edges
of its kernel forms and batch geometry: the cases of subg_fused_cases.py (test_subg_fused_cases.py
shows on the CPU that each sits on its edge and that the oracle's records there are informative).

Through k_subg_fused_w<DGP, 16|32> and k_subg_fused (dcor_sim_launch) and k_grid_subg_w<DGP, 16|32>
and k_grid_subg (the batched grid).  Bar: the suite's standing one (helpers.assert_close: 1e-12
relative, 1e-13 floor, as test_gpu_parity), NaN positions equal; launch-shape properties (split,
offset, entry point, rows past the range) bit for bit."""
import ctypes as C

import numpy as np
import pytest

import subg_fused_cases as T
from helpers import assert_close

pytestmark = pytest.mark.gpu

SENTINEL = -12345.6789


@pytest.fixture(scope="module")
def dc():
    import torch
    assert torch.cuda.is_available()
    import dcor
    return dcor


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle
    return oracle


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _vs_oracle(got, ref, what):
    assert np.array_equal(np.isnan(got), np.isnan(ref)), f"{what}: NaN positions\n got {got!r}\n ref {ref!r}"
    assert_close(got, ref, what=what)


def _case(cid):
    return T.CASES[T.CASE_IDS.index(cid)]


# one cell per kernel form for the launch-shape tests: odd m with a tail and the sender on the Y side
# (wave), m = 8 with a one-sample tail and eta1 != eta2 (workgroup)
FORM_CASE = {"wave": "n3001-senderY", "wg": "n16385-first-wg"}


# ------------------------------------------------------------------ geometry
@pytest.mark.parametrize("case", T.CASES, ids=T.CASE_IDS)
def test_subg_fused_geometry_vs_oracle(dc, orc, case):
    from dcor.sim import simulate
    T.assert_geometry(case, dc.api.batch_geometry)
    cell = T.cell_of(case)
    got = simulate(cell, T.REPS, rep_begin=T.REP_BEGIN).cpu().numpy()
    ref = orc.sim_reps(cell.to_c(), T.REP_BEGIN, T.REP_BEGIN + T.REPS)
    if case.k == 1:
        assert np.all(np.isnan(ref[:, 1:3])) and np.all(np.isfinite(ref[:, [0, 3, 4, 5]]))
    _vs_oracle(got, ref, f"{case.id} (k={case.k}, m={case.m}, tail={case.tail}, {case.form}): {case.why}")


# ---------------------------------------------------------------- key counts
@pytest.mark.parametrize("nsim,alpha", T.KEY_RUNS)
@pytest.mark.parametrize("form", ["wave", "wg"])
def test_subg_fused_key_counts_vs_oracle(dc, orc, form, nsim, alpha):
    """The kernels draw their own mixquant keys: odd key counts and nsim = 1 (the guards 2b < nsim and
    2b + 1 < nsim, the NaN padding of unused slots), both selector widths, the first and the last
    order statistic."""
    from dcor.sim import CellSpec, simulate
    pos = T.mix_pos(nsim, alpha)
    if alpha == 1e-6:
        assert pos == nsim - 1
    if (nsim, alpha) in ((3, 1.999), (1025, 1.999), (2048, 1.9995)):
        assert pos == 0
    cell = CellSpec(nsim=nsim, alpha=alpha, **T.KEY_CELLS[form])
    assert T.form_of(cell.n) == form
    got = simulate(cell, T.KEY_REPS).cpu().numpy()
    ref = orc.sim_reps(cell.to_c(), 0, T.KEY_REPS)
    assert np.all(np.isfinite(ref)) and T.unclamped(ref, 4, 5).all(), ref
    _vs_oracle(got, ref, f"{form} nsim={nsim} alpha={alpha} pos={pos}")


@pytest.mark.parametrize("form", ["wave", "wg"])
def test_subg_fused_key_count_over_2048_refused(dc, orc, form):
    from dcor.sim import CellSpec, simulate
    cell = CellSpec(nsim=2049, **T.KEY_CELLS[form])
    with pytest.raises(dc.DcorError) as e:
        simulate(cell, 1)
    assert e.value.code == dc._lib.DCOR_EINVAL
    with pytest.raises(RuntimeError):
        orc.sim_reps(cell.to_c(), 0, 1)


# ------------------------------------------------------- the whole-wave guard
PARTIAL_CELLS = {"wave-nsim1000": ("n527-k65-tail7", 1000), "wave-nsim2000": ("n3001-senderX", 2000),
                 "wg": ("n16385-first-wg", 1000)}


@pytest.mark.parametrize("reps", [1, 3, 4, 5])
@pytest.mark.parametrize("which", list(PARTIAL_CELLS))
def test_subg_fused_partial_wave_leaves_next_row(dc, which, reps):
    """dcor_sim_launch writes rows [0, reps) and nothing after them: the wave kernels' last workgroup
    holds waves past the range when reps is no multiple of four."""
    import torch
    from dcor import _lib
    from dcor.sim import simulate
    cid, nsim = PARTIAL_CELLS[which]
    cell = T.cell_of(_case(cid), nsim=nsim)
    assert T.form_of(cell.n) == which.split("-")[0]
    buf = torch.full((reps + 2, 6), SENTINEL, dtype=torch.float64, device="cuda")
    c = cell.to_c()
    _lib.check(_lib.lib.dcor_sim_launch(C.byref(c), 3, reps, C.c_void_p(buf.data_ptr()),
                                        C.c_void_p(int(torch.cuda.current_stream().cuda_stream))))
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    want = simulate(cell, reps, rep_begin=3).cpu().numpy()
    assert np.array_equal(_bits(got[reps:]), _bits(np.full((2, 6), SENTINEL))), got[reps:]
    assert np.array_equal(_bits(got[:reps]), _bits(want))
    assert not np.any(_bits(want) == _bits(np.array(SENTINEL)))


# ------------------------------------------------- split and offset invariance
@pytest.mark.parametrize("form", ["wave", "wg"])
def test_subg_fused_split_and_offset_invariance(dc, form):
    from dcor.sim import simulate
    cell = T.cell_of(_case(FORM_CASE[form]))
    whole = simulate(cell, 11).cpu().numpy()
    parts = np.concatenate([simulate(cell, 4, 0).cpu().numpy(), simulate(cell, 7, 4).cpu().numpy()])
    assert np.array_equal(_bits(whole), _bits(parts))
    for r in range(11):
        alone = simulate(cell, 1, r).cpu().numpy()
        assert np.array_equal(_bits(alone[0]), _bits(whole[r])), r
    assert len({whole[r].tobytes() for r in range(11)}) == 11


# --------------------------------------------- the top of the replicate counter
@pytest.mark.parametrize("form", ["wave", "wg"])
def test_subg_fused_top_of_replicate_counter(dc, orc, form):
    """The last replicate range dcor_sim_launch accepts ([2^32 - 1 - reps, 2^32 - 1): the range check
    of test_abi.py) against the oracle on the same range; the next range is refused."""
    import torch
    from dcor import _lib
    from dcor.sim import simulate
    reps = 5
    top = 0xffffffff - reps
    cell = T.cell_of(_case(FORM_CASE[form]))
    got = simulate(cell, reps, rep_begin=top).cpu().numpy()
    ref = orc.sim_reps(cell.to_c(), top, top + reps)
    assert np.all(np.isfinite(ref))
    _vs_oracle(got, ref, f"{form} rep_begin={top:#x}")
    # not the records of the range's low 31 bits
    low = simulate(cell, reps, rep_begin=top & 0x7fffffff).cpu().numpy()
    assert not np.any(_bits(low)[:, [0, 3]] == _bits(got)[:, [0, 3]])
    buf = torch.full((reps, 6), SENTINEL, dtype=torch.float64, device="cuda")
    c = cell.to_c()
    st = _lib.lib.dcor_sim_launch(C.byref(c), top + 1, reps, C.c_void_p(buf.data_ptr()),
                                  C.c_void_p(int(torch.cuda.current_stream().cuda_stream)))
    assert st == _lib.DCOR_EINVAL
    torch.cuda.synchronize()
    assert np.array_equal(_bits(buf.cpu().numpy()), _bits(np.full((reps, 6), SENTINEL)))


# ------------------------------------------------------------------ the grid
# wave and workgroup cells, nsim <= 1024 and > 1024, all four DGPs in both forms: several
# (kind, dgp, vpl32) groups in one call (the two n of about 2e5 left out)
GRID_CELLS = [("n16384-last-wave", 1000), ("n63-m1", 1000), ("n64-m1", 2000), ("n65-m1", 1025),
              ("n193-m3", 2048), ("n527-k65-tail7", 1000), ("n3001-senderY", 1024), ("n15-k1", 3),
              ("n16377-senderX-eta2-.5", 2000), ("n512-k64", 1500), ("n16385-first-wg", 1000),
              ("n16385-m800", 2000), ("n20003-senderY-eta.5-2", 1000), ("n16399-wg-bernoulli", 1025)]


def test_subg_grid_equals_single_launches(dc):
    """One batched grid call (k_grid_subg_w<DGP, 16|32>, k_grid_subg) gives each cell the records of
    its own dcor_sim_launch bit for bit; B = 13 leaves a partial last wave group."""
    from dcor.sim import run_grid, simulate
    B = 13
    cells = [T.cell_of(_case(cid), nsim=nsim) for cid, nsim in GRID_CELLS]
    for form in ("wave", "wg"):
        sub = [c for c in cells if T.form_of(c.n) == form]
        assert {c.dgp for c in sub} == {"gaussian", "bernoulli", "bounded_factor", "mix_gaussian"}
        assert any(c.nsim <= 1024 for c in sub) and any(c.nsim > 1024 for c in sub)
    res = run_grid(cells, B, detail=True, devices=[0])
    for (cid, nsim), cell, r in zip(GRID_CELLS, cells, res):
        single = simulate(cell, B).cpu().numpy()
        assert np.array_equal(_bits(r["records"]), _bits(single)), (cid, nsim)
