"""The segment cursor (csrc/dcor_segtab.h) through every segment-table entry reachable from Python:
a table of many short segments, so a work unit's stride steps across several of them, then one
long segment it stays in.  Consecutive replicate ranges of one key are one long segment by the
entries' contract, so the reference is one single-segment call per key (and column pair), its rows
gathered by out_row; compared as uint64, all equal."""
import os
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "distributed-correlation_amd", "csrc")
# the table's record count: a prime not of the form 2^k +- 1, so the binary search's halves are
# uneven at every depth; NKEPT - 1 short segments and the long final one
NKEPT = 601
assert all(NKEPT % d for d in range(2, 25)) and all(abs(NKEPT - 2**k) != 1 for k in range(1, 12))


def _define(name, file):
    with open(os.path.join(CSRC, file)) as fh:
        return int(re.search(rf"^#define {name} (\d+)\s*$", fh.read(), re.M).group(1))


def _min_items():
    """Items of a call that exceed every entry's persistent grid at least four times.  A CU holds
    2048 threads, so 8 workgroups of DCOR_BLOCK = 256 threads (the sign and sub-G kernels) or 4 of
    DICT_NT = 512 (the HRS kernels): no grid is larger than 8 x multi_processor_count."""
    import torch
    assert _define("DCOR_BLOCK", "dcor_device.h") == 256 and _define("DICT_NT", "dcor_premat.hip") == 512
    return 4 * 8 * torch.cuda.get_device_properties(0).multi_processor_count


def _plan(nkeys):
    """[(key, rep offset within the key, reps)] in call order and the replicates per key: the short
    segments hold 1, 2, 3, 1, ... replicates and take the keys in turn, every third one is followed
    by a segment without replicates (the planner drops it from the table), the last one is long."""
    plan, used = [], [0] * nkeys
    for j in range(NKEPT - 1):
        key, reps = j % nkeys, 1 + j % 3
        plan.append((key, used[key], reps))
        used[key] += reps
        if j % 3 == 0:
            plan.append(((j + 1) % nkeys, used[(j + 1) % nkeys], 0))
    last = _min_items() - sum(used) + 37
    plan.append((nkeys - 1, used[nkeys - 1], last))
    used[nkeys - 1] += last
    assert sum(1 for _, _, c in plan if c > 0) == NKEPT and sum(used) >= _min_items()
    return plan, used


def _check(nkeys, run, segment, rep_begin):
    """run(segs) of the whole plan against one single-segment run(...) per key.  segment(key,
    rep_begin, reps): the entry's tuple; rep_begin[key]: the key's first replicate."""
    plan, used = _plan(nkeys)
    got = run([segment(key, rep_begin[key] + off, reps) for key, off, reps in plan])
    ref = [run([segment(key, rep_begin[key], used[key])]) for key in range(nkeys)]
    want = np.concatenate([ref[key][off:off + reps] for key, off, reps in plan])   # out_row order
    assert got.shape == want.shape == (sum(used), 6)
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))


def _panel(n, seed):
    g = np.random.default_rng(seed)
    x = g.standard_normal(n)
    return x, 0.5 * x + np.sqrt(0.75) * g.standard_normal(n)


# two (eps1, eps2, seed) keys: m = 8 and m = 2 at n = 64, seeds on either side of 2^32
EPS_KEYS = [(1.0, 1.0, 77), (2.0, 2.0, (5 << 32) + 9)]
REP_BEGIN = [0, 1001]


def test_sign_panel():
    from dcor import signpanel
    X, Y = _panel(64, 3)
    _check(2, lambda segs: signpanel.sweep_segments(X, Y, segs),
           lambda key, rb, reps: (*EPS_KEYS[key], rb, reps), REP_BEGIN)


def test_subg_panel():
    from dcor import subgpanel
    X, Y = _panel(64, 4)
    _check(2, lambda segs: subgpanel.sweep_segments(X, Y, segs),
           lambda key, rb, reps: (*EPS_KEYS[key], rb, reps), REP_BEGIN)


def test_sign_table():
    """Four keys: two column pairs x two (eps, seed) keys."""
    from dcor import signpanel
    D = signpanel.standin_table(64, 3, 0.5, seed=17)
    pairs = [(0, 1), (2, 0)]
    _check(4, lambda segs: signpanel.table_segments(D, segs),
           lambda key, rb, reps: (*pairs[key // 2], *EPS_KEYS[key % 2], rb, reps), REP_BEGIN * 2)


def _hrs_standin(n):
    from dcor import hrs
    age, bmi = hrs.standin_panel(n, -0.3, seed=5)
    z = hrs.standardize_panel(age, bmi, lap=np.array([0.3, -0.2, 0.1, 0.4]))
    return z["age_z"], z["bmi_z"], z["lambda_age_z"], z["lambda_bmi_z"]


def _hrs_continuous(n):
    x, y = _panel(n, 1)
    return x, -y, 2.2, 2.6


@pytest.mark.parametrize("panel", [_hrs_standin, _hrs_continuous], ids=["coded", "uncoded"])
def test_hrs_fused_sweep(panel):
    """The keys are the sweep's own per eps index: m = 2 (eps 2.0) and m = 8 (eps 1.05) at n = 1001."""
    from dcor import hrs
    args, grid = panel(1001), (2.0, 1.05)
    _check(2, lambda segs: hrs.sweep_segments(*args, grid, segs, mode="fused"),
           lambda key, rb, reps: (key, rb, reps), REP_BEGIN)


def test_hrs_table():
    """Four keys: two column pairs (one continuous, one on a coarse grid) x two (eps, seeds) keys."""
    from dcor import hrs, signpanel
    n = 1001
    x, y = _panel(n, 23)
    T = signpanel.standin_table(n, 2, 0.5, seed=23)
    Z = np.asfortranarray(np.stack([x, -y, T[:, 0], T[:, 1]], axis=1))
    lam = np.array([2.2, 2.6, 1.9, 2.4])
    pairs = [(0, 1), (3, 2)]
    keys = [(2.0, 2**33 + 1010, 2**34 + 1020), (1.05, 17, 18)]
    _check(4, lambda segs: hrs.table_segments(Z, lam, segs),
           lambda key, rb, reps: (*pairs[key // 2], *keys[key % 2], rb, reps), REP_BEGIN * 2)
