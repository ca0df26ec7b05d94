"""GPU test of bench.py's plain run and --dump-outputs: the plain run measures only its timed steps
(no CPU baseline, no live ceilings: those are --full's), and the arrays it dumps are what the last
timed step computed -- simulate() of that step's replicate range and its accumulators finalised."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_plain_run_dumps_last_timed_step(tmp_path):
    from dcor.sim import accum_from_bytes, accumulate, finalize, headline_cell, simulate
    steps, reps, n = 2, 64, 20_000
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps),
                        "--warmup", "1", "--reps", str(reps), "--n", str(n), "--dump-outputs", str(tmp_path)],
                       capture_output=True, text=True, timeout=180, env=env)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout
    d = json.loads(lines[0])
    assert d["steps"] == steps and d["ms_per_step"] > 0
    assert d["value"] == pytest.approx(reps * 1e3 / d["ms_per_step"], rel=1e-9)
    assert "cpu_baseline" not in d and d["roofline"]["issue"] is None    # --full only

    assert sorted(os.listdir(tmp_path)) == ["accum_summary.npy", "records.npy"]
    rec = np.load(tmp_path / "records.npy")
    summ = np.load(tmp_path / "accum_summary.npy")
    assert rec.dtype == np.float64 and rec.shape == (reps, 6)
    assert summ.dtype == np.float64 and summ.shape == (2, 5)
    # the last timed step of one rank covers replicates [(steps - 1) * reps, steps * reps)
    cell = headline_cell(n)
    want = simulate(cell, reps, (steps - 1) * reps)
    assert rec.tobytes() == want.cpu().numpy().tobytes()
    acc = accum_from_bytes(accumulate(want, cell.rho).cpu().numpy().tobytes())
    cols = ("mse", "bias", "var", "coverage", "ci_length")
    assert summ.tobytes() == np.array([[finalize(a, cell.rho)[c] for c in cols] for a in acc]).tobytes()
