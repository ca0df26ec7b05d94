"""Generate tests/golden/mc_oracle_stats.json: the statistics of tests/mc_stats.compare for the
seven grid cells and the n = 1e4 headline cell, computed from the CPU restatements of both
engines (oracle.sim_reps for the Philox side, oracle.rs_sim for the R-stream side) at B = 10,000:
recorded numbers only.  The R side takes 3-7 s per cell
on one thread, too long to recompute inside the GPU suite, so tests/test_gpu_mc.py compares the
engine's statistics with these recorded numbers, and tests/test_mc_oracle.py checks that they are
still what the restatements give (for the seven grid cells; the n = 1e4 cell takes 25 s).

Run: python tests/golden/make_mc_oracle_stats.py --write     (without --write: print only)
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [os.path.dirname(HERE), ROOT, os.path.join(ROOT, "distributed-correlation_amd")]

import mc_stats as S  # noqa: E402
from oracle import oracle  # noqa: E402


def main():
    threads = min(16, os.cpu_count() or 1)
    cells = {}
    for name, cell in {**S.GRID_CELLS, **S.GPU_ONLY_CELLS}.items():
        res = S.compare(oracle.sim_reps(cell.to_c(), 0, S.B, threads), oracle.rs_sim(cell.to_c(), S.B),
                        cell.rho)
        cells[name] = {"stats": res["stats"], "na": res["na"], "cover": res["cover"]}
        print(name)
        print(S.describe(res))
    text = json.dumps({"B": S.B, "cells": cells}, indent=1) + "\n"
    if "--write" in sys.argv[1:]:
        with open(os.path.join(HERE, "mc_oracle_stats.json"), "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
