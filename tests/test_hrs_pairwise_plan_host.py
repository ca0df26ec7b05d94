"""plan_hrs_table_pairwise (csrc/dcor_plan.cpp) checked by a stand-alone program: tests/host/
hrs_pairwise_plan_check.cpp and dcor_plan.cpp alone, compiled with g++ and no HIP include path.  The
pairs' counts n_ab against a per-row loop, the slots and their panels, every segment record against
the record plan_hrs_fused_sweep builds for a panel of n_ab samples, every rejection (see the
program).  The program is built and run a second time under AddressSanitizer and
UndefinedBehaviorSanitizer where the host compiler links such a program; no sanitizer touches code
loaded into Python."""
import os
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "distributed-correlation_amd", "csrc")
SOURCES = [os.path.join(ROOT, "tests", "host", "hrs_pairwise_plan_check.cpp"), os.path.join(CSRC, "dcor_plan.cpp")]
FLAGS = ["-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-I" + CSRC]
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def _build_and_run(d, extra):
    exe = os.path.join(d, "hrs_pairwise_plan_check")
    subprocess.run(["g++"] + FLAGS + extra + ["-o", exe] + SOURCES, check=True)
    return subprocess.run([exe], capture_output=True, text=True)


def test_hrs_pairwise_plan_check_builds_without_hip_and_passes():
    with tempfile.TemporaryDirectory() as d:
        r = _build_and_run(d, [])
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == "hrs_pairwise_plan_check: ok"


def _sanitizers_link():
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "t.cpp")
        with open(src, "w") as fh:
            fh.write("int main() { return 0; }\n")
        r = subprocess.run(["g++"] + SAN + ["-o", os.path.join(d, "t"), src], capture_output=True)
        return r.returncode == 0


def test_hrs_pairwise_plan_check_under_sanitizers():
    if not _sanitizers_link():
        pytest.skip("the host compiler does not link -fsanitize=address,undefined programs")
    with tempfile.TemporaryDirectory() as d:
        r = _build_and_run(d, SAN)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == "hrs_pairwise_plan_check: ok" and r.stderr.strip() == ""
