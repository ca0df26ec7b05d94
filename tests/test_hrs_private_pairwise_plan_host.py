"""The private pairwise HRS-table planner (plan_hrs_private_pairwise in csrc/dcor_plan.cpp):
tests/host/hrs_private_pairwise_plan_check.cpp and dcor_plan.cpp alone, compiled with g++ and no HIP
include path, as tests/test_hrs_private_plan_host.py builds the private planner's program; built and
run again under AddressSanitizer and UndefinedBehaviorSanitizer where the host compiler links such a
program.  No sanitizer touches code loaded into Python."""
import os
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "distributed-correlation_amd", "csrc")
PROG = "hrs_private_pairwise_plan_check"
# the engine's own contraction setting: the program compares doubles with ==
FLAGS = ["-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off", "-I" + CSRC]
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def _build_and_run(d, extra):
    exe = os.path.join(d, PROG)
    subprocess.run(["g++"] + FLAGS + extra + ["-o", exe, os.path.join(ROOT, "tests", "host", PROG + ".cpp"),
                                              os.path.join(CSRC, "dcor_plan.cpp")], check=True)
    return subprocess.run([exe], capture_output=True, text=True)


def test_check_builds_without_hip_and_passes():
    with tempfile.TemporaryDirectory() as d:
        r = _build_and_run(d, [])
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == PROG + ": ok"


def _sanitizers_link():
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "t.cpp")
        with open(src, "w") as fh:
            fh.write("int main() { return 0; }\n")
        return subprocess.run(["g++"] + SAN + ["-o", os.path.join(d, "t"), src], capture_output=True).returncode == 0


def test_check_under_sanitizers():
    if not _sanitizers_link():
        pytest.skip("the host compiler does not link -fsanitize=address,undefined programs")
    with tempfile.TemporaryDirectory() as d:
        r = _build_and_run(d, SAN)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == PROG + ": ok" and r.stderr.strip() == ""
