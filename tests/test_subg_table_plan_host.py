"""plan_subg_table and SubgTableLayout (csrc/dcor_plan.cpp, csrc/dcor_engine.h) checked by a
stand-alone program: tests/host/subg_table_plan_check.cpp and dcor_plan.cpp alone, compiled with g++
and no HIP include path.  Every kept record equals, as bytes over its SubgSegConst part, the record
plan_subg_panel builds for the segment's reference call, the slot list is the segments' distinct m in
order of first use, the clips are make_subg's l1 / l2 bits, the layout's regions do not overlap, an
overflowing p * npad is refused and the checks come in the header's order (see the program).  The
program is built and run a second time under AddressSanitizer and UndefinedBehaviorSanitizer where
the host compiler links such a program; no sanitizer touches code loaded into Python."""
import os
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "distributed-correlation_amd", "csrc")
SOURCES = [os.path.join(ROOT, "tests", "host", "subg_table_plan_check.cpp"), os.path.join(CSRC, "dcor_plan.cpp")]
FLAGS = ["-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-I" + CSRC]
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
OK = "subg_table_plan_check: ok"


def _build_and_run(d, extra):
    exe = os.path.join(d, "subg_table_plan_check")
    subprocess.run(["g++"] + FLAGS + extra + ["-o", exe] + SOURCES, check=True)
    return subprocess.run([exe], capture_output=True, text=True)


def test_subg_table_plan_check_builds_without_hip_and_passes():
    with tempfile.TemporaryDirectory() as d:
        r = _build_and_run(d, [])
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == OK


def _sanitizers_link():
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "t.cpp")
        with open(src, "w") as fh:
            fh.write("int main() { return 0; }\n")
        r = subprocess.run(["g++"] + SAN + ["-o", os.path.join(d, "t"), src], capture_output=True)
        return r.returncode == 0


def test_subg_table_plan_check_under_sanitizers():
    if not _sanitizers_link():
        pytest.skip("the host compiler does not link -fsanitize=address,undefined programs")
    with tempfile.TemporaryDirectory() as d:
        r = _build_and_run(d, SAN)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == OK and r.stderr.strip() == ""
