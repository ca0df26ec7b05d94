"""The planning unit (csrc/dcor_plan.cpp with dcor_plan.h and dcor_layout.h) is plain C++: each
stand-alone program of tests/host/ and dcor_plan.cpp alone, compiled with g++ and no HIP include
path, link into a program that checks one part of it (the planners' tables, every rejection, the
check order, the scratch layouts; see the programs and tests/host/check.h).  Each is built and run
again under AddressSanitizer and UndefinedBehaviorSanitizer where the host compiler links such a
program; no sanitizer touches code loaded into Python."""
import os
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "distributed-correlation_amd", "csrc")
PROGRAMS = ["plan_check", "hrs_table_plan_check", "hrs_pairwise_plan_check", "subg_panel_plan_check",
            "subg_table_plan_check", "layout_check"]
FLAGS = ["-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-I" + CSRC]
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def test_planning_unit_names_no_hip_header():
    """Neither file, nor a header they include, reads the HIP runtime."""
    seen, todo = set(), [os.path.join(CSRC, "dcor_plan.cpp")]
    while todo:
        path = os.path.normpath(todo.pop())
        if path in seen:
            continue
        seen.add(path)
        for line in open(path):
            line = line.strip()
            if line.startswith("#include"):
                assert "hip" not in line, (path, line)
                if '"' in line:
                    todo.append(os.path.join(os.path.dirname(path), line.split('"')[1]))
    assert {os.path.basename(p) for p in seen} == {"dcor_plan.cpp", "dcor_plan.h", "dcor_engine.h",
                                                   "dcor_layout.h", "dcor.h"}


def _build_and_run(d, prog, extra):
    exe = os.path.join(d, prog)
    subprocess.run(["g++"] + FLAGS + extra + ["-o", exe, os.path.join(ROOT, "tests", "host", prog + ".cpp"),
                                              os.path.join(CSRC, "dcor_plan.cpp")], check=True)
    return subprocess.run([exe], capture_output=True, text=True)


@pytest.mark.parametrize("prog", PROGRAMS)
def test_check_builds_without_hip_and_passes(prog):
    with tempfile.TemporaryDirectory() as d:
        r = _build_and_run(d, prog, [])
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == prog + ": ok"


def _sanitizers_link():
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "t.cpp")
        with open(src, "w") as fh:
            fh.write("int main() { return 0; }\n")
        r = subprocess.run(["g++"] + SAN + ["-o", os.path.join(d, "t"), src], capture_output=True)
        return r.returncode == 0


@pytest.mark.parametrize("prog", PROGRAMS)
def test_check_under_sanitizers(prog):
    if not _sanitizers_link():
        pytest.skip("the host compiler does not link -fsanitize=address,undefined programs")
    with tempfile.TemporaryDirectory() as d:
        r = _build_and_run(d, prog, SAN)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == prog + ": ok" and r.stderr.strip() == ""
