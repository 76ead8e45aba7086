"""Regrouping a run's head in the capture-overlap planner (aqlm_amd/csrc/capture_overlap.h) on the CPU: tests/capture_head_host.cpp
is compiled as a stand-alone program with the address and undefined-behaviour sanitizers and run; nothing is loaded into this
process."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ["alternating head", "no script", "random sequences", "stopped scripts"]


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    if cxx is None and os.path.exists("/opt/rocm/llvm/bin/clang++"):
        cxx = "/opt/rocm/llvm/bin/clang++"
    assert cxx, "no C++ compiler found"
    exe = str(tmp_path_factory.mktemp("capture_head") / "capture_head_host")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tests", "capture_head_host.cpp"), "-o", exe],
                   check=True, capture_output=True, text=True)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(run.stdout, run.stderr)
    assert run.returncode == 0, run.stdout + run.stderr
    return run.stdout


@pytest.mark.parametrize("case", CASES)
def test_planner_case(report, case):
    assert f"{case}: ok" in report.splitlines()
