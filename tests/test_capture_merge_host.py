"""Grouped launches of the capture-overlap planner (aqlm_amd/csrc/capture_overlap.h) on the CPU: tests/capture_merge_host.cpp is
compiled as a stand-alone program with the address and undefined-behaviour sanitizers and run; nothing is loaded into this process.

And the ISA of the grouped kernel: the fill wait of its four instances counts the loads behind the last LDS-DMA, the property
tests/test_isa_invariants.py holds the single-layer kernels to (its pattern does not match the new names)."""
import os
import re
import shutil
import subprocess

import pytest

from tests import test_isa_invariants as isa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ["alternating shapes", "window of one", "hazards, keys and broken runs", "random sequences"]


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    if cxx is None and os.path.exists("/opt/rocm/llvm/bin/clang++"):
        cxx = "/opt/rocm/llvm/bin/clang++"
    assert cxx, "no C++ compiler found"
    exe = str(tmp_path_factory.mktemp("capture_merge") / "capture_merge_host")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tests", "capture_merge_host.cpp"), "-o", exe],
                   check=True, capture_output=True, text=True)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(run.stdout, run.stderr)
    assert run.returncode == 0, run.stdout + run.stderr
    return run.stdout


@pytest.mark.parametrize("case", CASES)
def test_planner_case(report, case):
    assert f"{case}: ok" in report.splitlines()


@pytest.mark.skipif(not os.path.exists(isa.HIPCC), reason="hipcc not available")
def test_group_kernel_fill_wait_counts_the_loads_behind_the_last_lds_dma(tmp_path):
    out = tmp_path / "gemv_packed.s"
    subprocess.run([isa.HIPCC] + isa.FLAGS + [os.path.join(ROOT, "aqlm_amd", "csrc", "gemv_packed.hip"), "-o", str(out)], check=True,
                   stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=600)
    # check_asm as it stands, on the grouped kernels only: their labels are rewritten to a name its pattern takes
    text, found = re.subn(r"(?m)^(_ZN4aqlm\w+gemv_1x16_packed)_group(_kernel\w+):", r"\1\2:", out.read_text())
    kept, name = [], None
    for line in text.split("\n"):
        m = re.match(r"^(_Z\w+):", line)
        if m:
            name = m.group(1)
        if name is not None and "PackedGroupParams" in name:
            kept.append(line)
    n, bad = isa.check_asm("\n".join(kept))
    assert found == 4 and n == 4, f"{found} grouped kernels in the ISA, {n} fill waits checked"
    assert not bad, f"fill wait does not match the loads issued behind the LDS-DMA: {bad}"
