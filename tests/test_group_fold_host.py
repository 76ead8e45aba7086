"""Folded grouped launches (aqlm_amd/csrc/group_fold.h) on the CPU: tests/group_fold_host.cpp drives the block -> (segment, slice,
pass -> stream) mapping that the kernel and the launch code share, as a stand-alone program built with the address and
undefined-behaviour sanitizers and run; nothing is loaded into this process.

And the ISA of gemv_1x16_packed_group_fold_kernel: the fill wait of its two instances counts the loads behind the last LDS-DMA,
the property tests/test_isa_invariants.py holds the single-layer kernels to (its pattern does not match the new name); no LDS-DMA
is issued behind that wait, no pass loop drains the entry ring at its barrier, and the instances use no scratch."""
import os
import re
import shutil
import subprocess

import pytest

from tests import test_isa_invariants as isa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ["fold 1", "fold 2", "fold 4", "choose"]


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    if cxx is None and os.path.exists("/opt/rocm/llvm/bin/clang++"):
        cxx = "/opt/rocm/llvm/bin/clang++"
    assert cxx, "no C++ compiler found"
    exe = str(tmp_path_factory.mktemp("group_fold") / "group_fold_host")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tests", "group_fold_host.cpp"), "-o", exe],
                   check=True, capture_output=True, text=True)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(run.stdout, run.stderr)
    assert run.returncode == 0, run.stdout + run.stderr
    return run.stdout


@pytest.mark.parametrize("case", CASES)
def test_mapping_case(report, case):
    assert f"{case}: ok" in report.splitlines()


@pytest.fixture(scope="module")
def fold_kernels(tmp_path_factory):
    """name -> ISA text of the folded instances (gemv_packed.hip compiled once for the module)"""
    out = tmp_path_factory.mktemp("group_fold_isa") / "gemv_packed.s"
    subprocess.run([isa.HIPCC] + isa.FLAGS + [os.path.join(ROOT, "aqlm_amd", "csrc", "gemv_packed.hip"), "-o", str(out)], check=True,
                   stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=600)
    kernels, name = {}, None
    for line in out.read_text().split("\n"):
        m = re.match(r"^(_ZN4aqlm\w+gemv_1x16_packed_group_fold_kernel\w+):", line)
        if m:
            name = m.group(1)
            kernels[name] = []
        if name is not None:
            kernels[name].append(line)
            if line.startswith("; Occupancy"):  # the last line of the compiler's "Kernel info" comment behind the code
                name = None
    return {k: "\n".join(v) for k, v in kernels.items()}


needs_hipcc = pytest.mark.skipif(not os.path.exists(isa.HIPCC), reason="hipcc not available")


@needs_hipcc
def test_fold_kernel_fill_wait_counts_the_loads_behind_the_last_lds_dma(fold_kernels):
    assert len(fold_kernels) == 2, sorted(fold_kernels)
    # check_asm as it stands: the labels are rewritten to a name its pattern takes
    text = re.sub(r"(?m)^(_ZN4aqlm\w+gemv_1x16_packed)_group_fold(_kernel\w+):", r"\1\2:", "\n".join(fold_kernels.values()))
    n, bad = isa.check_asm(text)
    assert n == 2, f"{n} fill waits checked"
    assert not bad, f"fill wait does not match the loads issued behind the LDS-DMA: {bad}"


@needs_hipcc
def test_fold_kernel_keeps_the_ring_in_flight_over_the_pass_barrier(fold_kernels):
    for name, text in fold_kernels.items():
        lines = text.split("\n")
        barriers = [i for i, l in enumerate(lines) if re.search(r"\bs_barrier\b", l)]
        dmas = [i for i, l in enumerate(lines) if "global_load_lds" in l]
        # fill barrier, the barrier behind a pass's loop, the barrier in front of the next pass's loop
        assert len(barriers) == 3, f"{name}: {len(barriers)} barriers"
        assert dmas and max(dmas) < barriers[0], f"{name}: an LDS-DMA behind the fill barrier"
        # the last barrier is the one between epilogue j and loop j + 1: the next pass's ring was requested in front of the
        # epilogue, and the wait that precedes this barrier (for the row starts of the next pass, which are older) must leave
        # the three ring steps in flight
        k = barriers[-1]
        prev_wait = next(l for l in reversed(lines[:k]) if "s_waitcnt" in l)
        vm = re.search(r"vmcnt\((\d+)\)", prev_wait)
        assert vm is None or int(vm.group(1)) >= 3, f"{name}: '{prev_wait.strip()}' in front of the pass barrier drains the ring"
        ring = [i for i, l in enumerate(lines) if re.search(r"\bbuffer_load_dwordx4\b", l) and barriers[1] < i < k]
        assert len(ring) == 3, f"{name}: {len(ring)} ring requests between the loop barrier and the pass barrier"
        scratch = re.search(r"(?m)^; ScratchSize: (\d+)", text)
        assert scratch and int(scratch.group(1)) == 0, f"{name}: scratch in use"
        vgprs = re.search(r"(?m)^; NumVgprs: (\d+)", text)
        # 20 waves on a CU (4096->4096 beside 4096->11008) are 5 per SIMD: 512 registers / 5 waves, in blocks of 8
        assert vgprs and int(vgprs.group(1)) <= 96, f"{name}: {vgprs and vgprs.group(1)} VGPRs cost waves per SIMD at 20 waves per CU"
