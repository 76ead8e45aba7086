"""The chain-prefetch hint (aqlm_amd/csrc/chain_hint.h) on the CPU: tests/chain_hint_host.cpp walks the requests the prefetch waves of
aqlm_hip_gemv_1x16_packed_chain make for the next layer's entry stream -- waves 1..16, steps 1..40, 3- and 4-byte entries,
relabelled or not, 1..7 prefetch waves, every workgroup -- against the rule the entry calls, as a stand-alone program built with the
address and undefined-behaviour sanitizers and run; nothing is loaded into this process.

Whenever the hint is kept, the last byte requested lies inside the buffer's used_bytes; it is dropped only where a request would
leave the buffer (3-byte entries that end the buffer, at a stream size that is no whole number of KiB) and for variable geometry.
Keeping every hint, the rule before the header existed, is shown to fail the same walk."""
import ctypes
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ["entry bytes 3 relabelled 0", "entry bytes 3 relabelled 1", "entry bytes 4 relabelled 0", "entry bytes 4 relabelled 1", "edges"]


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    if cxx is None and os.path.exists("/opt/rocm/llvm/bin/clang++"):
        cxx = "/opt/rocm/llvm/bin/clang++"
    assert cxx, "no C++ compiler found"
    exe = str(tmp_path_factory.mktemp("chain_hint") / "chain_hint_host")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tests", "chain_hint_host.cpp"), "-o", exe],
                   check=True, capture_output=True, text=True)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(run.stdout[-4000:], run.stderr[-4000:])
    assert run.returncode == 0, run.stdout[-4000:] + run.stderr[-4000:]
    return run.stdout


@pytest.mark.parametrize("case", CASES)
def test_hint_case(report, case):
    assert f"{case}: ok" in report.splitlines()


# The entry itself, through its report aqlm_hip_gemv_1x16_packed_chain_plan (no GPU: descriptors are built from the numpy model's
# layout, as tests/test_compact_window_host.py builds them, and read on the host).
@pytest.fixture(scope="module")
def native():
    from aqlm_amd import _native

    return _native


def desc(native, fout, fin, waves, steps, entry_bytes=4, groups=None, relabel=False, absmax=1.5):
    from tests import packed_model as pm

    lay = pm.layout(fout, fin // 8, waves, steps, entry_bytes, groups, relabel)
    flags = (native.PACKED_VARGEOM if groups else 0) | ((native.PACKED_RELABELLED | native.PACKED_HAS_CODEBOOK) if relabel else 0)
    return native.PackedDesc(pm.MAGIC, pm.VERSION, fout, fin, 4, waves, steps, entry_bytes, lay["used"], 1, absmax, flags, lay["RG"],
                             (ctypes.c_uint8 * 32)(*(groups or [16] * 16)))


@pytest.fixture
def keys(native):
    names = ("packed_prefetch_waves", "packed_fused_finalize")
    old = [native.get_tuning(k) for k in names]
    yield
    for k, v in zip(names, old):
        native.set_tuning(k, v)


def test_the_entry_keeps_and_drops_the_hint_as_the_rule_says(native, keys):
    A = desc(native, 512, 1024, 4, 1)
    for waves in (1, 4, 11, 16):
        for steps in (1, 3, 8, 32):
            bb3 = waves * steps * 776
            for eb, relabel, kept in ((4, False, True), (4, True, True), (3, True, True), (3, False, bb3 % 1024 == 0)):
                got = native.packed_chain_plan(A, desc(native, 512, 1024, waves, steps, eb, None, relabel))
                assert got[:2] == (kept, 2 if kept else 0), (waves, steps, eb, relabel, got)
    assert native.packed_chain_plan(A, desc(native, 512, 1024, 16, 8, 3))[0]          # 97 KiB per block: whole requests
    assert not native.packed_chain_plan(A, desc(native, 512, 1024, 4, 1, 3))[0]       # 3104 bytes per block, 992 over
    vg = desc(native, 512, 2048, 4, 2, groups=[17, 15] + [16] * 14)
    assert native.packed_chain_plan(A, vg)[:2] == (False, 0)                          # a variable-geometry next layer
    assert native.packed_chain_plan(vg, A)[:2] == (False, 0)                          # ... and a variable-geometry launch has no prefetch waves
    assert native.packed_chain_plan(A, None)[:2] == (False, 0)
    assert native.packed_chain_plan(desc(native, 512, 1024, 4, 1, absmax=0.0), A)[:2] == (False, 0)   # no codebook range: two kernels
    native.set_tuning("packed_fused_finalize", 0)
    assert native.packed_chain_plan(A, A)[:2] == (False, 0)


def test_prefetch_waves_are_capped_by_the_key_the_block_and_the_lds(native, keys):
    B = desc(native, 512, 1024, 4, 1)
    for waves in range(1, 17):
        A = desc(native, 512, 1024, waves, 1)
        for rows in (1, 3):
            image = native.packed_image(A, rows)[0]
            for key, want in ((-1, 0), (0, 2), (1, 1), (3, 3), (7, 7), (9, 7)):
                native.set_tuning("packed_prefetch_waves", key)
                n = min(want, 16 - waves)
                assert native.packed_chain_plan(A, B, rows) == (True, n, image + 1024 * n), (waves, rows, key)
    # no room in the LDS: rows whose image leaves less than the 7 KiB of landing zones under 160 KiB lose all prefetch waves
    native.set_tuning("packed_prefetch_waves", 7)
    tight = roomy = 0
    for fout in (512, 4096):
        for fin in range(1024, 20000, 512):
            A, before = desc(native, fout, fin, 4, 4), 0
            for rows in range(1, 9):
                image = native.packed_image(A, rows)[0]
                if image <= before:   # these rows no longer fit one image: the call splits them
                    break
                before = image
                kept, n, lds = native.packed_chain_plan(A, B, rows)
                assert kept and lds <= 160 * 1024
                if image + 7 * 1024 > 160 * 1024:
                    tight += 1
                    assert (n, lds) == (0, image), (fout, fin, rows)
                else:
                    roomy += 1
                    assert (n, lds) == (7, image + 7 * 1024), (fout, fin, rows)
    assert roomy > 0
    assert tight > 0, "no layer of the sweep runs out of LDS"


def test_plan_rejections(native):
    L = native.lib
    A = desc(native, 512, 1024, 4, 1)
    bad = native.PackedDesc.from_ints(A.as_ints())
    bad.used_bytes += 1
    out = ctypes.c_int(0)
    for d, rows, dt, nxt in ((A, 0, native.F16, A), (A, 9, native.F16, A), (A, 1, 7, A), (bad, 1, native.F16, A), (A, 1, native.F16, bad)):
        assert L.aqlm_hip_gemv_1x16_packed_chain_plan(ctypes.byref(d), rows, dt, ctypes.byref(nxt), ctypes.byref(out), None, None) == native.E_INVALID
    assert L.aqlm_hip_gemv_1x16_packed_chain_plan(None, 1, native.F16, None, None, None, None) == native.E_INVALID
    assert L.aqlm_hip_gemv_1x16_packed_chain_plan(ctypes.byref(A), 1, native.F16, ctypes.byref(A), None, None, None) == 0
