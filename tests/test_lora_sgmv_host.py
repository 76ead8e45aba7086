"""The segmented LoRA adapter GEMM (aqlm_hip_lora_sgmv), the parts that need no GPU: header, bindings and exports, the supported
shapes and the workspace size, the argument checks (they return before anything touches a device), the route predicates as truth
tables, the resource report of the two kernels (no scratch, no FLAT access, the matrix instruction in both), and the --prefill
mode of tools/lora_benchmark.py."""
import ctypes
import itertools
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
ISA_FLAGS = ["-O3", "-std=c++17", "--offload-arch=gfx950", "-fPIC", "-ffp-contract=fast", "-mllvm",
             "-amdgpu-kernarg-preload-count=14", "--cuda-device-only", "-S"]
MAX_ROWS = 65536


def test_sgmv_symbols_are_declared_bound_and_exported():
    from aqlm_amd import _native as nat

    header = open(os.path.join(ROOT, "include", "aqlm_hip.h")).read()
    declared = set(re.findall(r"\b(aqlm_hip_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S)))
    raw = ctypes.CDLL(nat.LIB_PATH)
    for name in ("aqlm_hip_lora_sgmv", "aqlm_hip_lora_sgmv_supported", "aqlm_hip_lora_sgmv_workspace_bytes"):
        assert name in declared and name in nat.SIGNATURES and hasattr(raw, name), name
    assert nat.lib.aqlm_hip_abi_version() == nat.ABI_VERSION == 9
    assert re.search(rf"#define AQLM_HIP_MAX_LORA_SGMV_ROWS {MAX_ROWS}\b", header)
    assert nat.MAX_LORA_SGMV_ROWS == MAX_ROWS


def test_supported_shapes_and_workspace_size():
    from aqlm_amd import _native as nat

    L = nat.lib
    good = [(300, 520, 24, 70), (1, 8, 8, 1), (298, 1032, 128, MAX_ROWS)]
    bad = [(300, 516, 24, 70), (300, 520, 136, 70), (300, 520, 12, 70), (300, 520, 24, MAX_ROWS + 1)]
    for out, fin, rank, rows in good:
        assert L.aqlm_hip_lora_sgmv_supported(out, fin, rank, rows) == 1, (out, fin, rank, rows)
        n = L.aqlm_hip_lora_sgmv_workspace_bytes(rows, rank, fin)
        assert n >= rows * rank * 4 and n % 16 == 0, (rows, rank, fin, n)
    for out, fin, rank, rows in bad:
        assert L.aqlm_hip_lora_sgmv_supported(out, fin, rank, rows) == 0, (out, fin, rank, rows)
        assert L.aqlm_hip_lora_sgmv_workspace_bytes(rows, rank, fin) == 0, (rows, rank, fin)
    # the size is a function of (rows, max_rank, in_features): out_features is no argument, and the size grows with the rows alone
    # by whole rows -- the cut of the sum over in_features does not depend on the row count
    per_row = L.aqlm_hip_lora_sgmv_workspace_bytes(1, 16, 4096)
    assert per_row >= 16 * 4
    for rows in (2, 17, 96, 4096):
        assert L.aqlm_hip_lora_sgmv_workspace_bytes(rows, 16, 4096) == rows * per_row


def test_argument_checks_return_before_anything_touches_a_device():
    from aqlm_amd import _native as nat

    L = nat.lib
    buf = ctypes.create_string_buffer(1 << 17)
    p = (ctypes.addressof(buf) + 15) // 16 * 16
    need = L.aqlm_hip_lora_sgmv_workspace_bytes(4, 16, 512)
    assert need >= 4 * 16 * 4
    args = lambda **kw: [kw.get(n, d) for n, d in (  # noqa: E731
        ("table", p), ("n", 2), ("max_rank", 16), ("ids", p + 1024), ("i64", 1), ("rows", 4), ("x", p + 4096), ("xs", 512),
        ("y", p + 16384), ("ys", 300), ("out", 300), ("in", 512), ("dt", nat.F16), ("ws", p + 32768), ("ws_bytes", need),
        ("stream", None))]
    call = L.aqlm_hip_lora_sgmv
    for null in ("table", "x", "y", "ws"):
        assert call(*args(**{null: None})) == nat.E_INVALID and "null pointer" in nat.last_error(), null
    assert call(*args(table=p + 4)) == nat.E_INVALID and "misaligned" in nat.last_error()
    assert call(*args(ids=p + 1028)) == nat.E_INVALID and "misaligned" in nat.last_error()
    assert call(*args(ws=p + 32768 + 8)) == nat.E_INVALID and "misaligned" in nat.last_error()
    assert call(*args(y=p + 16385)) == nat.E_INVALID and "misaligned" in nat.last_error()
    assert call(*args(rows=0)) == nat.E_INVALID
    assert call(*args(y=p + 4096)) == nat.E_INVALID and "aliases x" in nat.last_error()          # y == x
    assert call(*args(y=p + 4096 + 512)) == nat.E_INVALID and "aliases x" in nat.last_error()    # y inside x
    assert call(*args(ys=296)) == nat.E_INVALID and "strides" in nat.last_error()
    assert call(*args(xs=504)) == nat.E_INVALID and "strides" in nat.last_error()
    assert call(*args(ws_bytes=need - 4)) == nat.E_INVALID and f"{need} bytes needed" in nat.last_error()
    assert call(*args(dt=7)) == nat.E_UNSUPPORTED and "float16 and bfloat16" in nat.last_error()
    assert call(*args(max_rank=12, ws_bytes=1 << 14)) == nat.E_UNSUPPORTED and "multiple of 8" in nat.last_error()
    assert call(*args(max_rank=136, ws_bytes=1 << 14)) == nat.E_UNSUPPORTED
    assert call(*args(**{"in": 516, "xs": 520})) == nat.E_UNSUPPORTED
    assert call(*args(x=p + 4096 + 8)) == nat.E_UNSUPPORTED and "16-byte aligned" in nat.last_error()
    # (addresses are compared, never followed: y lies past the 1 MiB that 65537 rows of x would span)
    assert call(*args(rows=MAX_ROWS + 1, xs=8, **{"in": 8}, y=p + (1 << 22), ys=8, out=8, ws_bytes=1 << 30)) == nat.E_UNSUPPORTED
    # new here: the expand writes y in 8-byte groups
    assert call(*args(y=p + 16384 + 2)) == nat.E_UNSUPPORTED and "8-byte aligned" in nat.last_error()   # an address % 8 == 2
    assert call(*args(rows=2, ys=302, out=298)) == nat.E_UNSUPPORTED and "8-byte aligned" in nat.last_error()


def test_sgmv_route_predicate_is_a_pure_table(monkeypatch):
    import aqlm.lora as lora

    assert lora.AQLM_HIP_MAX_LORA_SGMV_ROWS == MAX_ROWS
    monkeypatch.setattr(lora, "SGMV_MIN_ROWS", 65)
    monkeypatch.setattr(lora, "SGMV_MAX_ROWS", 4096)
    for cuda, dtype_ok, grad, compiling, supported in itertools.product((False, True), repeat=5):
        for rows in (0, 1, 64, 65, 96, 4096, 4097):
            want = cuda and dtype_ok and not grad and not compiling and supported and 65 <= rows <= 4096
            assert lora.takes_sgmv_route(cuda, dtype_ok, grad, compiling, rows, supported) is want
    monkeypatch.setattr(lora, "SGMV_MAX_ROWS", 0)  # switched off
    assert not any(lora.takes_sgmv_route(True, True, False, False, rows, True) for rows in (1, 64, 65, 96, 4096, MAX_ROWS))
    monkeypatch.setattr(lora, "SGMV_MAX_ROWS", 10 ** 9)  # never beyond what one launch takes
    assert lora.takes_sgmv_route(True, True, False, False, MAX_ROWS, True)
    assert not lora.takes_sgmv_route(True, True, False, False, MAX_ROWS + 1, True)
    assert not lora.takes_sgmv_route(True, True, False, False, 64, True)


def test_shipped_sgmv_limit_is_the_measured_one():
    import json

    import aqlm.lora as lora

    with open(os.path.join(ROOT, "profiles", "lora_sgmv.json")) as f:
        measured = json.load(f)
    counts = [r["rows"] for r in measured["rows"]]
    assert sorted(set(counts)) == [96, 128, 256, 512, 1024, 2048, 4096]
    best = measured["sgmv_max_rows"]
    assert lora.SGMV_MIN_ROWS == 65
    assert lora.SGMV_MAX_ROWS == (MAX_ROWS if best == 4096 else best)


def test_bgmv_route_predicate_is_unchanged(monkeypatch):
    import aqlm.lora as lora

    monkeypatch.setattr(lora, "BGMV_MAX_ROWS", 16)
    monkeypatch.setattr(lora, "SGMV_MAX_ROWS", 4096)  # the new route changes nothing about the old predicate
    for cuda, dtype_ok, grad, compiling, supported in itertools.product((False, True), repeat=5):
        for rows in (0, 1, 16, 17):
            want = cuda and dtype_ok and not grad and not compiling and supported and 1 <= rows <= 16
            assert lora.takes_bgmv_route(cuda, dtype_ok, grad, compiling, rows, supported) is want
    monkeypatch.setattr(lora, "BGMV_MAX_ROWS", 0)
    assert not any(lora.takes_bgmv_route(True, True, False, False, rows, True) for rows in (1, 2, 64))
    monkeypatch.setattr(lora, "BGMV_MAX_ROWS", 10_000)
    assert lora.takes_bgmv_route(True, True, False, False, 256, True)
    assert not lora.takes_bgmv_route(True, True, False, False, 257, True)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_sgmv_kernels_use_the_matrix_unit_no_scratch_and_no_flat_access(tmp_path):
    out = tmp_path / "lora_sgmv.s"
    subprocess.run([HIPCC] + ISA_FLAGS + [os.path.join(ROOT, "aqlm_amd", "csrc", "lora_sgmv.hip"), "-o", str(out)], check=True,
                   stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=900)
    text = out.read_text()
    pattern = r"_ZN4aqlm\d+lora_sgmv_(?:shrink|expand)_kernel\w+"
    names = set(re.findall(rf"^\s+\.name:\s+({pattern})", text, re.M))
    assert len(names) == 4, names  # shrink / expand x fp16 / bf16
    assert sum("shrink" in n for n in names) == 2 and sum("BF16" in n for n in names) == 2
    seen = 0
    for m in re.finditer(rf"\.name:\s+({pattern})(.*?)(?=\n  - |\Z)", text, re.S):
        assert re.search(r"\.private_segment_fixed_size:\s+0\b", m.group(2)), m.group(1)
        seen += 1
    assert seen == 4
    for name in names:
        body = re.split(rf"^{name}:", text, maxsplit=1, flags=re.M)[1].split(".Lfunc_end", 1)[0]
        assert "v_mfma_f32_16x16x32" in body, f"{name}: no 16x16x32 matrix instruction"
        assert not re.search(r"\bflat_(load|store)", body), f"{name}: FLAT access"


def test_benchmark_tool_lists_prefill_and_needs_a_gpu():
    import torch

    tool = os.path.join(ROOT, "tools", "lora_benchmark.py")
    out = subprocess.run([sys.executable, tool, "--help"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "--prefill" in out.stdout
    if not torch.cuda.is_available():
        out = subprocess.run([sys.executable, tool, "--prefill"], capture_output=True, text=True, timeout=300)
        assert out.returncode != 0 and "measures on the GPU; none found" in out.stderr
