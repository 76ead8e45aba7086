"""The segmented adapter GEMM on the routed Mixtral experts (aqlm_hip_lora_sgmv_routed), the parts that need no GPU: the C ABI
(symbols, workspace size, support query, argument checks on a host buffer in their documented order), the route predicate as a
truth table, and the code object of lora_sgmv_routed.hip (the fp16 and bf16 shrink and expand kernels, no scratch)."""
import ctypes
import itertools
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
ISA_FLAGS = ["-O3", "-std=c++17", "--offload-arch=gfx950", "-fPIC", "-ffp-contract=fast", "-mllvm",
             "-amdgpu-kernarg-preload-count=14", "--cuda-device-only", "-S"]  # the flags of tests/test_lora_moe_host.py
NEW = ("aqlm_hip_lora_sgmv_routed", "aqlm_hip_lora_sgmv_routed_supported", "aqlm_hip_lora_sgmv_routed_workspace_bytes")
MAX_PAIRS = 65536


def test_symbols_are_declared_bound_and_exported_and_the_abi_version_stays():
    from aqlm_amd import _native as nat

    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "aqlm_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(aqlm_hip_[a-z0-9_]+)\s*\(", text))
    raw = ctypes.CDLL(nat.LIB_PATH)
    for name in NEW:
        assert name in declared and name in nat.SIGNATURES and hasattr(raw, name), name
    assert re.search(r"#define\s+AQLM_HIP_MAX_LORA_SGMV_ROUTED_PAIRS\s+65536\b", text)
    assert nat.MAX_LORA_SGMV_ROUTED_PAIRS == MAX_PAIRS
    assert nat.lib.aqlm_hip_abi_version() == nat.ABI_VERSION == 9


def test_workspace_size_follows_the_k_cut_of_the_dense_launch():
    from aqlm_amd import _native as nat

    ws, dense = nat.lib.aqlm_hip_lora_sgmv_routed_workspace_bytes, nat.lib.aqlm_hip_lora_sgmv_workspace_bytes
    for fin, splits in ((64, 1), (1032, 2), (14336, 8)):
        for pairs, S, rank in ((300, 2, 128), (300, 1, 16), (1, 1, 8), (MAX_PAIRS, 2, 128)):
            assert ws(pairs, S, rank, fin) == pairs * S * splits * rank * 4, (fin, pairs, S, rank)
        assert ws(7, 1, 24, fin) == dense(7, 24, fin)  # one segment: the dense launch's workspace, the same sgmv_splits
    for bad in ((0, 1, 16, 64), (MAX_PAIRS + 1, 1, 16, 64), (6, 0, 16, 64), (6, 3, 16, 64), (6, 2, 12, 64), (6, 2, 136, 64),
                (6, 2, 0, 64), (6, 2, 16, 60), (6, 2, 16, 0)):
        assert ws(*bad) == 0, bad


def test_supported_query():
    from aqlm_amd import _native as nat

    ok = nat.lib.aqlm_hip_lora_sgmv_routed_supported
    assert ok(300, 520, 24, 300, 4, 2) == 1 and ok(4, 8, 8, 1, 1, 1) == 1 and ok(14336, 4096, 128, MAX_PAIRS, 8, 2) == 1
    assert ok(4096, 14336, 16, 8192, nat.MAX_ROUTED_EXPERTS, 1) == 1
    assert ok(298, 520, 24, 300, 4, 2) == 0   # out_features % 4: y rows are written in 8-byte groups at stride out_features
    assert ok(300, 516, 24, 300, 4, 2) == 0   # in_features % 8
    assert ok(300, 520, 12, 300, 4, 2) == 0 and ok(300, 520, 136, 300, 4, 2) == 0
    assert ok(300, 520, 24, MAX_PAIRS + 1, 4, 2) == 0 and ok(300, 520, 24, 0, 4, 2) == 0
    assert ok(300, 520, 24, 300, 4, 3) == 0 and ok(300, 520, 24, 300, 4, 0) == 0
    assert ok(300, 520, 24, 300, nat.MAX_ROUTED_EXPERTS + 1, 2) == 0 and ok(300, 520, 24, 300, 0, 2) == 0


def test_argument_checks_report_the_documented_codes_in_the_documented_order():
    """Dummy host pointers: every call returns before any launch."""
    from aqlm_amd import _native as nat

    buf = ctypes.create_string_buffer(1 << 17)
    p = (ctypes.addressof(buf) + 15) // 16 * 16
    need = 4 * 2 * 16 * 4  # pairs x segments x one K slice x max_rank x 4
    args = lambda **kw: [kw.get(n, d) for n, d in (  # noqa: E731
        ("table", p), ("n", 2), ("E", 4), ("S", 2), ("max_rank", 16), ("aids", p + 2048), ("a64", 1), ("eids", p + 3072), ("e64", 1),
        ("bucket", p + 1024), ("pairs", 4), ("k", 2), ("x", p + 4096), ("xs", 512), ("per_pair", 0), ("y", p + 16384), ("out", 300),
        ("in", 512), ("dt", nat.F16), ("ws", p + 65536), ("ws_bytes", need), ("stream", None))]
    call = nat.lib.aqlm_hip_lora_sgmv_routed
    # as aqlm_hip_lora_bgmv_routed, in the same order
    for null in ("table", "x", "y", "ws", "eids"):
        assert call(*args(**{null: None})) == nat.E_INVALID and "null pointer" in nat.last_error(), null
    assert call(*args(eids=p + 3076)) == nat.E_INVALID and "misaligned" in nat.last_error()
    assert call(*args(aids=p + 2052)) == nat.E_INVALID and "misaligned" in nat.last_error()
    assert call(*args(ws=p + 65536 + 8)) == nat.E_INVALID and "misaligned" in nat.last_error()
    assert call(*args(y=p + 16385)) == nat.E_INVALID and "misaligned" in nat.last_error()
    for bad in ({"pairs": 0, "k": 1}, {"E": 0}, {"S": 0}, {"k": 0}, {"n": 0}, {"out": 0}, {"max_rank": 0}):
        assert call(*args(**bad)) == nat.E_INVALID and "bad sizes" in nat.last_error(), bad
    assert call(*args(pairs=3)) == nat.E_INVALID and "multiple of top_k" in nat.last_error()
    assert call(*args(xs=504)) == nat.E_INVALID and "strides" in nat.last_error()
    assert call(*args(y=p + 4096)) == nat.E_INVALID and "aliases x" in nat.last_error()
    assert call(*args(y=p + 32768 - 7 * 300 * 2 - 16, x=p + 32768)) == nat.E_INVALID and "aliases x" in nat.last_error()
    assert call(*args(dt=2)) == nat.E_UNSUPPORTED and "float16 and bfloat16" in nat.last_error()
    # (x and y far apart: 65536 rows of either are past the buffer, and nothing is dereferenced)
    assert call(*args(pairs=MAX_PAIRS + 1, k=1, x=p + (1 << 24), xs=8, **{"in": 8}, y=p + (1 << 26), out=8,
                      ws_bytes=1 << 30)) == nat.E_UNSUPPORTED
    assert "shape outside" in nat.last_error()
    assert call(*args(max_rank=12)) == nat.E_UNSUPPORTED and "multiple of 8" in nat.last_error()
    assert call(*args(**{"in": 100, "xs": 104})) == nat.E_UNSUPPORTED
    assert call(*args(x=p + 4096 + 8)) == nat.E_UNSUPPORTED and "16-byte aligned" in nat.last_error()
    # then the bucket ...
    assert call(*args(bucket=None)) == nat.E_INVALID and "null pointer" in nat.last_error()
    assert call(*args(bucket=p + 1024 + 8)) == nat.E_INVALID and "misaligned" in nat.last_error() and "bucket" in nat.last_error()
    assert call(*args(bucket=None, dt=2)) == nat.E_UNSUPPORTED, "the bucket is checked after the shared checks"
    # ... then what this launch declines in addition ...
    assert call(*args(S=3, ws_bytes=1 << 16)) == nat.E_UNSUPPORTED and "segments" in nat.last_error()
    assert call(*args(E=nat.MAX_ROUTED_EXPERTS + 1)) == nat.E_UNSUPPORTED and "experts" in nat.last_error()
    assert call(*args(S=3, bucket=None, ws_bytes=1 << 16)) == nat.E_INVALID, "the bucket is checked before the segments"
    assert call(*args(out=298)) == nat.E_UNSUPPORTED and "8-byte aligned" in nat.last_error()
    assert call(*args(y=p + 16384 + 4)) == nat.E_UNSUPPORTED and "8-byte aligned" in nat.last_error()
    # ... and last the workspace: in_features 1032 needs two K slices
    assert call(*args(ws_bytes=need - 4)) == nat.E_INVALID and f"{need} bytes needed" in nat.last_error()
    assert call(*args(**{"in": 1032, "xs": 1032})) == nat.E_INVALID and f"{2 * need} bytes needed" in nat.last_error()
    assert call(*args(out=298, ws_bytes=0)) == nat.E_UNSUPPORTED, "the y groups are checked before the workspace"


def test_route_predicate_is_a_pure_table(monkeypatch):
    import aqlm.lora as lora

    assert lora.ROUTED_SGMV_MIN_PAIRS == 257 and lora.AQLM_HIP_MAX_LORA_SGMV_ROUTED_PAIRS == MAX_PAIRS
    monkeypatch.setattr(lora, "ROUTED_SGMV_MAX_PAIRS", 1024)
    for cuda, dtype_ok, grad, compiling, supported in itertools.product((False, True), repeat=5):
        for pairs in (0, 1, 256, 257, 1024, 1025):
            want = cuda and dtype_ok and not grad and not compiling and supported and 257 <= pairs <= 1024
            assert lora.takes_routed_sgmv_route(cuda, dtype_ok, grad, compiling, pairs, supported) is want
    monkeypatch.setattr(lora, "ROUTED_SGMV_MAX_PAIRS", 0)  # switched off
    assert not any(lora.takes_routed_sgmv_route(True, True, False, False, pairs, True) for pairs in (1, 256, 257, 512, MAX_PAIRS))
    monkeypatch.setattr(lora, "ROUTED_SGMV_MAX_PAIRS", 10 ** 6)  # never beyond what one launch takes
    assert lora.takes_routed_sgmv_route(True, True, False, False, MAX_PAIRS, True)
    assert not lora.takes_routed_sgmv_route(True, True, False, False, MAX_PAIRS + 1, True)
    assert not lora.takes_routed_sgmv_route(True, True, False, False, 256, True)
    # the calls of up to 256 pairs keep their predicate whatever the new constant says
    monkeypatch.setattr(lora, "ROUTED_BGMV_MAX_PAIRS", 16)
    assert lora.takes_routed_bgmv_route(True, True, False, False, 16, True)
    assert not lora.takes_routed_bgmv_route(True, True, False, False, 17, True)
    assert not lora.takes_routed_sgmv_route(True, True, False, False, 17, True)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_code_object_holds_the_four_kernels_without_scratch(tmp_path):
    out = tmp_path / "lora_sgmv_routed.s"
    subprocess.run([HIPCC] + ISA_FLAGS + [os.path.join(ROOT, "aqlm_amd", "csrc", "lora_sgmv_routed.hip"), "-o", str(out)], check=True,
                   stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=900)
    text = out.read_text()
    pattern = r"_ZN4aqlm\d+lora_sgmv_routed_(?:shrink|expand)_kernel\w+"
    names = set(re.findall(rf"^\s+\.name:\s+({pattern})", text, re.M))
    assert len(names) == 4, names  # shrink / expand x fp16 / bf16
    assert sum("shrink" in n for n in names) == 2 and sum("expand" in n for n in names) == 2
    assert sum("BF16" in n for n in names) == 2 and sum("F16" in n and "BF16" not in n for n in names) == 2
    seen = 0
    for m in re.finditer(rf"\.name:\s+({pattern})(.*?)(?=\n  - |\Z)", text, re.S):
        assert re.search(r"\.private_segment_fixed_size:\s+0\b", m.group(2)), m.group(1)
        seen += 1
    assert seen == 4
    for name in names:
        body = re.split(rf"^{name}:", text, maxsplit=1, flags=re.M)[1].split(".Lfunc_end", 1)[0]
        assert "v_mfma_f32_16x16x32" in body, f"{name}: no matrix instruction"
        assert not re.search(r"\bscratch_(load|store)", body), f"{name}: scratch access"
