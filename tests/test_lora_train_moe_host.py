"""Training the adapters of the routed Mixtral experts on device launches (aqlm_hip_lora_transpose_routed,
aqlm_hip_lora_grad_routed), the parts that need no GPU: the C ABI (symbols, the buffer size, the support queries, the argument
checks of the entries on host buffers in their documented order, return code by return code), the new route predicate as a truth
table with the four older predicates unchanged, the layout of the transposed table against a numpy model, the switch
``ROUTED_TRAIN_MAX_PAIRS = 0``, and the code object of lora_routed_bwd.hip (three kernels, no scratch)."""
import ctypes
import itertools
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from tests.test_lora_moe_host import _wrapped, mc, tiny  # noqa: F401  (tiny: the fixture of the host block)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
ISA_FLAGS = ["-O3", "-std=c++17", "--offload-arch=gfx950", "-fPIC", "-ffp-contract=fast", "-mllvm",
             "-amdgpu-kernarg-preload-count=14", "--cuda-device-only", "-S"]  # the flags of tests/test_lora_moe_host.py
NEW = ("aqlm_hip_lora_transpose_routed", "aqlm_hip_lora_transpose_routed_bytes", "aqlm_hip_lora_transpose_routed_supported",
       "aqlm_hip_lora_grad_routed", "aqlm_hip_lora_grad_routed_supported")
MAX_PAIRS = 65536


def test_symbols_are_declared_bound_and_exported_and_the_abi_version_stays():
    from aqlm_amd import _native as nat

    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "aqlm_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(aqlm_hip_[a-z0-9_]+)\s*\(", text))
    raw = ctypes.CDLL(nat.LIB_PATH)
    for name in NEW:
        assert name in declared and name in nat.SIGNATURES and hasattr(raw, name), name
    assert nat.lib.aqlm_hip_abi_version() == nat.ABI_VERSION == 9
    from aqlm_amd.inference_kernels import hip_kernel  # noqa: F401  (registers the ops)

    for op in ("lora_transpose_routed_", "lora_grad_routed"):
        assert hasattr(torch.ops.aqlm, op)


def test_buffer_size_and_supported_queries():
    from aqlm_amd import _native as nat

    size, tr, gr = (nat.lib.aqlm_hip_lora_transpose_routed_bytes, nat.lib.aqlm_hip_lora_transpose_routed_supported,
                    nat.lib.aqlm_hip_lora_grad_routed_supported)
    assert size(3, 4, 2, 24, 296, 520) == 3 * 4 * 2 * 24 * (296 + 520) * 2
    assert size(4, 8, 2, 16, 14336, 4096) == 4 * 8 * 2 * 16 * (14336 + 4096) * 2
    for bad in ((0, 4, 2, 24, 296, 520), (3, 0, 2, 24, 296, 520), (3, 4, 3, 24, 296, 520), (3, 4, 2, 12, 296, 520),
                (3, 4, 2, 136, 296, 520), (3, 4, 2, 24, 300, 520), (3, 4, 2, 24, 296, 516), (3, nat.MAX_ROUTED_EXPERTS + 1, 2, 24, 296, 520)):
        assert size(*bad) == 0, bad
    assert tr(296, 520, 24, 4, 2) == 1 and tr(8, 8, 8, 1, 1) == 1 and tr(14336, 4096, 128, nat.MAX_ROUTED_EXPERTS, 2) == 1
    assert tr(300, 520, 24, 4, 2) == 0   # out_features % 8: the transposed call reads grad_y rows in 16-byte pieces
    assert tr(296, 516, 24, 4, 2) == 0 and tr(296, 520, 12, 4, 2) == 0 and tr(296, 520, 136, 4, 2) == 0
    assert tr(296, 520, 24, 0, 2) == 0 and tr(296, 520, 24, 4, 3) == 0 and tr(296, 520, 24, 4, 0) == 0
    assert gr(296, 24, 300, 4, 2) == 1 and gr(8, 8, 1, 1, 1) == 1 and gr(14336, 128, MAX_PAIRS, nat.MAX_ROUTED_EXPERTS, 2) == 1
    assert gr(300, 24, 300, 4, 2) == 0 and gr(0, 24, 300, 4, 2) == 0
    assert gr(296, 12, 300, 4, 2) == 0 and gr(296, 136, 300, 4, 2) == 0
    assert gr(296, 24, 0, 4, 2) == 0 and gr(296, 24, MAX_PAIRS + 1, 4, 2) == 0
    assert gr(296, 24, 300, 0, 2) == 0 and gr(296, 24, 300, nat.MAX_ROUTED_EXPERTS + 1, 2) == 0 and gr(296, 24, 300, 4, 3) == 0


def _host_buffer():
    buf = ctypes.create_string_buffer(1 << 17)
    return buf, (ctypes.addressof(buf) + 15) // 16 * 16


def test_transpose_argument_checks_report_the_documented_codes_in_the_documented_order():
    """Dummy host pointers: every call returns before any launch."""
    from aqlm_amd import _native as nat

    buf, p = _host_buffer()
    args = lambda **kw: [kw.get(n, d) for n, d in (  # noqa: E731
        ("table", p), ("transposed", p + 1024), ("n", 2), ("E", 4), ("S", 2), ("max_rank", 16), ("out", 296), ("in", 520),
        ("buffer", p + 4096), ("bytes", 1 << 16), ("stream", None))]
    call = nat.lib.aqlm_hip_lora_transpose_routed
    for null in ("table", "transposed", "buffer"):
        assert call(*args(**{null: None})) == nat.E_INVALID and "null pointer" in nat.last_error(), null
    for name, off in (("table", p + 4), ("transposed", p + 1028), ("buffer", p + 4096 + 8)):
        assert call(*args(**{name: off})) == nat.E_INVALID and "misaligned" in nat.last_error(), name
    assert call(*args(table=None, max_rank=12)) == nat.E_INVALID, "null pointers are reported before the shape"
    for bad in ({"n": 0}, {"E": 0}, {"S": 0}, {"max_rank": 0}, {"out": 0}, {"in": 0}, {"bytes": 0}):
        assert call(*args(**bad)) == nat.E_INVALID and "bad sizes" in nat.last_error(), bad
    assert call(*args(buffer=p + 4096 + 8, n=0)) == nat.E_INVALID and "misaligned" in nat.last_error()
    for bad in ({"max_rank": 12}, {"max_rank": 136}, {"out": 300}, {"in": 516}, {"S": 3}, {"E": nat.MAX_ROUTED_EXPERTS + 1}):
        assert call(*args(**bad)) == nat.E_UNSUPPORTED and "shape outside" in nat.last_error(), bad
    assert call(*args(max_rank=12, bytes=0)) == nat.E_INVALID, "sizes below 1 are reported before the shape"
    assert call(*args(n=300, E=256)) == nat.E_UNSUPPORTED and "table entries" in nat.last_error()


def test_grad_argument_checks_report_the_documented_codes_in_the_documented_order():
    """Dummy host pointers: every call returns before any launch."""
    from aqlm_amd import _native as nat

    buf, p = _host_buffer()
    need = 4 * 2 * 16 * 296 * 4  # experts x segments x max_rank x dim x 4
    args = lambda **kw: [kw.get(n, d) for n, d in (  # noqa: E731
        ("table", p), ("n", 2), ("E", 4), ("S", 2), ("max_rank", 16), ("adapter", 1), ("aids", p + 2048), ("a64", 1),
        ("eids", p + 3072), ("e64", 1), ("bucket", p + 1024), ("pairs", 4), ("k", 2), ("v", p + 4096), ("vrs", 296), ("vss", 0),
        ("per_pair", 0), ("dim", 296), ("w", p + 16384), ("wps", 64), ("wss", 32), ("splits", 2), ("wsp", 16), ("g", p + 32768),
        ("g_bytes", need), ("dt", nat.F16), ("stream", None))]
    call = nat.lib.aqlm_hip_lora_grad_routed
    for null in ("table", "eids", "bucket", "v", "w", "g"):
        assert call(*args(**{null: None})) == nat.E_INVALID and "null pointer" in nat.last_error(), null
    for name, off in (("table", p + 4), ("aids", p + 2052), ("eids", p + 3076), ("bucket", p + 1032), ("w", p + 16386), ("g", p + 32776)):
        assert call(*args(**{name: off})) == nat.E_INVALID and "misaligned" in nat.last_error(), name
    assert call(*args(aids=p + 2052, a64=0, dt=2)) == nat.E_UNSUPPORTED, "int32 ids are aligned to 4 bytes"
    assert call(*args(aids=None, dt=2)) == nat.E_UNSUPPORTED, "adapter_ids may be NULL: adapter 0 for every pair"
    for bad in ({"n": 0}, {"E": 0}, {"S": 0}, {"max_rank": 0}, {"k": 0}, {"pairs": 0, "k": 1}, {"pairs": 3}, {"dim": 0, "vrs": 8},
                {"splits": 0}, {"adapter": -1}, {"adapter": 2}):
        assert call(*args(**bad)) == nat.E_INVALID and "bad sizes" in nat.last_error(), bad
    for bad in ({"vrs": 288}, {"vss": -8}, {"wps": 8}, {"wss": -1}, {"wsp": 8}):
        assert call(*args(**bad)) == nat.E_INVALID and "strides" in nat.last_error(), bad
    assert call(*args(splits=1, wsp=0, dt=2)) == nat.E_UNSUPPORTED, "one slice: its stride is not looked at"
    assert call(*args(dt=2)) == nat.E_UNSUPPORTED and "float16 and bfloat16" in nat.last_error()
    assert call(*args(dt=2, vrs=288)) == nat.E_INVALID, "strides are reported before the dtype"
    for bad in ({"max_rank": 12, "wps": 64}, {"max_rank": 136, "wps": 136, "wsp": 136}, {"dim": 300, "vrs": 304}, {"S": 3},
                {"E": nat.MAX_ROUTED_EXPERTS + 1}, {"pairs": MAX_PAIRS + 2}, {"splits": 9}, {"v": p + 4096 + 8}, {"vrs": 300},
                {"vss": 4}):
        assert call(*args(**bad)) == nat.E_UNSUPPORTED and "shape outside" in nat.last_error(), bad
    assert call(*args(dt=2, max_rank=12)) == nat.E_UNSUPPORTED and "float16" in nat.last_error(), "the dtype is reported before the shape"
    assert call(*args(g_bytes=need - 4)) == nat.E_INVALID and f"{need} bytes needed" in nat.last_error()
    assert call(*args(g_bytes=0, max_rank=12)) == nat.E_UNSUPPORTED, "the shape is reported before the output size"


def test_route_predicates_are_pure_tables_and_the_older_four_are_unchanged(monkeypatch):
    import aqlm.lora as lora

    assert lora.ROUTED_TRAIN_MIN_PAIRS == 1 and lora.AQLM_HIP_MAX_LORA_SGMV_ROUTED_PAIRS == MAX_PAIRS
    monkeypatch.setattr(lora, "ROUTED_TRAIN_MAX_PAIRS", 1024)
    for cuda, dtype_ok, grad, compiling, supported in itertools.product((False, True), repeat=5):
        for pairs in (0, 1, 16, 256, 257, 1024, 1025):
            want = cuda and dtype_ok and grad and not compiling and supported and 1 <= pairs <= 1024
            assert lora.takes_routed_train_route(cuda, dtype_ok, grad, compiling, pairs, supported) is want
    monkeypatch.setattr(lora, "ROUTED_TRAIN_MAX_PAIRS", 0)  # switched off
    assert not any(lora.takes_routed_train_route(True, True, True, False, pairs, True) for pairs in (1, 16, 256, 257, 512, MAX_PAIRS))
    monkeypatch.setattr(lora, "ROUTED_TRAIN_MAX_PAIRS", 10 ** 6)  # never beyond what one launch takes
    assert lora.takes_routed_train_route(True, True, True, False, MAX_PAIRS, True)
    assert not lora.takes_routed_train_route(True, True, True, False, MAX_PAIRS + 1, True)
    # the four older predicates, whatever the new constant says: a gradient needed -> False, and their own ranges
    monkeypatch.setattr(lora, "BGMV_MAX_ROWS", 64)
    monkeypatch.setattr(lora, "SGMV_MAX_ROWS", 65536)
    monkeypatch.setattr(lora, "ROUTED_BGMV_MAX_PAIRS", 256)
    monkeypatch.setattr(lora, "ROUTED_SGMV_MAX_PAIRS", 65536)
    older = ((lora.takes_bgmv_route, 1, 64), (lora.takes_sgmv_route, 65, 65536), (lora.takes_routed_bgmv_route, 1, 256),
             (lora.takes_routed_sgmv_route, 257, 65536))
    for fn, lo, hi in older:
        for cuda, dtype_ok, grad, compiling, supported in itertools.product((False, True), repeat=5):
            for n in (0, lo - 1, lo, hi, hi + 1):
                want = cuda and dtype_ok and not grad and not compiling and supported and lo <= n <= hi
                assert fn(cuda, dtype_ok, grad, compiling, n, supported) is want, (fn.__name__, n)


def test_transposed_table_layout_against_a_numpy_model():
    from aqlm_amd import _native as nat
    from aqlm_amd.inference_kernels import hip_kernel as hk

    n, E, S, M, Kin = 3, 4, 2, 296, 520
    rng = np.random.default_rng(0)
    ranks = rng.choice([0, 8, 12, 24, 128], size=(n, E, S))
    ranks[0, 0, 0], ranks[2, 3, 1] = 8, 128
    scal = rng.uniform(0.25, 4.0, size=(n, E, S)).astype(np.float32)
    base = 0x7F0000001000
    structs, offsets, elements = hk.lora_routed_transposed_layout(ranks.tolist(), scal.tolist(), M, Kin, base)
    words = np.frombuffer(bytes(structs), dtype=np.int64).reshape(S, n, E, nat.LORA_ENTRY_WORDS)  # [s][a][e]: a segment is one table
    at = 0
    for s in range(S):
        for a in range(n):
            for e in range(E):
                r = int(ranks[a, e, s])
                ent = words[s, a, e]
                rank_word = int(ent[2]) & 0xFFFFFFFF
                scaling = np.frombuffer(np.int64(ent[2]).tobytes(), dtype=np.float32)[1]
                if r == 0 or r % 8:
                    assert (a, e, s) not in offsets and not ent.any(), "an entry without weights or of an odd rank is a zero entry"
                    continue
                assert offsets[(a, e, s)] == (at, at + r * M)
                assert int(ent[0]) == base + 2 * at, "a: B^T [r, M]"
                assert int(ent[1]) == base + 2 * (at + r * M), "b: A^T [K, r], behind it"
                assert rank_word == r and scaling == scal[a, e, s]
                assert int(ent[0]) % 16 == 0 and int(ent[1]) % 16 == 0
                at += r * (M + Kin)
    assert elements == at <= nat.lib.aqlm_hip_lora_transpose_routed_bytes(n, E, S, 128, M, Kin) // 2
    # what the transposed call of segment s is handed: [n][E] entries, contiguous
    per_segment = n * E * nat.LORA_ENTRY_WORDS
    flat = np.frombuffer(bytes(structs), dtype=np.int64)
    assert np.array_equal(flat[per_segment:2 * per_segment].reshape(n, E, -1), words[1])


def test_train_limit_zero_leaves_the_torch_path(tiny, monkeypatch):  # noqa: F811
    """On the host every call is the torch path; with ROUTED_TRAIN_MAX_PAIRS = 0 the predicate says the same for a device call, and
    ``on_pairs`` with a gradient needed reaches ``_torch_pairs`` without asking the library anything."""
    import aqlm.lora as lora

    monkeypatch.setattr(lora, "ROUTED_TRAIN_MAX_PAIRS", 0)
    wrapper, bank, _ = _wrapped(tiny)
    for p in wrapper.lora_A["ad0"].parameters():
        p.requires_grad_(True)
    calls = []
    real = lora._ExpertAdapters._torch_pairs
    monkeypatch.setattr(lora._ExpertAdapters, "_torch_pairs", lambda self, *a: (calls.append(a[0].shape), real(self, *a))[1])
    T, k = 6, 2
    gen = torch.Generator().manual_seed(1)
    x = torch.randn((T, mc.HID), generator=gen).requires_grad_()
    idx = torch.topk(torch.rand((T, mc.EXPERTS), generator=gen), k, dim=-1).indices
    out = torch.zeros((T * k, 2, mc.INTER))
    y = lora._ExpertAdapters(wrapper, "ad0", None).on_pairs(out, x, idx, ("w1", "w3"), False)
    assert calls == [out.shape] and y is not out and y.requires_grad
    y.sum().backward()
    assert x.grad is not None and wrapper.lora_A["ad0"]["0"]["w1"].weight.grad is not None
    assert not lora.takes_routed_train_route(True, True, True, False, T * k, True)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_code_object_holds_the_three_kernels_without_scratch(tmp_path):
    out = tmp_path / "lora_routed_bwd.s"
    subprocess.run([HIPCC] + ISA_FLAGS + [os.path.join(ROOT, "aqlm_amd", "csrc", "lora_routed_bwd.hip"), "-o", str(out)], check=True,
                   stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=900)
    text = out.read_text()
    pattern = r"_ZN4aqlm\d+lora_routed_(?:transpose|grad)_kernel\w+"
    names = set(re.findall(rf"^\s+\.name:\s+({pattern})", text, re.M))
    assert len(names) == 3, names  # the transpose, and the reduction in fp16 and bf16
    assert sum("grad" in n for n in names) == 2 and sum("BF16" in n for n in names) == 1
    seen = 0
    for m in re.finditer(rf"\.name:\s+({pattern})(.*?)(?=\n  - |\Z)", text, re.S):
        assert re.search(r"\.private_segment_fixed_size:\s+0\b", m.group(2)), m.group(1)
        assert re.search(r"\.vgpr_spill_count:\s+0\b", m.group(2)), m.group(1)
        seen += 1
    assert seen == 3
    for name in names:
        body = re.split(rf"^{name}:", text, maxsplit=1, flags=re.M)[1].split(".Lfunc_end", 1)[0]
        assert not re.search(r"\bscratch_(load|store)", body), f"{name}: scratch access"
        if "grad" in name:
            assert re.search(r"\bv_(pk_)?fma", body), f"{name}: no fused multiply-add"
            assert "v_mfma" not in body, f"{name}: the reduction runs on the VALU"
