"""Training codebooks and scales of K x 8 layers, the parts that need no GPU: the C ABI of aqlm_hip_codebook_grad_kx8 /
aqlm_hip_scales_grad_kx8 (symbols, the support and workspace queries, the argument checks on host buffers in their documented
order), the route predicate as a truth table, the numpy model of the fixed-point arithmetic against the fp64 sums within the
documented bound, and the code object of codebook_grad_kx8.hip (22 kernels, no scratch, 64-bit integer LDS adds in the accumulate
kernels only, no float or global atomic)."""
import ctypes
import itertools
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from tests import kx8_grad_model as model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
ISA_FLAGS = ["-O3", "-std=c++17", "--offload-arch=gfx950", "-fPIC", "-ffp-contract=fast", "-mllvm",
             "-amdgpu-kernarg-preload-count=14", "--cuda-device-only", "-S"]  # the Makefile's flags
NEW = ("aqlm_hip_codebook_grad_kx8_supported", "aqlm_hip_codebook_grad_kx8_workspace_bytes", "aqlm_hip_codebook_grad_kx8",
       "aqlm_hip_scales_grad_kx8_supported", "aqlm_hip_scales_grad_kx8")
SHAPES = [(24, 64, 8, 2), (40, 192, 16, 4), (264, 520, 8, 2), (72, 320, 32, 8), (520, 64, 8, 1)]  # (out, in, g, K)


def _row_blocks(out, K, g):
    passes = -(-K // (64 // g))
    return min(out, max(1, 256 // passes))


# ---------------------------------------------------------------------------------------------------------------------------
# 1. symbols and queries
# ---------------------------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_bound_and_exported_and_the_abi_version_stays():
    from aqlm_amd import _native as nat

    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "aqlm_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(aqlm_hip_[a-z0-9_]+)\s*\(", text))
    raw = ctypes.CDLL(nat.LIB_PATH)
    for name in NEW:
        assert name in declared and name in nat.SIGNATURES and hasattr(raw, name), name
    assert nat.lib.aqlm_hip_abi_version() == nat.ABI_VERSION == 9
    from aqlm_amd.inference_kernels import hip_kernel  # noqa: F401  (registers the ops)

    for op in ("codebook_grad_kx8", "scales_grad_kx8"):
        assert hasattr(torch.ops.aqlm, op)
    for fn in ("codebook_grad_kx8_supported", "codebook_grad_kx8", "scales_grad_kx8"):
        assert callable(getattr(hip_kernel, fn))


def test_supported_queries():
    from aqlm_amd import _native as nat
    from aqlm_amd.inference_kernels import hip_kernel as hk

    for fn in (nat.lib.aqlm_hip_codebook_grad_kx8_supported, nat.lib.aqlm_hip_scales_grad_kx8_supported):
        for out, fin, K, g in ((24, 64, 2, 8), (40, 192, 4, 16), (72, 320, 8, 32), (520, 64, 1, 8), (14336, 4096, 2, 8)):
            assert fn(out, fin, K, g) == 1, (out, fin, K, g)
        for K in (0, 9, -1):
            assert fn(24, 64, K, 8) == 0, K
        for g in (4, 12, 64, 0, -8):
            assert fn(24, 192, 2, g) == 0, g
        assert fn(24, 60, 2, 8) == 0 and fn(24, 72, 2, 16) == 0 and fn(24, 48, 2, 32) == 0  # in_features % g
        assert fn(0, 64, 2, 8) == 0 and fn(24, 0, 2, 8) == 0 and fn(-1, 64, 2, 8) == 0 and fn(24, -64, 2, 8) == 0
        assert fn(1 << 17, 1 << 16, 2, 8) == 0       # P = 2^30
        assert fn((1 << 17) - 1, 1 << 16, 2, 8) == 1  # P = 2^30 - 2^13
    assert hk.codebook_grad_kx8_supported(24, 64, 2, 8) and not hk.codebook_grad_kx8_supported(24, 64, 9, 8)


def test_workspace_is_the_documented_formula_and_stays_below_64_mib():
    from aqlm_amd import _native as nat

    ws = nat.lib.aqlm_hip_codebook_grad_kx8_workspace_bytes
    bench = [(4096, 4096, 2, 8), (11008, 4096, 2, 8), (4096, 11008, 2, 8), (4096, 4096, 8, 32), (28672, 8192, 8, 32)]
    for out, fin, K, g in [(o, i, k, g) for o, i, g, k in SHAPES] + bench + [(3, 64, 8, 8), (4096, 4096, 8, 8), (4096, 4096, 5, 32)]:
        want = _row_blocks(out, K, g) * K * 256 * g * 8 + 8192
        assert ws(out, fin, K, g) == want and want <= 64 << 20, (out, fin, K, g)
    assert ws(4096, 4096, 2, 8) == 256 * 2 * 256 * 8 * 8 + 8192      # 8.4 MB
    assert ws(4096, 4096, 8, 32) == 64 * 8 * 256 * 32 * 8 + 8192     # 33.5 MB
    # the largest image any supported (K, g) takes
    assert max(_row_blocks(1 << 20, K, g) * K * 256 * g * 8 for K in range(1, 9) for g in (8, 16, 32)) + 8192 <= 64 << 20
    assert ws(24, 64, 9, 8) == 0 and ws(24, 64, 2, 12) == 0 and ws(0, 64, 2, 8) == 0 and ws(24, 60, 2, 8) == 0


# ---------------------------------------------------------------------------------------------------------------------------
# 2. argument checks, on dummy host pointers: every call returns before a launch
# ---------------------------------------------------------------------------------------------------------------------------
def _host_buffer():
    buf = ctypes.create_string_buffer(1 << 17)
    return buf, (ctypes.addressof(buf) + 15) // 16 * 16


def test_codebook_grad_argument_checks_report_the_documented_codes_in_the_documented_order():
    from aqlm_amd import _native as nat

    buf, p = _host_buffer()
    need = nat.lib.aqlm_hip_codebook_grad_kx8_workspace_bytes(24, 64, 2, 8)
    args = lambda **kw: [kw.get(n, d) for n, d in (  # noqa: E731
        ("dw", p), ("stride", 64), ("dwt", nat.F16), ("scales", p + 4096), ("dt", nat.F16), ("codes", p + 8193), ("out", 24), ("in", 64),
        ("K", 2), ("g", 8), ("y", p + 16384), ("yt", nat.F32), ("ws", p + 32768), ("ws_bytes", need), ("stream", None))]
    call = nat.lib.aqlm_hip_codebook_grad_kx8
    for null in ("dw", "codes", "y", "ws"):
        assert call(*args(**{null: None})) == nat.E_INVALID and "null pointer" in nat.last_error(), null
    for name, off in (("dw", p + 8), ("scales", p + 4097), ("y", p + 16384 + 8), ("ws", p + 32768 + 4)):
        assert call(*args(**{name: off})) == nat.E_INVALID and "misaligned" in nat.last_error(), name
    assert call(*args(dw=None, g=12)) == nat.E_INVALID and "null pointer" in nat.last_error(), "null pointers come first"
    for bad in ({"out": 0}, {"in": 0}, {"g": 0}, {"in": 60}, {"out": -3}):
        assert call(*args(**bad)) == nat.E_INVALID and "bad sizes" in nat.last_error(), bad
    assert call(*args(dw=p + 8, out=0)) == nat.E_INVALID and "misaligned" in nat.last_error(), "alignment comes before the sizes"
    assert call(*args(stride=56)) == nat.E_INVALID and "row stride" in nat.last_error()
    assert call(*args(ws_bytes=need - 4)) == nat.E_INVALID and f"{need} bytes are needed" in nat.last_error()
    assert call(*args(out=0, dwt=7)) == nat.E_INVALID, "sizes come before the dtypes"
    for bad in ({"dwt": 3}, {"dwt": -1}, {"yt": 3}):
        assert call(*args(**bad)) == nat.E_UNSUPPORTED and "float32" in nat.last_error(), bad
    assert call(*args(dt=nat.F32)) == nat.E_UNSUPPORTED and "float16 and bfloat16" in nat.last_error(), "scales are fp16 / bf16"
    assert call(*args(dt=nat.F32, K=9)) == nat.E_UNSUPPORTED and "float16 and bfloat16" in nat.last_error(), "dtypes come before K"
    for K in (0, 9):
        assert call(*args(K=K)) == nat.E_UNSUPPORTED and "codebooks of 256 entries" in nat.last_error(), K
    assert call(*args(K=9, g=4)) == nat.E_UNSUPPORTED and "codebooks of 256 entries" in nat.last_error(), "K comes before g"
    for g in (4, 64):
        assert call(*args(g=g)) == nat.E_UNSUPPORTED and "8, 16 or 32 features" in nat.last_error(), g
    assert call(*args(stride=68)) == nat.E_UNSUPPORTED and "shape outside" in nat.last_error()  # 136-byte rows
    assert call(*args(stride=66, dwt=nat.F32)) == nat.E_UNSUPPORTED  # 264-byte rows
    assert call(*args(out=1 << 17, **{"in": 1 << 16, "stride": 1 << 16})) == nat.E_UNSUPPORTED and "shape outside" in nat.last_error()
    # NULL scales are a valid argument: the first complaint is the next one in line
    assert call(*args(scales=None, g=64)) == nat.E_UNSUPPORTED and "8, 16 or 32 features" in nat.last_error()


def test_scales_grad_argument_checks_report_the_documented_codes_in_the_documented_order():
    from aqlm_amd import _native as nat

    buf, p = _host_buffer()
    args = lambda **kw: [kw.get(n, d) for n, d in (  # noqa: E731
        ("dw", p), ("stride", 64), ("dwt", nat.BF16), ("codes", p + 4097), ("cb", p + 8192), ("dt", nat.BF16), ("out", 24), ("in", 64),
        ("K", 2), ("g", 8), ("y", p + 16384 + 4), ("yt", nat.BF16), ("stream", None))]
    call = nat.lib.aqlm_hip_scales_grad_kx8
    for null in ("dw", "codes", "cb", "y"):
        assert call(*args(**{null: None})) == nat.E_INVALID and "null pointer" in nat.last_error(), null
    for name, off in (("dw", p + 8), ("cb", p + 8192 + 8), ("y", p + 16386)):
        assert call(*args(**{name: off})) == nat.E_INVALID and "misaligned" in nat.last_error(), name
    assert call(*args(y=None, g=12)) == nat.E_INVALID and "null pointer" in nat.last_error()
    for bad in ({"out": 0}, {"in": 0}, {"g": 0}, {"in": 60}):
        assert call(*args(**bad)) == nat.E_INVALID and "bad sizes" in nat.last_error(), bad
    assert call(*args(cb=p + 8192 + 8, out=0)) == nat.E_INVALID and "misaligned" in nat.last_error()
    assert call(*args(stride=56)) == nat.E_INVALID and "row stride" in nat.last_error()
    assert call(*args(stride=56, dwt=9)) == nat.E_INVALID, "sizes come before the dtypes"
    for bad in ({"dwt": 3}, {"yt": -1}):
        assert call(*args(**bad)) == nat.E_UNSUPPORTED and "float32" in nat.last_error(), bad
    assert call(*args(dt=nat.F32)) == nat.E_UNSUPPORTED and "float16 and bfloat16" in nat.last_error(), "the codebooks are fp16 / bf16"
    for K in (0, 9):
        assert call(*args(K=K)) == nat.E_UNSUPPORTED and "codebooks of 256 entries" in nat.last_error(), K
    for g in (4, 64):
        assert call(*args(g=g)) == nat.E_UNSUPPORTED and "8, 16 or 32 features" in nat.last_error(), g
    assert call(*args(stride=68)) == nat.E_UNSUPPORTED and "shape outside" in nat.last_error()
    assert call(*args(out=1 << 17, **{"in": 1 << 16, "stride": 1 << 16})) == nat.E_UNSUPPORTED


# ---------------------------------------------------------------------------------------------------------------------------
# 3. the predicates
# ---------------------------------------------------------------------------------------------------------------------------
SCHEMES = ((1, 16, 1, 8), (1, 16, 1, 16), (1, 16, 1, 32), (1, 16, 2, 8), (2, 8, 1, 8), (8, 8, 1, 32), (1, 8, 1, 8), (2, 16, 1, 8),
           (4, 8, 1, 16), (8, 8, 1, 8), (9, 8, 1, 8), (0, 8, 1, 8), (2, 8, 2, 8), (2, 8, 1, 4), (2, 8, 1, 64), (2, 8, 1, 12), (2, 4, 1, 8),
           (16, 8, 1, 8))


def test_route_predicates_are_pure_tables(monkeypatch):
    import aqlm.tuning as tuning

    assert tuning.CODEBOOK_GRAD_KERNEL is True
    for switch in (True, False):
        monkeypatch.setattr(tuning, "CODEBOOK_GRAD_KERNEL", switch)
        for scheme in SCHEMES:
            K, nbits, ogs, g = scheme
            for on_gpu, dtypes_ok, supported, compiling in itertools.product((False, True), repeat=4):
                rest = on_gpu and dtypes_ok and supported and not compiling
                want = switch and nbits == 8 and 1 <= K <= 8 and ogs == 1 and g in (8, 16, 32) and rest
                assert tuning.takes_codebook_grad_kernel_kx8(*scheme, on_gpu, dtypes_ok, supported, compiling) is want, scheme
                old = switch and scheme in ((1, 16, 1, 8), (1, 16, 1, 16)) and rest
                assert tuning.takes_codebook_grad_kernel(*scheme, on_gpu, dtypes_ok, supported, compiling) is old, scheme
                assert not (want and old)


def test_host_layers_keep_the_torch_route_and_prepare_builds_nothing():
    import aqlm
    import aqlm.tuning as tuning

    layer = aqlm.QuantizedLinear(64, 24, 8, 1, 2, 8, bias=True, dtype=torch.float16)
    assert layer._takes_codebook_grad_kernel_kx8(None) is False and layer._takes_codebook_grad_kernel_kx8(torch.zeros(2, 64)) is False
    assert layer._takes_codebook_grad_kernel(None) is False
    params = tuning.make_trainable(torch.nn.Sequential(layer))
    assert len(params) == 2 and tuning.prepare(torch.nn.Sequential(layer)) == 0 and layer._grad_index is None


# ---------------------------------------------------------------------------------------------------------------------------
# 4. the numpy model of the fixed-point arithmetic against the fp64 sums
# ---------------------------------------------------------------------------------------------------------------------------
def _values(kind, out, nj, K, seed):
    rng = np.random.default_rng(seed)
    v = rng.integers(0, 256, size=(out, nj, K))
    if kind == "equal":
        v[:] = 200
    return v


@pytest.mark.parametrize("kind", ["uniform", "equal"])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16, torch.float32], ids=["fp16", "bf16", "fp32"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_model_stays_within_the_documented_bound_of_the_fp64_sums(shape, dtype, kind):
    out, fin, g, K = shape
    values = _values(kind, out, fin // g, K, 3)
    gen = torch.Generator().manual_seed(out + fin)
    storage = torch.float16 if dtype == torch.float32 else dtype
    dw64 = torch.randn((out, fin), generator=gen).to(dtype).double().numpy()
    s64 = (torch.rand((out,), generator=gen) + 0.5).to(storage).double().numpy()
    exact, _ = model.exact_dc(values, dw64, s64, g)
    got32 = model.fixed_point_dc(values, dw64, s64, g)
    for out_dtype in (torch.float32, storage):
        name = str(out_dtype)[6:]
        got = torch.from_numpy(got32).to(out_dtype).double().numpy()
        bound = model.dc_bound(values, dw64, s64, g, name)
        assert (np.abs(got - exact) <= bound).all(), (name, float((np.abs(got - exact) / bound).max()))
    unused = model.counts(values) == 0
    assert (got32[unused] == 0).all()


def test_model_special_cases_and_headroom():
    out, fin, g, K = SHAPES[2]
    nj = fin // g
    values = np.zeros((out, nj, K), dtype=np.int64)
    assert out * nj == 17160 and model.shift_of(out, fin, g) == 62 - 15
    got = model.fixed_point_dc(values, np.full((out, fin), 65504.0), np.full(out, 2.0), g)
    assert (got[:, 0, :] == 2248097280.0).all() and (got[:, 1:, :] == 0).all() and 17160 * 65504 * 2 == 2248097280
    assert (model.fixed_point_dc(values, np.zeros((out, fin)), np.ones(out), g) == 0).all()
    dw = np.ones((out, fin))
    dw[3, 5] = np.inf
    assert np.isnan(model.fixed_point_dc(values, dw, np.ones(out), g)).all()
    # integer data: the scaled terms are integers already, the result is the fp64 sum rounded once
    rng = np.random.default_rng(0)
    values = rng.integers(0, 256, size=(out, nj, K))
    dw = rng.integers(-8, 9, size=(out, fin)).astype(np.float64)
    s = rng.choice([0.5, 1.0, 2.0], size=out)
    exact, _ = model.exact_dc(values, dw, s, g)
    assert np.array_equal(model.fixed_point_dc(values, dw, s, g), exact.astype(np.float32))


# ---------------------------------------------------------------------------------------------------------------------------
# 5. the code object
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_code_object_holds_the_kernels_without_scratch_or_float_atomics(tmp_path):
    out = tmp_path / "codebook_grad_kx8.s"
    subprocess.run([HIPCC] + ISA_FLAGS + [os.path.join(ROOT, "aqlm_amd", "csrc", "codebook_grad_kx8.hip"), "-o", str(out)], check=True,
                   stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=900)
    text = out.read_text()
    pattern = r"_ZN4aqlm\d+(?:codebook_grad_kx8_maxima|codebook_grad_kx8_accumulate|codebook_grad_kx8_finish|scales_grad_kx8)_kernel\w+"
    names = set(re.findall(rf"^\s+\.name:\s+({pattern})", text, re.M))
    # maxima per dW dtype, accumulate and scale gradient per dW dtype x g 8 / 16 / 32, one finish
    count = {k: sum(k in n for n in names) for k in ("maxima", "accumulate", "finish", "scales_grad")}
    assert count == {"maxima": 3, "accumulate": 9, "finish": 1, "scales_grad": 9} and len(names) == 22, names
    seen = 0
    for m in re.finditer(rf"\.name:\s+({pattern})(.*?)(?=\n  - |\Z)", text, re.S):
        assert re.search(r"\.private_segment_fixed_size:\s+0\b", m.group(2)), m.group(1)
        assert re.search(r"\.vgpr_spill_count:\s+0\b", m.group(2)) and re.search(r"\.sgpr_spill_count:\s+0\b", m.group(2)), m.group(1)
        seen += 1
    assert seen == 22
    assert re.findall(r"\.max_flat_workgroup_size:\s+(\d+)", text) == ["256"] * 22  # __launch_bounds__(256) on every kernel
    assert "global_atomic" not in text and "flat_atomic" not in text and "buffer_atomic" not in text
    assert not re.search(r"\bds_(add_f32|add_rtn_f32|add_f64|add_rtn_f64|pk_add)", text), "a float LDS atomic"
    for name in names:
        body = re.split(rf"^{name}:", text, maxsplit=1, flags=re.M)[1].split(".Lfunc_end", 1)[0]
        assert not re.search(r"\bscratch_(load|store)", body), f"{name}: scratch access"
        adds = len(re.findall(r"\bds_add_u64\b", body))
        lds_atomics = len(re.findall(r"\bds_(add|sub|inc|dec|min|max|and|or|xor|cmpst|wrxchg)_(rtn_)?[a-z]*\d+\b", body))
        if "accumulate" in name:
            assert adds > 0 and lds_atomics == adds, f"{name}: {adds} ds_add_u64 of {lds_atomics} LDS atomics"
        else:
            assert lds_atomics == 0, f"{name}: an LDS atomic"
