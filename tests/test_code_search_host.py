"""Updating the codes of AQLM layers (the V step of PV-tuning), the parts that need no GPU: the C ABI of aqlm_hip_code_search_1x16
(symbols, the support and workspace queries, the argument checks on host buffers in their documented order), the route predicate
as a truth table, the torch route of ``aqlm.tuning.find_optimal_codes`` against codes the reference's ``beam_search_optimal_codes``
produced (tests/golden/code_update_golden.npz, written by tools/gen_code_update_golden.py: inputs on a dyadic grid, so every fp32
sum is exact and the expected codes hold on any BLAS), ``update_codes_`` on host layers, and the code object of code_search.hip (8
kernels, no scratch, no atomics)."""
import ctypes
import itertools
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
ISA_FLAGS = ["-O3", "-std=c++17", "--offload-arch=gfx950", "-fPIC", "-ffp-contract=fast", "-mllvm",
             "-amdgpu-kernarg-preload-count=14", "--cuda-device-only", "-S"]  # the Makefile's flags
NEW = ("aqlm_hip_code_search_1x16_supported", "aqlm_hip_code_search_1x16_workspace_bytes", "aqlm_hip_code_search_1x16")
MAX_GROUPS = 2**31 - 1


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
    assert re.search(r"#define AQLM_HIP_F32 2\b", text) and nat.F32 == 2
    eps = float(re.search(r"#define AQLM_HIP_CODE_SEARCH_EPS ([0-9.e+-]+)", text).group(1))
    assert eps == nat.CODE_SEARCH_EPS == 2.0 ** -17
    from aqlm_amd.inference_kernels import hip_kernel  # noqa: F401  (registers the ops)

    assert hasattr(torch.ops.aqlm, "code_search_1x16")
    for fn in ("code_search_1x16_supported", "code_search_1x16"):
        assert callable(getattr(hip_kernel, fn))
    assert hip_kernel.CODE_SEARCH_EPS == eps


def test_supported_query():
    from aqlm_amd import _native as nat
    from aqlm_amd.inference_kernels import hip_kernel as hk

    fn = nat.lib.aqlm_hip_code_search_1x16_supported
    for out, fin, g in ((1, 8, 8), (1, 16, 16), (3, 40, 8), (67, 72, 8), (64, 512, 16), (4096, 4096, 8), (14336, 4096, 8), (4096, 14336, 16)):
        assert fn(out, fin, g) == 1, (out, fin, g)
    for g in (4, 12, 32, 64, 0, -8):
        assert fn(64, 192, g) == 0, g
    assert fn(64, 60, 8) == 0 and fn(64, 72, 16) == 0  # in_features % g
    assert fn(0, 64, 8) == 0 and fn(64, 0, 8) == 0 and fn(-1, 64, 8) == 0 and fn(64, -64, 8) == 0
    assert fn(1 << 15, 1 << 19, 8) == 0               # 2^31 groups
    assert fn((1 << 15) - 1, 1 << 19, 8) == 1         # 2^31 - 2^16 groups
    assert fn(1 << 16, 1 << 19, 16) == 0 and fn((1 << 16) - 1, 1 << 19, 16) == 1
    assert hk.code_search_1x16_supported(64, 256, 8) and not hk.code_search_1x16_supported(64, 256, 32)


def test_workspace_is_the_documented_formula():
    from aqlm_amd import _native as nat

    ws = nat.lib.aqlm_hip_code_search_1x16_workspace_bytes
    for groups in (1, 15, 2048, 2097152, 7340032, MAX_GROUPS):
        for g in (8, 16):
            assert ws(groups, g) == 65536 * 4, (groups, g)  # |C_c|^2 in fp32, whatever the number of groups
    assert ws(0, 8) == 0 and ws(-5, 8) == 0 and ws(MAX_GROUPS + 1, 8) == 0
    for g in (4, 12, 32, 0):
        assert ws(2048, g) == 0, g


# ---------------------------------------------------------------------------------------------------------------------------
# 2. argument checks, on dummy host pointers: every call returns before a launch
# ---------------------------------------------------------------------------------------------------------------------------
def test_argument_checks_report_the_documented_codes_in_the_documented_order():
    from aqlm_amd import _native as nat

    buf = ctypes.create_string_buffer(1 << 17)
    p = (ctypes.addressof(buf) + 15) // 16 * 16
    need = nat.lib.aqlm_hip_code_search_1x16_workspace_bytes(2048, 8)
    args = lambda **kw: [kw.get(n, d) for n, d in (  # noqa: E731
        ("ref", p), ("rt", nat.F32), ("stride", 256), ("scales", p + 4098), ("cb", p + 8192), ("dt", nat.F16), ("out", 64), ("in", 256),
        ("g", 8), ("ids", None), ("ids64", 0), ("n", 2048), ("codes", p + 16386), ("ws", p + 32768), ("ws_bytes", need), ("stream", None))]
    call = nat.lib.aqlm_hip_code_search_1x16
    for null in ("ref", "cb", "codes", "ws"):
        assert call(*args(**{null: None})) == nat.E_INVALID and "null pointer" in nat.last_error(), null
    assert call(*args(ref=None, g=12, n=0)) == nat.E_INVALID and "null pointer" in nat.last_error(), "null pointers come first"
    misaligned = (("ref", p + 2, {}), ("ref", p + 1, {"rt": nat.F16}), ("scales", p + 4097, {}), ("cb", p + 8192 + 8, {}), ("codes", p + 16385, {}),
                  ("ws", p + 32768 + 8, {}), ("ids", p + 65536 + 2, {"n": 7}), ("ids", p + 65536 + 4, {"n": 7, "ids64": 1}))
    for name, addr, more in misaligned:
        assert call(*args(**{name: addr}, **more)) == nat.E_INVALID and "misaligned" in nat.last_error(), name
    # a 16-bit reference is 2-byte aligned: the complaint is the last one in line, the workspace (nothing is launched)
    assert call(*args(ref=p + 2, rt=nat.F16, ws_bytes=0)) == nat.E_INVALID and "bytes are needed" in nat.last_error()
    assert call(*args(ref=p + 2, rt=nat.BF16, scales=p + 4100, codes=p + 16388, ws_bytes=need - 1)) == nat.E_INVALID and "bytes are needed" in nat.last_error()
    assert call(*args(cb=p + 8192 + 8, out=0)) == nat.E_INVALID and "misaligned" in nat.last_error(), "alignment comes before the sizes"
    for bad in ({"out": 0}, {"in": 0}, {"g": 0}, {"in": 252}, {"out": -3}):
        assert call(*args(**bad)) == nat.E_INVALID and "bad sizes" in nat.last_error(), bad
    assert call(*args(stride=248)) == nat.E_INVALID and "row stride" in nat.last_error()
    for n in (0, -1, 2047, 2049):  # without group_ids the call covers the layer
        assert call(*args(n=n)) == nat.E_INVALID and "bad sizes" in nat.last_error(), n
    assert call(*args(ids=p + 65536, n=0)) == nat.E_INVALID and "bad sizes" in nat.last_error()
    assert call(*args(out=0, rt=7)) == nat.E_INVALID, "sizes come before the dtypes"
    for rt in (3, -1):
        assert call(*args(rt=rt)) == nat.E_UNSUPPORTED and "float32" in nat.last_error(), rt
    assert call(*args(dt=nat.F32)) == nat.E_UNSUPPORTED and "float16 and bfloat16" in nat.last_error(), "the codebook is fp16 / bf16"
    assert call(*args(rt=5, dt=nat.F32)) == nat.E_UNSUPPORTED and "float32 (dtype id 5)" in nat.last_error(), "the reference's dtype comes first"
    assert call(*args(dt=nat.F32, g=32, n=512)) == nat.E_UNSUPPORTED and "float16 and bfloat16" in nat.last_error(), "dtypes come before the shape"
    for g in (4, 32):
        assert call(*args(g=g, n=64 * 256 // g)) == nat.E_UNSUPPORTED and "8 or 16 features" in nat.last_error(), g
    huge = {"out": 1 << 15, "in": 1 << 19, "stride": 1 << 19, "n": 1 << 31}
    assert call(*args(**huge)) == nat.E_UNSUPPORTED and "shape outside" in nat.last_error()
    assert call(*args(ids=p + 65536, n=1 << 31)) == nat.E_UNSUPPORTED and "shape outside" in nat.last_error()
    assert call(*args(g=32, n=512, ws_bytes=0)) == nat.E_UNSUPPORTED, "the shape comes before the workspace"
    assert call(*args(ws_bytes=need - 4)) == nat.E_INVALID and f"{need} bytes are needed" in nat.last_error()
    # NULL scales and NULL group_ids are valid arguments: the first complaint is the next one in line
    assert call(*args(scales=None, ws_bytes=0)) == nat.E_INVALID and "bytes are needed" in nat.last_error()


# ---------------------------------------------------------------------------------------------------------------------------
# 3. the predicate
# ---------------------------------------------------------------------------------------------------------------------------
SCHEMES = ((1, 16, 1, 8), (1, 16, 1, 16), (1, 16, 1, 32), (1, 16, 1, 4), (1, 16, 2, 8), (2, 16, 1, 8), (0, 16, 1, 8), (1, 8, 1, 8), (2, 8, 1, 8),
           (8, 8, 1, 32), (1, 12, 1, 8), (1, 16, 1, 12))


def test_route_predicate_is_a_pure_table(monkeypatch):
    import aqlm.tuning as tuning

    assert tuning.CODE_SEARCH_KERNEL is True
    for switch in (True, False):
        monkeypatch.setattr(tuning, "CODE_SEARCH_KERNEL", switch)
        for scheme in SCHEMES:
            for on_gpu, dtypes_ok, supported in itertools.product((False, True), repeat=3):
                want = switch and scheme in ((1, 16, 1, 8), (1, 16, 1, 16)) and on_gpu and dtypes_ok and supported
                assert tuning.takes_code_search_kernel(*scheme, on_gpu, dtypes_ok, supported) is want, (scheme, on_gpu, dtypes_ok, supported)
    monkeypatch.setattr(tuning, "CODE_SEARCH_KERNEL", True)
    base = [1, 16, 1, 8, True, True, True]
    assert tuning.takes_code_search_kernel(*base) is True
    for i, other in enumerate((2, 8, 2, 32, False, False, False)):  # flipping any one argument flips the result
        flipped = list(base)
        flipped[i] = other
        assert tuning.takes_code_search_kernel(*flipped) is False, i
    # the switch of the gradient kernels is another switch
    monkeypatch.setattr(tuning, "CODEBOOK_GRAD_KERNEL", False)
    assert tuning.takes_code_search_kernel(*base) is True


# ---------------------------------------------------------------------------------------------------------------------------
# 4. the torch route against the reference's codes
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden():
    z = np.load(os.path.join(ROOT, "tests", "golden", "code_update_golden.npz"))
    return z, json.loads(str(z["meta"]))


def _golden_case(golden, case):
    from aqlm_amd.utils import pack_int_data

    z, meta = golden
    info = meta["cases"][case]
    name = info["layer"]
    out_features, in_features, K, nbits, ogs, g = meta["layers"][name]["shape"]
    books = torch.from_numpy(z[f"{name}_codebook_k"].astype(np.float32) * meta["grid"])
    target = torch.from_numpy(z[f"{name}_reference_k"].astype(np.float32) * meta["grid"])
    scales = torch.from_numpy(2.0 ** z[f"{name}_scale_exp"].astype(np.float32)).reshape(-1, 1, 1, 1)
    prev = pack_int_data(torch.from_numpy(z[f"{name}_prev_codes"].astype(np.int64)), nbits)
    expected = pack_int_data(torch.from_numpy(z[f"{case}_expected"].astype(np.int64)), nbits)
    assert tuple(books.shape) == (K, 2 ** nbits, ogs, g) and tuple(target.shape) == (out_features, in_features)
    assert tuple(prev.shape) == (out_features // ogs, in_features // g, K) == tuple(expected.shape)
    options = {k: v for k, v in info["options"].items() if k not in ("admitted", "changed_share")}
    return target, books, prev, scales, options, expected, info["options"]


# (a) 1x16 g8 full update, (b) a tenth of the groups, (c) ... under a trust ratio that admits some of them, (d) 2x8 g8 greedy,
# (e) beam 4, (f) 4x8 g16 beam 2 in the order 2, 0, 3, 1, (g) out_group_size 2
GOLDEN_SCHEMES = {"a": (1, 16, 1, 8), "b": (1, 16, 1, 8), "c": (1, 16, 1, 8), "d": (2, 8, 1, 8), "e": (2, 8, 1, 8), "f": (4, 8, 1, 16),
                  "g": (2, 8, 2, 8)}


@pytest.mark.parametrize("case", sorted(GOLDEN_SCHEMES))
def test_torch_route_reproduces_the_reference_code_for_code(golden, case):
    import aqlm.tuning as tuning

    target, books, prev, scales, options, expected, recorded = _golden_case(golden, case)
    K, nbits = GOLDEN_SCHEMES[case][:2]
    assert (books.shape[0], int(np.log2(books.shape[1])), books.shape[2], books.shape[3]) == GOLDEN_SCHEMES[case]
    assert options.get("beam_size") == {"e": 4, "f": 2, "g": 2}.get(case, 1)
    assert ("max_update_fraction" in options) == (case in "bcg") and ("trust_ratio" in options) == (case == "c")
    assert options.get("dim_order") == ([2, 0, 3, 1] if case == "f" else None)
    before = prev.clone()
    got = tuning.find_optimal_codes(target, books, prev, scales, **options)
    assert got.dtype == prev.dtype == (torch.int16 if nbits == 16 else torch.int8) and got.shape == prev.shape
    assert torch.equal(prev, before), "prev_codes is not written"
    assert torch.equal(got, expected), f"{int((got != expected).any(-1).sum())} groups differ"
    changed = int((got != prev).any(-1).sum())
    assert 0 < changed < prev.shape[0] * prev.shape[1] and changed == round(recorded["changed_share"] * prev.shape[0] * prev.shape[1])
    if case == "c":  # some, not all, of the selected changes were admitted
        selected = int(np.ceil(options["max_update_fraction"] * prev.shape[0] * prev.shape[1]))
        assert 1 < recorded["admitted"] < selected and changed <= recorded["admitted"]
    if case == "a":  # with one codebook the beam width does not change the answer; scales None = 1
        assert torch.equal(tuning.find_optimal_codes(target, books, prev, scales, beam_size=3), expected)
        assert torch.equal(tuning.find_optimal_codes(target / scales.reshape(-1, 1), books, prev, None), expected)


def test_find_optimal_codes_options(golden):
    import aqlm.tuning as tuning

    target, books, prev, scales, _, expected, _ = _golden_case(golden, "d")
    for name in ("stochastic_rounding_tau", "force_update"):
        with pytest.raises(NotImplementedError, match=name):
            tuning.find_optimal_codes(target, books, prev, scales, **{name: 0.1})
    with pytest.raises(TypeError, match="bogus"):
        tuning.find_optimal_codes(target, books, prev, scales, bogus=1)
    for bad in ({"max_update_fraction": 0.0}, {"max_update_fraction": 1.5}, {"trust_ratio": 0.0}, {"beam_size": 0}, {"dim_order": [0, 0]}):
        with pytest.raises(ValueError):
            tuning.find_optimal_codes(target, books, prev, scales, **bad)
    with pytest.raises(ValueError, match="one layer"):
        tuning.find_optimal_codes(target[:, :-8], books, prev, scales)
    # sampled selection: as many groups as the fraction allows may change, the draw follows the generator
    gen = lambda: torch.Generator().manual_seed(5)  # noqa: E731
    first = tuning.find_optimal_codes(target, books, prev, scales, max_update_fraction=0.1, code_selection_temperature=1.0, generator=gen())
    again = tuning.find_optimal_codes(target, books, prev, scales, max_update_fraction=0.1, code_selection_temperature=1.0, generator=gen())
    assert torch.equal(first, again) and 0 < int((first != prev).any(-1).sum()) <= int(np.ceil(0.1 * prev.shape[0] * prev.shape[1]))
    changed = (first != prev).any(-1)
    assert torch.equal(first[changed], expected[changed]), "a searched group gets the code the full update gives it"
    # a group whose target is not finite keeps its codes; the others are unaffected
    poisoned = target.clone()
    poisoned[3, 8] = float("nan")
    poisoned[5, 17] = float("inf")
    got = tuning.find_optimal_codes(poisoned, books, prev, scales)
    keep = torch.zeros(prev.shape[:2], dtype=torch.bool)
    keep[3, 1] = keep[5, 2] = True
    assert torch.equal(got[keep], prev[keep]) and torch.equal(got[~keep], expected[~keep])


# ---------------------------------------------------------------------------------------------------------------------------
# 5. update_codes_ on host layers
# ---------------------------------------------------------------------------------------------------------------------------
def _host_layer(golden, case="d"):
    import aqlm

    target, books, prev, scales, options, expected, _ = _golden_case(golden, case)
    K, size, ogs, g = books.shape
    layer = aqlm.QuantizedLinear(target.shape[1], target.shape[0], g, ogs, K, int(np.log2(size)), bias=True, dtype=torch.float32)
    with torch.no_grad():
        layer.codebooks.copy_(books)
        layer.codes.copy_(prev)
        layer.scales.copy_(scales)
        layer.bias.copy_(torch.linspace(-1, 1, target.shape[0]))
    return layer, target, options, expected


def test_update_codes_writes_in_place_and_the_next_forward_uses_the_new_codes(golden):
    import aqlm.tuning as tuning
    from aqlm_amd.utils import _dequantize_weight, unpack_int_data

    layer, target, options, expected = _host_layer(golden)
    x = torch.randn(3, layer.in_features, generator=torch.Generator().manual_seed(1))
    with torch.no_grad():
        y_before = layer(x)
    param, version, old = layer.codes, layer.codes._version, layer.codes.clone()
    changed = tuning.update_codes_(layer, target, **options)
    assert layer.codes is param and layer.codes._version > version and not layer.codes.requires_grad
    assert torch.equal(layer.codes, expected) and not torch.equal(expected, old)
    assert isinstance(changed, torch.Tensor) and changed.dim() == 0 and int(changed) == int((expected != old).any(-1).sum()) > 0
    weight = _dequantize_weight(unpack_int_data(layer.codes, layer.nbits_per_codebook), layer.codebooks, layer.scales)
    with torch.no_grad():
        y = layer(x)
    want = F.linear(x, weight, layer.bias)
    assert torch.allclose(y, want, rtol=1e-5, atol=1e-4) and not torch.allclose(y, y_before, rtol=1e-3, atol=1e-2)
    # the update brought the layer closer to its target, and a second one changes nothing more for a greedy search over one ...
    before = _dequantize_weight(unpack_int_data(old, layer.nbits_per_codebook), layer.codebooks, layer.scales)
    assert float((target - weight).square().sum()) < float((target - before).square().sum())


def test_update_codes_restores_dropped_codes_first(golden):
    import aqlm.tuning as tuning

    layer, target, options, expected = _host_layer(golden)
    calls = []
    restore = layer.restore_canonical_codes
    layer.restore_canonical_codes = lambda: (calls.append(layer.codes._version), restore())[1]
    version = layer.codes._version
    tuning.update_codes_(layer, target, **options)
    assert calls == [version], "restore_canonical_codes runs once, before the codes are written"
    assert torch.equal(layer.codes, expected)


def test_update_codes_refuses_what_make_trainable_skips(golden):
    import aqlm
    import aqlm.tuning as tuning
    from aqlm_amd.moe import QuantizedMixtralExperts
    from aqlm_amd.sharded import ShardedQuantizedLinear

    layer, target, options, _ = _host_layer(golden)
    old = layer.codes.clone()
    for name in ("stochastic_rounding_tau", "force_update"):
        with pytest.raises(NotImplementedError, match=name):
            tuning.update_codes_(layer, target, **{name: True})
    with torch.inference_mode():
        frozen, _, _, _ = _host_layer(golden)
    assert frozen.codes.is_inference()
    kept = frozen.codes
    with pytest.raises(RuntimeError, match="inference tensor"):
        tuning.update_codes_(frozen, target, **options)
    assert frozen.codes is kept
    layer._moe_expert = True
    with pytest.raises(TypeError, match="QuantizedLinear.*expert"):
        tuning.update_codes_(layer, target)
    assert torch.equal(layer.codes, old)
    for cls in (QuantizedMixtralExperts, ShardedQuantizedLinear):
        module = cls.__new__(cls)
        torch.nn.Module.__init__(module)
        with pytest.raises(TypeError, match=cls.__name__):
            tuning.update_codes_(module, target)
    with pytest.raises(TypeError, match="Linear"):
        tuning.update_codes_(torch.nn.Linear(8, 8), target)
    assert aqlm.tuning.find_optimal_codes is tuning.find_optimal_codes


# ---------------------------------------------------------------------------------------------------------------------------
# 6. the code object
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_code_object_holds_the_kernels_without_scratch_or_atomics(tmp_path):
    out = tmp_path / "code_search.s"
    subprocess.run([HIPCC] + ISA_FLAGS + [os.path.join(ROOT, "aqlm_amd", "csrc", "code_search.hip"), "-o", str(out)], check=True,
                   stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=900)
    text = out.read_text()
    pattern = r"_ZN4aqlm\d+(?:code_search_norms|code_search_1x16)_kernel\w+"
    names = set(re.findall(rf"^\s+\.name:\s+({pattern})", text, re.M))
    # the norms and the search for the codebook in fp16 / bf16 x g 8 / 16
    assert len(names) == 8 and sum("norms" in n for n in names) == 4 and sum("search_1x16" in n for n in names) == 4, names
    seen = 0
    for m in re.finditer(rf"\.name:\s+({pattern})(.*?)(?=\n  - |\Z)", text, re.S):
        assert re.search(r"\.private_segment_fixed_size:\s+0\b", m.group(2)), m.group(1)
        assert re.search(r"\.vgpr_spill_count:\s+0\b", m.group(2)) and re.search(r"\.sgpr_spill_count:\s+0\b", m.group(2)), m.group(1)
        seen += 1
    assert seen == 8
    assert re.findall(r"\.max_flat_workgroup_size:\s+(\d+)", text) == ["256"] * 8  # __launch_bounds__(256) on every kernel
    assert "global_atomic" not in text and "flat_atomic" not in text and "buffer_atomic" not in text
    for name in names:
        body = re.split(rf"^{name}:", text, maxsplit=1, flags=re.M)[1].split(".Lfunc_end", 1)[0]
        assert not re.search(r"\bscratch_(load|store)", body), f"{name}: scratch access"
        assert not re.search(r"\bds_(add|sub|inc|dec|min|max|and|or|xor|cmpst|wrxchg)_(rtn_)?[a-z]*\d+\b", body), f"{name}: an LDS atomic"
        mfma = len(re.findall(r"\bv_mfma_f32_32x32x16_(f16|bf16)\b", body))
        if "search_1x16" in name:
            # four group tiles per codeword tile, one instruction each at g 8, two at g 16; the division of r by the scale is IEEE
            assert mfma == (4 if "Li8E" in name else 8), f"{name}: {mfma} MFMAs"
            assert ("v_mfma_f32_32x32x16_f16" in body) == ("3F16" in name) and "v_div_scale_f32" in body and "v_div_fixup_f32" in body, name
            assert "v_min3_f32" in body or "v_pk_min" in body or "v_min_f32" in body, name
        else:
            assert mfma == 0, name
