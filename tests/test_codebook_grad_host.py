"""Training codebooks, scales and biases of quantized layers, the parts that need no GPU: the C ABI of
aqlm_hip_codebook_grad_1x16 / aqlm_hip_scales_grad_1x16 (symbols, the chunk / workspace / support queries, the argument checks on
host buffers in their documented order), the inverted-index builder against a numpy model, the route predicate as a truth table,
the gradients of host layers of four schemes against fp64 autograd through the reference definition, the frozen layer left as it
was, ``make_trainable`` on the tiny Mixtral, and the code object of codebook_grad.hip (fourteen kernels, no scratch)."""
import ctypes
import itertools
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
ISA_FLAGS = ["-O3", "-std=c++17", "--offload-arch=gfx950", "-fPIC", "-ffp-contract=fast", "-mllvm",
             "-amdgpu-kernarg-preload-count=14", "--cuda-device-only", "-S"]  # the Makefile's flags
NEW = ("aqlm_hip_codebook_grad_chunk", "aqlm_hip_codebook_grad_1x16_supported", "aqlm_hip_codebook_grad_1x16_max_chunks",
       "aqlm_hip_codebook_grad_1x16_workspace_bytes", "aqlm_hip_codebook_grad_1x16", "aqlm_hip_scales_grad_1x16_supported",
       "aqlm_hip_scales_grad_1x16")
ENTRIES = 65536


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
    assert nat.F32 == 2 and re.search(r"#define AQLM_HIP_F32 2\b", text)
    from aqlm_amd.inference_kernels import hip_kernel  # noqa: F401  (registers the ops)

    for op in ("codebook_grad_1x16", "scales_grad_1x16"):
        assert hasattr(torch.ops.aqlm, op)
    import aqlm

    assert aqlm.tuning is __import__("aqlm_amd").tuning


def test_chunk_workspace_and_supported_queries():
    from aqlm_amd import _native as nat
    from aqlm_amd.inference_kernels import hip_kernel as hk

    lib = nat.lib
    chunk = lib.aqlm_hip_codebook_grad_chunk()
    assert chunk == hk.CODEBOOK_GRAD_CHUNK and chunk >= 16 and chunk % 16 == 0
    for fn in (lib.aqlm_hip_codebook_grad_1x16_supported, lib.aqlm_hip_scales_grad_1x16_supported):
        assert fn(24, 64, 8) == 1 and fn(40, 192, 16) == 1 and fn(264, 520, 8) == 1 and fn(14336, 4096, 8) == 1 and fn(1, 8, 8) == 1
        for g in (0, 1, 4, 12, 32, -8):
            assert fn(24, 64, g) == 0, g
        assert fn(0, 64, 8) == 0 and fn(24, 0, 8) == 0 and fn(-1, 64, 8) == 0 and fn(24, -64, 8) == 0
        assert fn(24, 60, 8) == 0 and fn(24, 72, 16) == 0  # in_features % g
        assert fn(1 << 20, 1 << 14, 8) == 0                # more codes than a 32-bit position table takes
    mc, ws = lib.aqlm_hip_codebook_grad_1x16_max_chunks, lib.aqlm_hip_codebook_grad_1x16_workspace_bytes
    for out, fin, g in ((24, 64, 8), (40, 192, 16), (264, 520, 8), (4096, 4096, 8), (14336, 4096, 16)):
        n = out * (fin // g)
        assert mc(out, fin, g) == min(n, ENTRIES) + n // chunk
        assert ws(out, fin, g) == mc(out, fin, g) * g * 4
    assert mc(24, 64, 12) == 0 and ws(24, 64, 12) == 0 and mc(0, 64, 8) == 0 and ws(24, 0, 8) == 0


# ---------------------------------------------------------------------------------------------------------------------------
# 2. argument checks, on dummy host pointers: every call returns before a launch
# ---------------------------------------------------------------------------------------------------------------------------
def _host_buffer():
    buf = ctypes.create_string_buffer(1 << 17)
    return buf, (ctypes.addressof(buf) + 15) // 16 * 16


def test_codebook_grad_argument_checks_report_the_documented_codes_in_the_documented_order():
    from aqlm_amd import _native as nat

    buf, p = _host_buffer()
    need = nat.lib.aqlm_hip_codebook_grad_1x16_workspace_bytes(24, 64, 8)
    args = lambda **kw: [kw.get(n, d) for n, d in (  # noqa: E731
        ("dw", p), ("stride", 64), ("dwt", nat.F16), ("scales", p + 4096), ("dt", nat.F16), ("starts", p + 8192), ("order", p + 8192),
        ("chunks", p + 8192), ("cstarts", p + 8192), ("out", 24), ("in", 64), ("g", 8), ("y", p + 16384), ("yt", nat.F32),
        ("ws", p + 32768), ("ws_bytes", need), ("stream", None))]
    call = nat.lib.aqlm_hip_codebook_grad_1x16
    for null in ("dw", "starts", "order", "chunks", "cstarts", "y", "ws"):
        assert call(*args(**{null: None})) == nat.E_INVALID and "null pointer" in nat.last_error(), null
    for name, off in (("dw", p + 8), ("scales", p + 4097), ("starts", p + 8194), ("order", p + 8194), ("chunks", p + 8194),
                      ("cstarts", p + 8194), ("y", p + 16384 + 8), ("ws", p + 32768 + 4)):
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
    for g in (4, 32):
        assert call(*args(g=g)) == nat.E_UNSUPPORTED and "8 or 16 features" in nat.last_error(), g
    assert call(*args(stride=68)) == nat.E_UNSUPPORTED and "shape outside" in nat.last_error()  # 136-byte rows
    assert call(*args(stride=66, dwt=nat.F32)) == nat.E_UNSUPPORTED  # 264-byte rows
    assert call(*args(out=1 << 20, **{"in": 1 << 14, "stride": 1 << 14})) == nat.E_UNSUPPORTED and "shape outside" in nat.last_error()
    # NULL scales are a valid argument: the first complaint is the next one in line
    assert call(*args(scales=None, g=32)) == nat.E_UNSUPPORTED and "8 or 16 features" in nat.last_error()


def test_scales_grad_argument_checks_report_the_documented_codes_in_the_documented_order():
    from aqlm_amd import _native as nat

    buf, p = _host_buffer()
    args = lambda **kw: [kw.get(n, d) for n, d in (  # noqa: E731
        ("dw", p), ("stride", 64), ("dwt", nat.BF16), ("codes", p + 4096), ("cb", p + 8192), ("dt", nat.BF16), ("out", 24), ("in", 64),
        ("g", 8), ("y", p + 16384), ("yt", nat.BF16), ("stream", None))]
    call = nat.lib.aqlm_hip_scales_grad_1x16
    for null in ("dw", "codes", "cb", "y"):
        assert call(*args(**{null: None})) == nat.E_INVALID and "null pointer" in nat.last_error(), null
    for name, off in (("dw", p + 8), ("codes", p + 4097), ("cb", p + 8192 + 8), ("y", p + 16386)):
        assert call(*args(**{name: off})) == nat.E_INVALID and "misaligned" in nat.last_error(), name
    assert call(*args(y=None, g=12)) == nat.E_INVALID and "null pointer" in nat.last_error()
    for bad in ({"out": 0}, {"in": 0}, {"g": 0}, {"in": 60}):
        assert call(*args(**bad)) == nat.E_INVALID and "bad sizes" in nat.last_error(), bad
    assert call(*args(cb=p + 8192 + 8, out=0)) == nat.E_INVALID and "misaligned" in nat.last_error()
    assert call(*args(stride=56)) == nat.E_INVALID and "row stride" in nat.last_error()
    assert call(*args(stride=56, dwt=9)) == nat.E_INVALID, "sizes come before the dtypes"
    for bad in ({"dwt": 3}, {"yt": -1}):
        assert call(*args(**bad)) == nat.E_UNSUPPORTED and "float32" in nat.last_error(), bad
    assert call(*args(dt=nat.F32)) == nat.E_UNSUPPORTED and "float16 and bfloat16" in nat.last_error(), "the codebook is fp16 / bf16"
    assert call(*args(g=32)) == nat.E_UNSUPPORTED and "8 or 16 features" in nat.last_error()
    assert call(*args(stride=68)) == nat.E_UNSUPPORTED and "shape outside" in nat.last_error()
    assert call(*args(out=1 << 20, **{"in": 1 << 14, "stride": 1 << 14})) == nat.E_UNSUPPORTED


# ---------------------------------------------------------------------------------------------------------------------------
# 3. the index builder against a numpy model
# ---------------------------------------------------------------------------------------------------------------------------
def _model_index(codes, chunk):
    """Per entry the ascending positions; the chunk rows in entry order then list order."""
    values = codes.reshape(-1).astype(np.int64) % ENTRIES
    lists = {}
    for pos, v in enumerate(values):  # ascending positions by construction
        lists.setdefault(int(v), []).append(pos)
    order, starts, rows, cstarts = [], [0], [], [0]
    for e in range(ENTRIES):
        lst = lists.get(e, [])
        for b in range(0, len(lst), chunk):
            rows.append((e, len(order) + b, len(order) + min(b + chunk, len(lst))))
        order.extend(lst)
        starts.append(len(order))
        cstarts.append(len(rows))
    return np.array(order), np.array(starts), np.array(rows).reshape(-1, 3), np.array(cstarts)


def _index_cases():
    from aqlm_amd.inference_kernels import hip_kernel as hk

    chunk = hk.CODEBOOK_GRAD_CHUNK
    rng = np.random.default_rng(5)
    uniform = rng.integers(-32768, 32768, size=(24, 8, 1)).astype(np.int16)
    uniform.reshape(-1)[[0, 5, 77, 191]] = (-32768, -1, 0, 32767)
    # entry 1234 has CHUNK + 1 uses, entry 65535 (the container -1) exactly CHUNK, eight other entries one each; shuffled
    boundary = np.full(2 * chunk + 9, 1234, dtype=np.int16)
    boundary[chunk + 1:2 * chunk + 1] = -1
    boundary[2 * chunk + 1:] = (np.arange(8) * 7 - 32768).astype(np.int16)
    boundary = rng.permutation(boundary).reshape(-1, 1, 1)
    equal = np.full((40, 12, 1), -32768, dtype=np.int16)
    return chunk, {"uniform": uniform, "boundary": boundary.astype(np.int16), "equal": equal}


@pytest.mark.parametrize("case", ["uniform", "boundary", "equal"])
def test_index_builder_against_a_numpy_model(case):
    from aqlm_amd.inference_kernels import hip_kernel as hk

    chunk, cases = _index_cases()
    codes = cases[case]
    n = codes.shape[0] * codes.shape[1]
    with torch.inference_mode():  # a checkpoint loaded under inference mode hands over inference tensors
        t = torch.from_numpy(codes.copy())
    index = hk.build_codebook_grad_index(t, 8)
    assert not index.order.is_inference() and index.nbytes() == 4 * (n + 2 * (ENTRIES + 1) + 3 * index.chunks.shape[0])
    order, starts, rows, cstarts = _model_index(codes, chunk)
    assert index.order.dtype == index.starts.dtype == index.chunks.dtype == index.chunk_starts.dtype == torch.int32
    assert np.array_equal(index.order.numpy(), order) and np.array_equal(index.starts.numpy(), starts)
    assert int(index.starts[ENTRIES]) == n and index.starts.shape == (ENTRIES + 1,)
    max_chunks = hk.codebook_grad_max_chunks(codes.shape[0], codes.shape[1] * 8, 8)
    got = index.chunks.numpy()
    assert got.shape == (max_chunks, 3) and len(rows) <= max_chunks
    assert np.array_equal(got[:len(rows)], rows), "entry order, then list order; unused entries absent"
    assert (got[len(rows):, 0] == -1).all() and (got[len(rows):, 1:] == 0).all()
    assert np.array_equal(index.chunk_starts.numpy(), cstarts) and int(index.chunk_starts[ENTRIES]) == len(rows)
    # ascending inside every list, no chunk longer than CHUNK, every position exactly once
    values = codes.reshape(-1).astype(np.int64) % ENTRIES
    o = index.order.numpy()
    for e in np.unique(values):
        lst = o[starts[e]:starts[e + 1]]
        assert (np.diff(lst) > 0).all() and (values[lst] == e).all()
    assert (rows[:, 2] - rows[:, 1] <= chunk).all() and (rows[:, 2] > rows[:, 1]).all()
    covered = np.concatenate([o[b:e] for _, b, e in rows])
    assert np.array_equal(np.sort(covered), np.arange(n))
    if case == "boundary":
        lengths = {int(e): [int(r[2] - r[1]) for r in rows if r[0] == e] for e in (1234, 65535)}
        assert lengths == {1234: [chunk, 1], 65535: [chunk]}
    if case == "equal":
        assert len(rows) == -(-n // chunk) and (rows[:, 0] == 32768).all()


def test_index_is_derived_state_of_the_layer():
    """Keyed on the fingerprint of the codes, forgotten by invalidate_derived_state(), rebuilt when the codes change, not pickled,
    listed by memory_report."""
    import copy
    import pickle

    import aqlm
    from aqlm_amd.checkpoint import memory_report

    layer = _host_layer(1, 16, 1, 8, 64, 24, seed=3)
    a = layer.codebook_grad_index()
    assert layer.codebook_grad_index() is a
    rep = memory_report(torch.nn.Sequential(layer))
    assert rep["codebook_grad_index_layers"] == 1 and rep["codebook_grad_index"] == a.nbytes() >= 4 * layer.codes.numel()
    assert copy.deepcopy(layer)._grad_index is None and pickle.loads(pickle.dumps(layer))._grad_index is None
    layer.invalidate_derived_state()
    assert layer._grad_index is None
    b = layer.codebook_grad_index()
    with torch.no_grad():
        layer.codes[0, 0, 0] += 1  # a versioned write: another fingerprint
    c = layer.codebook_grad_index()
    assert c is not b and not torch.equal(c.starts, b.starts) and isinstance(layer, aqlm.QuantizedLinear)
    layer.codes.data[0, 1, 0] += 1  # behind the version counter's back: the checksum of the codes sees it
    assert layer._derived_checks is not None and "codes" in layer._derived_checks
    assert layer.verify_derived_state() is False and layer._grad_index is None


# ---------------------------------------------------------------------------------------------------------------------------
# 4. the predicate
# ---------------------------------------------------------------------------------------------------------------------------
def test_route_predicate_is_a_pure_table(monkeypatch):
    import aqlm.tuning as tuning

    assert tuning.CODEBOOK_GRAD_KERNEL is True and tuning.CODEBOOK_GRAD_FP32_DW is False
    schemes = ((1, 16, 1, 8), (1, 16, 1, 16), (1, 16, 1, 32), (1, 16, 2, 8), (2, 8, 1, 8), (8, 8, 1, 32), (1, 8, 1, 8), (2, 16, 1, 8))
    for switch in (True, False):
        monkeypatch.setattr(tuning, "CODEBOOK_GRAD_KERNEL", switch)
        for scheme in schemes:
            for on_gpu, dtypes_ok, supported, compiling in itertools.product((False, True), repeat=4):
                want = switch and scheme in ((1, 16, 1, 8), (1, 16, 1, 16)) and on_gpu and dtypes_ok and supported and not compiling
                assert tuning.takes_codebook_grad_kernel(*scheme, on_gpu, dtypes_ok, supported, compiling) is want
    monkeypatch.setattr(tuning, "CODEBOOK_GRAD_KERNEL", True)
    layer = _host_layer(1, 16, 1, 8, 64, 24, seed=3)
    assert layer._takes_codebook_grad_kernel(None) is False and layer._takes_codebook_grad_kernel(torch.zeros(2, 64)) is False  # host
    layer.codebooks.requires_grad_(True)
    assert tuning.param_grad_needed(layer)
    with torch.no_grad():
        assert not tuning.param_grad_needed(layer)


# ---------------------------------------------------------------------------------------------------------------------------
# 5. host layers: gradients of all three parameters (fails without the feature: they were None)
# ---------------------------------------------------------------------------------------------------------------------------
def _host_layer(K, nbits, ogs, g, fin, fout, seed, dtype=torch.float32, bias=True):
    import aqlm

    gen = torch.Generator().manual_seed(seed)
    m = aqlm.QuantizedLinear(fin, fout, g, ogs, K, nbits, bias=bias, dtype=dtype)
    lo, hi = -(2 ** (nbits - 1)), 2 ** (nbits - 1)
    with torch.no_grad():
        m.codes.copy_(torch.randint(lo, hi, m.codes.shape, generator=gen).to(m.codes.dtype))
        m.codebooks.copy_(torch.randn(m.codebooks.shape, generator=gen))
        m.scales.copy_(torch.rand(m.scales.shape, generator=gen) + 0.5)
        if bias:
            m.bias.copy_(torch.randn(m.bias.shape, generator=gen))
    return m


def _definition(x, codes, codebooks, scales, bias, nbits):
    from aqlm_amd.utils import _dequantize_weight

    return torch.nn.functional.linear(x, _dequantize_weight(codes.to(torch.int64) % 2 ** nbits, codebooks, scales), bias)


def _definition_grads(layer, x, wy, dtype, absolute=False, input_grad=True):
    """y and the four gradients of sum(y * wy) through the reference definition in ``dtype``; ``absolute``: of the same expression
    on the absolute values -- the sum of the magnitudes of the terms of every gradient element."""
    f = (lambda t: t.detach().abs()) if absolute else (lambda t: t.detach())
    leaves = [f(t).to(dtype).requires_grad_(True) for t in (x, layer.codebooks, layer.scales, layer.bias)]
    y = _definition(leaves[0], layer.codes, leaves[1], leaves[2], leaves[3], layer.nbits_per_codebook)
    (y * f(wy).to(dtype)).sum().backward()
    return y.detach(), [t.grad for t in leaves][0 if input_grad else 1:]


HOST_SCHEMES = {"1x16g8": (1, 16, 1, 8, 64, 24), "2x8g8": (2, 8, 1, 8, 64, 24), "8x8g32": (8, 8, 1, 32, 64, 16),
                "2x8g4_out2": (2, 8, 2, 4, 32, 12)}


@pytest.mark.parametrize("input_grad", [True, False], ids=["x_grad", "x_frozen"])
@pytest.mark.parametrize("rows", [2, 9])
@pytest.mark.parametrize("scheme", sorted(HOST_SCHEMES))
def test_host_layers_give_every_parameter_its_gradient(scheme, rows, input_grad):
    import aqlm.tuning as tuning

    K, nbits, ogs, g, fin, fout = HOST_SCHEMES[scheme]
    layer = _host_layer(K, nbits, ogs, g, fin, fout, seed=11)
    params = tuning.make_trainable(torch.nn.Sequential(layer), bias=True)
    assert len(params) == 3 and all(p.requires_grad for p in params) and not layer.codes.requires_grad
    gen = torch.Generator().manual_seed(rows)
    x = torch.randn((rows, fin), generator=gen).requires_grad_(input_grad)
    wy = torch.randn((rows, fout), generator=gen)
    y = layer(x)
    assert y.requires_grad
    (y * wy).sum().backward()
    got = ([x.grad] if input_grad else []) + [layer.codebooks.grad, layer.scales.grad, layer.bias.grad]
    assert all(t is not None for t in got) and (input_grad or x.grad is None)
    # the host route IS the reference definition: bit for bit the fp32 run of it
    y32, same = _definition_grads(layer, x, wy, torch.float32, input_grad=input_grad)
    assert torch.equal(y.detach(), y32)
    for a, b in zip(got, same):
        assert a.dtype == torch.float32 and a.shape == b.shape and torch.equal(a, b)
    # ... and fp64 autograd through it, to within the fp32 rounding of that computation: every gradient element is a sum of at
    # most N = rows * in_features * K products of at most 4 factors, so |error| <= (N + 4) * 2^-24 * (sum of the terms' magnitudes)
    _, exact = _definition_grads(layer, x, wy, torch.float64, input_grad=input_grad)
    _, magnitude = _definition_grads(layer, x, wy, torch.float64, absolute=True, input_grad=input_grad)
    n_terms = rows * fin * K + 4
    for a, e, mag in zip(got, exact, magnitude):
        assert ((a.double() - e).abs() <= n_terms * 2.0 ** -24 * mag + 1e-300).all()
    assert layer.codebooks.grad.abs().sum() > 0 and layer.scales.grad.abs().sum() > 0
    # an optimizer steps on something now
    before = layer.codebooks.detach().clone()
    torch.optim.SGD(params, lr=0.1).step()
    assert not torch.equal(before, layer.codebooks.detach())


# ---------------------------------------------------------------------------------------------------------------------------
# 6. a frozen layer is untouched
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [2, 9])
@pytest.mark.parametrize("scheme", ["1x16g8", "2x8g8"])
def test_frozen_layer_keeps_its_op_and_its_grad_input(scheme, rows):
    from aqlm_amd.inference_kernels import get_backward_pass_kernel

    K, nbits, ogs, g, fin, fout = HOST_SCHEMES[scheme]
    layer = _host_layer(K, nbits, ogs, g, fin, fout, seed=12)
    gen = torch.Generator().manual_seed(rows)
    x = torch.randn((rows, fin), generator=gen).requires_grad_(True)
    wy = torch.randn((rows, fout), generator=gen)
    y = layer(x)
    assert type(y.grad_fn).__name__ == "_QuantizedMatmulBackward"
    (y * wy).sum().backward()
    want = get_backward_pass_kernel(layer.codebooks, rows > 6)(wy.contiguous(), layer.codes, layer.codebooks, layer.scales, None)
    assert torch.equal(x.grad, want)
    assert layer.codebooks.grad is None and layer.scales.grad is None and layer.bias.grad is None and layer._grad_index is None
    # trainable parameters under no_grad: the frozen routes, the same bits
    layer.codebooks.requires_grad_(True)
    with torch.no_grad():
        assert torch.equal(layer(x.detach()), y.detach())


# ---------------------------------------------------------------------------------------------------------------------------
# 7. make_trainable on the tiny Mixtral
# ---------------------------------------------------------------------------------------------------------------------------
def test_make_trainable_returns_the_dense_layers_and_skips_the_expert_blocks():
    pytest.importorskip("transformers")
    from transformers import MixtralForCausalLM

    import aqlm
    from aqlm_amd.moe import replace_moe_experts
    from tests import moe_checkpoint as mc

    torch.manual_seed(0)
    model = MixtralForCausalLM(mc.config())
    assert replace_moe_experts(model, mc.SCHEME) == mc.LAYERS
    q = aqlm.QuantizedLinear(mc.HID, mc.HID, 8, 1, 1, 16, bias=True)
    model.model.layers[0].self_attn.q_proj = q
    params = aqlm.tuning.make_trainable(model)
    assert [id(p) for p in params] == [id(q.codebooks), id(q.scales)] and not q.bias.requires_grad and not q.codes.requires_grad
    assert params.skipped == [f"model.layers.{i}.mlp.experts" for i in range(mc.LAYERS)]
    block = model.model.layers[0].mlp.experts
    assert not any(p.requires_grad for p in block.parameters())
    params = aqlm.tuning.make_trainable(model, codebooks=False, scales=False, bias=True)
    assert [id(p) for p in params] == [id(q.bias)]
    assert aqlm.tuning.prepare(model) == 0  # host layers take the torch route: nothing to build


# ---------------------------------------------------------------------------------------------------------------------------
# 8. the code object
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_code_object_holds_the_kernels_without_scratch(tmp_path):
    out = tmp_path / "codebook_grad.s"
    subprocess.run([HIPCC] + ISA_FLAGS + [os.path.join(ROOT, "aqlm_amd", "csrc", "codebook_grad.hip"), "-o", str(out)], check=True,
                   stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=900)
    text = out.read_text()
    pattern = r"_ZN4aqlm\d+(?:codebook_grad_chunk|codebook_grad_finish|scales_grad)_kernel\w+"
    names = set(re.findall(rf"^\s+\.name:\s+({pattern})", text, re.M))
    # the chunk sum and the scale gradient for dW in fp16 / bf16 / fp32 x g 8 / 16, the finish launch for g 8 / 16
    assert len(names) == 14, names
    assert sum("chunk" in n for n in names) == 6 and sum("scales_grad" in n for n in names) == 6 and sum("finish" in n for n in names) == 2
    seen = 0
    for m in re.finditer(rf"\.name:\s+({pattern})(.*?)(?=\n  - |\Z)", text, re.S):
        assert re.search(r"\.private_segment_fixed_size:\s+0\b", m.group(2)), m.group(1)
        assert re.search(r"\.vgpr_spill_count:\s+0\b", m.group(2)), m.group(1)
        seen += 1
    assert seen == 14
    for name in names:
        body = re.split(rf"^{name}:", text, maxsplit=1, flags=re.M)[1].split(".Lfunc_end", 1)[0]
        assert not re.search(r"\bscratch_(load|store)", body), f"{name}: scratch access"
        assert "_atomic" not in body and not re.search(r"\bds_(add|cmpst|min|max)_", body), f"{name}: an atomic"
