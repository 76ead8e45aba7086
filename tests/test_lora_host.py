"""LoRA adapters on quantized layers, the parts that need no GPU: the PEFT-format loader (key mapping, scaling, refusals by name,
state_dict names, detach), ``LoraQuantizedLinear`` on a small host layer (torch path) against an fp64 evaluation of the definition,
gradients of x, A and B against fp64 autograd, the route predicate as a truth table, the C ABI of aqlm_hip_lora_bgmv (struct size,
workspace size, argument checks), and the resource report of the two new kernels (no scratch, no FLAT access)."""
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

from oracle import aqlm_oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
ISA_FLAGS = ["-O3", "-std=c++17", "--offload-arch=gfx950", "-fPIC", "-ffp-contract=fast", "-mllvm",
             "-amdgpu-kernarg-preload-count=14", "--cuda-device-only", "-S"]
FIN, FOUT = 64, 24


def _layer(seed, fin=FIN, fout=FOUT, dtype=torch.float32):
    import aqlm

    L = orc.make_layer(seed, fin, fout, 2, 8, 8, batch=1, bias=True, float_dtype=np.float32)
    m = aqlm.QuantizedLinear(fin, fout, 8, 1, 2, 8, bias=True, dtype=dtype)
    with torch.no_grad():
        m.codes.copy_(torch.from_numpy(L["codes"]))
        m.codebooks.copy_(torch.from_numpy(L["codebooks"]).to(dtype))
        m.scales.copy_(torch.from_numpy(L["scales"]).to(dtype))
        m.bias.copy_(torch.from_numpy(L["bias"]).to(dtype))
    # W^T in fp64 from the oracle: the layer applied to the identity, without the bias
    w64 = torch.from_numpy(orc.dequantize_gemm(np.eye(fin, dtype=np.float32), L["codes"], L["codebooks"], L["scales"], None)).double().T
    return m, w64.contiguous(), torch.from_numpy(L["bias"]).double()


class _Attn(torch.nn.Module):
    def __init__(self, seed):
        super().__init__()
        self.q_proj, _, _ = _layer(seed)
        self.v_proj, _, _ = _layer(seed + 1)
        self.o_proj = torch.nn.Linear(FOUT, FIN, bias=False)


class _Model(torch.nn.Module):
    """model.layers.N.self_attn.{q,v}_proj, as a Hugging Face decoder names them."""

    def __init__(self):
        super().__init__()
        self.model = torch.nn.Module()
        self.model.layers = torch.nn.ModuleList()
        for i in range(2):
            layer = torch.nn.Module()
            layer.self_attn = _Attn(10 * i + 1)
            self.model.layers.append(layer)


def _state(seed, r, paths, fin=FIN, fout=FOUT):
    gen = torch.Generator().manual_seed(seed)
    state = {}
    for p in paths:
        state[f"base_model.model.{p}.lora_A.weight"] = torch.randn((r, fin), generator=gen) / fin ** 0.5
        state[f"base_model.model.{p}.lora_B.weight"] = torch.randn((fout, r), generator=gen) / r ** 0.5
    return state


def _config(r, alpha, **extra):
    return dict({"peft_type": "LORA", "r": r, "lora_alpha": alpha, "bias": "none", "target_modules": ["q_proj", "v_proj"],
                 "use_rslora": False, "use_dora": False, "modules_to_save": None, "rank_pattern": {}, "alpha_pattern": {}}, **extra)


def _write_dir(path, state, config):
    from safetensors.torch import save_file

    os.makedirs(path)
    save_file({k: v.contiguous() for k, v in state.items()}, os.path.join(path, "adapter_model.safetensors"))
    with open(os.path.join(path, "adapter_config.json"), "w") as f:
        json.dump(config, f)
    return str(path)


QV = [f"model.layers.{i}.self_attn.{n}" for i in range(2) for n in ("q_proj", "v_proj")]


def test_loader_maps_keys_scales_and_round_trips_peft_names(tmp_path):
    import aqlm
    import aqlm.lora as lora

    assert lora is aqlm.lora and "lora" in aqlm_amd_all()
    model = _Model()
    originals = {p: model.get_submodule(p) for p in QV}
    s_math, s_code = _state(1, 8, QV), _state(2, 16, QV[:1])
    bank = lora.attach_adapters(model, {"math": _write_dir(tmp_path / "math", s_math, _config(8, 32)),
                                        "code": (s_code, _config(16, 8, use_rslora=True))})
    assert bank.names == ["math", "code"] and model._aqlm_adapter_bank is bank
    for p in QV:
        w = model.get_submodule(p)
        assert isinstance(w, lora.LoraQuantizedLinear) and w.base_layer is originals[p]
        assert torch.equal(w.lora_A["math"].weight, s_math[f"base_model.model.{p}.lora_A.weight"])
        assert torch.equal(w.lora_B["math"].weight, s_math[f"base_model.model.{p}.lora_B.weight"])
        assert w.scaling["math"] == 32 / 8                      # alpha / r
        assert not w.lora_A["math"].weight.requires_grad and w.lora_A["math"].bias is None
        assert ("code" in w.lora_A) == (p == QV[0])             # "code" targets one layer only
    w0 = model.get_submodule(QV[0])
    assert w0.scaling["code"] == pytest.approx(8 / 16 ** 0.5)   # rslora: alpha / sqrt(r)
    assert torch.equal(w0.lora_B["code"].weight, s_code[f"base_model.model.{QV[0]}.lora_B.weight"])
    assert isinstance(model.model.layers[0].self_attn.o_proj, torch.nn.Linear)  # not targeted: left alone
    keys = set(model.state_dict())
    for p in QV:  # PEFT's names
        assert {f"{p}.lora_A.math.weight", f"{p}.lora_B.math.weight", f"{p}.base_layer.codes", f"{p}.base_layer.codebooks",
                f"{p}.base_layer.scales", f"{p}.base_layer.bias"} <= keys
    assert f"{QV[0]}.lora_A.code.weight" in keys and f"{QV[1]}.lora_A.code.weight" not in keys
    with pytest.raises(RuntimeError, match="already attached"):
        lora.attach_adapters(model, {"again": (s_math, _config(8, 8))})
    lora.detach_adapters(model)
    assert all(model.get_submodule(p) is originals[p] for p in QV) and model._aqlm_adapter_bank is None
    assert not any("lora_" in k for k in model.state_dict())
    # target_modules restricts the layers
    bank = lora.attach_adapters(model, {"math": (s_math, _config(8, 32))}, target_modules=["v_proj"])
    assert [isinstance(model.get_submodule(p), lora.LoraQuantizedLinear) for p in QV] == [False, True, False, True]
    lora.detach_adapters(model)


def aqlm_amd_all():
    import aqlm_amd

    return aqlm_amd.__all__


@pytest.mark.parametrize("extra,exc,message", [
    ({"use_dora": True}, NotImplementedError, "use_dora"),
    ({"bias": "all"}, NotImplementedError, "bias='all'"),
    ({"modules_to_save": ["lm_head"]}, NotImplementedError, "modules_to_save"),
    ({"rank_pattern": {"q_proj": 4}}, NotImplementedError, "rank_pattern"),
    ({"alpha_pattern": {"q_proj": 4}}, NotImplementedError, "alpha_pattern"),
])
def test_loader_refuses_by_name_what_it_does_not_implement(extra, exc, message):
    import aqlm.lora as lora

    model = _Model()
    with pytest.raises(exc, match=re.escape(message)):
        lora.attach_adapters(model, {"x": (_state(1, 8, QV), _config(8, 8, **extra))})
    assert not any(isinstance(m, lora.LoraQuantizedLinear) for m in model.modules())  # nothing was wrapped


def test_loader_refuses_other_targets_and_routed_experts():
    import aqlm.lora as lora

    model = _Model()
    o = "model.layers.0.self_attn.o_proj"
    with pytest.raises(TypeError, match="not a QuantizedLinear"):
        lora.attach_adapters(model, {"x": (_state(1, 8, [o], FOUT, FIN), _config(8, 8))})
    with pytest.raises(ValueError, match="no module"):
        lora.attach_adapters(model, {"x": (_state(1, 8, ["model.layers.7.self_attn.q_proj"]), _config(8, 8))})
    with pytest.raises(NotImplementedError, match="lora_embedding_A"):
        lora.attach_adapters(model, {"x": ({"base_model.model.model.embed.lora_embedding_A": torch.zeros(8, 4)}, _config(8, 8))})
    with pytest.raises(ValueError, match="r=16"):
        lora.attach_adapters(model, {"x": (_state(1, 8, QV), _config(16, 8))})
    model.get_submodule(QV[0])._moe_expert = True
    with pytest.raises(NotImplementedError, match="routed experts are not supported"):
        lora.attach_adapters(model, {"x": (_state(1, 8, QV), _config(8, 8))})
    assert not any(isinstance(m, lora.LoraQuantizedLinear) for m in model.modules())


# ---------------------------------------------------------------------------------------------------------------------------
# the wrapper on a host layer: torch path against fp64
# ---------------------------------------------------------------------------------------------------------------------------
def _wrapped(ranks=(8, 24, 16)):
    import aqlm.lora as lora

    base, w64, b64 = _layer(3)
    block = torch.nn.Module()
    block.proj = base
    ads = {}
    for i, r in enumerate(ranks):
        ads[f"ad{i}"] = (_state(20 + i, r, ["proj"]), _config(r, 2 * r + i))
    bank = lora.attach_adapters(block, ads)
    return block, bank, w64, b64


def _ref64(block, x, ids, w64, b64):
    w = block.proj
    x64 = x.double().reshape(-1, x.shape[-1])
    y = x64 @ w64.T + b64
    for b, a in enumerate(ids):
        if 0 <= a < len(w.bank.names):
            A, B, s = w._weights(w.bank.names[a])
            y[b] += s * (B.double() @ (A.double() @ x64[b]))
    return y.reshape(x.shape[:-1] + (y.shape[-1],))


def _close(y, y64):
    err = float((y.double() - y64).abs().mean() / y64.abs().mean())
    assert err < 1e-5, err  # the host path's tolerance (tests/test_cpu_path.py): fp32 maths against the fp64 oracle


def test_wrapper_on_a_host_layer_matches_fp64_for_every_selection():
    block, bank, w64, b64 = _wrapped()
    gen = torch.Generator().manual_seed(7)
    x = torch.randn((5, FIN), generator=gen)
    with torch.no_grad():
        bare = block.proj.base_layer(x)
        assert torch.equal(block.proj(x), bare)                  # nothing selected yet
        bank.select("ad1")
        _close(block.proj(x), _ref64(block, x, [1] * 5, w64, b64))
        ids = [2, -1, 0, 3, 1]                                   # -1 and len(bank) are out of range: base rows
        for dt in (torch.int64, torch.int32):
            bank.select(torch.tensor(ids, dtype=dt))
            y = block.proj(x)
            _close(y, _ref64(block, x, ids, w64, b64))
            assert torch.equal(y[1], bare[1]) and torch.equal(y[3], bare[3]) and not torch.equal(y[0], bare[0])
        bank.select(None)
        assert torch.equal(block.proj(x), bare)
        # per-sequence ids of a [B, S, K] input are broadcast over S
        x3 = torch.randn((3, 4, FIN), generator=gen)
        seq = [1, 5, 0]
        bank.select(torch.tensor(seq))
        y3 = block.proj(x3)
        assert y3.shape == (3, 4, FOUT)
        _close(y3, _ref64(block, x3, [s for s in seq for _ in range(4)], w64, b64))
        bank.select(torch.tensor([0, 1]))
        with pytest.raises(ValueError, match="one per row"):
            block.proj(x3)
    with pytest.raises(KeyError, match="no adapter named"):
        bank.select("nope")
    with pytest.raises(ValueError, match="1-D int64 / int32"):
        bank.select(torch.zeros(3))


def test_gradients_of_x_a_and_b_match_fp64_autograd():
    block, bank, w64, b64 = _wrapped()
    w = block.proj
    for p in list(w.lora_A.parameters()) + list(w.lora_B.parameters()):
        p.requires_grad_(True)
    ids = [2, 0, 7, 1, 0]
    bank.select(torch.tensor(ids))
    gen = torch.Generator().manual_seed(8)
    x = torch.randn((5, FIN), generator=gen, requires_grad=True)
    gy = torch.randn((5, FOUT), generator=gen)
    (w(x) * gy).sum().backward()
    # the same function in fp64
    x64 = x.detach().double().requires_grad_(True)
    leaves = {n: (w.lora_A[n].weight.detach().double().requires_grad_(True), w.lora_B[n].weight.detach().double().requires_grad_(True))
              for n in bank.names}
    y = x64 @ w64.T + b64
    rows = []
    for b, a in enumerate(ids):
        row = y[b]
        if 0 <= a < len(bank.names):
            A, B = leaves[bank.names[a]]
            row = row + w.scaling[bank.names[a]] * (B @ (A @ x64[b]))
        rows.append(row)
    (torch.stack(rows) * gy.double()).sum().backward()

    def close(g, g64, what):
        assert g is not None, what
        err = float((g.double() - g64).abs().max() / g64.abs().max())
        assert err < 1e-4, (what, err)  # the host backward's tolerance in tests/test_cpu_path.py is rtol 1e-4

    close(x.grad, x64.grad, "x")
    for n in bank.names:
        close(w.lora_A[n].weight.grad, leaves[n][0].grad, f"A {n}")
        close(w.lora_B[n].weight.grad, leaves[n][1].grad, f"B {n}")
    assert all(p.grad is None for p in w.base_layer.parameters())


def test_route_predicate_is_a_pure_table(monkeypatch):
    import aqlm.lora as lora
    from aqlm_amd import _native as nat

    assert lora.AQLM_HIP_MAX_LORA_ROWS == nat.MAX_LORA_ROWS == 256
    assert re.search(r"#define AQLM_HIP_MAX_LORA_ROWS 256\b", open(os.path.join(ROOT, "include", "aqlm_hip.h")).read())
    monkeypatch.setattr(lora, "BGMV_MAX_ROWS", 16)
    for cuda, dtype_ok, grad, compiling, supported in itertools.product((False, True), repeat=5):
        for rows in (0, 1, 16, 17):
            want = cuda and dtype_ok and not grad and not compiling and supported and 1 <= rows <= 16
            assert lora.takes_bgmv_route(cuda, dtype_ok, grad, compiling, rows, supported) is want
    monkeypatch.setattr(lora, "BGMV_MAX_ROWS", 0)  # switched off
    assert not any(lora.takes_bgmv_route(True, True, False, False, rows, True) for rows in (1, 2, 64))
    monkeypatch.setattr(lora, "BGMV_MAX_ROWS", 10_000)  # never beyond what one launch takes
    assert lora.takes_bgmv_route(True, True, False, False, 256, True)
    assert not lora.takes_bgmv_route(True, True, False, False, 257, True)


# ---------------------------------------------------------------------------------------------------------------------------
# C ABI without a GPU
# ---------------------------------------------------------------------------------------------------------------------------
def test_lora_abi_header_bindings_struct_and_argument_checks():
    from aqlm_amd import _native as nat

    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "aqlm_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(aqlm_hip_[a-z0-9_]+)\s*\(", text))
    raw = ctypes.CDLL(nat.LIB_PATH)
    for name in ("aqlm_hip_lora_bgmv", "aqlm_hip_lora_bgmv_supported", "aqlm_hip_lora_workspace_bytes"):
        assert name in declared and name in nat.SIGNATURES and hasattr(raw, name), name
    assert nat.lib.aqlm_hip_abi_version() == nat.ABI_VERSION == 9
    assert ctypes.sizeof(nat.LoraEntry) == 24 and nat.LORA_ENTRY_WORDS == 3
    assert nat.LoraEntry.rank.offset == 16 and nat.LoraEntry.scaling.offset == 20

    L = nat.lib
    assert L.aqlm_hip_lora_workspace_bytes(3, 16) == 192
    assert L.aqlm_hip_lora_workspace_bytes(256, 128) == 256 * 128 * 4
    assert L.aqlm_hip_lora_workspace_bytes(257, 16) == 0 and L.aqlm_hip_lora_workspace_bytes(3, 12) == 0
    assert L.aqlm_hip_lora_bgmv_supported(300, 520, 24, 70) == 1 and L.aqlm_hip_lora_bgmv_supported(1, 8, 8, 1) == 1
    assert L.aqlm_hip_lora_bgmv_supported(300, 516, 24, 70) == 0 and L.aqlm_hip_lora_bgmv_supported(300, 520, 136, 70) == 0

    buf = ctypes.create_string_buffer(1 << 16)
    p = (ctypes.addressof(buf) + 15) // 16 * 16
    need = 4 * 16 * 4
    args = lambda **kw: [kw.get(n, d) for n, d in (  # noqa: E731
        ("table", p), ("n", 2), ("max_rank", 16), ("ids", p + 1024), ("i64", 1), ("rows", 4), ("x", p + 4096), ("xs", 512),
        ("y", p + 16384), ("ys", 300), ("out", 300), ("in", 512), ("dt", nat.F16), ("ws", p + 32768), ("ws_bytes", need),
        ("stream", None))]
    call = L.aqlm_hip_lora_bgmv
    for null in ("table", "x", "y", "ws"):
        assert call(*args(**{null: None})) == nat.E_INVALID and "null pointer" in nat.last_error(), null
    assert call(*args(y=p + 4096)) == nat.E_INVALID and "aliases x" in nat.last_error()          # y == x
    assert call(*args(y=p + 4096 + 512)) == nat.E_INVALID and "aliases x" in nat.last_error()    # y inside x
    assert call(*args(ws_bytes=need - 4)) == nat.E_INVALID and f"{need} bytes needed" in nat.last_error()
    assert call(*args(ws=p + 32768 + 8)) == nat.E_INVALID and "misaligned" in nat.last_error()
    assert call(*args(ids=p + 1028)) == nat.E_INVALID and "misaligned" in nat.last_error()
    assert call(*args(y=p + 16385)) == nat.E_INVALID and "misaligned" in nat.last_error()
    assert call(*args(ys=299)) == nat.E_INVALID and "strides" in nat.last_error()
    assert call(*args(rows=0)) == nat.E_INVALID
    assert call(*args(max_rank=12, ws_bytes=1 << 14)) == nat.E_UNSUPPORTED and "multiple of 8" in nat.last_error()
    assert call(*args(max_rank=136, ws_bytes=1 << 14)) == nat.E_UNSUPPORTED
    assert call(*args(**{"in": 516, "xs": 520})) == nat.E_UNSUPPORTED
    assert call(*args(rows=257, xs=8, **{"in": 8}, ys=8, out=8, ws_bytes=1 << 15)) == nat.E_UNSUPPORTED
    assert call(*args(x=p + 4096 + 8)) == nat.E_UNSUPPORTED and "16-byte aligned" in nat.last_error()
    assert call(*args(dt=2)) == nat.E_UNSUPPORTED and "float16 and bfloat16" in nat.last_error()


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_lora_kernels_use_no_scratch_and_no_flat_access(tmp_path):
    out = tmp_path / "lora_bgmv.s"
    subprocess.run([HIPCC] + ISA_FLAGS + [os.path.join(ROOT, "aqlm_amd", "csrc", "lora_bgmv.hip"), "-o", str(out)], check=True,
                   stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=900)
    text = out.read_text()
    pattern = r"_ZN4aqlm\d+lora_(?:shrink|expand)_kernel\w+"
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
        assert not re.search(r"\b(scratch_|flat_)(load|store)", body), f"{name}: scratch or FLAT access"
