"""LoRA adapters on the routed Mixtral experts, the parts that need no GPU: the C ABI of aqlm_hip_lora_bgmv_routed (symbols,
workspace size, argument checks on a host buffer), the resource report of its two kernels (no scratch, no FLAT access), the loader
on the tiny Mixtral of tests/moe_checkpoint.py (expert keys in both spellings, partial coverage, expert + dense targets, refusals,
state_dict names, detach), ``LoraQuantizedMixtralExperts`` on that host block (per-expert loop + torch path, fp32) against an fp64
evaluation of the block definition with adapters, gradients of hidden_states, A and B against fp64 autograd, and the route
predicate as a truth table."""
import ctypes
import itertools
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

transformers = pytest.importorskip("transformers")

from oracle import aqlm_oracle as orc  # noqa: E402
from tests import moe_checkpoint as mc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
ISA_FLAGS = ["-O3", "-std=c++17", "--offload-arch=gfx950", "-fPIC", "-ffp-contract=fast", "-mllvm",
             "-amdgpu-kernarg-preload-count=14", "--cuda-device-only", "-S"]  # the flags of tests/test_lora_host.py
NEW = ("aqlm_hip_lora_bgmv_routed", "aqlm_hip_lora_bgmv_routed_supported", "aqlm_hip_lora_bgmv_routed_workspace_bytes")


# ---------------------------------------------------------------------------------------------------------------------------
# C ABI without a GPU
# ---------------------------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_bound_and_exported_and_the_abi_version_stays():
    from aqlm_amd import _native as nat

    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "aqlm_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(aqlm_hip_[a-z0-9_]+)\s*\(", text))
    raw = ctypes.CDLL(nat.LIB_PATH)
    for name in NEW:
        assert name in declared and name in nat.SIGNATURES and hasattr(raw, name), name
    assert nat.lib.aqlm_hip_abi_version() == nat.ABI_VERSION == 9


def test_workspace_size_and_supported_query():
    from aqlm_amd import _native as nat

    ws, ok = nat.lib.aqlm_hip_lora_bgmv_routed_workspace_bytes, nat.lib.aqlm_hip_lora_bgmv_routed_supported
    assert ws(6, 2, 16) == 6 * 2 * 16 * 4 and ws(256, 2, 128) == 256 * 2 * 128 * 4 and ws(1, 1, 8) == 32
    assert ws(257, 1, 16) == 0 and ws(6, 3, 16) == 0 and ws(6, 0, 16) == 0 and ws(6, 2, 12) == 0 and ws(0, 1, 16) == 0
    assert ok(300, 520, 24, 256, 4, 2) == 1 and ok(1, 8, 8, 1, 1, 1) == 1 and ok(300, 520, 128, 2, nat.MAX_ROUTED_EXPERTS, 1) == 1
    assert ok(300, 516, 24, 6, 4, 2) == 0 and ok(300, 520, 136, 6, 4, 2) == 0 and ok(300, 520, 24, 257, 4, 2) == 0
    assert ok(300, 520, 24, 6, nat.MAX_ROUTED_EXPERTS + 1, 2) == 0 and ok(300, 520, 24, 6, 4, 3) == 0


def test_argument_checks_report_the_documented_codes_and_messages():
    from aqlm_amd import _native as nat

    buf = ctypes.create_string_buffer(1 << 17)
    p = (ctypes.addressof(buf) + 15) // 16 * 16
    need = 4 * 2 * 16 * 4
    args = lambda **kw: [kw.get(n, d) for n, d in (  # noqa: E731
        ("table", p), ("n", 2), ("E", 4), ("S", 2), ("max_rank", 16), ("aids", p + 2048), ("a64", 1), ("eids", p + 3072), ("e64", 1),
        ("pairs", 4), ("k", 2), ("x", p + 4096), ("xs", 512), ("per_pair", 0), ("y", p + 16384), ("out", 300), ("in", 512),
        ("dt", nat.F16), ("ws", p + 65536), ("ws_bytes", need), ("stream", None))]
    call = nat.lib.aqlm_hip_lora_bgmv_routed
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
    # the y extent is pairs x S rows: its LAST row (pair 3, segment 1) reaches x here, row 0 does not
    assert call(*args(y=p + 32768 - 7 * 300 * 2 - 16, x=p + 32768)) == nat.E_INVALID and "aliases x" in nat.last_error()
    assert call(*args(ws_bytes=need - 4)) == nat.E_INVALID and f"{need} bytes needed" in nat.last_error()
    assert call(*args(pairs=257, k=1, xs=8, **{"in": 8}, out=8, ws_bytes=1 << 16)) == nat.E_UNSUPPORTED and "shape outside" in nat.last_error()
    assert call(*args(max_rank=12)) == nat.E_UNSUPPORTED and "multiple of 8" in nat.last_error()
    assert call(*args(**{"in": 100, "xs": 104})) == nat.E_UNSUPPORTED
    assert call(*args(S=3, ws_bytes=1 << 16)) == nat.E_UNSUPPORTED and "segments" in nat.last_error()
    assert call(*args(E=nat.MAX_ROUTED_EXPERTS + 1)) == nat.E_UNSUPPORTED
    assert call(*args(x=p + 4096 + 8)) == nat.E_UNSUPPORTED and "16-byte aligned" in nat.last_error()
    assert call(*args(dt=2)) == nat.E_UNSUPPORTED and "float16 and bfloat16" in nat.last_error()


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_routed_lora_kernels_use_no_scratch_and_no_flat_access(tmp_path):
    out = tmp_path / "lora_bgmv_routed.s"
    subprocess.run([HIPCC] + ISA_FLAGS + [os.path.join(ROOT, "aqlm_amd", "csrc", "lora_bgmv_routed.hip"), "-o", str(out)], check=True,
                   stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=900)
    text = out.read_text()
    pattern = r"_ZN4aqlm\d+lora_routed_(?:shrink|expand)_kernel\w+"
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


def test_route_predicate_is_a_pure_table(monkeypatch):
    import aqlm.lora as lora

    monkeypatch.setattr(lora, "ROUTED_BGMV_MAX_PAIRS", 16)
    for cuda, dtype_ok, grad, compiling, supported in itertools.product((False, True), repeat=5):
        for pairs in (0, 1, 16, 17):
            want = cuda and dtype_ok and not grad and not compiling and supported and 1 <= pairs <= 16
            assert lora.takes_routed_bgmv_route(cuda, dtype_ok, grad, compiling, pairs, supported) is want
    monkeypatch.setattr(lora, "ROUTED_BGMV_MAX_PAIRS", 0)  # switched off
    assert not any(lora.takes_routed_bgmv_route(True, True, False, False, pairs, True) for pairs in (1, 2, 64))
    monkeypatch.setattr(lora, "ROUTED_BGMV_MAX_PAIRS", 10_000)  # never beyond what one launch takes
    assert lora.takes_routed_bgmv_route(True, True, False, False, 256, True)
    assert not lora.takes_routed_bgmv_route(True, True, False, False, 257, True)


# ---------------------------------------------------------------------------------------------------------------------------
# the tiny Mixtral on the host
# ---------------------------------------------------------------------------------------------------------------------------
def _fill(lin, seed):
    """Codes, codebooks and scales of one 1x16 g8 layer (fp32 parameters) -> its dense W in fp64 [out, in]."""
    L = orc.make_layer(seed, lin.in_features, lin.out_features, 1, 16, 8, batch=1, bias=False, edge_codes=False)
    cb = (L["codebooks"].astype(np.float32) * 0.05).astype(np.float16).astype(np.float32)
    sc = (np.abs(L["scales"].astype(np.float32)) * 0.2 + 0.05).astype(np.float16).astype(np.float32)
    with torch.no_grad():
        lin.codes.copy_(torch.from_numpy(L["codes"]))
        lin.codebooks.copy_(torch.from_numpy(cb))
        lin.scales.copy_(torch.from_numpy(sc))
    return torch.from_numpy(orc.dequantize_weight(L["codes_unsigned"], cb, sc).astype(np.float64))


@pytest.fixture(scope="module")
def tiny():
    """The tiny Mixtral (fp32, host) with quantized experts (``replace_moe_experts``) and a quantized q_proj in layer 0; the
    dense fp64 W of every expert layer of layer 0.  Never modified: every test attaches to a deep copy."""
    from transformers import MixtralForCausalLM

    import aqlm
    from aqlm_amd.moe import replace_moe_experts

    torch.manual_seed(0)
    model = MixtralForCausalLM(mc.config())
    assert replace_moe_experts(model, mc.SCHEME) == mc.LAYERS
    dense = {}
    seed = 700
    for li in range(mc.LAYERS):
        block = model.model.layers[li].mlp.experts
        for e in range(mc.EXPERTS):
            for w in ("w1", "w3", "w2"):
                seed += 1
                W = _fill(getattr(block.expert(e), w), seed)
                if li == 0:
                    dense[(e, w)] = W
    q = aqlm.QuantizedLinear(mc.HID, mc.HID, 8, 1, 1, 16, bias=False)
    _fill(q, 999)
    model.model.layers[0].self_attn.q_proj = q
    return model, dense


def _copy(tiny):
    import copy

    return copy.deepcopy(tiny[0])


BLOCK = "model.layers.0.mlp.experts"
SHAPES = {"w1": (mc.HID, mc.INTER), "w3": (mc.HID, mc.INTER), "w2": (mc.INTER, mc.HID)}  # (in, out)


def _state(seed, r, targets):
    """targets: (module path, in_features, out_features) -> a PEFT adapter state dict of rank r."""
    gen = torch.Generator().manual_seed(seed)
    state = {}
    for path, fin, fout in targets:
        state[f"base_model.model.{path}.lora_A.weight"] = torch.randn((r, fin), generator=gen) / fin ** 0.5
        state[f"base_model.model.{path}.lora_B.weight"] = torch.randn((fout, r), generator=gen) / r ** 0.5
    return state


def _expert_targets(layer, experts, ws, spelling):
    return [(f"model.layers.{layer}.{spelling}.experts.{e}.{w}",) + SHAPES[w] for e in experts for w in ws]


def _config(r, alpha, **extra):
    return dict({"peft_type": "LORA", "r": r, "lora_alpha": alpha, "bias": "none", "target_modules": ["w1", "w2", "w3"],
                 "use_rslora": False, "use_dora": False, "modules_to_save": None, "rank_pattern": {}, "alpha_pattern": {}}, **extra)


def test_loader_takes_expert_keys_in_both_spellings_partial_coverage_and_dense_targets(tiny):
    import aqlm.lora as lora
    from aqlm_amd.moe import QuantizedMixtralExperts

    model = _copy(tiny)
    blocks = [model.get_submodule(f"model.layers.{li}.mlp.experts") for li in range(mc.LAYERS)]
    q = model.model.layers[0].self_attn.q_proj
    full = _state(1, 8, _expert_targets(0, range(mc.EXPERTS), ("w1", "w2", "w3"), "block_sparse_moe")
                  + _expert_targets(1, range(mc.EXPERTS), ("w1", "w2", "w3"), "block_sparse_moe"))
    part = _state(2, 16, _expert_targets(0, (0, 2), ("w1", "w2"), "mlp"))
    mixed = _state(3, 8, _expert_targets(0, (1,), ("w3",), "mlp") + [("model.layers.0.self_attn.q_proj", mc.HID, mc.HID)])
    bank = lora.attach_adapters(model, {"full": (full, _config(8, 16)), "part": (part, _config(16, 8)), "mixed": (mixed, _config(8, 8))})
    assert bank.names == ["full", "part", "mixed"]
    w0, w1 = (model.get_submodule(f"model.layers.{li}.mlp.experts") for li in range(mc.LAYERS))
    assert isinstance(w0, lora.LoraQuantizedMixtralExperts) and isinstance(w1, lora.LoraQuantizedMixtralExperts)
    assert w0.base_layer is blocks[0] and w1.base_layer is blocks[1] and isinstance(w0.base_layer, QuantizedMixtralExperts)
    wq = model.model.layers[0].self_attn.q_proj
    assert isinstance(wq, lora.LoraQuantizedLinear) and wq.base_layer is q and list(wq.lora_A) == ["mixed"]
    assert {type(m) for m in bank.layers} == {lora.LoraQuantizedMixtralExperts, lora.LoraQuantizedLinear} and len(bank.layers) == 3
    # the published spelling landed on the mlp block, values and scaling intact
    key = "base_model.model.model.layers.0.block_sparse_moe.experts.3.w2.lora_{}.weight"
    assert torch.equal(w0.lora_A["full"]["3"]["w2"].weight, full[key.format("A")])
    assert torch.equal(w0.lora_B["full"]["3"]["w2"].weight, full[key.format("B")])
    assert w0.scaling == {"full": 2.0, "part": 0.5, "mixed": 1.0} and list(w1.lora_A) == ["full"]
    assert not w0.lora_A["full"]["3"]["w2"].weight.requires_grad and w0.lora_A["full"]["3"]["w2"].bias is None
    # partial coverage
    assert sorted(w0.lora_A["part"]) == ["0", "2"] and sorted(w0.lora_A["part"]["0"]) == ["w1", "w2"]
    assert w0._weights("part", 1, "w1") is None and w0._weights("part", 0, "w3") is None and w0._weights("part", 2, "w2") is not None
    assert sorted(w0.lora_A["mixed"]) == ["1"] and sorted(w0.lora_A["mixed"]["1"]) == ["w3"]
    # state_dict names
    keys = set(model.state_dict())
    for e in range(mc.EXPERTS):
        for w in ("w1", "w2", "w3"):
            assert {f"{BLOCK}.base_layer.{e}.{w}.codes", f"{BLOCK}.base_layer.{e}.{w}.codebooks", f"{BLOCK}.base_layer.{e}.{w}.scales",
                    f"{BLOCK}.lora_A.full.{e}.{w}.weight", f"{BLOCK}.lora_B.full.{e}.{w}.weight"} <= keys
    assert f"{BLOCK}.lora_A.part.2.w1.weight" in keys and f"{BLOCK}.lora_A.part.1.w1.weight" not in keys
    assert f"{BLOCK}.lora_B.mixed.1.w3.weight" in keys and "model.layers.0.self_attn.q_proj.lora_A.mixed.weight" in keys
    # detach restores the very block objects
    lora.detach_adapters(model)
    assert [model.get_submodule(f"model.layers.{li}.mlp.experts") for li in range(mc.LAYERS)] == blocks
    assert all(a is b for a, b in zip((model.get_submodule(f"model.layers.{li}.mlp.experts") for li in range(mc.LAYERS)), blocks))
    assert model.model.layers[0].self_attn.q_proj is q and not any("lora_" in k for k in model.state_dict())
    # target_modules restricts the projections
    bank = lora.attach_adapters(model, {"full": (full, _config(8, 16))}, target_modules=["w2"])
    w0 = model.get_submodule(BLOCK)
    assert sorted(w0.lora_A["full"]["0"]) == ["w2"]
    lora.detach_adapters(model)


def test_loader_refuses_wrong_rank_shape_and_experts_without_a_block(tiny):
    import aqlm.lora as lora

    model = _copy(tiny)
    t = _expert_targets(0, (0,), ("w1",), "mlp")
    with pytest.raises(ValueError, match="r=16"):
        lora.attach_adapters(model, {"x": (_state(1, 8, t), _config(16, 8))})
    with pytest.raises(ValueError, match=r"lora_A must be \[r, 64\]"):
        lora.attach_adapters(model, {"x": (_state(1, 8, [(t[0][0], mc.INTER, mc.INTER)]), _config(8, 8))})
    with pytest.raises(ValueError, match=r"lora_B \[64, r\]"):
        lora.attach_adapters(model, {"x": (_state(1, 8, [(f"{BLOCK}.1.w2", mc.INTER, mc.INTER)]), _config(8, 8))})
    with pytest.raises(ValueError, match="no module"):
        lora.attach_adapters(model, {"x": (_state(1, 8, _expert_targets(0, (mc.EXPERTS,), ("w1",), "block_sparse_moe")), _config(8, 8))})
    assert not any(isinstance(m, (lora.LoraQuantizedMixtralExperts, lora.LoraQuantizedLinear)) for m in model.modules())
    # an expert layer with no QuantizedMixtralExperts two levels up keeps the refusal
    holder = torch.nn.Module()
    holder.experts = torch.nn.Module()
    holder.experts.add_module("0", torch.nn.Module())
    lin = model.get_submodule(f"{BLOCK}.0.w1")
    holder.experts.get_submodule("0").w1 = lin
    with pytest.raises(NotImplementedError, match="routed experts are not supported"):
        lora.attach_adapters(holder, {"x": (_state(1, 8, [("experts.0.w1",) + SHAPES["w1"]]), _config(8, 8))})


# ---------------------------------------------------------------------------------------------------------------------------
# the wrapper on the host block: per-expert loop + torch path against fp64
# ---------------------------------------------------------------------------------------------------------------------------
RANKS = (8, 24, 16)
T, K = 6, mc.TOP_K


def _wrapped(tiny):
    """Layer 0's block with three adapters: ad0 on everything, ad1 on experts 0 and 2 / w1 and w2 only, ad2 on w3 and w2."""
    import aqlm.lora as lora

    model = _copy(tiny)
    cover = [(range(mc.EXPERTS), ("w1", "w3", "w2")), ((0, 2), ("w1", "w2")), (range(mc.EXPERTS), ("w3", "w2"))]
    ads = {f"ad{i}": (_state(40 + i, r, _expert_targets(0, ex, ws, "mlp")), _config(r, 2 * r + i))
           for i, (r, (ex, ws)) in enumerate(zip(RANKS, cover))}
    bank = lora.attach_adapters(model, ads)
    return model.get_submodule(BLOCK), bank, tiny[1]


def _inputs(seed, t=T):
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn((t, mc.HID), generator=gen) * 0.5
    idx = torch.topk(torch.rand((t, mc.EXPERTS), generator=gen), K, dim=-1).indices
    idx[t - 1, 1] = mc.EXPERTS  # an id == num_experts: skipped
    wts = torch.rand((t, K), generator=gen)
    return x, idx, wts


def _ref64(wrapper, dense, x, idx, wts, ids, leaves=None):
    """The block definition with adapters in fp64: adapters added before the activation and after w2, weighted sum over top_k.
    ``leaves``: {(name, e, w): (A, B)} fp64 tensors to use in the place of the wrapper's (autograd)."""
    names = wrapper.bank.names
    rows = []
    for t in range(x.shape[0]):
        row = torch.zeros(mc.HID, dtype=torch.float64)
        for j in range(idx.shape[1]):
            e = int(idx[t, j])
            if not 0 <= e < mc.EXPERTS:
                continue

            def proj(w, v):
                out = dense[(e, w)] @ v
                a = ids[t]
                if 0 <= a < len(names) and wrapper._weights(names[a], e, w) is not None:
                    A, B, s = wrapper._weights(names[a], e, w)
                    A, B = leaves[(names[a], e, w)] if leaves and (names[a], e, w) in leaves else (A.double(), B.double())
                    out = out + s * (B @ (A @ v))
                return out

            h = torch.nn.functional.silu(proj("w1", x[t])) * proj("w3", x[t])
            row = row + wts[t, j].double() * proj("w2", h)
        rows.append(row)
    return torch.stack(rows)


def _close(y, y64, what):
    err = float((y.double() - y64).abs().max() / y64.abs().max())
    mean = float((y.double() - y64).abs().mean() / y64.abs().mean())
    print(f"{what}: max error / max|y| {err:.3g}, mean error / mean|y| {mean:.3g}")
    assert err < 1e-4, (what, err)    # the fp32 torch path against fp64: rtol 1e-4 of max|y|
    assert mean < 1e-5, (what, mean)  # the constant of the dense wrapper's host test (tests/test_lora_host.py::_close)


def test_wrapper_on_the_host_block_matches_fp64_for_every_selection(tiny):
    wrapper, bank, dense = _wrapped(tiny)
    x, idx, wts = _inputs(7)
    x64 = x.double()
    with torch.no_grad():
        bare = wrapper.base_layer(x, idx, wts)
        assert torch.equal(wrapper(x, idx, wts), bare)               # nothing selected yet
        _close(bare, _ref64(wrapper, dense, x64, idx, wts, [-1] * T), "bare block")
        for name in ("ad0", "ad1", "ad2"):
            bank.select(name)
            y = wrapper(x, idx, wts)
            _close(y, _ref64(wrapper, dense, x64, idx, wts, [bank.index(name)] * T), name)
            assert not torch.equal(y, bare)
        ids = [2, -1, 0, 3, 1, 0]                                    # -1 and len(names) are out of range: base rows
        for dt in (torch.int64, torch.int32):
            bank.select(torch.tensor(ids, dtype=dt))
            y = wrapper(x, idx, wts)
            _close(y, _ref64(wrapper, dense, x64, idx, wts, ids), f"per-token ids {dt}")
            assert torch.equal(y[1], bare[1]) and torch.equal(y[3], bare[3]) and not torch.equal(y[0], bare[0])
        seq = [1, 3, 0]                                              # per sequence: T / 3 consecutive rows each
        bank.select(torch.tensor(seq))
        y = wrapper(x, idx, wts)
        _close(y, _ref64(wrapper, dense, x64, idx, wts, [s for s in seq for _ in range(T // 3)]), "per-sequence ids")
        bank.select(torch.tensor([s for s in seq for _ in range(T // 3)]))
        assert torch.equal(wrapper(x, idx, wts), y)
        bank.select(torch.tensor([0, 1, 2, 0]))
        with pytest.raises(ValueError, match="one per row"):
            wrapper(x, idx, wts)
        bank.select(None)
        assert torch.equal(wrapper(x, idx, wts), bare)


def test_pair_batched_torch_path_matches_the_per_expert_loop(tiny):
    """The provider's pair-batched torch path (what the routed and grouped routes call beyond the HIP route) on host tensors,
    against the same adapters applied per expert: both evaluate PEFT's formula in fp32."""
    import aqlm.lora as lora

    wrapper, bank, dense = _wrapped(tiny)
    x, idx, wts = _inputs(9)
    ids = torch.tensor([2, -1, 0, 3, 1, 0])
    for sel, tok_ids in (("ad1", None), (ids, ids)):
        prov = lora._ExpertAdapters(wrapper, sel, tok_ids)
        gen = torch.Generator().manual_seed(3)
        for segments, rows_x, per_pair, fin, fout in ((("w1", "w3"), x, False, mc.HID, mc.INTER),
                                                      (("w2",), torch.randn((T * K, mc.INTER), generator=gen), True, mc.INTER, mc.HID)):
            out = torch.randn((T * K, len(segments), fout), generator=gen)
            got = prov.on_pairs(out, rows_x, idx, segments, per_pair)
            assert got is not out
            want = out.double().clone()
            for p in range(T * K):
                e, a = int(idx.reshape(-1)[p]), (bank.index(sel) if tok_ids is None else int(tok_ids[p // K]))
                for s, w in enumerate(segments):
                    wt = wrapper._weights(bank.names[a], e, w) if 0 <= a < len(bank.names) and 0 <= e < mc.EXPERTS else None
                    if wt is not None:
                        xr = rows_x[p if per_pair else p // K].double()
                        want[p, s] += wt[2] * (wt[1].double() @ (wt[0].double() @ xr))
                    else:
                        assert torch.equal(got[p, s], out[p, s])
            _close(got, want, f"on_pairs {segments}")


def test_gradients_of_hidden_states_a_and_b_match_fp64_autograd(tiny):
    wrapper, bank, dense = _wrapped(tiny)
    for p in list(wrapper.lora_A.parameters()) + list(wrapper.lora_B.parameters()):
        p.requires_grad_(True)
    ids = [2, 0, 7, 1, 0, 2]
    bank.select(torch.tensor(ids))
    x, idx, wts = _inputs(8)
    x.requires_grad_(True)
    gy = torch.randn((T, mc.HID), generator=torch.Generator().manual_seed(5))
    (wrapper(x, idx, wts) * gy).sum().backward()
    x64 = x.detach().double().requires_grad_(True)
    leaves = {(n, e, w): (wrapper._weights(n, e, w)[0].detach().double().requires_grad_(True),
                          wrapper._weights(n, e, w)[1].detach().double().requires_grad_(True))
              for n in bank.names for e in range(mc.EXPERTS) for w in ("w1", "w3", "w2") if wrapper._weights(n, e, w) is not None}
    (_ref64(wrapper, dense, x64, idx, wts, ids, leaves) * gy.double()).sum().backward()

    def close(g, g64, what):
        assert g is not None and g64 is not None, what
        err = float((g.double() - g64).abs().max() / g64.abs().max())
        assert err < 1e-4, (what, err)  # the host backward's tolerance in tests/test_cpu_path.py and tests/test_lora_host.py

    close(x.grad, x64.grad, "hidden_states")
    checked = 0
    for (n, e, w), (A64, B64) in leaves.items():
        A, B, _ = wrapper._weights(n, e, w)
        if A64.grad is None or float(A64.grad.abs().max()) == 0.0:
            continue  # no token with this adapter reached this expert
        close(A.grad, A64.grad, f"A {n} {e} {w}")
        close(B.grad, B64.grad, f"B {n} {e} {w}")
        checked += 1
    assert checked >= 3
    assert all(p.grad is None for p in wrapper.base_layer.parameters())
