"""Mixtral AQLM checkpoints on the host: the quantized experts load by name through aqlm_amd.moe, match the dense twin, the
hook is opt-in and restores what it wraps, prepack_model leaves the experts alone, and the routing helpers match numpy."""
import numpy as np
import pytest
import torch

transformers = pytest.importorskip("transformers")
pytest.importorskip("safetensors.torch")

from tests import moe_checkpoint as mc  # noqa: E402


@pytest.fixture(scope="module")
def checkpoint(tmp_path_factory):
    path = tmp_path_factory.mktemp("moe") / "aqlm_tiny_mixtral"
    dense = mc.build(path)
    return dense, str(path)


def test_loads_every_expert_by_name_and_matches_the_dense_twin(checkpoint):
    from aqlm_amd.moe import QuantizedMixtralExperts

    dense, path = checkpoint
    model, info = mc.load(path, "cpu")
    assert not info["missing_keys"] and not info["unexpected_keys"], info
    experts = [m for m in model.modules() if type(m).__name__.endswith("Experts")]
    assert len(experts) == mc.LAYERS and all(isinstance(m, QuantizedMixtralExperts) for m in experts)
    assert not any(p.is_meta for p in model.parameters())
    w = model.model.layers[1].mlp.experts.expert(3).w2
    assert tuple(w.codes.shape) == (mc.HID, mc.INTER // 8, 1) and w.codes.dtype == torch.int16
    sd = model.state_dict()
    for e in range(mc.EXPERTS):
        for s in ("w1", "w2", "w3"):
            for t in ("codes", "codebooks", "scales"):
                assert f"model.layers.0.mlp.experts.{e}.{s}.{t}" in sd
    missing, unexpected = model.load_state_dict(sd, strict=True)
    assert not missing and not unexpected
    ids = torch.randint(0, mc.VOCAB, (2, 9), generator=torch.Generator().manual_seed(1))
    with torch.no_grad():
        a, b = model(ids).logits.float(), dense(ids).logits.float()
    rel = ((a - b).abs().mean() / b.abs().mean()).item()
    assert rel < 2e-2, rel


def test_without_the_hook_loading_is_unchanged(checkpoint):
    from aqlm_amd.moe import QuantizedMixtralExperts

    _, path = checkpoint
    model, info = mc.load(path, "cpu", hook=False)
    assert not any(isinstance(m, QuantizedMixtralExperts) for m in model.modules())
    assert any(k.endswith("experts.gate_up_proj") for k in info["missing_keys"])
    assert any(".experts.0.w1.codes" in k for k in info["unexpected_keys"])


def test_hook_restores_the_transformers_name():
    import transformers.quantizers.quantizer_aqlm as qa

    from aqlm_amd.moe import quantized_experts

    original = qa.replace_with_aqlm_linear
    with quantized_experts():
        assert qa.replace_with_aqlm_linear is not original
        assert qa.replace_with_aqlm_linear.__wrapped__ is original
    assert qa.replace_with_aqlm_linear is original
    with pytest.raises(KeyError):
        with quantized_experts():
            raise KeyError("inside")
    assert qa.replace_with_aqlm_linear is original


def test_alias_package_exports():
    import aqlm
    import aqlm_amd

    assert aqlm.quantized_experts is aqlm_amd.quantized_experts
    assert aqlm.QuantizedMixtralExperts is aqlm_amd.moe.QuantizedMixtralExperts


def test_replace_moe_experts_counts_and_keeps_the_device():
    from transformers import MixtralForCausalLM

    from aqlm_amd.moe import QuantizedMixtralExperts, replace_moe_experts

    with torch.device("meta"):
        model = MixtralForCausalLM(mc.config())
    n = replace_moe_experts(model, mc.SCHEME)
    assert n == mc.LAYERS
    ex = model.model.layers[0].mlp.experts
    assert isinstance(ex, QuantizedMixtralExperts) and ex.expert(0).w1.codes.is_meta
    assert replace_moe_experts(model, mc.SCHEME) == 0


def test_prepack_model_leaves_the_experts_alone(checkpoint, monkeypatch):
    from aqlm_amd import checkpoint as ck
    from aqlm_amd.inference import QuantizedLinear

    _, path = checkpoint
    model, _ = mc.load(path, "cpu")
    # keep only the experts' layers quantized: a host model's other QuantizedLinears would make prepack_model refuse (GPU-only)
    others = [n for n, m in model.named_modules() if isinstance(m, QuantizedLinear) and not getattr(m, "_moe_expert", False)]
    for n in others:
        model.set_submodule(n, torch.nn.Identity())
    before = {n: p.clone() for n, p in model.named_parameters() if ".experts." in n and n.endswith(".codes")}
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    ck.prepack_model(model)
    for n, m in model.named_modules():
        if isinstance(m, QuantizedLinear):
            assert m._packed_codes is None and not m._codes_dropped, n
    after = dict(model.named_parameters())
    for n, t in before.items():
        assert torch.equal(after[n], t), n


def test_routing_helpers_match_numpy():
    from aqlm_amd.inference_kernels import hip_kernel

    rng = np.random.default_rng(0)
    for T, k in [(1, 2), (3, 2), (32, 2), (33, 2), (70, 2), (64, 1), (65, 1), (21, 3), (100, 8)]:
        chunks = hip_kernel.routed_chunks(T, k)
        assert chunks[0][0] == 0 and chunks[-1][1] == T
        assert all(a[1] == b[0] for a, b in zip(chunks, chunks[1:]))
        assert all(0 < (t1 - t0) * k <= 64 for t0, t1 in chunks)
        assert len(chunks) == -(-T * k // ((64 // k) * k))
        # pair layout: pair p = t * k + j reads token row p // k (w1 / w3) or pair row p (w2), expert ids[t, j]
        ids = rng.integers(0, 8, size=(T, k))
        for t0, t1 in chunks:
            p = np.arange(t0 * k, t1 * k)
            assert np.array_equal(p // k, np.repeat(np.arange(t0, t1), k))
            assert np.array_equal(ids.reshape(-1)[p], ids[t0:t1].reshape(-1))


def _loop_reference(experts, x, ids, w):
    """numpy model of the block: out[t] = sum_j w[t, j] * W2_e (silu(W1_e x_t) * W3_e x_t), e = ids[t, j] (fp64)."""
    out = np.zeros((x.shape[0], experts.hidden_dim))
    for t in range(x.shape[0]):
        for j in range(ids.shape[1]):
            e = int(ids[t, j])
            if not 0 <= e < experts.num_experts:
                continue
            ex = experts.expert(e)
            Wd = {s: getattr(ex, s) for s in ("w1", "w3", "w2")}
            dq = {s: _dense(m) for s, m in Wd.items()}
            g, u = dq["w1"] @ x[t], dq["w3"] @ x[t]
            h = g / (1 + np.exp(-g)) * u
            out[t] += w[t, j] * (dq["w2"] @ h)
    return out


def _dense(lin):
    from oracle import aqlm_oracle as orc

    codes = lin.codes.detach().numpy().astype(np.int64) & 0xFFFF
    return orc.dequantize_weight(codes, lin.codebooks.detach().float().numpy(), lin.scales.detach().float().numpy()).astype(np.float64)


def test_host_forward_matches_numpy(checkpoint):
    _, path = checkpoint
    model, _ = mc.load(path, "cpu")
    experts = model.model.layers[0].mlp.experts
    rng = np.random.default_rng(2)
    x = (rng.standard_normal((5, mc.HID)) * 0.5).astype(np.float16)
    ids = np.array([[0, 1], [1, 0], [3, 2], [2, 2], [3, mc.EXPERTS]])  # a duplicate and an id == num_experts (skipped)
    w = rng.random((5, 2)).astype(np.float32)
    with torch.no_grad():
        y = experts(torch.from_numpy(x), torch.from_numpy(ids), torch.from_numpy(w)).float().numpy()
    ref = _loop_reference(experts, x.astype(np.float64), ids, w.astype(np.float64))
    rel = np.abs(y - ref).mean() / np.abs(ref).mean()
    assert rel < 1e-2, rel


def test_routed_entry_rejects_bad_arguments_without_a_gpu():
    import ctypes

    from aqlm_amd import _native as nat

    L = nat.lib
    buf = ctypes.create_string_buffer(4096)
    p = (ctypes.addressof(buf) + 15) // 16 * 16
    args = lambda **kw: [kw.get(n, d) for n, d in (  # noqa: E731
        ("table", p), ("E", 8), ("S", 2), ("ids", p), ("i64", 1), ("pairs", 2), ("k", 2), ("x", p), ("xs", 4096), ("per_pair", 0),
        ("y", p), ("out", 14336), ("inf", 4096), ("g", 8), ("dt", nat.F16), ("stream", None))]
    assert L.aqlm_hip_gemv_1x16_routed(*args(table=None)) == nat.E_INVALID and "null pointer" in nat.last_error()
    assert L.aqlm_hip_gemv_1x16_routed(*args(E=nat.MAX_ROUTED_EXPERTS + 1)) == nat.E_INVALID
    assert L.aqlm_hip_gemv_1x16_routed(*args(S=3)) == nat.E_INVALID
    assert L.aqlm_hip_gemv_1x16_routed(*args(pairs=nat.MAX_ROUTED_PAIRS + 2)) == nat.E_INVALID
    assert L.aqlm_hip_gemv_1x16_routed(*args(pairs=3)) == nat.E_INVALID  # not a multiple of top_k
    assert L.aqlm_hip_gemv_1x16_routed(*args(ids=p + 4)) == nat.E_INVALID and "misaligned" in nat.last_error()
    assert L.aqlm_hip_gemv_1x16_routed(*args(dt=7)) == nat.E_UNSUPPORTED and "float16 and bfloat16" in nat.last_error()
    assert L.aqlm_hip_gemv_1x16_routed(*args(g=4)) == nat.E_UNSUPPORTED and "8 or 16" in nat.last_error()
    assert L.aqlm_hip_gemv_1x16_routed(*args(inf=4104)) == nat.E_UNSUPPORTED  # 513 groups: outside the direct kernel
    assert L.aqlm_hip_gemv_1x16_routed(*args(inf=40960, xs=40960)) == nat.E_UNSUPPORTED  # x row above 64 KiB
