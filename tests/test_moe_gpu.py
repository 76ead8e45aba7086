"""Mixtral experts on the MI355X: the expert-routed 1x16 matvec (aqlm_hip_gemv_1x16_routed) against the fp64 oracle and
bit-for-bit against aqlm_hip_gemv_1x16, the QuantizedMixtralExperts forward against the per-expert loop and the dense
MixtralExperts, no host sync on the routed path, hipGraph capture of a whole MoE block, and the tiny checkpoint end to end.

Tolerances (restated from tests/test_hip_parity.py): fp16 mean|y - y64| / mean|y64| <= 1e-3 and per element
|y - y64| <= 2e-3 * mean|y64| + 4 ulp(|y64|); bf16 8e-3 / 1.6e-2 with bf16 ulps."""
import os
import re
import shutil
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
ISA_FLAGS = ["-O3", "-std=c++17", "--offload-arch=gfx950", "-fPIC", "-ffp-contract=fast", "-mllvm",
             "-amdgpu-kernarg-preload-count=14", "--cuda-device-only", "-S"]
TOL = {torch.float16: (1e-3, 2e-3, 10), torch.bfloat16: (8e-3, 1.6e-2, 7)}  # mean rel, per-element rel, mantissa bits
E = 8


def _check(y, y64, dtype, what):
    y = y.double()
    mean_rel, elem_rel, mant = TOL[dtype]
    scale = y64.abs().mean().item()
    err = (y - y64).abs()
    assert err.mean().item() / scale <= mean_rel, f"{what}: mean rel {err.mean().item() / scale:.3e}"
    ulp = torch.exp2(torch.floor(torch.log2(y64.abs().clamp_min(1e-30))) - mant)
    bad = err > elem_rel * scale + 4 * ulp
    assert not bad.any(), f"{what}: {int(bad.sum())} elements out of bound"


def _experts(seed, S, fin, fout, g, dtype, dev):
    gen = torch.Generator(device=dev).manual_seed(seed)
    layers = []
    for _ in range(E):
        per = []
        for _ in range(S):
            codes = torch.randint(-32768, 32768, (fout, fin // g, 1), generator=gen, device=dev, dtype=torch.int32).to(torch.int16)
            cb = torch.randn((1, 65536, 1, g), generator=gen, device=dev).to(dtype)
            sc = (torch.rand((fout, 1, 1, 1), generator=gen, device=dev) * 0.5 + 0.25).to(dtype)
            per.append((codes, cb, sc, None))
        layers.append(per)
    return layers


def _w64(layer):
    codes, cb, sc, _ = layer
    fout = codes.shape[0]
    idx = codes.reshape(fout, -1).long() & 0xFFFF
    return (cb[0, :, 0, :].double()[idx].reshape(fout, -1)) * sc.double().reshape(fout, 1)


def _routings(T, k, gen, dev):
    scores = torch.rand((T, E), generator=gen, device=dev)
    rnd = torch.topk(scores, k, dim=-1).indices
    one = torch.full((T, k), 5, dtype=torch.int64, device=dev)
    dup = rnd[:, :1].repeat(1, k)
    oob = rnd.clone()
    bad = torch.tensor([-1, E, 1000, -(2 ** 40), 2 ** 40 + 3], device=dev)
    oob.view(-1)[::2] = bad[torch.arange(oob.numel(), device=dev)[::2] % bad.numel()]
    return {"random": rnd, "one_expert": one, "duplicates": dup, "out_of_range": oob.to(torch.int32)}


SHAPES = [("w13", 2, 4096, 14336, False), ("w2", 1, 14336, 4096, True), ("odd", 2, 1536, 808, False)]


@pytest.mark.gpu
@pytest.mark.parametrize("g", [8, 16])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("shape", SHAPES, ids=[s[0] for s in SHAPES])
def test_routed_op_matches_oracle_and_direct_kernel(g, dtype, shape):
    from aqlm_amd.inference_kernels import hip_kernel as hk

    name, S, fin, fout, per_pair = shape
    dev = torch.device("cuda:0")
    layers = _experts(10 * g + SHAPES.index(shape), S, fin, fout, g, dtype, dev)
    table = hk.routed_table(layers, dev)
    gen = torch.Generator(device=dev).manual_seed(7)
    w64 = {}
    for T in (1, 2, 3, 8, 32):
        for k in (1, 2):
            for rname, ids in _routings(T, k, gen, dev).items():
                rows = T * k if per_pair else T
                x = torch.randn((rows, fin), generator=gen, device=dev).to(dtype)
                y = torch.ops.aqlm.code1x16_moe_matmat(x, ids, table, [E, S, fout, fin, g, k], per_pair)
                assert tuple(y.shape) == (T * k, S, fout)
                ids_h = ids.long().cpu().view(-1).tolist()
                for p, e in enumerate(ids_h):
                    xr = x[p if per_pair else p // k]
                    what = f"{name} g{g} {dtype} T{T} k{k} {rname} pair {p} expert {e}"
                    if not 0 <= e < E:
                        assert torch.count_nonzero(y[p]) == 0, what
                        continue
                    for s in range(S):
                        if (e, s) not in w64:
                            w64[(e, s)] = _w64(layers[e][s])
                        _check(y[p, s], w64[(e, s)] @ xr.double(), dtype, f"{what} seg {s}")
                        codes, cb, sc, _ = layers[e][s]
                        ref = hk._gemv(xr.view(1, -1), codes, cb, sc, None, "1x16")
                        assert torch.equal(y[p, s].view(1, -1), ref), f"{what} seg {s}: not bit-identical to aqlm_hip_gemv_1x16"
    torch.cuda.synchronize()


OFF_TRACK_SHAPES = [("w13", 2, 1024, 808, False), ("w2", 1, 2048, 512, True)]


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("top_k", [1, 4, 8])
@pytest.mark.parametrize("num_experts", [1, 3, 60])
def test_routed_op_with_other_expert_counts_top_k_bias_and_strided_x(num_experts, top_k, dtype):
    """Off the 8 experts / top-2 / no bias track of the test above: 1, 3 and 60 experts (ids E - 1, E and -1 present), top_k
    1 / 4 / 8 up to exactly 64 pairs, a bias per expert and projection, x rows taken from a wider tensor.  Same bounds, same
    bit-identity partner (aqlm_hip_gemv_1x16 of that expert on that row)."""
    from aqlm_amd.inference_kernels import hip_kernel as hk
    from tests import moe_experts as mx

    dev, g, n = torch.device("cuda:0"), 8, num_experts
    gen = torch.Generator(device=dev).manual_seed(9)
    for name, S, fin, fout, per_pair in OFF_TRACK_SHAPES:
        layers = mx.plain_experts(n, 400 + n, S, fin, fout, g, dtype, dev, bias=True)
        table = hk.routed_table(layers, dev)
        w64 = {}
        for T in (64 // top_k, 3):
            for ids_dtype in (torch.int64, torch.int32):
                ids = mx.router_ids(T, top_k, n, gen, dev, ids_dtype)
                flat = ids.view(-1)
                flat[0] = n - 1
                if flat.numel() > 2:
                    flat[1], flat[2] = n, -1
                x = mx.strided_rows(T * top_k if per_pair else T, fin, gen, dev, dtype)
                y = torch.ops.aqlm.code1x16_moe_matmat(x, ids, table, [n, S, fout, fin, g, top_k], per_pair)
                assert tuple(y.shape) == (T * top_k, S, fout)
                for p, e in enumerate(flat.cpu().tolist()):
                    xr = x[p if per_pair else p // top_k]
                    what = f"{name} E{n} k{top_k} {dtype} T{T} {ids_dtype} pair {p} expert {e}"
                    if not 0 <= e < n:
                        assert torch.count_nonzero(y[p]) == 0, what
                        continue
                    for s in range(S):
                        codes, cb, sc, bias = layers[e][s]
                        if (e, s) not in w64:
                            w64[(e, s)] = _w64(layers[e][s])
                        _check(y[p, s], w64[(e, s)] @ xr.double() + bias.double(), dtype, f"{what} seg {s}")
                        ref = hk._gemv(xr.view(1, -1), codes, cb, sc, bias, "1x16")
                        assert torch.equal(y[p, s].view(1, -1), ref), f"{what} seg {s}: not bit-identical to aqlm_hip_gemv_1x16"
    torch.cuda.synchronize()


def _module(H, I, dtype, dev, seed=0):
    from transformers import MixtralConfig
    from transformers.models.mixtral.modeling_mixtral import MixtralExperts

    from aqlm_amd.moe import QuantizedMixtralExperts

    cfg = MixtralConfig(hidden_size=H, intermediate_size=I, num_local_experts=E, num_experts_per_tok=2, num_attention_heads=4,
                        num_key_value_heads=4, router_jitter_noise=0.0)
    q = QuantizedMixtralExperts(cfg, dict(in_group_size=8, out_group_size=1, num_codebooks=1, nbits_per_codebook=16),
                                device=dev, dtype=dtype)
    dense = MixtralExperts(cfg).to(dev, dtype)
    gen = torch.Generator(device=dev).manual_seed(seed)
    with torch.no_grad():
        for e in range(E):
            ws = {}
            for s in ("w1", "w3", "w2"):
                lin = getattr(q.expert(e), s)
                lin.codes.copy_(torch.randint(-32768, 32768, lin.codes.shape, generator=gen, device=dev, dtype=torch.int32))
                lin.codebooks.copy_(torch.randn(lin.codebooks.shape, generator=gen, device=dev) * 0.05)
                lin.scales.copy_(torch.rand(lin.scales.shape, generator=gen, device=dev) * 0.2 + 0.05)
                ws[s] = _w64((lin.codes, lin.codebooks, lin.scales, None)).to(dtype)
            dense.gate_up_proj[e].copy_(torch.cat([ws["w1"], ws["w3"]], 0))
            dense.down_proj[e].copy_(ws["w2"])
    return cfg, q, dense


def _route(T, k, gen, dev):
    logits = torch.randn((T, E), generator=gen, device=dev)
    w, ids = torch.topk(torch.softmax(logits, -1), k, dim=-1)
    return ids, w / w.sum(-1, keepdim=True)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_experts_forward_matches_loop_and_dense(dtype):
    dev = torch.device("cuda:0")
    _, q, dense = _module(1024, 2048, dtype, dev)
    gen = torch.Generator(device=dev).manual_seed(3)
    for T in (1, 2, 4, 16, 32, 40):
        x = torch.randn((T, 1024), generator=gen, device=dev).to(dtype)
        ids, w = _route(T, 2, gen, dev)
        with torch.no_grad():
            assert q.takes_routed_path(x, ids) == (T * 2 <= 64)
            y = q(x, ids, w).double()
            y_loop = q._forward_loop(x, ids, w).double()
            y_dense = dense(x, ids, w).double()
        for ref, what in ((y_loop, "loop"), (y_dense, "dense")):
            rel = ((y - ref).abs().mean() / ref.abs().mean()).item()
            assert rel < (2e-3 if dtype == torch.float16 else 1.6e-2), (T, what, rel)


@pytest.mark.gpu
def test_routed_forward_makes_no_host_sync():
    dev = torch.device("cuda:0")
    _, q, _ = _module(1024, 2048, torch.float16, dev)
    gen = torch.Generator(device=dev).manual_seed(4)
    x = torch.randn((4, 1024), generator=gen, device=dev).half()
    ids, w = _route(4, 2, gen, dev)
    with torch.no_grad():
        q(x, ids, w)  # builds the device tables (one host-to-device copy)
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            y = q(x, ids, w)
        finally:
            torch.cuda.set_sync_debug_mode("default")
    assert torch.isfinite(y.float()).all()


@pytest.mark.gpu
@pytest.mark.parametrize("T", [1, 4])
def test_moe_block_decode_step_replays_from_a_graph(T):
    from transformers.models.mixtral.modeling_mixtral import MixtralSparseMoeBlock

    dev = torch.device("cuda:0")
    cfg, q, _ = _module(1024, 2048, torch.float16, dev, seed=5)
    block = MixtralSparseMoeBlock(cfg).to(dev, torch.float16).eval()
    with torch.no_grad():
        block.gate.weight.normal_(0, 0.5)
    block.experts = q
    gen = torch.Generator(device=dev).manual_seed(6)
    inputs = [torch.randn((1, T, 1024), generator=gen, device=dev).half() for _ in range(3)]
    static = inputs[0].clone()
    with torch.no_grad():
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(2):
                block(static)
        torch.cuda.current_stream().wait_stream(s)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = block(static)
        routes = set()
        for x in inputs:
            static.copy_(x)
            graph.replay()
            eager = block(x)
            torch.cuda.synchronize()
            assert torch.equal(out, eager)
            routes.add(tuple(block.gate(x.view(-1, 1024))[2].view(-1).tolist()))
    assert len(routes) == 3, "the three inputs should route differently"


@pytest.mark.gpu
def test_tiny_mixtral_checkpoint_end_to_end_on_gpu(tmp_path):
    pytest.importorskip("transformers")
    from tests import moe_checkpoint as mc

    dense = mc.build(tmp_path / "aqlm_tiny_mixtral")
    model, info = mc.load(str(tmp_path / "aqlm_tiny_mixtral"), "cuda:0")
    assert not info["missing_keys"] and not info["unexpected_keys"]
    dense = dense.to("cuda:0").eval()
    gen = torch.Generator().manual_seed(0)
    with torch.no_grad():
        for shape in ((1, 9), (2, 40)):  # 9 tokens: routed launches; 80 tokens: the per-expert loop
            ids = torch.randint(0, mc.VOCAB, shape, generator=gen).to("cuda:0")
            a, b = model(ids).logits.float(), dense(ids).logits.float()
            rel = ((a - b).abs().mean() / b.abs().mean()).item()
            assert rel < 2e-2, (shape, rel)
        prompt = torch.randint(0, mc.VOCAB, (1, 6), generator=gen).to("cuda:0")
        kw = dict(max_new_tokens=12, do_sample=False, pad_token_id=0)
        got = model.generate(prompt, **kw)[0, 6:]
        want = dense.generate(prompt, **kw)[0, 6:]
    agree = (got == want).float().mean().item()
    assert agree >= 0.8, agree


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_routed_kernel_isa_uses_no_scratch(tmp_path):
    out = tmp_path / "gemv_routed.s"
    subprocess.run([HIPCC] + ISA_FLAGS + [os.path.join(ROOT, "aqlm_amd", "csrc", "gemv_routed.hip"), "-o", str(out)], check=True,
                   stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=600)
    text = out.read_text()
    names = re.findall(r"^\s+\.name:\s+(_ZN4aqlm23gemv_1x16_routed_kernel\w+)", text, re.M)
    assert len(names) == 16, names
    for m in re.finditer(r"\.name:\s+(_ZN4aqlm23gemv_1x16_routed_kernel\w+)(.*?)(?=\n  - |\Z)", text, re.S):
        body = m.group(2)
        assert re.search(r"\.private_segment_fixed_size:\s+0\b", body), m.group(1)
    code = text.split(".amdgpu_metadata")[0]
    assert not re.search(r"\bscratch_(load|store)", code)
