"""Mixtral decode on prepacked experts, on the MI355X: the routed packed launch (aqlm_hip_gemv_1x16_routed_packed) bit for bit
against aqlm_hip_gemv_1x16_packed at batch 1 and against the fp64 oracle, hostile ids, cells at rest, no host sync, hipGraph replay
with changing routings, the block before / after ``prepack_experts``, staleness after a codebook write, and the tiny checkpoint.

Bounds are the project's existing ones, restated: ``check_rounded`` of tests/test_hip_parity.py (every element within one ulp of
the storage type + 2e-5 sigma of fp32 noise of the correctly rounded fp64 result, and bit-equal to it on >= 0.97 of fp16 / 0.995
of bf16 elements); block level: mean |y - ref| / mean |ref| < 2e-3 (fp16) / 1.6e-2 (bf16) as in tests/test_moe_gpu.py; end to end:
< 2e-2 on the logits as there.  The block tests set ``moe.ROUTED_PACKED_MAX_PAIRS`` themselves: the shipped value is a measured
cross-over (profiles/moe_block_packed.json), not part of what is checked here."""
import numpy as np
import pytest
import torch

from oracle import aqlm_oracle as orc
from tests.test_moe_gpu import E, _experts, _module, _route

pytestmark = pytest.mark.gpu


def _ulp(y, dtype):
    mant = 10 if dtype == torch.float16 else 7
    return 2.0 ** (np.floor(np.log2(np.maximum(np.abs(y), 2.0 ** -14))) - mant)


def check_rounded(y, y64, dtype, what=""):
    y, y64 = np.asarray(y, dtype=np.float64), np.asarray(y64, dtype=np.float64)
    yr = torch.from_numpy(y64).to(dtype).double().numpy()
    sigma = float(np.sqrt(np.mean(y64 * y64)))
    err = np.abs(y - yr)
    bad = err > _ulp(y64, dtype) + 2e-5 * sigma
    assert not bad.any(), f"{what}: {bad.sum()} elements more than one ulp (+ fp32 noise) from the rounded oracle, worst {err.max():.4g}"
    exact = float(np.mean(y == yr))
    assert exact >= (0.97 if dtype == torch.float16 else 0.995), f"{what}: only {exact:.4f} of the outputs equal the correctly rounded result"


def _oracle(layer, x):
    codes, cb, sc, _ = layer
    f = lambda t: t.float().cpu().numpy()  # noqa: E731
    return orc.dequantize_gemm(f(x.view(1, -1)), codes.cpu().numpy(), f(cb), f(sc), None)[0]


def _packed_layers(layers, g):
    from aqlm_amd.inference_kernels import hip_kernel as hk

    out = []
    for per in layers:
        row = []
        for codes, cb, sc, bias in per:
            packed = hk.prepack_1x16(codes, g, codebooks=cb, uniform_only=True)
            assert packed is not None
            row.append((packed, cb, sc, bias))
        out.append(row)
    return out


def _routings(T, k, gen, dev):
    rnd = torch.topk(torch.rand((T, E), generator=gen, device=dev), k, dim=-1).indices
    return {"distinct": rnd, "one_expert": torch.full((T, k), 5, dtype=torch.int64, device=dev),
            "duplicates": rnd[:, :1].repeat(1, k).to(torch.int32)}


def _cells_at_rest():
    from aqlm_amd.inference_kernels import hip_kernel as hk

    torch.cuda.synchronize()
    assert hk._ROUTED_PACKED_CELLS, "no accumulator cells were allocated"
    return all(int(torch.count_nonzero(c)) == 0 for c in hk._ROUTED_PACKED_CELLS.values())


def _run_and_check(layers, packed, table, tail, S, fin, fout, g, dtype, per_pair, cases, gen, dev, what, oracle_pairs):
    from aqlm_amd.inference_kernels import hip_kernel as hk

    for T, k in cases:
        for rname, ids in _routings(T, k, gen, dev).items():
            rows = T * k if per_pair else T
            x = torch.randn((rows, fin), generator=gen, device=dev).to(dtype)
            y = torch.ops.aqlm.code1x16_moe_matmat_packed(x, ids, table, [E, S, fout, fin, g, k] + tail, per_pair)
            assert tuple(y.shape) == (T * k, S, fout)
            assert _cells_at_rest(), f"{what} T{T} k{k} {rname}: cells not zero after the launch"
            for p, e in enumerate(ids.long().cpu().view(-1).tolist()):
                xr = x[p if per_pair else p // k]
                for s in range(S):
                    pk, cb, sc, _ = packed[e][s]
                    ref = hk.code1x16_matmat_packed(xr.view(1, -1), pk, cb, sc, None)
                    tag = f"{what} T{T} k{k} {rname} pair {p} expert {e} seg {s}"
                    assert torch.equal(y[p, s].view(1, -1), ref), f"{tag}: not bit-identical to aqlm_hip_gemv_1x16_packed at batch 1"
                    if p < oracle_pairs:
                        check_rounded(y[p, s].float().cpu().numpy(), _oracle(layers[e][s], xr), dtype, tag)


SMALL = [("w13", 2, 512, 1024, False), ("w2", 1, 1024, 512, True)]
FULL = [("w13", 2, 4096, 14336, False), ("w2", 1, 14336, 4096, True)]


@pytest.mark.parametrize("g", [8, 16])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("shape", SMALL, ids=[s[0] for s in SMALL])
def test_routed_packed_op_is_bit_identical_and_matches_the_oracle_small_blocks(g, dtype, shape):
    from aqlm_amd.inference_kernels import hip_kernel as hk

    name, S, fin, fout, per_pair = shape
    dev = torch.device("cuda:0")
    layers = _experts(100 + 10 * g + SMALL.index(shape), S, fin, fout, g, dtype, dev)
    packed = _packed_layers(layers, g)
    table, tail = hk.routed_packed_table(packed, dev)
    gen = torch.Generator(device=dev).manual_seed(11)
    # pairs 1, 2, 7, 64
    _run_and_check(layers, packed, table, tail, S, fin, fout, g, dtype, per_pair, [(1, 1), (1, 2), (7, 1), (32, 2)], gen, dev,
                   f"{name} g{g} {dtype}", oracle_pairs=8)


@pytest.mark.parametrize("g", [8, 16])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("shape", FULL, ids=[s[0] for s in FULL])
def test_routed_packed_op_is_bit_identical_and_matches_the_oracle_full_size_block(g, dtype, shape):
    from aqlm_amd.inference_kernels import hip_kernel as hk

    name, S, fin, fout, per_pair = shape
    dev = torch.device("cuda:0")
    layers = _experts(200 + 10 * g + FULL.index(shape), S, fin, fout, g, dtype, dev)
    packed = _packed_layers(layers, g)
    assert hk.routed_packed_supported([p[0] for per in packed for p in per])
    table, tail = hk.routed_packed_table(packed, dev)
    gen = torch.Generator(device=dev).manual_seed(12)
    _run_and_check(layers, packed, table, tail, S, fin, fout, g, dtype, per_pair, [(1, 1), (1, 2), (7, 1)], gen, dev,
                   f"full {name} g{g} {dtype}", oracle_pairs=1)
    # 64 pairs, once per shape: all on one expert (64 passes of its workgroups) and a router's distinct picks
    for rname, ids in _routings(32, 2, gen, dev).items():
        if rname == "duplicates":
            continue
        x = torch.randn((64 if per_pair else 32, fin), generator=gen, device=dev).to(dtype)
        y = torch.ops.aqlm.code1x16_moe_matmat_packed(x, ids, table, [E, S, fout, fin, g, 2] + tail, per_pair)
        assert _cells_at_rest()
        for p, e in list(enumerate(ids.long().cpu().view(-1).tolist()))[::9]:
            xr = x[p if per_pair else p // 2]
            for s in range(S):
                pk, cb, sc, _ = packed[e][s]
                assert torch.equal(y[p, s].view(1, -1), hk.code1x16_matmat_packed(xr.view(1, -1), pk, cb, sc, None)), (rname, p, e, s)


def test_hostile_ids_give_zero_rows_and_leave_the_others_alone():
    """-1, num_experts, 2^40 and random int64 garbage: zero rows for those pairs, correct rows for the rest, cells at rest."""
    from aqlm_amd.inference_kernels import hip_kernel as hk

    dev, g, dtype, S, fin, fout = torch.device("cuda:0"), 8, torch.float16, 2, 512, 1024
    layers = _experts(300, S, fin, fout, g, dtype, dev)
    packed = _packed_layers(layers, g)
    table, tail = hk.routed_packed_table(packed, dev)
    gen = torch.Generator(device=dev).manual_seed(13)
    T, k = 16, 2
    ids = torch.topk(torch.rand((T, E), generator=gen, device=dev), k, dim=-1).indices
    garbage = torch.randint(-2 ** 62, 2 ** 62, (8,), generator=gen, device=dev, dtype=torch.int64)
    garbage = torch.where((garbage >= 0) & (garbage < E), garbage + E, garbage)
    bad = torch.cat([torch.tensor([-1, E, 2 ** 40, -(2 ** 40)], device=dev), garbage])
    flat = ids.view(-1)
    flat[::3] = bad[torch.arange(flat[::3].numel(), device=dev) % bad.numel()]
    x = torch.randn((T, fin), generator=gen, device=dev).to(dtype)
    y = torch.ops.aqlm.code1x16_moe_matmat_packed(x, ids, table, [E, S, fout, fin, g, k] + tail, False)
    assert _cells_at_rest()
    n_bad = 0
    for p, e in enumerate(flat.cpu().tolist()):
        if not 0 <= e < E:
            n_bad += 1
            assert torch.count_nonzero(y[p]) == 0, (p, e)
            continue
        for s in range(S):
            pk, cb, sc, _ = packed[e][s]
            assert torch.equal(y[p, s].view(1, -1), hk.code1x16_matmat_packed(x[p // k].view(1, -1), pk, cb, sc, None)), (p, e, s)
    assert n_bad >= 8
    ids32 = ids.clamp(-5, E + 5).to(torch.int32)  # int32 ids, some still out of range
    y32 = torch.ops.aqlm.code1x16_moe_matmat_packed(x, ids32, table, [E, S, fout, fin, g, k] + tail, False)
    for p, e in enumerate(ids32.view(-1).cpu().tolist()):
        if not 0 <= e < E:
            assert torch.count_nonzero(y32[p]) == 0, (p, e)
    assert _cells_at_rest()


def _prepacked_module(monkeypatch, H, I, dtype, dev, seed=0, max_pairs=64):
    import aqlm_amd.moe as moe

    cfg, q, dense = _module(H, I, dtype, dev, seed=seed)
    monkeypatch.setattr(moe, "ROUTED_PACKED_MAX_PAIRS", max_pairs)
    rep = moe.prepack_experts(q, min_codes=1)
    assert rep["blocks"] == 1 and rep["layers_packed"] == 3 * E and rep["blocks_served"] == 1 and rep["blocks_fallback"] == 0
    assert rep["packed_bytes"] > 0
    return cfg, q, dense


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_block_forward_after_prepack_experts(monkeypatch, dtype):
    """Against the same block before prepacking within the block test's tolerance (direct and packed kernel sum in different
    orders), and the projection outputs bit for bit against the per-expert loop on the prepacked experts."""
    from aqlm_amd.inference_kernels import hip_kernel as hk

    dev = torch.device("cuda:0")
    _, plain, _ = _module(1024, 2048, dtype, dev)
    _, q, _ = _prepacked_module(monkeypatch, 1024, 2048, dtype, dev)
    gen = torch.Generator(device=dev).manual_seed(3)
    calls = []
    real = torch.ops.aqlm.code1x16_moe_matmat_packed

    for T in (1, 2, 4, 16, 32, 40):
        x = torch.randn((T, 1024), generator=gen, device=dev).to(dtype)
        ids, w = _route(T, 2, gen, dev)
        with torch.no_grad():
            tables = q._routed_packed_tables_for(x, ids)
            assert (tables is not None) == (T * 2 <= 64), T
            y, y_plain = q(x, ids, w).double(), plain(x, ids, w).double()
            rel = ((y - y_plain).abs().mean() / y_plain.abs().mean()).item()
            assert rel < (2e-3 if dtype == torch.float16 else 1.6e-2), (T, rel)
            if tables is None:
                assert torch.equal(y, y_plain)  # beyond the cross-over nothing changes
                continue
            (tab13, tail13), (tab2, tail2) = tables
            gu = real(x, ids, tab13, [E, 2, 2048, 1024, 8, 2] + tail13, False)
            h = q.act_fn(gu[:, 0]) * gu[:, 1]
            y2 = real(h, ids, tab2, [E, 1, 1024, 2048, 8, 2] + tail2, True)
            for p, e in enumerate(ids.view(-1).cpu().tolist()):  # the per-expert loop on the prepacked experts
                ex = q.expert(e)
                for s, lin in enumerate((ex.w1, ex.w3)):
                    ref = hk.code1x16_matmat_packed(x[p // 2].view(1, -1), lin._packed_codes, lin.codebooks, lin.scales, None)
                    assert torch.equal(gu[p, s].view(1, -1), ref), (T, p, e, s)
                ref = hk.code1x16_matmat_packed(h[p].view(1, -1), ex.w2._packed_codes, ex.w2.codebooks, ex.w2.scales, None)
                assert torch.equal(y2[p, 0].view(1, -1), ref), (T, p, e)
            calls.append(T)
    assert calls == [1, 2, 4, 16, 32]
    # a gradient needed: today's route (the packed launch has no backward)
    xg = torch.randn((2, 1024), generator=gen, device=dev).to(dtype).requires_grad_()
    ids, w = _route(2, 2, gen, dev)
    assert q._routed_packed_tables_for(xg, ids) is None
    q(xg, ids, w).float().sum().backward()
    assert torch.isfinite(xg.grad.float()).all()


def test_routed_packed_forward_makes_no_host_sync(monkeypatch):
    dev = torch.device("cuda:0")
    _, q, _ = _prepacked_module(monkeypatch, 1024, 2048, torch.float16, dev)
    gen = torch.Generator(device=dev).manual_seed(4)
    x = torch.randn((4, 1024), generator=gen, device=dev).half()
    ids, w = _route(4, 2, gen, dev)
    with torch.no_grad():
        assert q._routed_packed_tables_for(x, ids) is not None
        q(x, ids, w)  # tables and cells exist now
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            y = q(x, ids, w)
        finally:
            torch.cuda.set_sync_debug_mode("default")
    assert torch.isfinite(y.float()).all()


@pytest.mark.parametrize("T", [1, 4])
def test_prepacked_block_decode_step_replays_from_a_graph(monkeypatch, T):
    from transformers.models.mixtral.modeling_mixtral import MixtralSparseMoeBlock

    dev = torch.device("cuda:0")
    cfg, q, _ = _prepacked_module(monkeypatch, 1024, 2048, torch.float16, dev, seed=5)
    block = MixtralSparseMoeBlock(cfg).to(dev, torch.float16).eval()
    with torch.no_grad():
        block.gate.weight.normal_(0, 0.5)
    block.experts = q
    taken = []
    real = q._forward_routed_packed
    monkeypatch.setattr(q, "_forward_routed_packed", lambda *a: (taken.append(1), real(*a))[1])
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
        assert len(taken) == 3, "the captured step did not take the routed packed launches"
        routes = set()
        for x in inputs:
            static.copy_(x)
            graph.replay()
            eager = block(x)
            torch.cuda.synchronize()
            assert torch.equal(out, eager)
            routes.add(tuple(block.gate(x.view(-1, 1024))[2].view(-1).tolist()))
    assert len(routes) == 3, "the three inputs should route differently"
    assert _cells_at_rest()


def test_a_rewritten_codebook_is_never_served_stale(monkeypatch):
    """``codebooks.data.mul_(2)`` changes neither identity nor version of the parameter: the next forward must still compute
    with the new codebook.  Versioned writes and ``invalidate_derived_state()`` rebuild the packed copy and the table."""
    dev, dtype = torch.device("cuda:0"), torch.float16
    _, q, _ = _prepacked_module(monkeypatch, 1024, 2048, dtype, dev, seed=7)
    _, fresh, _ = _module(1024, 2048, dtype, dev, seed=7)  # the same weights, never prepacked: today's route on the live tensors
    gen = torch.Generator(device=dev).manual_seed(8)
    x = torch.randn((2, 1024), generator=gen, device=dev).to(dtype)
    ids = torch.tensor([[0, 3], [3, 5]], device=dev)
    w = torch.full((2, 2), 0.5, device=dev)

    def agree(what):
        with torch.no_grad():
            assert q._routed_packed_tables_for(x, ids) is not None, what
            y, ref = q(x, ids, w).double(), fresh(x, ids, w).double()
        rel = ((y - ref).abs().mean() / ref.abs().mean()).item()
        assert rel < 2e-3, (what, rel)
        return y

    y0 = agree("before")
    for blk in (q, fresh):
        blk.expert(3).w1.codebooks.data.mul_(2)
    y1 = agree("codebook written through .data")
    assert ((y1 - y0).abs().mean() / y0.abs().mean()).item() > 1e-2, "the doubled codebook should change the output"
    with torch.no_grad():
        for blk in (q, fresh):
            blk.expert(0).w2.codebooks.mul_(0.5)  # versioned write: range and table are rebuilt
    table_before = q._packed_tables
    agree("codebook written in place")
    assert q._packed_tables is not table_before
    with torch.no_grad():
        new_codes = torch.randint(-32768, 32768, q.expert(5).w3.codes.shape, generator=gen, device=dev, dtype=torch.int32).to(torch.int16)
        for blk in (q, fresh):
            blk.expert(5).w3.codes.copy_(new_codes)  # the packed copy is derived from the codes: repacked
    agree("codes written in place")
    packed_before = q.expert(3).w1._packed_codes
    q.expert(3).w1.invalidate_derived_state()
    table_before = q._packed_tables
    agree("after invalidate_derived_state()")
    assert q._packed_tables is not table_before and q.expert(3).w1._packed_codes is not packed_before


def test_tiny_mixtral_checkpoint_end_to_end_with_prepacked_experts(monkeypatch, tmp_path):
    pytest.importorskip("transformers")
    import aqlm_amd.moe as moe
    from tests import moe_checkpoint as mc

    mc.build(tmp_path / "ckpt")
    model, info = mc.load(str(tmp_path / "ckpt"), "cuda:0")
    plain, _ = mc.load(str(tmp_path / "ckpt"), "cuda:0")
    assert not info["missing_keys"] and not info["unexpected_keys"]
    monkeypatch.setattr(moe, "ROUTED_PACKED_MAX_PAIRS", 64)
    rep = moe.prepack_experts(model, min_codes=1)
    assert rep["blocks"] == mc.LAYERS and rep["blocks_served"] == mc.LAYERS and rep["layers_packed"] == mc.LAYERS * mc.EXPERTS * 3
    taken = []
    for blk in (m for m in model.modules() if isinstance(m, moe.QuantizedMixtralExperts)):
        real = blk._forward_routed_packed
        monkeypatch.setattr(blk, "_forward_routed_packed", lambda *a, real=real: (taken.append(1), real(*a))[1])
    gen = torch.Generator().manual_seed(0)
    with torch.no_grad():
        for shape in ((1, 9), (2, 40)):  # 18 pairs: routed packed launches; 160 pairs: today's route
            ids = torch.randint(0, mc.VOCAB, shape, generator=gen).to("cuda:0")
            a, b = model(ids).logits.float(), plain(ids).logits.float()
            rel = ((a - b).abs().mean() / b.abs().mean()).item()
            assert rel < 2e-2, (shape, rel)
    assert len(taken) == mc.LAYERS, "only the 9-token call takes the routed packed launches"
