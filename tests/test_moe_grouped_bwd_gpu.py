"""The backward of the expert-grouped 1x16 GEMM on the MI355X: the transposed grouped launch (aqlm_hip_gemm_1x16_grouped_transposed,
``aqlm::code1x16_moe_matmat_grouped_transposed``) against the fp64 oracle -- both projection groups, ragged shapes, every tile
size, other expert counts and top_k --, bit-for-bit independent of the other pairs, zero rows for ids without an expert, and the
QuantizedMixtralExperts backward on it: no host sync, gradients against autograd through a dense fp64 twin (device route and the
per-expert loop), forward + backward captured in one hipGraph, one check at Mixtral's size.

gx[p] = sum_s (gy[p, s] * scales) @ Wq is fp32; the bounds are ``_check``'s for the storage type (tests/test_moe_gpu.py ``TOL``),
applied to that fp32 output.  The launch rounds gy * scales once to the storage type: a relative error of at most 2^-11 (fp16) /
2^-8 (bf16) per operand, independent between the terms of a sum, i.e. about 3.5e-4 / 2.8e-3 of mean |y| per element -- inside the
per-element bounds of 2e-3 / 1.6e-2."""
import pytest
import torch

from tests.test_moe_gpu import E, _check, _experts, _module, _route, _w64

K = 2
OP_SHAPES = [("w13", 2, 1024, 2048), ("w2", 1, 2048, 1024)]  # name, segments, in_features (columns of gx), out_features (of gy)
DTYPES = [torch.float16, torch.bfloat16]


def _ids(T, gen, dev, n=E, k=K):
    return torch.topk(torch.rand((T, n), generator=gen, device=dev), k, dim=-1).indices


def _bwd(gy, ids, table, n, S, fin, fout, g):
    """the transposed grouped launch on the ids' own bucket -> (gx fp32 [P, fin], tile_pairs, bucket)"""
    from aqlm_amd.inference_kernels import hip_kernel as hk

    assert hk.grouped_transposed_supported(fout, fin, g), f"the entry declined {fin} <- {fout} g{g}"
    P, k = ids.numel(), ids.shape[1]
    tp = hk.grouped_tile_pairs(P, n)
    bucket = torch.ops.aqlm.moe_bucket(ids, n, tp)
    gx = torch.ops.aqlm.code1x16_moe_matmat_grouped_transposed(gy, bucket, table, [n, S, fout, fin, g, k, tp, P])
    assert gx.dtype == torch.float32 and tuple(gx.shape) == (P, fin)
    return gx, tp, bucket


def _check_bwd(gx, gy, ids, layers, dtype, what, w64=None, experts=None):
    """Per expert: gx[pairs] against sum_s gy64[pairs, s] @ _w64(layer) (``_w64`` includes the scales); pairs without an expert:
    zero rows.  ``w64``: a cache {(e, s): matrix} shared between calls on the same layers."""
    n = len(layers)
    flat = ids.reshape(-1).long()
    orphans = (flat < 0) | (flat >= n)
    assert torch.count_nonzero(gx[orphans]) == 0, f"{what}: rows of pairs without an expert must be zero"
    w64 = {} if w64 is None else w64
    seen = int(orphans.sum())
    for e in range(n):
        pairs = torch.nonzero(flat == e).squeeze(1)
        seen += pairs.numel()
        if pairs.numel() == 0 or (experts is not None and e not in experts):
            continue
        ref = None
        for s in range(len(layers[e])):
            if (e, s) not in w64:
                w64[(e, s)] = _w64(layers[e][s])
            part = gy[pairs, s].double() @ w64[(e, s)]
            ref = part if ref is None else ref + part
        _check(gx[pairs], ref, dtype, f"{what} expert {e}")
    assert seen == flat.numel()


# ---------------------------------------------------------------------------------------------------------------------------
# (a) the op against the fp64 oracle
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("g", [8, 16])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", OP_SHAPES, ids=[s[0] for s in OP_SHAPES])
def test_transposed_op_matches_oracle(g, dtype, shape):
    from aqlm_amd.inference_kernels import hip_kernel as hk

    name, S, fin, fout = shape
    dev = torch.device("cuda:0")
    layers = _experts(200 + g, S, fin, fout, g, dtype, dev)
    table = hk.routed_table(layers, dev)
    gen = torch.Generator(device=dev).manual_seed(31)
    w64 = {}
    for T in (1, 33, 100, 300):
        ids = _ids(T, gen, dev)
        gy = torch.randn((T * K, S, fout), generator=gen, device=dev).to(dtype)
        gx, _, _ = _bwd(gy, ids, table, E, S, fin, fout, g)
        _check_bwd(gx, gy, ids, layers, dtype, f"{name} g{g} {dtype} T{T}", w64)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------------
# (b) ragged edges: 2064 = 16 x 129 output rows (a half step of 16 rows at the end), 1088 = 17 x 64 columns (a partial column block)
# ---------------------------------------------------------------------------------------------------------------------------
RAGGED = [("out2064_in1088_S2", 2, 1088, 2064), ("out2064_in1088_S1", 1, 1088, 2064), ("out1088_in2064_S1", 1, 2064, 1088)]


@pytest.mark.gpu
@pytest.mark.parametrize("g", [8, 16])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", RAGGED, ids=[s[0] for s in RAGGED])
def test_transposed_op_on_ragged_shapes(g, dtype, shape):
    from aqlm_amd.inference_kernels import hip_kernel as hk

    name, S, fin, fout = shape
    dev = torch.device("cuda:0")
    layers = _experts(300 + g, S, fin, fout, g, dtype, dev)  # (no bias)
    table = hk.routed_table(layers, dev)
    gen = torch.Generator(device=dev).manual_seed(32)
    w64 = {}
    for T in (5, 100):
        ids = _ids(T, gen, dev)
        gy = torch.randn((T * K, S, fout), generator=gen, device=dev).to(dtype)
        gx, _, _ = _bwd(gy, ids, table, E, S, fin, fout, g)
        _check_bwd(gx, gy, ids, layers, dtype, f"{name} g{g} {dtype} T{T}", w64)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------------
# (c) tile edges
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("tile_pairs", [16, 32, 64, 128])
def test_transposed_op_at_the_tile_edges(tile_pairs, dtype):
    """As test_grouped_op_at_the_tile_edges: for every tile size an expert with exactly one tile of pairs next to one with one pair
    more, 300 pairs on the last expert, 65 routed pairs."""
    from aqlm_amd.inference_kernels import hip_kernel as hk
    from tests import moe_experts as mx

    dev, g, tp = torch.device("cuda:0"), 8, tile_pairs
    name, S, fin, fout = OP_SHAPES[0]
    all_layers = mx.plain_experts(60, 700, S, fin, fout, g, dtype, dev)
    gen = torch.Generator(device=dev).manual_seed(33)
    w64 = {}

    def run(n, ids, what):
        layers = all_layers[:n]
        P = ids.numel()
        assert P % 16 != 0 and hk.grouped_tile_pairs(P, n) == tp, (what, P, n, hk.grouped_tile_pairs(P, n))
        gy = torch.randn((P, S, fout), generator=gen, device=dev).to(dtype)
        gx, got_tp, bucket = _bwd(gy, ids, hk.routed_table(layers, dev), n, S, fin, fout, g)
        counts = torch.bincount(ids.view(-1), minlength=n).tolist()
        tiles = sum(-(-c // tp) for c in counts)
        assert got_tp == tp and bucket[:4].tolist() == [tiles, 0, P, 0], (what, bucket[:4].tolist(), tiles)
        _check_bwd(gx, gy, ids, layers, dtype, f"{what} tp{tp} {dtype}", w64)
        return tiles

    P = 3 * tp - 5
    ids = torch.cat([torch.full((tp,), 0), torch.full((tp + 1,), 1), torch.full((P - 2 * tp - 1,), 2)])
    ids = ids[torch.randperm(P)].view(P, 1).to(dev)
    assert run(3, ids, "full tile and full tile + 1") == 4
    n = {16: 60, 32: 16, 64: 8, 128: 3}[tp]
    assert run(n, torch.full((300, 1), n - 1, dtype=torch.int64, device=dev), "300 pairs on one expert") == -(-300 // tp)
    n = {16: 60, 32: 3, 64: 2, 128: 1}[tp]
    run(n, mx.router_ids(65, 1, n, gen, dev), "65 pairs")
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------------
# (d) independence and determinism
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", OP_SHAPES, ids=[s[0] for s in OP_SHAPES])
def test_transposed_rows_do_not_depend_on_the_other_pairs(shape, dtype):
    from aqlm_amd.inference_kernels import hip_kernel as hk

    name, S, fin, fout = shape
    dev = torch.device("cuda:0")
    layers = _experts(9, S, fin, fout, 8, dtype, dev)
    table = hk.routed_table(layers, dev)
    gen = torch.Generator(device=dev).manual_seed(34)
    T = 300
    ids = _ids(T, gen, dev)
    gy = torch.randn((T, K, S, fout), generator=gen, device=dev).to(dtype)

    def run(sel=None):
        i, y = (ids, gy) if sel is None else (ids[sel], gy[sel])
        return _bwd(y.reshape(-1, S, fout), i, table, E, S, fin, fout, 8)[0].view(-1, K, fin)

    gx = run()
    assert torch.equal(run(), gx), "two calls differ"
    perm = torch.randperm(T, generator=gen, device=dev)
    assert torch.equal(run(perm), gx[perm]), "permuting the tokens changed a pair's bits"
    for keep in (40, 17, 1):  # fewer pairs: other tile sizes, other tiles, other slots
        sel = perm[:keep]
        assert torch.equal(run(sel), gx[sel]), f"dropping pairs changed a pair's bits ({keep} tokens kept)"
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------------
# (e) ids without an expert
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("ids_dtype", [torch.int64, torch.int32])
@pytest.mark.parametrize("shape", OP_SHAPES, ids=[s[0] for s in OP_SHAPES])
def test_transposed_out_of_range_ids_give_zero_rows(shape, ids_dtype):
    from aqlm_amd.inference_kernels import hip_kernel as hk

    name, S, fin, fout = shape
    dev = torch.device("cuda:0")
    layers = _experts(10, S, fin, fout, 16, torch.float16, dev)
    table = hk.routed_table(layers, dev)
    gen = torch.Generator(device=dev).manual_seed(35)
    T = 100
    ids = _ids(T, gen, dev)
    gy = torch.randn((T * K, S, fout), generator=gen, device=dev).half()
    gx = _bwd(gy, ids, table, E, S, fin, fout, 16)[0]
    bad = ids.clone()
    values = torch.tensor([-1, E, 1000, -(2 ** 31), 2 ** 31], device=dev)  # (int32: 2^31 wraps to -2^31, as invalid)
    sel = torch.arange(bad.numel(), device=dev)[::3]
    bad.view(-1)[sel] = values[sel % values.numel()]
    gxb = _bwd(gy, bad.to(ids_dtype), table, E, S, fin, fout, 16)[0]
    hit = torch.zeros(bad.numel(), dtype=torch.bool, device=dev)
    hit[sel] = True
    assert torch.count_nonzero(gxb[hit]) == 0
    assert torch.equal(gxb[~hit], gx[~hit])
    every = torch.full_like(ids, -5).to(ids_dtype)  # no pair on any expert: every row zero
    assert torch.count_nonzero(_bwd(gy, every, table, E, S, fin, fout, 16)[0]) == 0
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------------
# (f) other expert counts and top_k
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("top_k", [1, 4, 8])
@pytest.mark.parametrize("num_experts", [1, 3, 60])
def test_transposed_op_with_other_expert_counts_and_top_k(num_experts, top_k, dtype):
    """As test_grouped_op_with_other_expert_counts_top_k_bias_and_strided_x: 1, 3 and 60 experts (ids E - 1, E and -1 present),
    top_k 1 / 4 / 8, 99 / 100 / 104 pairs, a bias per layer (which must not enter), gy a contiguous copy of a strided tensor."""
    from aqlm_amd.inference_kernels import hip_kernel as hk
    from tests import moe_experts as mx

    dev, g, n = torch.device("cuda:0"), 8, num_experts
    gen = torch.Generator(device=dev).manual_seed(36)
    T = {1: 99, 4: 25, 8: 13}[top_k]
    for name, S, fin, fout in OP_SHAPES:
        layers = mx.plain_experts(n, 800 + n, S, fin, fout, g, dtype, dev, bias=True)
        table = hk.routed_table(layers, dev)
        w64 = {}
        for ids_dtype in (torch.int64, torch.int32):
            ids = mx.router_ids(T, top_k, n, gen, dev, ids_dtype)
            ids.view(-1)[:3] = torch.tensor([n - 1, n, -1], dtype=ids_dtype, device=dev)
            wide = torch.randn((T * top_k, S, fout + 24), generator=gen, device=dev).to(dtype)[:, :, 8:8 + fout]
            assert not wide.is_contiguous()
            gy = wide.contiguous()
            gx, _, _ = _bwd(gy, ids, table, n, S, fin, fout, g)
            _check_bwd(gx, gy, ids, layers, dtype, f"{name} E{n} k{top_k} {dtype} {ids_dtype}", w64)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------------
# (g) module level
# ---------------------------------------------------------------------------------------------------------------------------
def _step(q, x0, ids, w0, r):
    x, w = x0.clone().requires_grad_(), w0.clone().requires_grad_()
    y = q(x, ids, w)
    (y.float() * r).sum().backward()
    return x.grad, w.grad


@pytest.mark.gpu
@pytest.mark.parametrize("T", [3, 40, 200])
def test_forward_and_backward_make_no_host_sync(T):
    dev = torch.device("cuda:0")
    _, q, _ = _module(1024, 2048, torch.float16, dev, seed=37)
    gen = torch.Generator(device=dev).manual_seed(38)
    x0 = torch.randn((T, 1024), generator=gen, device=dev).half()
    ids, w0 = _route(T, K, gen, dev)
    r = torch.randn((T, 1024), generator=gen, device=dev)
    _step(q, x0, ids, w0, r)  # warm-up: builds the device tables (one host-to-device copy)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        gx, gw = _step(q, x0, ids, w0, r)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.isfinite(gx.float()).all() and torch.isfinite(gw.float()).all()


@pytest.mark.gpu
@pytest.mark.parametrize("device_route", [True, False], ids=["device", "loop"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_gradients_match_a_dense_fp64_twin_on_both_routes(dtype, device_route, monkeypatch):
    """The bounds of test_gradients_match_a_dense_fp64_twin (5e-3 fp16, 3e-2 bf16), on the transposed grouped launch and, with
    GROUPED_BACKWARD off, on the per-expert loop."""
    from aqlm_amd import moe
    from tests.test_moe_grouped_gpu import _dense64, _moe64, _rel

    monkeypatch.setattr(moe, "GROUPED_BACKWARD", device_route)
    dev = torch.device("cuda:0")
    _, q, _ = _module(1024, 2048, dtype, dev, seed=39)
    gate_up, down = _dense64(q)
    gen = torch.Generator(device=dev).manual_seed(40)
    bound = 5e-3 if dtype == torch.float16 else 3e-2
    calls = []
    real = moe._GroupedProjection.backward

    def spy(ctx, grad_y):
        calls.append(moe.takes_grouped_backward(moe.GROUPED_BACKWARD, ctx.experts._grouped_backward_shapes(*ctx.geometry[2:5])))
        return real(ctx, grad_y)

    monkeypatch.setattr(moe._GroupedProjection, "backward", staticmethod(spy))
    for T in (3, 40, 200):
        x0 = torch.randn((T, 1024), generator=gen, device=dev).to(dtype)
        ids, w0 = _route(T, K, gen, dev)
        r = torch.randn((T, 1024), generator=gen, device=dev)
        gx, gw = _step(q, x0, ids, w0, r)
        x64, w64 = x0.double().requires_grad_(), w0.double().requires_grad_()
        (_moe64(gate_up, down, x64, ids, w64) * r.double()).sum().backward()
        assert _rel(gx, x64.grad) <= bound, (T, "x.grad", _rel(gx, x64.grad))
        assert _rel(gw, w64.grad) <= bound, (T, "top_k_weights.grad", _rel(gw, w64.grad))
    assert calls == [device_route] * 6, calls  # two projection groups per step, each on the route asked for


@pytest.mark.gpu
@pytest.mark.parametrize("T", [48, 200])
def test_training_step_of_the_experts_replays_from_a_graph(T):
    dev = torch.device("cuda:0")
    _, q, _ = _module(1024, 2048, torch.float16, dev, seed=41)
    gen = torch.Generator(device=dev).manual_seed(42)
    cases = []
    for _ in range(3):
        x0 = torch.randn((T, 1024), generator=gen, device=dev).half()
        ids, w0 = _route(T, K, gen, dev)
        cases.append((x0, ids, w0, torch.randn((T, 1024), generator=gen, device=dev).half()))
    assert len({tuple(c[1].view(-1).tolist()) for c in cases}) == 3, "the three inputs should route differently"
    x = cases[0][0].clone().requires_grad_()
    s_ids, s_w, s_gy = cases[0][1].clone(), cases[0][2].clone(), cases[0][3].clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            x.grad = None
            q(x, s_ids, s_w).backward(s_gy)
    torch.cuda.current_stream().wait_stream(s)
    x.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        q(x, s_ids, s_w).backward(s_gy)
    grad = x.grad
    for x0, ids, w0, gy in cases:
        with torch.no_grad():
            x.copy_(x0)
        s_ids.copy_(ids)
        s_w.copy_(w0)
        s_gy.copy_(gy)
        graph.replay()
        xe = x0.clone().requires_grad_()
        q(xe, ids, w0).backward(gy)
        torch.cuda.synchronize()
        assert torch.equal(grad, xe.grad)


@pytest.mark.gpu
def test_full_mixtral_shapes_at_64_tokens():
    from aqlm_amd.inference_kernels import hip_kernel as hk

    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(43)
    T = 64
    ids = _ids(T, gen, dev)
    for name, S, fin, fout in (("w13", 2, 4096, 14336), ("w2", 1, 14336, 4096)):
        layers = _experts(22, S, fin, fout, 8, torch.float16, dev)
        table = hk.routed_table(layers, dev)
        gy = torch.randn((T * K, S, fout), generator=gen, device=dev).half()
        gx, _, _ = _bwd(gy, ids, table, E, S, fin, fout, 8)
        assert torch.isfinite(gx).all()
        _check_bwd(gx, gy, ids, layers, torch.float16, name, experts=(0, 5))  # (an fp64 W of 14336 x 4096 is 470 MB)
        del layers, table
    torch.cuda.synchronize()
