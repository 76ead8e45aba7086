"""Mixtral experts on the MI355X, more than 64 (token, expert) pairs or a gradient: the expert-grouped 1x16 GEMM
(aqlm_hip_moe_bucket + aqlm_hip_gemm_1x16_grouped) against the fp64 oracle, bit for bit against code1x16_matmat_dequant under
gemm_variant = 2, independent of the other pairs, the device bucket against a numpy model, and the QuantizedMixtralExperts forward
on it: no host sync, hipGraph capture of prefill-sized MoE blocks, gradients against autograd through a dense fp64 twin.

Tolerances are those of tests/test_moe_gpu.py (restated there from tests/test_hip_parity.py)."""
import numpy as np
import pytest
import torch

from tests.test_moe_gpu import E, _check, _experts, _module, _route, _w64

TOKENS = (33, 40, 100, 300)
K = 2


def _ids(T, gen, dev):
    return torch.topk(torch.rand((T, E), generator=gen, device=dev), K, dim=-1).indices


def _grouped(x, ids, table, S, fin, fout, g, per_pair):
    from aqlm_amd.inference_kernels import hip_kernel as hk

    P = ids.numel()
    tp = hk.grouped_tile_pairs(P, E)
    bucket = torch.ops.aqlm.moe_bucket(ids, E, tp)
    return torch.ops.aqlm.code1x16_moe_matmat_grouped(x, bucket, table, [E, S, fout, fin, g, K, tp, P], per_pair)


class _Variant:
    """gemm_variant = 2: the large-batch op runs its 16-row kernel wherever it applies (restored on exit)."""

    def __enter__(self):
        from aqlm_amd import _native

        self.old = _native.get_tuning("gemm_variant")
        _native.set_tuning("gemm_variant", 2)

    def __exit__(self, *exc):
        from aqlm_amd import _native

        _native.set_tuning("gemm_variant", self.old)


def _check_bits(y, x, ids, layers, per_pair, what):
    """each expert's rows == code1x16_matmat_dequant on that expert's x rows, bit for bit"""
    flat = ids.reshape(-1).long()
    for e in range(E):
        pairs = torch.nonzero(flat == e).squeeze(1)
        if pairs.numel() == 0:
            continue
        xe = x[pairs if per_pair else pairs // K]
        for s, (codes, cb, sc, _) in enumerate(layers[e]):
            ref = torch.ops.aqlm.code1x16_matmat_dequant(xe, codes, cb, sc, None)
            assert torch.equal(y[pairs, s], ref), f"{what} expert {e} seg {s}: not bit-identical to code1x16_matmat_dequant"


OP_SHAPES = [("w13", 2, 1024, 2048, False), ("w2", 1, 2048, 1024, True)]


@pytest.mark.gpu
@pytest.mark.parametrize("g", [8, 16])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("shape", OP_SHAPES, ids=[s[0] for s in OP_SHAPES])
def test_grouped_op_matches_oracle_and_the_mfma_op(g, dtype, shape):
    from aqlm_amd.inference_kernels import hip_kernel as hk

    name, S, fin, fout, per_pair = shape
    dev = torch.device("cuda:0")
    layers = _experts(100 + g, S, fin, fout, g, dtype, dev)
    table = hk.routed_table(layers, dev)
    w64 = [[_w64(layers[e][s]) for s in range(S)] for e in range(E)]
    gen = torch.Generator(device=dev).manual_seed(11)
    for T in TOKENS:
        ids = _ids(T, gen, dev)
        x = torch.randn((T * K if per_pair else T, fin), generator=gen, device=dev).to(dtype)
        y = _grouped(x, ids, table, S, fin, fout, g, per_pair)
        assert tuple(y.shape) == (T * K, S, fout)
        flat = ids.reshape(-1)
        for e in range(E):
            pairs = torch.nonzero(flat == e).squeeze(1)
            xe = x[pairs if per_pair else pairs // K].double()
            for s in range(S):
                _check(y[pairs, s], xe @ w64[e][s].T, dtype, f"{name} g{g} {dtype} T{T} expert {e} seg {s}")
        with _Variant():
            _check_bits(y, x, ids, layers, per_pair, f"{name} g{g} {dtype} T{T}")
    torch.cuda.synchronize()


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_grouped_rows_do_not_depend_on_the_other_pairs(dtype):
    from aqlm_amd.inference_kernels import hip_kernel as hk

    dev = torch.device("cuda:0")
    layers = _experts(7, 2, 1024, 2048, 8, dtype, dev)
    table = hk.routed_table(layers, dev)
    gen = torch.Generator(device=dev).manual_seed(12)
    T = 300
    ids = _ids(T, gen, dev)
    x = torch.randn((T, 1024), generator=gen, device=dev).to(dtype)
    y = _grouped(x, ids, table, 2, 1024, 2048, 8, False).view(T, K, 2, 2048)
    perm = torch.randperm(T, generator=gen, device=dev)
    yp = _grouped(x[perm], ids[perm], table, 2, 1024, 2048, 8, False).view(T, K, 2, 2048)
    assert torch.equal(yp, y[perm]), "permuting the tokens changed a pair's bits"
    for keep in (40, 33, 17, 1):  # fewer pairs: other tile sizes, other tiles, other slots
        sel = perm[:keep]
        ys = _grouped(x[sel], ids[sel], table, 2, 1024, 2048, 8, False).view(keep, K, 2, 2048)
        assert torch.equal(ys, y[sel]), f"dropping pairs changed a pair's bits ({keep} tokens kept)"
    torch.cuda.synchronize()


@pytest.mark.gpu
@pytest.mark.parametrize("ids_dtype", [torch.int64, torch.int32])
def test_out_of_range_ids_give_zero_rows(ids_dtype):
    from aqlm_amd.inference_kernels import hip_kernel as hk

    dev = torch.device("cuda:0")
    layers = _experts(8, 1, 2048, 1024, 16, torch.float16, dev)
    table = hk.routed_table(layers, dev)
    gen = torch.Generator(device=dev).manual_seed(13)
    T = 100
    ids = _ids(T, gen, dev)
    h = torch.randn((T * K, 2048), generator=gen, device=dev).half()
    y = _grouped(h, ids, table, 1, 2048, 1024, 16, True)
    bad = ids.clone()
    values = torch.tensor([-1, E, 1000, -(2 ** 31), 2 ** 31 - 1], device=dev)
    sel = torch.arange(bad.numel(), device=dev)[::3]
    bad.view(-1)[sel] = values[sel % values.numel()]
    yb = _grouped(h, bad.to(ids_dtype), table, 1, 2048, 1024, 16, True)
    hit = torch.zeros(bad.numel(), dtype=torch.bool, device=dev)
    hit[sel] = True
    assert torch.count_nonzero(yb[hit]) == 0
    assert torch.equal(yb[~hit], y[~hit])
    every = torch.full_like(ids, -5)  # no pair on any expert: every row zero
    assert torch.count_nonzero(_grouped(h, every, table, 1, 2048, 1024, 16, True)) == 0
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------------
# off the 8 experts / top-2 / no bias track, and the tile edges
# ---------------------------------------------------------------------------------------------------------------------------
def _grouped_n(x, ids, table, n, S, fin, fout, g, per_pair):
    """``_grouped`` for ``n`` experts and the ids' own top_k -> (y, tile_pairs, bucket)"""
    from aqlm_amd.inference_kernels import hip_kernel as hk

    P, k = ids.numel(), ids.shape[1]
    tp = hk.grouped_tile_pairs(P, n)
    bucket = torch.ops.aqlm.moe_bucket(ids, n, tp)
    return torch.ops.aqlm.code1x16_moe_matmat_grouped(x, bucket, table, [n, S, fout, fin, g, k, tp, P], per_pair), tp, bucket


def _check_grouped_n(y, x, ids, layers, per_pair, dtype, what):
    """Every pair: the fp64 oracle within ``_check``; bit for bit code1x16_matmat_dequant (+ bias) of its expert under
    gemm_variant = 2, in slabs of at most FUSED_MFMA_MAX_ROWS rows (beyond, that op dequantises and calls the library GEMM); pairs
    without an expert: zero rows."""
    from aqlm_amd.inference_kernels import hip_kernel as hk

    n, k = len(layers), ids.shape[1]
    flat = ids.reshape(-1).long()
    orphans = (flat < 0) | (flat >= n)
    assert torch.count_nonzero(y[orphans]) == 0, f"{what}: rows of pairs without an expert must be zero"
    seen = int(orphans.sum())
    for e in range(n):
        pairs = torch.nonzero(flat == e).squeeze(1)
        if pairs.numel() == 0:
            continue
        seen += pairs.numel()
        xe = x[pairs if per_pair else pairs // k]
        for s, (codes, cb, sc, bias) in enumerate(layers[e]):
            y64 = xe.double() @ _w64(layers[e][s]).T
            if bias is not None:
                y64 = y64 + bias.double()
            _check(y[pairs, s], y64, dtype, f"{what} expert {e} seg {s}")
            with _Variant():
                for r0 in range(0, pairs.numel(), hk.FUSED_MFMA_MAX_ROWS):
                    sl = slice(r0, r0 + hk.FUSED_MFMA_MAX_ROWS)
                    ref = torch.ops.aqlm.code1x16_matmat_dequant(xe[sl].contiguous(), codes, cb, sc, bias)
                    assert torch.equal(y[pairs[sl], s], ref), f"{what} expert {e} seg {s}: not bit-identical to code1x16_matmat_dequant"
    assert seen == flat.numel()


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("top_k", [1, 4, 8])
@pytest.mark.parametrize("num_experts", [1, 3, 60])
def test_grouped_op_with_other_expert_counts_top_k_bias_and_strided_x(num_experts, top_k, dtype):
    """1, 3 and 60 experts (ids E - 1, E and -1 present), top_k 1 / 4 / 8, a bias per expert and projection, x rows taken from a
    wider tensor; 99 / 100 / 104 pairs: more than the routed launch takes, none a multiple of 16."""
    from aqlm_amd.inference_kernels import hip_kernel as hk
    from tests import moe_experts as mx

    dev, g, n = torch.device("cuda:0"), 8, num_experts
    gen = torch.Generator(device=dev).manual_seed(23)
    T = {1: 99, 4: 25, 8: 13}[top_k]
    assert (T * top_k) % 16 != 0 and T * top_k > 64
    for name, S, fin, fout, per_pair in OP_SHAPES:
        layers = mx.plain_experts(n, 500 + n, S, fin, fout, g, dtype, dev, bias=True)
        table = hk.routed_table(layers, dev)
        for ids_dtype in (torch.int64, torch.int32):
            ids = mx.router_ids(T, top_k, n, gen, dev, ids_dtype)
            ids.view(-1)[:3] = torch.tensor([n - 1, n, -1], dtype=ids_dtype, device=dev)
            x = mx.strided_rows(T * top_k if per_pair else T, fin, gen, dev, dtype)
            y, _, _ = _grouped_n(x, ids, table, n, S, fin, fout, g, per_pair)
            assert tuple(y.shape) == (T * top_k, S, fout)
            _check_grouped_n(y, x, ids, layers, per_pair, dtype, f"{name} E{n} k{top_k} {dtype} {ids_dtype}")
    torch.cuda.synchronize()


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("tile_pairs", [16, 32, 64, 128])
def test_grouped_op_at_the_tile_edges(tile_pairs, dtype):
    """For every tile size ``grouped_tile_pairs`` returns: an expert that holds exactly one tile of pairs next to one that holds
    one pair more; every one of 300 pairs on ONE expert (the most tiles an expert can have, within the tile-slot bound
    ceil(P / tp) + min(E, P)); 65 pairs, the first count the module hands to this kernel.  No count is a multiple of 16."""
    from aqlm_amd.inference_kernels import hip_kernel as hk
    from tests import moe_experts as mx

    dev, g, tp = torch.device("cuda:0"), 8, tile_pairs
    name, S, fin, fout, per_pair = OP_SHAPES[0]
    all_layers = mx.plain_experts(60, 600, S, fin, fout, g, dtype, dev, bias=True)
    gen = torch.Generator(device=dev).manual_seed(24)

    def run(n, ids, what):
        layers = all_layers[:n]
        P = ids.numel()
        assert P % 16 != 0 and hk.grouped_tile_pairs(P, n) == tp, (what, P, n, hk.grouped_tile_pairs(P, n))
        x = torch.randn((P, fin), generator=gen, device=dev).to(dtype)  # top_k = 1: token rows are pair rows
        y, got_tp, bucket = _grouped_n(x, ids, hk.routed_table(layers, dev), n, S, fin, fout, g, per_pair)
        counts = torch.bincount(ids.view(-1), minlength=n).tolist()
        tiles = sum(-(-c // tp) for c in counts)
        assert got_tp == tp and bucket[:4].tolist() == [tiles, 0, P, 0], (what, bucket[:4].tolist(), tiles)
        assert tiles <= -(-P // tp) + min(n, P)
        _check_grouped_n(y, x, ids, layers, per_pair, dtype, f"{what} tp{tp} {dtype}")
        return tiles

    # exactly one tile on expert 0, one pair more on expert 1, the rest on expert 2
    P = 3 * tp - 5
    ids = torch.cat([torch.full((tp,), 0), torch.full((tp + 1,), 1), torch.full((P - 2 * tp - 1,), 2)])
    ids = ids[torch.randperm(P)].view(P, 1).to(dev)
    assert run(3, ids, "full tile and full tile + 1") == 4
    # 300 pairs on the last expert
    n = {16: 60, 32: 16, 64: 8, 128: 3}[tp]
    assert run(n, torch.full((300, 1), n - 1, dtype=torch.int64, device=dev), "300 pairs on one expert") == -(-300 // tp)
    # 65 pairs as routed
    n = {16: 60, 32: 3, 64: 2, 128: 1}[tp]
    run(n, mx.router_ids(65, 1, n, gen, dev), "65 pairs")
    torch.cuda.synchronize()


def _bucket_model(ids, tp, num_experts):
    flat = ids.reshape(-1)
    valid = (flat >= 0) & (flat < num_experts)
    lists = [np.nonzero(flat == e)[0] for e in range(num_experts)]
    tiles = []
    first = 0
    for e, lst in enumerate(lists):
        for j in range(0, len(lst), tp):
            tiles.append((e, first + j, min(tp, len(lst) - j)))
        first += len(lst)
    order = np.concatenate(lists + [np.nonzero(~valid)[0]])
    return tiles, int((~valid).sum()), order


@pytest.mark.gpu
def test_bucket_matches_a_numpy_model():
    from aqlm_amd.inference_kernels import hip_kernel as hk

    dev = torch.device("cuda:0")
    rng = np.random.default_rng(5)
    cases = [(E, rng.integers(0, E, size=(T, K))) for T in (33, 40, 100, 300, 700)]
    cases.append((E, np.full((50, K), 3)))                           # one expert
    cases.append((E, rng.integers(-3, E + 3, size=(257, K))))        # out-of-range ids mixed in
    cases.append((E, rng.integers(0, E, size=(4096, 4))))            # several scatter rounds
    for n in (1, 3, 60, 256):                                        # other expert counts, up to the entry's limit
        cases += [(n, rng.integers(0, n, size=(T, k))) for T, k in ((33, 2), (300, 1), (130, 8))]
        cases.append((n, np.full((75, 4), n - 1)))                   # every pair on the last expert
        cases.append((n, rng.integers(-3, n + 3, size=(257, 2))))    # n and n - 1 both present, negative ids
    for n, ids in cases:
        P = ids.size
        for tp in (16, 32, 64, 128):
            for dt in (torch.int64, torch.int32):
                got = torch.ops.aqlm.moe_bucket(torch.from_numpy(ids).to(dev, dt), n, tp).cpu().numpy()
                tiles, nbad, order = _bucket_model(ids, tp, n)
                max_tiles = -(-P // tp) + min(n, P)
                assert got.size * 4 == hk._lib.aqlm_hip_moe_bucket_bytes(P, n, tp)
                assert list(got[:4]) == [len(tiles), nbad, P - nbad, 0], (n, ids.shape, tp)
                assert len(tiles) <= max_tiles
                table = got[4:4 + 4 * max_tiles].reshape(max_tiles, 4)[:len(tiles)]
                assert [tuple(t[:3]) for t in table] == tiles, (n, ids.shape, tp)
                assert np.array_equal(got[4 + 4 * max_tiles:4 + 4 * max_tiles + P], order), (n, ids.shape, tp)


@pytest.mark.gpu
def test_full_mixtral_shapes_at_256_tokens():
    from aqlm_amd.inference_kernels import hip_kernel as hk

    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(14)
    T = 256
    ids = _ids(T, gen, dev)
    for name, S, fin, fout, per_pair in (("w13", 2, 4096, 14336, False), ("w2", 1, 14336, 4096, True)):
        layers = _experts(21, S, fin, fout, 8, torch.float16, dev)
        table = hk.routed_table(layers, dev)
        x = torch.randn((T * K if per_pair else T, fin), generator=gen, device=dev).half()
        y = _grouped(x, ids, table, S, fin, fout, 8, per_pair)
        with _Variant():
            _check_bits(y, x, ids, layers, per_pair, name)
        flat = ids.reshape(-1)
        for e in (0, 5):  # the oracle on two experts (an fp64 W of 14336 x 4096 is 470 MB)
            pairs = torch.nonzero(flat == e).squeeze(1)
            xe = x[pairs if per_pair else pairs // K].double()
            for s in range(S):
                _check(y[pairs, s], xe @ _w64(layers[e][s]).T, torch.float16, f"{name} expert {e} seg {s}")
        del layers, table
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------------
# module level
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_grouped_forward_matches_loop_and_dense(dtype):
    dev = torch.device("cuda:0")
    _, q, dense = _module(1024, 2048, dtype, dev)
    gen = torch.Generator(device=dev).manual_seed(15)
    for T in TOKENS:
        x = torch.randn((T, 1024), generator=gen, device=dev).to(dtype)
        ids, w = _route(T, K, gen, dev)
        with torch.no_grad():
            assert not q.takes_routed_path(x, ids) and q.takes_grouped_path(x, ids)
            y = q(x, ids, w).double()
            y_loop = q._forward_loop(x, ids, w).double()
            y_dense = dense(x, ids, w).double()
        for ref, what in ((y_loop, "loop"), (y_dense, "dense")):
            rel = ((y - ref).abs().mean() / ref.abs().mean()).item()
            assert rel < (2e-3 if dtype == torch.float16 else 1.6e-2), (T, what, rel)


@pytest.mark.gpu
@pytest.mark.parametrize("T", [40, 300])
def test_grouped_forward_makes_no_host_sync(T):
    dev = torch.device("cuda:0")
    _, q, _ = _module(1024, 2048, torch.float16, dev)
    gen = torch.Generator(device=dev).manual_seed(16)
    x = torch.randn((T, 1024), generator=gen, device=dev).half()
    ids, w = _route(T, K, gen, dev)
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
@pytest.mark.parametrize("T", [48, 200])
def test_prefill_moe_block_replays_from_a_graph(T):
    from transformers.models.mixtral.modeling_mixtral import MixtralSparseMoeBlock

    dev = torch.device("cuda:0")
    cfg, q, _ = _module(1024, 2048, torch.float16, dev, seed=17)
    block = MixtralSparseMoeBlock(cfg).to(dev, torch.float16).eval()
    with torch.no_grad():
        block.gate.weight.normal_(0, 0.5)
    block.experts = q
    gen = torch.Generator(device=dev).manual_seed(18)
    inputs = [torch.randn((1, T, 1024), generator=gen, device=dev).half() for _ in range(3)]
    static = inputs[0].clone()
    with torch.no_grad():
        assert q.takes_grouped_path(static.view(T, 1024), torch.zeros((T, K), dtype=torch.int64, device=dev))
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


def _dense64(q):
    """the dequantised experts in fp64: (gate_up [E, 2I, H], down [E, H, I])"""
    gate_up, down = [], []
    for e in range(E):
        ex = q.expert(e)
        ws = {s: _w64((getattr(ex, s).codes, getattr(ex, s).codebooks, getattr(ex, s).scales, None)) for s in ("w1", "w3", "w2")}
        gate_up.append(torch.cat([ws["w1"], ws["w3"]], 0))
        down.append(ws["w2"])
    return torch.stack(gate_up), torch.stack(down)


def _moe64(gate_up, down, x, ids, w):
    """fp64 autograd reference of the experts block: out[t] = sum_j w[t, j] W2_e (silu(W1_e x_t) * W3_e x_t), e = ids[t, j]"""
    out = torch.zeros_like(x)
    inter = down.shape[2]
    for e in range(gate_up.shape[0]):
        tok, pos = torch.where(ids == e)
        if tok.numel() == 0:
            continue
        gu = x[tok] @ gate_up[e].T
        h = torch.nn.functional.silu(gu[:, :inter]) * gu[:, inter:]
        out = out.index_add(0, tok, (h @ down[e].T) * w[tok, pos, None])
    return out


def _rel(a, b):
    return ((a.double() - b.double()).abs().mean() / b.double().abs().mean()).item()


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_gradients_match_a_dense_fp64_twin(dtype):
    dev = torch.device("cuda:0")
    _, q, _ = _module(1024, 2048, dtype, dev, seed=19)
    gate_up, down = _dense64(q)
    gen = torch.Generator(device=dev).manual_seed(20)
    bound = 5e-3 if dtype == torch.float16 else 3e-2
    for T in (3, 40, 200):
        x0 = torch.randn((T, 1024), generator=gen, device=dev).to(dtype)
        ids, w0 = _route(T, K, gen, dev)
        r = torch.randn((T, 1024), generator=gen, device=dev)
        x, w = x0.clone().requires_grad_(), w0.clone().requires_grad_()
        assert q.takes_grouped_path(x, ids)
        y = q(x, ids, w)
        (y.float() * r).sum().backward()
        x64, w64 = x0.double().requires_grad_(), w0.double().requires_grad_()
        (_moe64(gate_up, down, x64, ids, w64) * r.double()).sum().backward()
        assert _rel(x.grad, x64.grad) <= bound, (T, "x.grad", _rel(x.grad, x64.grad))
        assert _rel(w.grad, w64.grad) <= bound, (T, "top_k_weights.grad", _rel(w.grad, w64.grad))
        for e in range(E):
            assert all(p.grad is None for p in q.expert(e).parameters())


@pytest.mark.gpu
def test_two_forwards_under_grad_are_bit_identical():
    dev = torch.device("cuda:0")
    _, q, _ = _module(1024, 2048, torch.float16, dev, seed=21)
    gen = torch.Generator(device=dev).manual_seed(22)
    for T in (5, 100):
        x = torch.randn((T, 1024), generator=gen, device=dev).half().requires_grad_()
        ids, w = _route(T, K, gen, dev)
        a, b = q(x, ids, w), q(x, ids, w)
        assert a.requires_grad and torch.equal(a, b)
        with torch.no_grad():
            c = q(x, ids, w)
        if T * K > 64:  # the no-grad call takes the grouped launches as well: same bits
            assert torch.equal(a, c)
