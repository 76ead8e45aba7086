"""The segmented adapter GEMM on the routed Mixtral experts, on the MI355X: the raw op ``torch.ops.aqlm.lora_sgmv_routed_``
(aqlm_hip_lora_sgmv_routed) bit for bit against a per-pair, per-segment loop of ``torch.ops.aqlm.lora_sgmv_`` on one row with a
one-slot table and within the project's per-element bound of the fp64 definition, the rows it must leave alone, strided x rows,
the independence of a pair from the other pairs, skewed routings and tile edges; and ``aqlm.lora.LoraQuantizedMixtralExperts``
over the grouped base route at 300 pairs: the new route against the torch path, rows outside the bank, the switch, per-sequence
ids, and hipGraph replay with both id tensors rewritten in place.

Bound: ``check_bound`` of tests/test_lora_sgmv_gpu.py (``2e-3`` / ``1.6e-2 * mean|y| + 4 ulp``).  The module tests set
``lora.ROUTED_SGMV_MAX_PAIRS`` themselves: the shipped value is a measured cross-over (profiles/lora_moe_prefill.json), not part
of what is checked here."""
import pytest
import torch

from tests import moe_experts as mx
from tests.test_lora_moe_gpu import (DEV, DTYPES, E, K, MODES, ODD, RANKS, ZERO, _block, _entries, _Holder, _ids, _live, _route,
                                     _slots)  # the setup of the routed BGMV tests: three adapters of ranks 8 / 24 / 128 on 4 experts
from tests.test_lora_sgmv_gpu import check_bound

pytestmark = pytest.mark.gpu

# (in_features, out_features): one K slice and one output tile; a last k-step of a single 8-element piece and an output tail of 12;
# the smallest in_features with two K slices
SHAPES = [(64, 16), (520, 300), (1032, 296)]
TOKENS = (1, 3, 40, 150)         # 300 pairs: several full 16-pair tiles and a partial one per expert
TILE = 16


def _inputs(seed, T, fin, fout, dtype, S, per_pair, k=K):
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn((T * k if per_pair else T, fin), generator=gen).to(dtype).to(DEV)
    y_in = torch.randn((T * k, S, fout), generator=gen).to(dtype).to(DEV)
    return x, y_in


def _run(y_in, x, aids, eids, entries, per_pair, a_dtype=torch.int64, e_dtype=torch.int64, table=None):
    from aqlm_amd.inference_kernels import hip_kernel as hk

    S, k = y_in.shape[1], len(eids[0])
    table = hk.lora_routed_table(entries, torch.device(DEV)) if table is None else table
    y = y_in.clone()
    at = None if aids is None else torch.tensor(aids, dtype=a_dtype, device=DEV)
    et = torch.tensor(eids, dtype=e_dtype, device=DEV)
    bucket = torch.ops.aqlm.moe_bucket(et, E, TILE)
    torch.ops.aqlm.lora_sgmv_routed_(y, x, at, et, bucket, table, [len(entries), E, S, max(RANKS), y.shape[2], x.shape[1], k], per_pair)
    return y


def _loop_of_sgmv(y_in, x, aids, eids, entries, per_pair, slots):
    """The dense op on one row, one call per (pair, segment), with that pair's entry as a one-slot table."""
    y = y_in.clone()
    k = len(eids[0])
    for p in range(y.shape[0]):
        t = p // k
        xr = x[p:p + 1] if per_pair else x[t:t + 1]
        for s in range(y.shape[1]):
            a, e = (0 if aids is None else aids[t]), eids[t][p % k]
            ent = _live(entries, a, e, s)
            if ent is None:
                continue
            torch.ops.aqlm.lora_sgmv_(y[p, s:s + 1], xr, None, slots[(a, e, s)], [1, ent[0].shape[0], y.shape[2], x.shape[1]])
    return y


def _ref64(y_in, x, aids, eids, entries, per_pair):
    """The definition in fp64, one masked batch per table entry."""
    P, S, _ = y_in.shape
    k = len(eids[0])
    y = y_in.double().clone()
    T = P // k
    at = torch.tensor([0] * T if aids is None else aids, device=DEV).repeat_interleave(k)
    et = torch.tensor(eids, device=DEV).reshape(-1)
    xp = (x if per_pair else x.repeat_interleave(k, dim=0)).double()
    for a in range(len(entries)):
        for e in range(E):
            rows = torch.nonzero((at == a) & (et == e)).squeeze(1)
            for s in range(S):
                ent = _live(entries, a, e, s)
                if ent is not None and rows.numel():
                    A, B, sc = ent
                    y[rows, s] += float(torch.tensor(sc, dtype=torch.float32)) * ((xp[rows] @ A.double().T) @ B.double().T)
    return y


@pytest.mark.parametrize("a_dtype,e_dtype", [(torch.int64, torch.int64), (torch.int32, torch.int32), (torch.int32, torch.int64)],
                         ids=["a64e64", "a32e32", "a32e64"])
@pytest.mark.parametrize("S,per_pair", MODES, ids=["w13", "w2"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
@pytest.mark.parametrize("fin,fout", SHAPES)
def test_bit_equal_to_a_loop_of_the_row_op_and_within_the_bound_of_fp64(fin, fout, dtype, S, per_pair, a_dtype, e_dtype):
    from aqlm_amd.inference_kernels import hip_kernel as hk

    entries = _entries(1, fin, fout, dtype, S)
    table, slots = hk.lora_routed_table(entries, torch.device(DEV)), _slots(entries)
    for T in TOKENS:
        x, y_in = _inputs(10 + T, T, fin, fout, dtype, S, per_pair)
        aids, eids = _ids(20 + T, T)
        y = _run(y_in, x, aids, eids, entries, per_pair, a_dtype, e_dtype, table)
        assert torch.equal(y, _loop_of_sgmv(y_in, x, aids, eids, entries, per_pair, slots)), f"T {T}: not bit-equal to lora_sgmv_ per pair"
        check_bound(y, _ref64(y_in, x, aids, eids, entries, per_pair), dtype, f"in {fin} out {fout} {dtype} S {S} T {T}")
    # NULL adapter ids: adapter 0 for every token
    x, y_in = _inputs(5, 3, fin, fout, dtype, S, per_pair)
    _, eids = _ids(6, 3)
    y = _run(y_in, x, None, eids, entries, per_pair, e_dtype=e_dtype, table=table)
    assert torch.equal(y, _run(y_in, x, [0] * 3, eids, entries, per_pair, a_dtype, e_dtype, table))
    assert torch.equal(y, _loop_of_sgmv(y_in, x, None, eids, entries, per_pair, slots))


@pytest.mark.parametrize("S,per_pair", MODES, ids=["w13", "w2"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
def test_rows_that_must_stay_are_bit_equal_and_every_other_row_changes(dtype, S, per_pair):
    fin, fout, T = 520, 300, 40
    entries = _entries(2, fin, fout, dtype, S)
    x, y_in = _inputs(3, T, fin, fout, dtype, S, per_pair)
    aids, eids = _ids(4, T)
    # adapter ids by token: t % 5 = 0 -> -1, 1 -> 0, 2 -> 3 (= num_adapters), 3 -> 1, 4 -> 2
    for t, bad in zip((1, 6, 11, 4), (-1, E, 2 ** 40, -(2 ** 40))):  # hostile expert ids under the valid adapters 0, 0, 0, 2
        eids[t][t % K] = bad
    eids[3] = [ZERO[1], 0]   # token 3, adapter 1: the zero entry on expert 2, served on expert 0
    eids[16] = [ODD[1], 1]   # token 16, adapter 0: the rank-12 entry on expert 3, served on expert 1
    assert aids[3] == ZERO[0] and aids[16] == ODD[0] and [aids[t] for t in (1, 6, 11, 4)] == [0, 0, 0, 2]
    y = _run(y_in, x, aids, eids, entries, per_pair)
    stay = 0
    for p in range(T * K):
        for s in range(S):
            if _live(entries, aids[p // K], eids[p // K][p % K], s) is None:
                assert torch.equal(y[p, s], y_in[p, s]), f"pair {p} segment {s} (adapter {aids[p // K]}, expert {eids[p // K][p % K]}) was written"
                stay += 1
            else:
                assert not torch.equal(y[p, s], y_in[p, s]), f"pair {p} segment {s} was not served"
    assert S * 38 <= stay < S * T * K  # 16 tokens without an adapter, 4 hostile expert ids, the zero and the rank-12 entry
    check_bound(y, _ref64(y_in, x, aids, eids, entries, per_pair), dtype, f"hostile ids {dtype} S {S}")
    # int32 expert ids (without the ids that need 64 bits)
    eids32 = [[v if abs(v) < 2 ** 31 else E + 5 for v in row] for row in eids]
    assert torch.equal(_run(y_in, x, aids, eids32, entries, per_pair, torch.int32, torch.int32), y)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
def test_strided_x_rows_change_nothing(dtype):
    fin, fout, T = 520, 300, 21
    gen = torch.Generator(device=DEV).manual_seed(7)
    for S, per_pair in MODES:
        entries = _entries(8, fin, fout, dtype, S)
        xs = mx.strided_rows(T * K if per_pair else T, fin, gen, DEV, dtype)
        assert xs.stride(0) != fin
        _, y_in = _inputs(9, T, fin, fout, dtype, S, per_pair)
        aids, eids = _ids(10, T)
        assert torch.equal(_run(y_in, xs, aids, eids, entries, per_pair), _run(y_in, xs.contiguous(), aids, eids, entries, per_pair))


@pytest.mark.parametrize("S,per_pair", MODES, ids=["w13", "w2"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
def test_a_pairs_bits_depend_on_that_pair_alone(dtype, S, per_pair):
    fin, fout, T = 1032, 296, 150
    entries = _entries(11, fin, fout, dtype, S)
    x, y_in = _inputs(12, T, fin, fout, dtype, S, per_pair)
    aids, eids = _ids(13, T)
    y = _run(y_in, x, aids, eids, entries, per_pair)
    assert torch.equal(y, _run(y_in, x, aids, eids, entries, per_pair)), "two runs differ"

    def tokens(sel):
        """The call on the tokens ``sel`` only, in that order -> (y, pair rows of the full call it must equal)."""
        pairs = [t * K + j for t in sel for j in range(K)]
        ys = _run(y_in[pairs], x[pairs] if per_pair else x[sel], [aids[t] for t in sel], [eids[t] for t in sel], entries, per_pair)
        return ys, y[pairs]

    perm = torch.randperm(T, generator=torch.Generator().manual_seed(14)).tolist()
    for sel in (perm, list(range(0, T, 2)), [3, 130, 8], [21]):
        got, want = tokens(sel)
        assert torch.equal(got, want), f"{len(sel)} of {T} tokens differ from the full call"
    # a NaN in one x row poisons its own pairs only
    victim = next(t for t in range(T) if aids[t] == 2 and (aids[t], eids[t][0]) not in (ZERO, ODD))
    xn = x.clone()
    xn[victim * K if per_pair else victim, 17] = float("nan")
    yn = _run(y_in, xn, aids, eids, entries, per_pair)
    hit = [victim * K] if per_pair else [victim * K + j for j in range(K) if _live(entries, 2, eids[victim][j], 0) is not None]
    assert hit and bool(torch.isnan(yn[hit]).all())
    keep = [p for p in range(T * K) if p not in hit]
    assert torch.equal(yn[keep], y[keep])


@pytest.mark.parametrize("S,per_pair", MODES, ids=["w13", "w2"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
def test_skewed_routings_and_tile_edges(dtype, S, per_pair):
    """top_k 1: all 150 tokens on one expert (three experts without a tile), and a routing that gives one expert exactly one full
    tile of 16 pairs and another 17 (a full tile and a tile of one pair)."""
    fin, fout = 520, 300
    entries = _entries(15, fin, fout, dtype, S)
    slots = _slots(entries)
    order = torch.randperm(40, generator=torch.Generator().manual_seed(16)).tolist()
    edge = [[([0] * 16 + [1] * 17 + [2] * 7)[i]] for i in order]
    for what, T, eids in (("one expert", 150, [[1]] * 150), ("16 and 17 pairs", 40, edge)):
        x, y_in = _inputs(17 + T, T, fin, fout, dtype, S, per_pair, k=1)
        aids = [(-1, 0, 3, 1, 2)[t % 5] for t in range(T)]
        if T == 40:
            assert [sum(e == [v] for e in eids) for v in range(E)] == [16, 17, 7, 0]
        y = _run(y_in, x, aids, eids, entries, per_pair)
        assert torch.equal(y, _loop_of_sgmv(y_in, x, aids, eids, entries, per_pair, slots)), what
        check_bound(y, _ref64(y_in, x, aids, eids, entries, per_pair), dtype, f"{what} {dtype} S {S}")
        served = [p for p in range(T) if _live(entries, aids[p], eids[p][0], 0) is not None]
        assert served and all(not torch.equal(y[p], y_in[p]) for p in served), what


# ---------------------------------------------------------------------------------------------------------------------------
# module level: a block of 4 experts, hidden 1024, intermediate 2048 (the SMALL_SHAPES of tests/moe_experts.py), 1x16 g8, fp16,
# over the grouped base route at T = 150 (300 pairs).
# ---------------------------------------------------------------------------------------------------------------------------
# The adapters are a fine-tune's correction: B as in tests/test_lora_moe_gpu.py (SIGMA_B there), and alpha such that at the BLOCK
# output the adapter term stays at or below half of the base output (the tests print the ratio).  Why: ``check_bound`` allows
# ``2e-3 * mean|y|`` with ONE mean over all rows of a call, and what it bounds here is the difference of two fp16 pipelines (HIP
# route and torch path round ``gu``, ``h`` and the pair outputs to fp16 at slightly different fp32 values, so some roundings flip,
# and a flip is proportional to the size of the row it happens in).  With per-token ids half of the rows are bare rows; an adapter
# whose term is twice the base output (alpha 32 at rank 16) makes its rows 2.2 x the bare rows and 1.7 x the mean, so its rows'
# flips are held to a bound 1.7 x tighter than in a call where every row has that adapter.  Measured with such an adapter, the
# worst error / bound over 12 input seeds was 0.57 .. 0.84 with the adapter on every row and 0.66 .. 1.33 with per-token ids (4
# seeds above 1, one element each, at |y| of 0.01 .. 0.2 of the mean) -- and 0.57 .. 1.09 for the routed BGMV route at 128 tokens,
# the same figures from the launches the tree already had: a property of one mean over rows of two scales, not of a route.  Rows
# of one scale are what the bound's model assumes, so that is what the test gives it (measured with the adapters below over the
# same 12 seeds: 0.45 .. 0.82 with "a" on every row, 0.34 .. 0.72 with per-token ids).
H, I = mx.SMALL_SHAPES[0][2], mx.SMALL_SHAPES[0][3]
ADAPTERS = (("a", 16, 8), ("b", 8, 4))  # name, rank, alpha
SIGMA_B = 0.03
T_MOD = 150


def _attach(lora, q, seed=1, dtype=torch.float16):
    gen = torch.Generator().manual_seed(seed)
    ads = {}
    for name, r, alpha in ADAPTERS:
        state = {}
        for e in range(E):
            for w, (fin, fout) in (("w1", (H, I)), ("w3", (H, I)), ("w2", (I, H))):
                state[f"base_model.model.experts.{e}.{w}.lora_A.weight"] = (torch.randn((r, fin), generator=gen) / fin ** 0.5).to(dtype)
                state[f"base_model.model.experts.{e}.{w}.lora_B.weight"] = (torch.randn((fout, r), generator=gen) * SIGMA_B).to(dtype)
        ads[name] = (state, {"peft_type": "LORA", "r": r, "lora_alpha": alpha, "bias": "none", "target_modules": ["w1", "w2", "w3"]})
    holder = _Holder(q)
    bank = lora.attach_adapters(holder, ads)
    assert isinstance(holder.experts, lora.LoraQuantizedMixtralExperts) and holder.experts.base_layer is q
    return holder, bank


@pytest.fixture()
def sgmv_limit(monkeypatch):
    import aqlm_amd.lora as lora

    monkeypatch.setattr(lora, "ROUTED_BGMV_MAX_PAIRS", 256)
    monkeypatch.setattr(lora, "ROUTED_SGMV_MAX_PAIRS", 65536)
    return lora


@pytest.fixture()
def launches(monkeypatch):
    """Counts the adapter launches of both routed routes through wrappers around the ``hip_kernel`` functions."""
    from aqlm_amd.inference_kernels import hip_kernel as hk

    calls = {"sgmv": [], "bgmv": []}
    real_s, real_b = hk.lora_sgmv_routed_, hk.lora_bgmv_routed_
    monkeypatch.setattr(hk, "lora_sgmv_routed_", lambda *a: (calls["sgmv"].append(a[0].shape[0]), real_s(*a))[1])
    monkeypatch.setattr(hk, "lora_bgmv_routed_", lambda *a: (calls["bgmv"].append(a[0].shape[0]), real_b(*a))[1])
    return calls


def test_new_route_over_the_grouped_base_against_the_torch_path(sgmv_limit, launches, monkeypatch):
    lora = sgmv_limit
    q = _block(30)
    holder, bank = _attach(lora, q)
    T = T_MOD
    gen = torch.Generator(device=DEV).manual_seed(31)
    x = torch.randn((T, H), generator=gen, device=DEV).half()
    idx, wts = _route(T, gen)
    ids = torch.tensor(([1, 0, 2, -1] * T)[:T], device=DEV)
    with torch.no_grad():
        assert q.takes_grouped_path(x, idx)
        bare = q(x, idx, wts)
        for which in ("a", "b", ids):
            bank.select(which)
            n = len(launches["sgmv"])
            y = holder.experts(x, idx, wts)
            assert launches["sgmv"][n:] == [T * K, T * K], "the new route was not taken once per projection group"
            monkeypatch.setattr(lora, "ROUTED_SGMV_MAX_PAIRS", 0)
            ref = holder.experts(x, idx, wts)
            monkeypatch.setattr(lora, "ROUTED_SGMV_MAX_PAIRS", 65536)
            assert len(launches["sgmv"]) == n + 2, "ROUTED_SGMV_MAX_PAIRS = 0 did not switch the route off"
            assert not torch.equal(ref, bare) and not torch.equal(y, bare)
            print(f"adapter term / base output: {float((ref.float() - bare.float()).abs().mean() / bare.float().abs().mean()):.3g}")
            check_bound(y, ref, torch.float16, f"grouped base, select {which if isinstance(which, str) else 'ids'}")
            if not isinstance(which, str):  # ids 2 and -1 are outside the bank: the bare block's rows on the new route
                assert torch.equal(y[2::4], bare[2::4]) and torch.equal(y[3::4], bare[3::4])
                assert not torch.equal(y[0::4], bare[0::4]) and not torch.equal(y[1::4], bare[1::4])
        assert not launches["bgmv"], "a call of 300 pairs took the BGMV route"
        # a call of up to 256 pairs keeps its route
        bank.select(ids[:128])
        holder.experts(x[:128], idx[:128], wts[:128])
        assert launches["bgmv"] == [256, 256] and len(launches["sgmv"]) == 6
    lora.detach_adapters(holder)
    assert holder.experts is q


def test_per_sequence_ids_equal_per_token_ids(sgmv_limit, launches):
    lora = sgmv_limit
    q = _block(32)
    holder, bank = _attach(lora, q)
    T = T_MOD
    gen = torch.Generator(device=DEV).manual_seed(33)
    x = torch.randn((T, H), generator=gen, device=DEV).half()
    idx, wts = _route(T, gen)
    with torch.no_grad():
        bare = q(x, idx, wts)
        bank.select(torch.tensor([1] * 50 + [0] * 50 + [1] * 50, device=DEV))
        y150 = holder.experts(x, idx, wts)
        bank.select(torch.tensor([1, 0, 1], device=DEV))  # three sequences of 50 rows
        n = len(launches["sgmv"])
        y3 = holder.experts(x, idx, wts)
        assert len(launches["sgmv"]) == n + 2 and torch.equal(y3, y150)
        assert not torch.equal(y150[0], bare[0]) and not torch.equal(y150[50], bare[50])


def test_captured_prefill_step_follows_both_id_tensors_rewritten_in_place(sgmv_limit, launches):
    lora = sgmv_limit
    q = _block(34)
    holder, bank = _attach(lora, q)
    T = T_MOD
    gen = torch.Generator(device=DEV).manual_seed(35)
    x = torch.randn((T, H), generator=gen, device=DEV).half()
    routes = [_route(T, gen)[0] for _ in range(2)]
    _, wts = _route(T, gen)
    assert not torch.equal(routes[0], routes[1])
    idx = routes[0].clone()
    ids = torch.full((T,), -1, dtype=torch.int64, device=DEV)
    bank.select(ids)
    cases = [([-1] * T, 0), (([0, 1] * T)[:T], 0), (([1, 1, 0, -1] * T)[:T], 1), ([0] * T, 1)]
    with torch.no_grad():
        eager = []
        for values, r in cases:
            ids.copy_(torch.tensor(values, device=DEV))
            idx.copy_(routes[r])
            eager.append(holder.experts(x, idx, wts).clone())
        assert torch.equal(eager[0], q(x, routes[0], wts)) and not torch.equal(eager[1], eager[0]) and not torch.equal(eager[2], eager[3])
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(2):
                holder.experts(x, idx, wts)
        torch.cuda.current_stream().wait_stream(s)
        n = len(launches["sgmv"])
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = holder.experts(x, idx, wts)
        assert len(launches["sgmv"]) == n + 2, "the captured step did not take the new route"
        for (values, r), want in zip(cases, eager):
            ids.copy_(torch.tensor(values, device=DEV))
            idx.copy_(routes[r])
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(out, want), f"replay with adapter ids {values[:4]}.. on routing {r}"
