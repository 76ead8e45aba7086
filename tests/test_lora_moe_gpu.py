"""LoRA adapters on the routed Mixtral experts, on the MI355X: the raw op ``torch.ops.aqlm.lora_bgmv_routed_``
(aqlm_hip_lora_bgmv_routed) bit for bit against a per-pair, per-segment loop of ``torch.ops.aqlm.lora_bgmv_`` with one-slot
tables and within the project's per-element bound of the fp64 definition, the rows it must leave alone, strided x rows, the
independence of a pair from the other pairs; and ``aqlm.lora.LoraQuantizedMixtralExperts`` on a GPU block: the HIP route on the
routed, the routed packed and the grouped base route against the torch path, ``select(None)``, per-sequence ids, hipGraph replay
with both id tensors rewritten in place, and gradients of hidden_states, A and B through the grouped base + torch path.

Bound: ``check_bound`` of tests/test_lora_gpu.py (``2e-3`` / ``1.6e-2 * mean|y| + 4 ulp``).  The module tests set
``lora.ROUTED_BGMV_MAX_PAIRS`` themselves: the shipped value is a measured cross-over (profiles/lora_moe.json), not part of what
is checked here."""
import pytest
import torch

from tests import moe_experts as mx
from tests.test_lora_gpu import check_bound

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
E, K = 4, 2
RANKS = (8, 24, 128)
SCALINGS = (2.0, 0.5, 1.25)
SHAPES = [(64, 16), (520, 300)]  # (in_features, out_features), as tests/test_lora_gpu.py: a wave-step tail, two expand workgroups
DTYPES = [torch.float16, torch.bfloat16]
MODES = [(2, False), (1, True)]  # (segments, x rows per pair): the gate / up launch and the down launch
TOKENS = (1, 3, 32, 128)         # 128 tokens x top_k 2 = the entry's 256-pair limit
ZERO = (1, 2)                    # (adapter, expert) without weights: a zero entry
ODD = (0, 3)                     # (adapter, expert) whose entry has rank 12: "no adapter" too


def _entries(seed, fin, fout, dtype, S):
    """entries[a][e][s] = (A, B, scaling) or None, three adapters of ranks RANKS on E experts."""
    gen = torch.Generator().manual_seed(seed)
    entries = []
    for a, (rank, scaling) in enumerate(zip(RANKS, SCALINGS)):
        per_adapter = []
        for e in range(E):
            r = 12 if (a, e) == ODD else rank
            per = []
            for _ in range(S):
                A = (torch.randn((r, fin), generator=gen) / fin ** 0.5).to(dtype).to(DEV)
                B = (torch.randn((fout, r), generator=gen) / r ** 0.5).to(dtype).to(DEV)
                per.append(None if (a, e) == ZERO else (A, B, scaling))
            per_adapter.append(per)
        entries.append(per_adapter)
    return entries


def _live(entries, a, e, s):
    """The entry the definition applies to (pair adapter a, expert e, segment s), or None: ids out of range, no weights, rank 12."""
    if not (0 <= a < len(entries) and 0 <= e < E):
        return None
    ent = entries[a][e][s]
    return None if ent is None or ent[0].shape[0] % 8 else ent


def _inputs(seed, T, fin, fout, dtype, S, per_pair):
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn((T * K if per_pair else T, fin), generator=gen).to(dtype).to(DEV)
    y_in = torch.randn((T * K, S, fout), generator=gen).to(dtype).to(DEV)
    return x, y_in


def _ids(seed, T):
    """-> (adapter id per token, expert ids [T, K]) as lists: every adapter, -1 and len(RANKS) mixed over the tokens (one token:
    the widest adapter), router-like distinct experts per token."""
    gen = torch.Generator().manual_seed(seed)
    aids = [len(RANKS) - 1] if T == 1 else [(-1, 0, 3, 1, 2)[t % 5] for t in range(T)]
    eids = torch.topk(torch.rand((T, E), generator=gen), K, dim=-1).indices.tolist()
    return aids, eids


def _run(y_in, x, aids, eids, entries, per_pair, a_dtype=torch.int64, e_dtype=torch.int64, table=None):
    from aqlm_amd.inference_kernels import hip_kernel as hk

    S = y_in.shape[1]
    table = hk.lora_routed_table(entries, torch.device(DEV)) if table is None else table
    y = y_in.clone()
    at = None if aids is None else torch.tensor(aids, dtype=a_dtype, device=DEV)
    et = torch.tensor(eids, dtype=e_dtype, device=DEV)
    torch.ops.aqlm.lora_bgmv_routed_(y, x, at, et, table, [len(entries), E, S, max(RANKS), y.shape[2], x.shape[1], K], per_pair)
    return y


def _loop_of_bgmv(y_in, x, aids, eids, entries, per_pair, slots):
    """The existing per-row op, one call per (pair, segment) with that pair's entry as a one-slot table."""
    y = y_in.clone()
    for p in range(y.shape[0]):
        t = p // K
        xr = x[p:p + 1] if per_pair else x[t:t + 1]
        for s in range(y.shape[1]):
            a, e = (0 if aids is None else aids[t]), eids[t][p % K]
            ent = _live(entries, a, e, s)
            if ent is None:
                continue
            torch.ops.aqlm.lora_bgmv_(y[p, s:s + 1], xr, None, slots[(a, e, s)], [1, ent[0].shape[0], y.shape[2], x.shape[1]])
    return y


def _slots(entries):
    from aqlm_amd.inference_kernels import hip_kernel as hk

    return {(a, e, s): hk.lora_table([ent], torch.device(DEV)) for a, pa in enumerate(entries) for e, pe in enumerate(pa)
            for s, ent in enumerate(pe) if ent is not None and ent[0].shape[0] % 8 == 0}


def _ref64(y_in, x, aids, eids, entries, per_pair):
    """The definition in fp64, one masked batch per table entry."""
    P, S, _ = y_in.shape
    y = y_in.double().clone()
    T = P // K
    at = torch.tensor([0] * T if aids is None else aids, device=DEV).repeat_interleave(K)
    et = torch.tensor(eids, device=DEV).reshape(-1)
    xp = (x if per_pair else x.repeat_interleave(K, dim=0)).double()
    for a in range(len(entries)):
        for e in range(E):
            rows = torch.nonzero((at == a) & (et == e)).squeeze(1)
            for s in range(S):
                ent = _live(entries, a, e, s)
                if ent is not None and rows.numel():
                    A, B, sc = ent
                    y[rows, s] += float(torch.tensor(sc, dtype=torch.float32)) * ((xp[rows] @ A.double().T) @ B.double().T)
    return y


@pytest.mark.parametrize("e_dtype", [torch.int64, torch.int32], ids=["e64", "e32"])
@pytest.mark.parametrize("a_dtype", [torch.int64, torch.int32], ids=["a64", "a32"])
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
        assert torch.equal(y, _loop_of_bgmv(y_in, x, aids, eids, entries, per_pair, slots)), f"T {T}: not bit-equal to lora_bgmv_ per pair"
        check_bound(y, _ref64(y_in, x, aids, eids, entries, per_pair), dtype, f"in {fin} out {fout} {dtype} S {S} T {T}")
    # NULL adapter ids: adapter 0 for every token
    x, y_in = _inputs(5, 3, fin, fout, dtype, S, per_pair)
    _, eids = _ids(6, 3)
    y = _run(y_in, x, None, eids, entries, per_pair, e_dtype=e_dtype, table=table)
    assert torch.equal(y, _run(y_in, x, [0] * 3, eids, entries, per_pair, a_dtype, e_dtype, table))
    assert torch.equal(y, _loop_of_bgmv(y_in, x, None, eids, entries, per_pair, slots))


@pytest.mark.parametrize("S,per_pair", MODES, ids=["w13", "w2"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
def test_rows_that_must_stay_are_bit_equal_and_every_other_row_changes(dtype, S, per_pair):
    fin, fout, T = 520, 300, 32
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
    assert S * 32 <= stay < S * T * K  # 13 tokens without an adapter, 4 hostile expert ids, the zero and the rank-12 entry
    check_bound(y, _ref64(y_in, x, aids, eids, entries, per_pair), dtype, f"hostile ids {dtype} S {S}")
    # int32 expert ids (without the ids that need 64 bits)
    eids32 = [[v if abs(v) < 2 ** 31 else E + 5 for v in row] for row in eids]
    assert torch.equal(_run(y_in, x, aids, eids32, entries, per_pair, torch.int32, torch.int32), y)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
def test_strided_x_rows_change_nothing(dtype):
    fin, fout, T = 520, 300, 5
    gen = torch.Generator(device=DEV).manual_seed(7)
    for S, per_pair in MODES:
        entries = _entries(8, fin, fout, dtype, S)
        xs = mx.strided_rows(T * K if per_pair else T, fin, gen, DEV, dtype)
        _, y_in = _inputs(9, T, fin, fout, dtype, S, per_pair)
        aids, eids = _ids(10, T)
        assert torch.equal(_run(y_in, xs, aids, eids, entries, per_pair), _run(y_in, xs.contiguous(), aids, eids, entries, per_pair))


@pytest.mark.parametrize("S,per_pair", MODES, ids=["w13", "w2"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
def test_a_pairs_bits_depend_on_that_pair_alone(dtype, S, per_pair):
    fin, fout, T = 520, 300, 32
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
    for sel in (perm, list(range(0, 32, 2)), [3, 30, 8], [21]):
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


# ---------------------------------------------------------------------------------------------------------------------------
# module level: a block of 4 experts, hidden 1024, intermediate 2048 (the SMALL_SHAPES of tests/moe_experts.py), 1x16 g8, fp16
# ---------------------------------------------------------------------------------------------------------------------------
H, I = mx.SMALL_SHAPES[0][2], mx.SMALL_SHAPES[0][3]
ADAPTERS = (("a", 16, 32), ("b", 8, 4))  # name, rank, alpha
# The adapters are scaled like a fine-tune's correction, not like a second model: their term is of the order of the base
# projection's output.  Base: W = codebook entry (sigma 0.05) x scale (0.05 .. 0.25), so a projection of K = 1024 unit inputs has
# sigma sqrt(1024) x 0.05 x 0.15 = 0.24.  Adapter "a": A ~ N(0, 1 / K) gives t ~ N(0, 1) per unit input, and the term
# scaling x sqrt(r) x sigma_B = 2 x 4 x sigma_B reaches 0.24 at sigma_B = 0.03 (tools/lora_benchmark.py uses 0.02 for its adapters).
# With B ~ N(0, 1 / r), the size tests/test_lora_gpu.py uses on a single layer, the term would be 8 x the base output after w1 / w3
# and far more after the activation: the block output would be a difference of pair outputs two binades above it, where one
# flipped rounding of an intermediate shows as several ulp of the result.
SIGMA_B = 0.03


class _Holder(torch.nn.Module):
    def __init__(self, experts):
        super().__init__()
        self.experts = experts


def _block(seed, dtype=torch.float16):
    from transformers import MixtralConfig

    from aqlm_amd.moe import QuantizedMixtralExperts

    cfg = MixtralConfig(hidden_size=H, intermediate_size=I, num_local_experts=E, num_experts_per_tok=K, num_attention_heads=4,
                        num_key_value_heads=4, router_jitter_noise=0.0)
    q = QuantizedMixtralExperts(cfg, dict(in_group_size=8, out_group_size=1, num_codebooks=1, nbits_per_codebook=16), device=DEV, dtype=dtype)
    gen = torch.Generator(device=DEV).manual_seed(seed)
    with torch.no_grad():
        for lin in q._expert_layers():
            lin.codes.copy_(torch.randint(-32768, 32768, lin.codes.shape, generator=gen, device=DEV, dtype=torch.int32))
            lin.codebooks.copy_(torch.randn(lin.codebooks.shape, generator=gen, device=DEV) * 0.05)
            lin.scales.copy_(torch.rand(lin.scales.shape, generator=gen, device=DEV) * 0.2 + 0.05)
    return q


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


def _route(T, gen):
    logits = torch.randn((T, E), generator=gen, device=DEV)
    w, ids = torch.topk(torch.softmax(logits, -1), K, dim=-1)
    return ids, w / w.sum(-1, keepdim=True)


@pytest.fixture()
def routed_limit(monkeypatch):
    import aqlm_amd.lora as lora

    monkeypatch.setattr(lora, "ROUTED_BGMV_MAX_PAIRS", 256)
    return lora


@pytest.fixture()
def launches(monkeypatch):
    """Counts the adapter launches through a wrapper around ``hk.lora_bgmv_routed_``."""
    from aqlm_amd.inference_kernels import hip_kernel as hk

    calls = []
    real = hk.lora_bgmv_routed_
    monkeypatch.setattr(hk, "lora_bgmv_routed_", lambda *a: (calls.append(a[0].shape[0]), real(*a))[1])
    return calls


@pytest.mark.parametrize("base", ["routed", "packed", "grouped"])
def test_hip_route_on_every_base_route_against_the_torch_path(routed_limit, launches, monkeypatch, base):
    from aqlm_amd import moe

    lora = routed_limit
    q = _block(30)
    if base == "packed":
        monkeypatch.setattr(moe, "ROUTED_PACKED_MAX_PAIRS", 64)
        rep = moe.prepack_experts(q, min_codes=1)
        assert rep["blocks_served"] == 1, rep
    T = 40 if base == "grouped" else 4
    holder, bank = _attach(lora, q)
    gen = torch.Generator(device=DEV).manual_seed(31)
    x = torch.randn((T, H), generator=gen, device=DEV).half()
    idx, wts = _route(T, gen)
    ids = torch.tensor([1, 0, 2, -1] * (T // 4), device=DEV)
    with torch.no_grad():
        assert q.takes_routed_path(x, idx) == (base != "grouped") and q.takes_grouped_path(x, idx) == (base == "grouped")
        assert (q._prepack is not None and q.served_by_routed_packed()) == (base == "packed")
        bare = q(x, idx, wts)
        for which in ("a", "b", ids):
            bank.select(which)
            n = len(launches)
            y = holder.experts(x, idx, wts)
            assert launches[n:] == [T * K, T * K], "the HIP route was not taken (one launch pair per projection group)"
            monkeypatch.setattr(lora, "ROUTED_BGMV_MAX_PAIRS", 0)
            ref = holder.experts(x, idx, wts)
            monkeypatch.setattr(lora, "ROUTED_BGMV_MAX_PAIRS", 256)
            assert len(launches) == n + 2, "ROUTED_BGMV_MAX_PAIRS = 0 did not switch the route off"
            assert not torch.equal(ref, bare) and not torch.equal(y, bare)
            print(f"adapter term / base output: {float((ref.float() - bare.float()).abs().mean() / bare.float().abs().mean()):.3g}")
            check_bound(y, ref, torch.float16, f"{base} base, select {which if isinstance(which, str) else 'ids'}")
            if not isinstance(which, str):  # ids 2 and -1 are outside the bank: the bare block's rows on the HIP route
                assert torch.equal(y[2::4], bare[2::4]) and torch.equal(y[3::4], bare[3::4])
    lora.detach_adapters(holder)
    assert holder.experts is q


def test_select_none_is_the_bare_block_and_per_sequence_ids_equal_per_token_ids(routed_limit, launches):
    lora = routed_limit
    q = _block(32)
    holder, bank = _attach(lora, q)
    gen = torch.Generator(device=DEV).manual_seed(33)
    T = 8
    x = torch.randn((T, H), generator=gen, device=DEV).half()
    idx, wts = _route(T, gen)
    with torch.no_grad():
        bare = q(x, idx, wts)
        bank.select("a")
        assert not torch.equal(holder.experts(x, idx, wts), bare)
        n = len(launches)
        bank.select(None)
        assert torch.equal(holder.experts(x, idx, wts), bare) and len(launches) == n, "select(None) is not the bare block"
        bank.select(torch.tensor([1, 1, 1, 1, 0, 0, 0, 0], device=DEV))
        y8 = holder.experts(x, idx, wts)
        bank.select(torch.tensor([1, 0], device=DEV))  # two sequences of four rows
        n = len(launches)
        y2 = holder.experts(x, idx, wts)
        assert len(launches) == n + 2 and torch.equal(y2, y8)
        assert not torch.equal(y8[0], bare[0]) and not torch.equal(y8[4], bare[4])
        bank.select(torch.tensor([1, 0, 1], device=DEV))
        with pytest.raises(ValueError, match="one per row"):
            holder.experts(x, idx, wts)


def test_captured_decode_step_follows_both_id_tensors_and_a_stale_table_raises(routed_limit, launches):
    lora = routed_limit
    q = _block(34)
    holder, bank = _attach(lora, q)
    gen = torch.Generator(device=DEV).manual_seed(35)
    T = 4
    x = torch.randn((T, H), generator=gen, device=DEV).half()
    routes = [_route(T, gen)[0] for _ in range(2)]
    _, wts = _route(T, gen)
    assert not torch.equal(routes[0], routes[1])
    idx = routes[0].clone()
    ids = torch.full((T,), -1, dtype=torch.int64, device=DEV)
    bank.select(ids)
    cases = [([-1] * 4, 0), ([0, 1, 0, 1], 0), ([1, 1, 0, -1], 1), ([0, 0, 0, 0], 1)]
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
        n = len(launches)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = holder.experts(x, idx, wts)
        assert len(launches) == n + 2, "the captured step did not take the HIP route"
        for (values, r), want in zip(cases, eager):
            ids.copy_(torch.tensor(values, device=DEV))
            idx.copy_(routes[r])
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(out, want), f"replay with adapter ids {values} on routing {r}"
        # an adapter written in place: the table is stale, and a capture cannot rebuild it
        holder.experts.lora_A["a"]["0"]["w1"].weight.mul_(1.0)
        stale = torch.cuda.CUDAGraph()
        with torch.cuda.graph(stale):
            with pytest.raises(RuntimeError, match="before capturing"):
                holder.experts(x, idx, wts)
        holder.experts(x, idx, wts)  # an eager call rebuilds it
        torch.cuda.synchronize()


def _moe_lora64(dense, adapters, x, idx, wts, aids):
    """fp64 autograd evaluation of the block definition with adapters: dense[(e, w)] the dequantised W, adapters[a][(e, w)] =
    (A, B, scaling); adapters added before the activation and after w2, weighted sum over top_k."""
    out = torch.zeros_like(x)
    for e in range(E):
        tok, pos = torch.where(idx == e)
        if tok.numel() == 0:
            continue

        def proj(w, v):
            y = v @ dense[(e, w)].T
            for a, per in enumerate(adapters):
                A, B, s = per[(e, w)]
                y = y + torch.where((aids[tok] == a)[:, None], s * ((v @ A.T) @ B.T), torch.zeros((), dtype=v.dtype, device=v.device))
            return y

        h = torch.nn.functional.silu(proj("w1", x[tok])) * proj("w3", x[tok])
        out = out.index_add(0, tok, proj("w2", h) * wts[tok, pos, None])
    return out


def test_training_through_the_grouped_base_and_the_torch_path_matches_fp64_autograd(routed_limit, launches):
    """Bound: the grouped-backward GPU test's for grad_x (tests/test_moe_grouped_bwd_gpu.py): mean |error| / mean |reference|
    <= 5e-3 in fp16."""
    from tests.test_moe_gpu import _w64

    lora = routed_limit
    q = _block(36)
    holder, bank = _attach(lora, q)
    wrapper = holder.experts
    trained = [p for store in (wrapper.lora_A, wrapper.lora_B) for p in store["a"].parameters()]
    for p in trained:
        p.requires_grad_(True)
    gen = torch.Generator(device=DEV).manual_seed(37)
    T = 8
    x0 = torch.randn((T, H), generator=gen, device=DEV).half()
    idx, wts = _route(T, gen)
    r = torch.randn((T, H), generator=gen, device=DEV)
    ids = torch.tensor([0, 1, 0, 0, -1, 0, 1, 0], device=DEV)
    bank.select(ids)
    x = x0.clone().requires_grad_()
    assert q.takes_grouped_path(x, idx), "a call that needs a gradient takes the grouped base route"
    n = len(launches)
    (wrapper(x, idx, wts).float() * r).sum().backward()
    assert len(launches) == n, "a call that needs a gradient takes the torch path"
    dense = {(e, w): _w64((lin.codes, lin.codebooks, lin.scales, None)) for e in range(E)
             for w, lin in ((w, getattr(q.expert(e), w)) for w in ("w1", "w3", "w2"))}
    leaves = [{(e, w): (wrapper._weights(n_, e, w)[0].detach().double().requires_grad_(), wrapper._weights(n_, e, w)[1].detach().double().requires_grad_(),
                        wrapper.scaling[n_]) for e in range(E) for w in ("w1", "w3", "w2")} for n_ in bank.names]
    x64 = x0.double().requires_grad_()
    (_moe_lora64(dense, leaves, x64, idx, wts.double(), ids) * r.double()).sum().backward()

    def rel(g, g64):
        return ((g.double() - g64).abs().mean() / g64.abs().mean()).item()

    bound = 5e-3
    print(f"hidden_states.grad: {rel(x.grad, x64.grad):.3g}")
    assert rel(x.grad, x64.grad) <= bound, ("hidden_states.grad", rel(x.grad, x64.grad))
    checked = 0
    for (e, w), (A64, B64, _) in leaves[0].items():
        A, B, _ = wrapper._weights("a", e, w)
        if float(A64.grad.abs().max()) == 0.0:
            assert A.grad is None or float(A.grad.abs().max()) == 0.0
            continue  # no token with adapter "a" reached this expert
        print(f"expert {e} {w}: A.grad {rel(A.grad, A64.grad):.3g}, B.grad {rel(B.grad, B64.grad):.3g}")
        assert rel(A.grad, A64.grad) <= bound, ("A.grad", e, w, rel(A.grad, A64.grad))
        assert rel(B.grad, B64.grad) <= bound, ("B.grad", e, w, rel(B.grad, B64.grad))
        checked += 1
    assert checked >= 3
    assert all(p.grad is None for p in q.parameters()) and all(p.grad is None for p in wrapper.lora_A["b"].parameters())
