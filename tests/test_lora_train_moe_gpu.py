"""Training the LoRA adapters on the routed Mixtral experts on device launches, on the MI355X.

Raw ops: ``torch.ops.aqlm.lora_transpose_routed_`` (every live entry's copies equal ``.t().contiguous()``, the rest of the buffer
and a canary stay); grad_x = ``lora_sgmv_routed_`` on the transposed table, bit for bit against ``lora_sgmv_`` on one row with
the transposed entry as a one-slot table and inside ``check_bound`` of the fp64 definition; ``torch.ops.aqlm.lora_grad_routed``
against the fp64 sum over the same inputs inside the standard bound of an fp32 summation in any order,
``(n + 3) * 2^-24 * scaling * sum_p |w| |V|`` with n = the pairs of that (adapter, expert) + the slices of w (derived: n - 1
additions of n products, each product one rounding of the fused multiply-add, the slices added first, one rounding for the
scaling; computed by the test), its reproducibility, its independence of other pairs, and what it must leave alone.

Module: ``aqlm.lora.LoraQuantizedMixtralExperts`` with trainable adapters takes the device route (``_torch_pairs`` patched to
raise), its forward has the bits of the serving route, and the gradients of hidden_states, A and B meet the training bound of
tests/test_lora_moe_gpu.py against its fp64 autograd model (mean |error| / mean |reference| <= 5e-3 in fp16, 8 x that in bf16: the
ratio of the unit roundoffs), as does the torch path on the same inputs; two backward runs are bit-equal; a captured forward +
backward follows both id tensors; and adapters train behind an input that does not require grad.

The module tests set ``lora.ROUTED_TRAIN_MAX_PAIRS`` themselves: the shipped value is a measured cross-over
(profiles/lora_moe_train.json), not part of what is checked here."""
import pytest
import torch

from tests.moe_experts import SMALL_SHAPES
from tests.test_lora_moe_gpu import (DEV, DTYPES, E, K, MODES, RANKS, _attach, _block, _entries, _ids, _live,
                                     _moe_lora64)
from tests.test_lora_sgmv_gpu import check_bound

pytestmark = pytest.mark.gpu

# (in_features, out_features): one K slice each way; a k-step tail both ways; two K slices in the forward AND in the transposed call
SHAPES = [(64, 16), (520, 296), (1032, 1048)]
TOKENS = (1, 3, 40, 150)  # 300 pairs: about five 16-pair tiles per expert and a partial one
TILE = 16
MAXR = max(RANKS)


def _hk():
    from aqlm_amd.inference_kernels import hip_kernel as hk

    return hk


def _tensors(aids, eids, a_dtype=torch.int64, e_dtype=torch.int64):
    at = None if aids is None else torch.tensor(aids, dtype=a_dtype, device=DEV)
    et = torch.tensor(eids, dtype=e_dtype, device=DEV)
    return at, et, torch.ops.aqlm.moe_bucket(et, E, TILE)


def _transposed(entries):
    """-> (forward table, buffer, transposed table, offsets), the copies written."""
    hk = _hk()
    table = hk.lora_routed_table(entries, torch.device(DEV))
    buffer, ttable, offsets = hk.lora_routed_transposed_table(entries, torch.device(DEV))
    S = len(entries[0][0])
    A, B, _ = next(ent for pa in entries for pe in pa for ent in pe if ent is not None)
    fout, fin = B.shape[0], A.shape[1]
    torch.ops.aqlm.lora_transpose_routed_(buffer, table, ttable, [len(entries), E, S, MAXR, fout, fin])
    return table, buffer, ttable, offsets


def _grad_x_call(gy, at, et, bucket, ttable, n, s, fin):
    """The transposed call of segment s -> (grad_x per pair [P, fin] in the storage type, u [P, splits, MAXR])."""
    hk = _hk()
    P, S, fout = gy.shape
    words = ttable.shape[0] // S
    u = torch.zeros((P, hk.lora_sgmv_splits(fout), MAXR), dtype=torch.float32, device=DEV)
    gx = torch.zeros((P, 1, fin), dtype=gy.dtype, device=DEV)
    hk.lora_sgmv_routed_(gx, gy[:, s, :], at, et, bucket, ttable[s * words:(s + 1) * words], [n, E, 1, MAXR, fin, fout, et.shape[1]],
                         True, workspace=u.view(-1))
    return gx.view(P, fin), u


# ---------------------------------------------------------------------------------------------------------------------------
# raw ops
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [2, 1], ids=["w13", "w2"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
@pytest.mark.parametrize("fin,fout", SHAPES)
def test_transpose_copies_every_live_entry_and_nothing_else(fin, fout, dtype, S):
    hk = _hk()
    entries = _entries(1, fin, fout, dtype, S)
    table = hk.lora_routed_table(entries, torch.device(DEV))
    ranks = [[[0 if ent is None else ent[0].shape[0] for ent in pe] for pe in pa] for pa in entries]
    scal = [[[0.0 if ent is None else ent[2] for ent in pe] for pe in pa] for pa in entries]
    _, offsets, elements = hk.lora_routed_transposed_layout(ranks, scal, fout, fin, 0)
    assert set(offsets) == {(a, e, s) for a in range(3) for e in range(E) for s in range(S) if _live(entries, a, e, s) is not None}
    assert elements == sum(r * (fin + fout) for pa in ranks for pe in pa for r in pe if r % 8 == 0)
    sentinel, canary = 0.25, -3.0
    big = torch.full((elements + 64,), sentinel, dtype=dtype, device=DEV)
    big[elements:] = canary
    structs, _, _ = hk.lora_routed_transposed_layout(ranks, scal, fout, fin, big.data_ptr())
    ttable = torch.frombuffer(bytearray(bytes(structs)), dtype=torch.int64).to(DEV)
    geometry = [3, E, S, MAXR, fout, fin]
    torch.ops.aqlm.lora_transpose_routed_(big[:elements], table, ttable, geometry)
    assert bool((big[elements:] == canary).all()), "the canary past the buffer was written"
    covered = 0
    for (a, e, s), (ob, oa) in offsets.items():
        A, B, _ = entries[a][e][s]
        r = A.shape[0]
        assert torch.equal(big[ob:ob + r * fout].view(r, fout), B.t().contiguous()), (a, e, s, "B^T")
        assert torch.equal(big[oa:oa + r * fin].view(fin, r), A.t().contiguous()), (a, e, s, "A^T")
        covered += r * (fin + fout)
    assert covered == elements  # the zero entry and the rank-12 entry own nothing
    # a buffer that ends before the last entry's copies: that entry is dropped on the device, every other copy is made again
    last = max(offsets, key=lambda k_: offsets[k_][0])
    big.fill_(sentinel)
    torch.ops.aqlm.lora_transpose_routed_(big[:elements - 8], table, ttable, geometry)
    ob, oa = offsets[last]
    assert bool((big[ob:] == sentinel).all()), "copies that do not fit the buffer were written"
    first = min(offsets, key=lambda k_: offsets[k_][0])
    assert torch.equal(big[:offsets[first][1]].view(-1, fout), entries[first[0]][first[1]][first[2]][1].t().contiguous())
    # a transposed entry of another rank (a table of other weights): its region stays as it was
    words = ttable.cpu().clone()
    s_, a_, e_ = first[2], first[0], first[1]
    w0 = ((s_ * 3 + a_) * E + e_) * 3 + 2
    words[w0] = (int(words[w0]) & ~0xFFFFFFFF) | (entries[a_][e_][s_][0].shape[0] + 8)
    big.fill_(sentinel)
    torch.ops.aqlm.lora_transpose_routed_(big[:elements], table, words.to(DEV), geometry)
    assert bool((big[:offsets[first][1] + 8] == sentinel).all()), "an entry whose transposed rank differs was copied"
    assert not bool((big[:elements] == sentinel).all())


def _grad_x_ref64(gy, aids, eids, entries, s, fin):
    P = gy.shape[0]
    k = len(eids[0])
    ref = torch.zeros((P, fin), dtype=torch.float64, device=DEV)
    at = torch.tensor([0] * (P // k) if aids is None else aids, device=DEV).repeat_interleave(k)
    et = torch.tensor(eids, device=DEV).reshape(-1)
    for a in range(len(entries)):
        for e in range(E):
            ent = _live(entries, a, e, s)
            rows = torch.nonzero((at == a) & (et == e)).squeeze(1)
            if ent is not None and rows.numel():
                A, B, sc = ent
                ref[rows] = float(torch.tensor(sc, dtype=torch.float32)) * ((gy[rows, s].double() @ B.double()) @ A.double())
    return ref


@pytest.mark.parametrize("a_dtype,e_dtype", [(torch.int64, torch.int64), (torch.int32, torch.int32)], ids=["i64", "i32"])
@pytest.mark.parametrize("S,per_pair", MODES, ids=["w13", "w2"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
@pytest.mark.parametrize("fin,fout", SHAPES)
def test_grad_x_is_the_row_op_on_the_transposed_entry_bit_for_bit(fin, fout, dtype, S, per_pair, a_dtype, e_dtype):
    hk = _hk()
    entries = _entries(2, fin, fout, dtype, S)
    _, buffer, ttable, offsets = _transposed(entries)
    slots = {}
    for (a, e, s), (ob, oa) in offsets.items():
        A, B, sc = entries[a][e][s]
        r = A.shape[0]
        slots[(a, e, s)] = (hk.lora_table([(buffer[ob:ob + r * fout].view(r, fout), buffer[oa:oa + r * fin].view(fin, r), sc)],
                                          torch.device(DEV)), r)
    gen = torch.Generator().manual_seed(3)
    for T in TOKENS:
        gy = (torch.randn((T * K, S, fout), generator=gen) / fout ** 0.5).to(dtype).to(DEV)
        aids, eids = _ids(20 + T, T)
        at, et, bucket = _tensors(aids, eids, a_dtype, e_dtype)
        for s in range(S):
            gx, _ = _grad_x_call(gy, at, et, bucket, ttable, 3, s, fin)
            want = torch.zeros_like(gx)
            for p in range(T * K):
                ent = _live(entries, aids[p // K], eids[p // K][p % K], s)
                if ent is not None:
                    tab, r = slots[(aids[p // K], eids[p // K][p % K], s)]
                    torch.ops.aqlm.lora_sgmv_(want[p:p + 1], gy[p, s:s + 1], None, tab, [1, r, fin, fout])
            assert torch.equal(gx, want), f"T {T} segment {s}: not bit-equal to lora_sgmv_ on the transposed entry"
            check_bound(gx, _grad_x_ref64(gy, aids, eids, entries, s, fin), dtype, f"grad_x in {fin} out {fout} {dtype} T {T} s {s}")
    # NULL adapter ids: adapter 0 for every token -- its [E] slice of each segment's table
    T = 3
    gy = (torch.randn((T * K, S, fout), generator=gen) / fout ** 0.5).to(dtype).to(DEV)
    _, eids = _ids(6, T)
    _, et, bucket = _tensors(None, eids, e_dtype=e_dtype)
    words = ttable.shape[0] // S
    for s in range(S):
        gx = torch.zeros((T * K, 1, fin), dtype=dtype, device=DEV)
        hk.lora_sgmv_routed_(gx, gy[:, s, :], None, et, bucket, ttable[s * words:s * words + words // 3], [1, E, 1, MAXR, fin, fout, K], True)
        at0, _, _ = _tensors([0] * T, eids)
        assert torch.equal(gx.view(T * K, fin), _grad_x_call(gy, at0, et, bucket, ttable, 3, s, fin)[0])


def test_a_call_whose_out_features_are_no_multiple_of_8_is_declined():
    hk = _hk()
    assert hk.lora_transpose_routed_supported(296, 520, 24, E, 2) and hk.lora_grad_routed_supported(296, 24, 300, E, 2)
    assert not hk.lora_transpose_routed_supported(300, 520, 24, E, 2) and not hk.lora_grad_routed_supported(300, 24, 300, E, 2)
    assert not hk.lora_sgmv_routed_supported(520, 300, 24, 300, E, 1)  # the transposed call: in_features = 300
    entries = _entries(4, 520, 300, torch.float16, 2)
    with pytest.raises(NotImplementedError):
        hk.lora_routed_transposed_table(entries, torch.device(DEV))


def _grad_setup(seed, T, dim, dtype, S, per_pair, splits, aids=None, eids=None):
    """Random operands of lora_grad_routed: V rows (token / pair rows shared by the segments, or [P, S, dim]) and fp32 w."""
    gen = torch.Generator().manual_seed(seed)
    P = T * K
    if per_pair is None:  # the grad_B^T layout: V = grad_y [P, S, dim]
        v = torch.randn((P, S, dim), generator=gen).to(dtype).to(DEV)
        vlay = [S * dim, dim, 1]
    else:
        v = torch.randn((P if per_pair else T, dim), generator=gen).to(dtype).to(DEV)
        vlay = [dim, 0, int(per_pair)]
    w = torch.randn((P, S, splits, MAXR), generator=gen).to(DEV)
    layout = vlay + [S * splits * MAXR, splits * MAXR, splits, MAXR]
    if aids is None:
        aids, eids = _ids(seed + 1, T)
    return v, w, layout, aids, eids


def _grad_ref64(v, w, layout, aids, eids, entries, a, pairs_of=None):
    """fp64 sum over the same inputs and the bound per element -> (G64 [E, S, MAXR, dim], bound)."""
    P, S = w.shape[0], w.shape[1]
    k = len(eids[0])
    dim = v.shape[-1]
    G = torch.zeros((E, S, MAXR, dim), dtype=torch.float64, device=DEV)
    bound = torch.zeros_like(G)
    at = torch.tensor([0] * (P // k) if aids is None else aids, device=DEV).repeat_interleave(k)
    et = torch.tensor(eids, device=DEV).reshape(-1)
    keep = torch.ones(P, dtype=torch.bool, device=DEV) if pairs_of is None else pairs_of
    for e in range(E):
        rows = torch.nonzero((at == a) & (et == e) & keep).squeeze(1)
        for s in range(S):
            ent = _live(entries, a, e, s)
            if ent is None or rows.numel() == 0:
                continue
            r, sc = ent[0].shape[0], float(torch.tensor(ent[2], dtype=torch.float32))
            if v.dim() == 3:
                vr = v[rows, s].double()
            else:
                vr = v[rows if layout[2] else rows // k].double()
            G[e, s, :r] = sc * (w[rows, s].double().sum(1)[:, :r].T @ vr)
            n = rows.numel() + w.shape[2]
            bound[e, s, :r] = (n + 3) * 2.0 ** -24 * sc * (w[rows, s].double().abs().sum(1)[:, :r].T @ vr.abs())
    return G, bound


def _grad_run(v, w, layout, at, et, bucket, table, a, out=None, n=3):
    return _hk().lora_grad_routed(v, w, at, et, bucket, table, [n, E, w.shape[1], MAXR, v.shape[-1], et.shape[1], a], layout, out=out)


@pytest.mark.parametrize("splits", [1, 2])
@pytest.mark.parametrize("S,per_pair", MODES + [(2, None), (1, None)], ids=["x-w13", "x-w2", "gy-w13", "gy-w2"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
@pytest.mark.parametrize("dim", [16, 296, 1048])
def test_grad_routed_against_the_fp64_sum_and_what_it_leaves_alone(dim, dtype, S, per_pair, splits):
    hk = _hk()
    entries = _entries(5, 64, 16, dtype, S)  # the table gives ranks and scalings only: the kernel never follows its pointers
    table = hk.lora_routed_table(entries, torch.device(DEV))
    for T, (a_dtype, e_dtype) in zip(TOKENS, [(torch.int64, torch.int64), (torch.int32, torch.int32)] * 2):
        v, w, layout, aids, eids = _grad_setup(30 + T, T, dim, dtype, S, per_pair, splits)
        at, et, bucket = _tensors(aids, eids, a_dtype, e_dtype)
        for a in range(3):
            numel = E * S * MAXR * dim
            big = torch.full((numel + 64,), 7.0, dtype=torch.float32, device=DEV)
            G = _grad_run(v, w, layout, at, et, bucket, table, a, out=big[:numel].view(E, S, MAXR, dim))
            assert bool((big[numel:] == 7.0).all()), "the canary past the output was written"
            G64, bound = _grad_ref64(v, w, layout, aids, eids, entries, a)
            hits = 0
            for e in range(E):
                for s in range(S):
                    ent = _live(entries, a, e, s)
                    if ent is None:
                        assert bool((G[e, s] == 7.0).all()), f"adapter {a} expert {e}: an entry that is not live was written"
                        continue
                    r = ent[0].shape[0]
                    assert bool((G[e, s, r:] == 0).all()), "ranks past the entry's rank are not zero"
                    err = (G[e, s, :r].double() - G64[e, s, :r]).abs()
                    assert bool((err <= bound[e, s, :r]).all()), (T, a, e, s, float((err / bound[e, s, :r].clamp_min(1e-300)).max()))
                    if not bool(G64[e, s].any()):
                        assert bool((G[e, s] == 0).all()), "an entry without pairs is not zero"
                    else:
                        hits += 1
            if T == 150:
                assert hits >= S * 3, "the routing does not reach the adapter's experts"
            assert torch.equal(_grad_run(v, w, layout, at, et, bucket, table, a), torch.where(G == 7.0, torch.zeros_like(G), G)), "two runs differ"
    # NULL adapter ids: adapter 0 for every token, on its [1][E][S] slice of the table
    v, w, layout, _, eids = _grad_setup(40, 3, dim, dtype, S, per_pair, splits)
    _, et, bucket = _tensors(None, eids)
    at0 = torch.zeros(3, dtype=torch.int64, device=DEV)
    words = table.shape[0] // 3
    assert torch.equal(_grad_run(v, w, layout, None, et, bucket, table[:words], 0, n=1), _grad_run(v, w, layout, at0, et, bucket, table, 0))


@pytest.mark.parametrize("S,per_pair", [(2, False), (1, True), (2, None)], ids=["x-w13", "x-w2", "gy-w13"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
def test_grad_routed_depends_on_its_own_pairs_alone(dtype, S, per_pair):
    hk = _hk()
    dim, T, a = 296, 150, 2
    entries = _entries(6, 64, 16, dtype, S)
    table = hk.lora_routed_table(entries, torch.device(DEV))
    v, w, layout, aids, eids = _grad_setup(50, T, dim, dtype, S, per_pair, 2)
    at, et, bucket = _tensors(aids, eids)
    G = _grad_run(v, w, layout, at, et, bucket, table, a)
    assert bool(G[0].any()) and bool(G[3].any())
    # rows of pairs of other adapters rewritten (NaN: any use would show)
    other_t = [t for t in range(T) if aids[t] != a]
    other_p = [t * K + j for t in other_t for j in range(K)]
    v2, w2 = v.clone(), w.clone()
    w2[other_p] = float("nan")
    if v.dim() == 3 or layout[2]:
        v2[other_p] = float("nan")
    else:
        v2[other_t] = float("nan")
    assert torch.equal(_grad_run(v2, w2, layout, at, et, bucket, table, a), G), "rows of other adapters' pairs entered the sum"
    # the pairs of ANOTHER EXPERT rewritten: the other experts' entries keep their bits
    et_flat = torch.tensor(eids).reshape(-1)
    p1 = torch.nonzero(et_flat == 1).squeeze(1).tolist()
    w3 = w.clone()
    w3[p1] = float("nan")
    G3 = _grad_run(v, w3, layout, at, et, bucket, table, a)
    assert torch.equal(G3[[0, 2, 3]], G[[0, 2, 3]]) and bool(torch.isnan(G3[1]).any())
    # pairs of other adapters ADDED at the end (tokens appended): the sums do not move
    extra = 10
    aids_x = aids + [(0, 1, -1, 3)[i % 4] for i in range(extra)]
    eids_x = eids + [[i % E, (i + 1) % E] for i in range(extra)]
    vx, wx, layout_x, _, _ = _grad_setup(51, T + extra, dim, dtype, S, per_pair, 2, aids_x, eids_x)
    wx[:T * K] = w
    vx[:v.shape[0]] = v
    atx, etx, bucketx = _tensors(aids_x, eids_x)
    assert torch.equal(_grad_run(vx, wx, layout_x, atx, etx, bucketx, table, a), G), "added pairs of other adapters changed the sums"


@pytest.mark.parametrize("S,per_pair", [(2, False), (1, True)], ids=["x-w13", "x-w2"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
def test_grad_routed_hostile_ids_and_foreign_bucket_records_change_nothing(dtype, S, per_pair):
    hk = _hk()
    dim, T, a = 296, 40, 0
    entries = _entries(7, 64, 16, dtype, S)
    table = hk.lora_routed_table(entries, torch.device(DEV))
    v, w, layout, aids, eids = _grad_setup(60, T, dim, dtype, S, per_pair, 1)
    # adapter ids by token: t % 5 = 0 -> -1, 1 -> 0, 2 -> 3 (= num_adapters), 3 -> 1, 4 -> 2; hostile expert ids under adapter 0
    hostile = {1: -1, 6: E, 11: 2 ** 40, 16: -(2 ** 40)}
    assert all(aids[t] == 0 for t in hostile)
    clean = [list(row) for row in eids]
    for t, bad in hostile.items():
        eids[t][t % K] = bad
    keep = torch.ones(T * K, dtype=torch.bool, device=DEV)
    for t in hostile:
        keep[t * K + t % K] = False
    at, et, bucket = _tensors(aids, eids)
    G = _grad_run(v, w, layout, at, et, bucket, table, a)
    G64, bound = _grad_ref64(v, w, layout, aids, clean, entries, a, keep)
    assert bool(((G.double() - G64).abs() <= bound).all()), "pairs with hostile expert ids entered the sum"
    # the same pairs with other out-of-range ids, and with their rows poisoned: not a bit moves
    for t in hostile:
        eids[t][t % K] = E + 7
    w2 = w.clone()
    w2[~keep] = float("nan")
    at2, et2, bucket2 = _tensors(aids, eids)
    assert torch.equal(_grad_run(v, w2, layout, at2, et2, bucket2, table, a), G)
    # a foreign bucket: the bucket of OTHER expert ids -- a listed pair whose expert id is not its tile's contributes nothing
    _, other = _ids(99, T)
    _, _, foreign = _tensors(aids, other)
    agree = torch.tensor([[eids[t][j] == other[t][j] for j in range(K)] for t in range(T)], device=DEV).reshape(-1)
    Gf = _grad_run(v, w, layout, at2, et2, foreign, table, a)
    G64f, boundf = _grad_ref64(v, w, layout, aids, clean, entries, a, keep & agree)
    assert bool(((Gf.double() - G64f).abs() <= boundf).all()) and not torch.equal(Gf, G)
    # records no bucket of these sizes holds: a count of 17, a first past the list, an expert id out of range -- the tile is dropped
    host = bucket2.cpu()
    max_tiles = (T * K + TILE - 1) // TILE + min(E, T * K)
    tiles = host[4:4 + 4 * max_tiles].view(max_tiles, 4)
    pairs = host[4 + 4 * max_tiles:]
    for field, bad in ((2, 17), (1, T * K), (1, -3), (2, 0)):
        broken = host.clone()
        rec = broken[4:4 + 4 * max_tiles].view(max_tiles, 4)
        slot = next(i for i in range(int(host[0])) if int(tiles[i, 0]) == 1)  # a tile of expert 1
        rec[slot, field] = bad
        dropped = pairs[int(tiles[slot, 1]):int(tiles[slot, 1]) + int(tiles[slot, 2])].tolist()
        keep_b = keep.clone()
        keep_b[dropped] = False
        Gb = _grad_run(v, w, layout, at2, et2, broken.to(DEV), table, a)
        G64b, boundb = _grad_ref64(v, w, layout, aids, clean, entries, a, keep_b)
        assert bool(((Gb.double() - G64b).abs() <= boundb).all()), (field, bad)
        assert torch.equal(Gb[[0, 2, 3]], G[[0, 2, 3]])
    # a list entry that is no pair: its tile is dropped too
    broken = host.clone()
    slot = next(i for i in range(int(host[0])) if int(tiles[i, 0]) == 2)
    broken[4 + 4 * max_tiles + int(tiles[slot, 1])] = T * K + 5
    dropped = pairs[int(tiles[slot, 1]):int(tiles[slot, 1]) + int(tiles[slot, 2])].tolist()
    keep_b = keep.clone()
    keep_b[dropped] = False
    Gb = _grad_run(v, w, layout, at2, et2, broken.to(DEV), table, a)
    G64b, boundb = _grad_ref64(v, w, layout, aids, clean, entries, a, keep_b)
    assert bool(((Gb.double() - G64b).abs() <= boundb).all())


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
def test_grad_routed_one_expert_takes_every_pair_and_one_is_empty(dtype):
    """top_k 1, every one of 150 pairs on expert 1: ten tiles walked by one workgroup, three experts whose entries are zeros."""
    hk = _hk()
    dim, T = 296, 150
    for S, per_pair in MODES:
        entries = _entries(8, 64, 16, dtype, S)
        table = hk.lora_routed_table(entries, torch.device(DEV))
        gen = torch.Generator().manual_seed(70)
        v = torch.randn((T, dim), generator=gen).to(dtype).to(DEV)
        w = torch.randn((T, S, 2, MAXR), generator=gen).to(DEV)
        layout = [dim, 0, int(per_pair), S * 2 * MAXR, 2 * MAXR, 2, MAXR]
        aids = [(-1, 0, 3, 1, 2)[t % 5] for t in range(T)]
        eids = [[1]] * T
        at = torch.tensor(aids, device=DEV)
        et = torch.tensor(eids, device=DEV)
        bucket = torch.ops.aqlm.moe_bucket(et, E, TILE)
        for a in range(3):
            G = hk.lora_grad_routed(v, w, at, et, bucket, table, [3, E, S, MAXR, dim, 1, a], layout)
            G64, bound = _grad_ref64(v, w, layout, aids, eids, entries, a)
            assert bool(((G.double() - G64).abs() <= bound).all()) and bool(G[1].any())
            assert not bool(G[[0, 2, 3]].any()), "an expert without pairs has a gradient"


# ---------------------------------------------------------------------------------------------------------------------------
# module level: the block of tests/test_lora_moe_gpu.py (4 experts, hidden 1024, intermediate 2048, 1x16 g8), adapter "a" trained
# ---------------------------------------------------------------------------------------------------------------------------
H, I = SMALL_SHAPES[0][2], SMALL_SHAPES[0][3]
BOUND = {torch.float16: 5e-3, torch.bfloat16: 8 * 5e-3}
IDS8 = [0, 1, 0, 0, -1, 0, 1, 0]  # the ids of the training test of tests/test_lora_moe_gpu.py


@pytest.fixture()
def train_on(monkeypatch):
    import aqlm_amd.lora as lora

    monkeypatch.setattr(lora, "ROUTED_BGMV_MAX_PAIRS", 256)
    monkeypatch.setattr(lora, "ROUTED_SGMV_MAX_PAIRS", 65536)
    monkeypatch.setattr(lora, "ROUTED_TRAIN_MAX_PAIRS", 65536)
    return lora


def _problem(seed, T, dtype, ids=None):
    """Inputs on the host generator (so the routing can be checked without a device): x0, expert ids, weights, cotangent, adapter ids."""
    gen = torch.Generator().manual_seed(seed)
    x0 = torch.randn((T, H), generator=gen).to(dtype).to(DEV)
    wts_all = torch.softmax(torch.randn((T, E), generator=gen), -1)
    wts, idx = torch.topk(wts_all, K, dim=-1)
    wts = (wts / wts.sum(-1, keepdim=True)).to(DEV)
    r = torch.randn((T, H), generator=gen).to(DEV)
    ids = torch.tensor(([0, 1, 0, 0, -1] * T)[:T] if ids is None else ids)
    return x0, idx.to(DEV), wts, r, ids.to(DEV)


def _train_setup(lora, seed, dtype=torch.float16):
    q = _block(seed, dtype)
    holder, bank = _attach(lora, q, dtype=dtype)
    wrapper = holder.experts
    for store in (wrapper.lora_A, wrapper.lora_B):
        for p in store["a"].parameters():
            p.requires_grad_(True)
    return q, wrapper, bank


def _step(wrapper, x0, idx, wts, r, x_grad=True):
    """One forward + backward -> (output, hidden_states.grad or None, {(e, w): (A.grad, B.grad)} of adapter "a")."""
    for p in wrapper.parameters():
        p.grad = None
    x = x0.clone().requires_grad_(x_grad)
    y = wrapper(x, idx, wts)
    (y.float() * r).sum().backward()
    grads = {(e, w): tuple(t.grad for t in wrapper._weights("a", e, w)[:2]) for e in range(E) for w in ("w1", "w3", "w2")}
    return y.detach(), x.grad, grads


def _fp64(q, wrapper, bank, x0, idx, wts, r, ids, x_grad=True):
    from tests.test_moe_gpu import _w64

    dense = {(e, w): _w64((lin.codes, lin.codebooks, lin.scales, None)) for e in range(E)
             for w, lin in ((w, getattr(q.expert(e), w)) for w in ("w1", "w3", "w2"))}
    leaves = [{(e, w): (wrapper._weights(n_, e, w)[0].detach().double().requires_grad_(),
                        wrapper._weights(n_, e, w)[1].detach().double().requires_grad_(), wrapper.scaling[n_])
               for e in range(E) for w in ("w1", "w3", "w2")} for n_ in bank.names]
    x64 = x0.double().requires_grad_(x_grad)
    (_moe_lora64(dense, leaves, x64, idx, wts.double(), ids) * r.double()).sum().backward()
    return x64.grad, leaves[0]


def _rel(g, g64):
    return ((g.double() - g64).abs().mean() / g64.abs().mean()).item()


def _check_grads(what, xg, grads, x64g, leaves, bound, every_entry):
    if x64g is not None:
        print(f"{what}: hidden_states.grad {_rel(xg, x64g):.3g}")
        assert _rel(xg, x64g) <= bound, (what, "hidden_states.grad", _rel(xg, x64g))
    checked = 0
    for (e, w), (A64, B64, _) in leaves.items():
        ga, gb = grads[(e, w)]
        if float(A64.grad.abs().max()) == 0.0:
            assert not every_entry, f"{what}: no token with adapter a reached expert {e}"
            assert ga is None or float(ga.abs().max()) == 0.0
            continue
        print(f"{what}: expert {e} {w}: A.grad {_rel(ga, A64.grad):.3g}, B.grad {_rel(gb, B64.grad):.3g}")
        assert _rel(ga, A64.grad) <= bound, (what, "A.grad", e, w, _rel(ga, A64.grad))
        assert _rel(gb, B64.grad) <= bound, (what, "B.grad", e, w, _rel(gb, B64.grad))
        checked += 1
    assert checked >= (3 * E if every_entry else 3)


def _raise(*a, **kw):
    raise AssertionError("the torch path was taken")


@pytest.mark.parametrize("T,dtype", [(8, torch.float16), (8, torch.bfloat16), (150, torch.float16)], ids=["T8-fp16", "T8-bf16", "T150-fp16"])
def test_training_on_the_device_route_matches_fp64_autograd_and_so_does_the_torch_path(train_on, monkeypatch, T, dtype):
    lora = train_on
    q, wrapper, bank = _train_setup(lora, 36, dtype)
    x0, idx, wts, r, ids = _problem(37, T, dtype, IDS8 if T == 8 else None)
    if T == 150:  # every (adapter a, expert) has pairs: nothing below may be skipped (holds for this seed on the host generator)
        assert all(bool(((ids == 0)[:, None] & (idx == e)).any()) for e in range(E))
    bank.select(ids)
    # forward bits: the serving route on the same inputs
    with torch.no_grad():
        served = wrapper(x0, idx, wts)
    with monkeypatch.context() as m:  # route taken: the torch path would raise
        m.setattr(lora._ExpertAdapters, "_torch_pairs", _raise)
        y, xg, grads = _step(wrapper, x0, idx, wts, r)
    if T == 150:  # (16 pairs: the base block serves on the routed launch and trains on the grouped one; see the test below)
        assert q.takes_grouped_path(x0, idx) and torch.equal(y, served), "the forward of the training route is not the serving route's"
    x64g, leaves = _fp64(q, wrapper, bank, x0, idx, wts, r, ids)
    _check_grads(f"device route T {T}", xg, grads, x64g, leaves, BOUND[dtype], every_entry=T == 150)
    assert all(p.grad is None for p in q.parameters()) and all(p.grad is None for p in wrapper.lora_A["b"].parameters())
    assert all(p.grad is None for p in wrapper.lora_B["b"].parameters())
    # run to run
    y2, xg2, grads2 = _step(wrapper, x0, idx, wts, r)
    assert torch.equal(y2, y) and torch.equal(xg2, xg)
    assert all(torch.equal(grads2[k_][i], grads[k_][i]) for k_ in grads for i in (0, 1)), "two backward runs differ"
    # the torch path on the same inputs, held to the same bound
    monkeypatch.setattr(lora, "ROUTED_TRAIN_MAX_PAIRS", 0)
    _, xg_t, grads_t = _step(wrapper, x0, idx, wts, r)
    _check_grads(f"torch path T {T}", xg_t, grads_t, x64g, leaves, BOUND[dtype], every_entry=T == 150)


def test_one_selected_adapter_trains_on_the_device_route(train_on, monkeypatch):
    """``select("a")``: NULL adapter ids, the adapter's own slice of both tables."""
    lora = train_on
    q, wrapper, bank = _train_setup(lora, 38)
    T = 40
    x0, idx, wts, r, _ = _problem(39, T, torch.float16)
    bank.select("a")
    monkeypatch.setattr(lora._ExpertAdapters, "_torch_pairs", _raise)
    y, xg, grads = _step(wrapper, x0, idx, wts, r)
    # forward bits at 80 pairs, where the serving route is the BGMV launch: the SGMV launch on the same inputs is the yardstick
    with monkeypatch.context() as m:
        m.setattr(lora, "ROUTED_BGMV_MAX_PAIRS", 0)
        m.setattr(lora, "ROUTED_SGMV_MIN_PAIRS", 1)
        with torch.no_grad():
            assert q.takes_grouped_path(x0, idx) and torch.equal(y, wrapper(x0, idx, wts)), "forward bits differ from the SGMV route"
    x64g, leaves = _fp64(q, wrapper, bank, x0, idx, wts, r, torch.zeros(T, dtype=torch.int64, device=DEV))
    _check_grads("select(a)", xg, grads, x64g, leaves, 5e-3, every_entry=True)


@pytest.mark.parametrize("limit", [65536, 0], ids=["device-route", "torch-path"])
def test_adapters_train_behind_an_input_that_does_not_require_grad(train_on, monkeypatch, limit):
    """The first block over a frozen embedding: hidden_states has no grad, the adapters of w1 / w3 sit behind the base w2 launch."""
    lora = train_on
    monkeypatch.setattr(lora, "ROUTED_TRAIN_MAX_PAIRS", limit)
    q, wrapper, bank = _train_setup(lora, 40)
    T = 8
    x0, idx, wts, r, ids = _problem(41, T, torch.float16, IDS8)
    bank.select(ids)
    _, xg, grads = _step(wrapper, x0, idx, wts, r, x_grad=False)
    assert xg is None
    _, leaves = _fp64(q, wrapper, bank, x0, idx, wts, r, ids, x_grad=False)
    for w in ("w1", "w3", "w2"):
        assert any(grads[(e, w)][0] is not None for e in range(E)), f"the {w} adapters got no gradient"
    _check_grads("frozen input", None, grads, None, leaves, 5e-3, every_entry=False)
    assert all(p.grad is None for p in q.parameters())
    # no gradient needed at all: the serving routes, as before
    for p in wrapper.parameters():
        p.requires_grad_(False)
    monkeypatch.setattr(lora._ExpertAdapters, "_torch_pairs", _raise)
    assert not wrapper(x0, idx, wts).requires_grad


def test_captured_training_step_follows_both_id_tensors_rewritten_in_place(train_on):
    lora = train_on
    q, wrapper, bank = _train_setup(lora, 42)
    T = 40
    x0, idx_a, wts, r, ids_a = _problem(43, T, torch.float16)
    _, idx_b, _, _, _ = _problem(44, T, torch.float16)
    ids_b = torch.tensor(([1, 0, 0, -1] * T)[:T], device=DEV)
    assert not torch.equal(idx_a, idx_b)
    idx, ids = idx_a.clone(), ids_a.clone()
    bank.select(ids)
    trained = [p for p in wrapper.parameters() if p.requires_grad]
    x = x0.clone().requires_grad_()

    def step():
        (wrapper(x, idx, wts).float() * r).sum().backward()

    eager = {}
    for name, (i_, a_) in (("b", (idx_b, ids_b)), ("a", (idx_a, ids_a))):
        idx.copy_(i_)
        ids.copy_(a_)
        x.grad = None
        for p in trained:
            p.grad = None
        step()
        eager[name] = [x.grad.clone()] + [p.grad.clone() for p in trained]
    assert not torch.equal(eager["a"][0], eager["b"][0])
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(s)
    x.grad = None
    for p in trained:
        p.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    for name, (i_, a_) in (("b", (idx_b, ids_b)), ("a", (idx_a, ids_a)), ("b", (idx_b, ids_b))):
        idx.copy_(i_)
        ids.copy_(a_)
        graph.replay()
        torch.cuda.synchronize()
        got = [x.grad] + [p.grad for p in trained]
        assert all(torch.equal(g, w_) for g, w_ in zip(got, eager[name])), f"replay on ids {name} differs from the eager step"
