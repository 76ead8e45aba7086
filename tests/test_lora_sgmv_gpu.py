"""LoRA adapters at prefill row counts, on the MI355X: the raw op ``torch.ops.aqlm.lora_sgmv_`` (aqlm_hip_lora_sgmv, the segmented
MFMA adapter GEMM) against an fp64 evaluation of ``y_in + scaling * B (A x)``, its bit-exact properties (a row's bits depend on its
own x row, its own y row and its adapter only; rows that name no adapter are never written), and ``aqlm.lora`` on a prepacked 1x16
g8 layer: SGMV route against torch path, per-sequence ids, ``select(None)``, hipGraph replay with the ids rewritten in place.

Bound: the one of tests/test_lora_gpu.py -- ``2e-3 * mean|y| + 4 ulp`` for fp16, ``1.6e-2 * mean|y| + 4 ulp``
for bf16, per element.  The share of elements bit-equal to the correctly rounded fp64 value is printed, not asserted (DESIGN.md
4.8h records it).  The module tests set ``lora.SGMV_MIN_ROWS`` / ``lora.SGMV_MAX_ROWS`` themselves: the shipped value is a measured
cross-over (profiles/lora_sgmv.json), not part of what is checked here.

The entry writes ``y`` in 8-byte groups and declines rows that are not 8-byte aligned, so ``_run`` hands it ``y`` with a row stride
rounded up to a multiple of 4 elements (``_rows4``): at out_features 298 that is a [rows, 298] view of a [rows, 300] buffer.  The
values, the shapes and every check are those of a contiguous ``y``."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
RANKS = (8, 24, 128)
SCALINGS = (2.0, 0.5, 1.25)
# (in_features, out_features): two k-steps and one output tile; a last k-step of a single 8-element piece and an output tail of
# 12; an out_features that is no multiple of 4
SHAPES = [(64, 16), (520, 300), (1032, 298)]
DTYPES = [torch.float16, torch.bfloat16]


def _ulp(y, dtype):
    mant = 10 if dtype == torch.float16 else 7
    return 2.0 ** (np.floor(np.log2(np.maximum(np.abs(y), 2.0 ** -14))) - mant)


def check_bound(y, y64, dtype, what):
    y, y64 = y.double().cpu().numpy(), y64.double().cpu().numpy()
    assert np.isfinite(y).all(), f"{what}: non-finite output"
    el_tol = 2e-3 if dtype == torch.float16 else 1.6e-2
    err = np.abs(y - y64)
    bound = el_tol * np.mean(np.abs(y64)) + 4 * _ulp(y64, dtype)
    exact = float(np.mean(y == torch.from_numpy(y64).to(dtype).double().numpy()))
    print(f"{what}: worst error / bound {float((err / bound).max()):.3f}, bit-equal to the rounded fp64 value: {exact:.4f}")
    assert not (err > bound).any(), f"{what}: {(err > bound).sum()} elements outside the bound, worst {err.max():.4g}"
    return exact


def _adapters(seed, fin, fout, dtype, ranks=RANKS, scalings=SCALINGS):
    gen = torch.Generator().manual_seed(seed)
    out = []
    for i, rank in enumerate(ranks):
        a = (torch.randn((rank, fin), generator=gen) / fin ** 0.5).to(dtype).to(DEV)
        b = (torch.randn((fout, rank), generator=gen) / rank ** 0.5).to(dtype).to(DEV)
        out.append((a, b, scalings[i % len(scalings)]))
    return out


def _inputs(seed, rows, fin, fout, dtype):
    gen = torch.Generator().manual_seed(seed)
    return torch.randn((rows, fin), generator=gen).to(dtype).to(DEV), torch.randn((rows, fout), generator=gen).to(dtype).to(DEV)


def _rows4(t):
    """A copy of ``t`` [rows, out] whose row stride is a multiple of 4 elements (``clone()`` of such a view would pack the rows)."""
    buf = torch.empty((t.shape[0], (t.shape[1] + 3) // 4 * 4), dtype=t.dtype, device=t.device)
    y = buf[:, :t.shape[1]]
    y.copy_(t)
    return y


def _mixed_ids(rows, n=3):
    """Every adapter, -1 and n, mixed over the rows."""
    return [(-1, 0, n, 1, 2)[b % 5] for b in range(rows)]


def _ref64(y_in, x, ads, ids):
    y = y_in.double().cpu().clone()
    for b, a in enumerate(ids):
        if 0 <= a < len(ads):
            A, B, s = ads[a]
            y[b] += float(np.float32(s)) * (B.double().cpu() @ (A.double().cpu() @ x[b].double().cpu()))
    return y


def _run(y_in, x, ads, ids, ids_dtype=torch.int64, table=None, max_rank=None):
    from aqlm_amd.inference_kernels import hip_kernel as hk

    table = hk.lora_table(ads, torch.device(DEV)) if table is None else table
    y = _rows4(y_in)
    idt = None if ids is None else torch.tensor(ids, dtype=ids_dtype, device=DEV)
    max_rank = max(a.shape[0] for a, _, _ in ads) if max_rank is None else max_rank
    torch.ops.aqlm.lora_sgmv_(y, x, idt, table, [len(ads), max_rank, y.shape[1], x.shape[1]])
    return y


@pytest.fixture(scope="module")
def mixed150():
    """The 150-row mixed-id case on (520, 300), computed once per dtype and left unchanged: (adapters, x, y_in, ids, y)."""
    cache = {}

    def get(dtype):
        if dtype not in cache:
            fin, fout, rows = 520, 300, 150
            ads = _adapters(7, fin, fout, dtype)
            x, y_in = _inputs(8, rows, fin, fout, dtype)
            ids = _mixed_ids(rows)
            cache[dtype] = (ads, x, y_in, ids, _run(y_in, x, ads, ids))
        return cache[dtype]

    return get


@pytest.mark.parametrize("ids_dtype", [torch.int64, torch.int32], ids=["i64", "i32"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
@pytest.mark.parametrize("fin,fout", SHAPES)
def test_mixed_ranks_at_any_row_count_match_fp64_and_hostile_ids_leave_their_rows(fin, fout, dtype, ids_dtype):
    ads = _adapters(1, fin, fout, dtype)
    for rows in (1, 15, 16, 17, 70, 150):
        x, y_in = _inputs(10 + rows, rows, fin, fout, dtype)
        ids = _mixed_ids(rows)
        y = _run(y_in, x, ads, ids, ids_dtype)
        check_bound(y, _ref64(y_in, x, ads, ids), dtype, f"in {fin} out {fout} {dtype} rows {rows}")
        for b, a in enumerate(ids):
            if not 0 <= a < len(ads):
                assert torch.equal(y[b], y_in[b]), f"row {b} with id {a} was written"
            else:
                assert not torch.equal(y[b], y_in[b]), f"row {b} with id {a} was not changed"


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
@pytest.mark.parametrize("fin,fout", SHAPES)
def test_prefill_shaped_ids_with_seams_inside_tiles(fin, fout, dtype):
    ads = _adapters(2, fin, fout, dtype)
    x, y_in = _inputs(3, 150, fin, fout, dtype)
    ids = [b // 50 for b in range(150)]  # seams at rows 50 and 100: inside tiles 3 and 6
    check_bound(_run(y_in, x, ads, ids), _ref64(y_in, x, ads, ids), dtype, f"segments in {fin} out {fout} {dtype}")


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
@pytest.mark.parametrize("fin,fout", SHAPES)
def test_one_tile_with_sixteen_different_adapters(fin, fout, dtype):
    ads = _adapters(4, fin, fout, dtype, ranks=(8,) * 17)
    x, y_in = _inputs(5, 16, fin, fout, dtype)
    ids = list(range(16, 0, -1))
    y = _run(y_in, x, ads, ids)
    check_bound(y, _ref64(y_in, x, ads, ids), dtype, f"16 adapters in one tile, in {fin} out {fout} {dtype}")
    assert all(not torch.equal(y[b], y_in[b]) for b in range(16))


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
def test_null_ids_mean_adapter_zero_for_every_row(dtype):
    fin, fout, rows = 520, 300, 70
    ads = _adapters(2, fin, fout, dtype)
    x, y_in = _inputs(4, rows, fin, fout, dtype)
    y = _run(y_in, x, ads, None)
    check_bound(y, _ref64(y_in, x, ads, [0] * rows), dtype, f"null ids {dtype}")
    assert torch.equal(y, _run(y_in, x, ads, [0] * rows))


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
def test_strided_rows_and_the_columns_past_out_features_stay_untouched(dtype):
    fin, fout, rows = 1032, 298, 70
    ads = _adapters(5, fin, fout, dtype)
    x, y_in = _inputs(6, rows, fin, fout, dtype)
    xw = torch.full((rows, fin + 24), float("nan"), dtype=dtype, device=DEV)  # rows stay 16-byte aligned: 1056 elements
    xw[:, :fin] = x
    yw = torch.full((rows, fout + 6), 7.0, dtype=dtype, device=DEV)           # row stride 304: a multiple of 4
    yw[:, :fout] = y_in
    ids = _mixed_ids(rows)
    from aqlm_amd.inference_kernels import hip_kernel as hk

    torch.ops.aqlm.lora_sgmv_(yw[:, :fout], xw[:, :fin], torch.tensor(ids, device=DEV), hk.lora_table(ads, torch.device(DEV)),
                              [len(ads), 128, fout, fin])
    assert torch.equal(yw[:, :fout], _run(y_in, x, ads, ids)), "strided rows change the result"
    assert bool((yw[:, fout:] == 7.0).all()), "columns past out_features were written"


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
def test_a_rows_bits_depend_on_that_row_alone(dtype, mixed150):
    ads, x, y_in, ids, y = mixed150(dtype)
    rows = len(ids)
    assert torch.equal(y, _run(y_in, x, ads, ids)), "two runs differ"
    perm = torch.randperm(rows, generator=torch.Generator().manual_seed(9)).tolist()
    yp = _run(y_in[perm], x[perm], ads, [ids[p] for p in perm])
    assert torch.equal(yp, y[perm]), "permuting the rows does not permute the outputs"
    for subset in (list(range(0, rows, 2)), [3, 41, 149, 8, 13, 96, 27], [33]):
        ys = _run(y_in[subset], x[subset], ads, [ids[p] for p in subset])
        assert torch.equal(ys, y[subset]), f"a subset of {len(subset)} rows differs from the full call"
    # a NaN in one x row poisons that row only
    victim = next(b for b, a in enumerate(ids) if a == 1)
    xn = x.clone()
    xn[victim, 17] = float("nan")
    yn = _run(y_in, xn, ads, ids)
    assert bool(torch.isnan(yn[victim]).all())
    keep = [b for b in range(rows) if b != victim]
    assert torch.equal(yn[keep], y[keep])
    # B = 0: y comes back as it went in
    zero = [(a, torch.zeros_like(b), s) for a, b, s in ads]
    assert torch.equal(_run(y_in, x, zero, ids), y_in)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
def test_entries_that_do_not_belong_leave_their_rows(dtype):
    """Argument hygiene: an entry of rank 12, and one of rank 136 in a launch with max_rank 128, count as 'no adapter'."""
    fin, fout, rows = 520, 300, 70
    ads = _adapters(11, fin, fout, dtype, ranks=(8, 12, 128, 136), scalings=(2.0, 0.5, 1.25, 1.0))
    x, y_in = _inputs(12, rows, fin, fout, dtype)
    ids = [b % 4 for b in range(rows)]
    y = _run(y_in, x, ads, ids, max_rank=128)
    good = [b for b in range(rows) if ids[b] in (0, 2)]
    bad = [b for b in range(rows) if ids[b] in (1, 3)]
    assert torch.equal(y[bad], y_in[bad]), "a row whose entry does not belong to the launch was written"
    ref = _ref64(y_in, x, ads, [a if a in (0, 2) else -1 for a in ids])
    check_bound(y[good], ref[good], dtype, f"entries that do not belong {dtype}")
    assert all(not torch.equal(y[b], y_in[b]) for b in good)


# ---------------------------------------------------------------------------------------------------------------------------
# module level: a prepacked 1x16 g8 layer
# ---------------------------------------------------------------------------------------------------------------------------
def _quantized(seed, fin, fout, dtype=torch.float16):
    from aqlm import QuantizedLinear
    from oracle import aqlm_oracle as orc

    L = orc.make_layer(seed, fin, fout, 1, 16, 8, batch=1, bias=True)
    m = QuantizedLinear(fin, fout, 8, 1, 1, 16, bias=True, device=DEV, dtype=dtype)
    f = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dtype).to(DEV)  # noqa: E731
    with torch.no_grad():
        m.codes.copy_(torch.from_numpy(L["codes"]).to(DEV))
        m.codebooks.copy_(f(L["codebooks"]))
        m.scales.copy_(f(L["scales"]).reshape(m.scales.shape))
        m.bias.copy_(f(L["bias"]))
    return m


class _Block(torch.nn.Module):
    def __init__(self, mods):
        super().__init__()
        for n, m in mods.items():
            setattr(self, n, m)


def _peft_pair(seed, shapes, r, alpha, dtype=torch.float16):
    """(state_dict, config) in PEFT's format for ``shapes`` = {module path: (in, out)}."""
    gen = torch.Generator().manual_seed(seed)
    state = {}
    for path, (fin, fout) in shapes.items():
        state[f"base_model.model.{path}.lora_A.weight"] = (torch.randn((r, fin), generator=gen) / fin ** 0.5).to(dtype)
        state[f"base_model.model.{path}.lora_B.weight"] = (torch.randn((fout, r), generator=gen) / r ** 0.5).to(dtype)
    return state, {"peft_type": "LORA", "r": r, "lora_alpha": alpha, "bias": "none", "target_modules": sorted(shapes)}


@pytest.fixture()
def sgmv_on(monkeypatch):
    import aqlm_amd.inference as inf
    import aqlm_amd.lora as lora

    monkeypatch.setattr(inf, "PREPACK_MIN_CODES", 10_000)
    monkeypatch.setattr(lora, "BGMV_MAX_ROWS", 64)
    monkeypatch.setattr(lora, "SGMV_MIN_ROWS", 65)
    monkeypatch.setattr(lora, "SGMV_MAX_ROWS", 4096)
    return lora


def test_module_sgmv_route_against_torch_path_and_select_none(sgmv_on, monkeypatch):
    lora = sgmv_on
    fin, fout = 1024, 256
    base = _quantized(21, fin, fout)
    block = _Block({"proj": base})
    bank = lora.attach_adapters(block, {"a": _peft_pair(1, {"proj": (fin, fout)}, 16, 32), "b": _peft_pair(2, {"proj": (fin, fout)}, 8, 4)})
    from aqlm_amd.inference_kernels import hip_kernel as hk

    sgmv, bgmv = [], []
    real_s, real_b = hk.lora_sgmv_, hk.lora_bgmv_
    monkeypatch.setattr(hk, "lora_sgmv_", lambda *a: (sgmv.append(a[0].shape[0]), real_s(*a))[1])
    monkeypatch.setattr(hk, "lora_bgmv_", lambda *a: (bgmv.append(a[0].shape[0]), real_b(*a))[1])
    gen = torch.Generator().manual_seed(3)
    x3 = torch.randn((2, 40, fin), generator=gen).half().to(DEV)
    x2 = torch.randn((80, fin), generator=gen).half().to(DEV)
    seq_ids = torch.tensor([1, 0], device=DEV)
    row_ids = torch.tensor([(1, 0, 2, 1, 0)[b % 5] for b in range(80)], device=DEV)  # 2 lies outside the bank
    with torch.no_grad():
        for x, ids in ((x3, seq_ids), (x2, row_ids)):
            bare = base(x)
            assert base._packed_codes is not None, "the layer did not take the prepacked route"
            for which in ("a", ids):
                bank.select(which)
                n = len(sgmv)
                y = block.proj(x)
                assert len(sgmv) == n + 1 and sgmv[-1] == 80 and not bgmv, "the SGMV route was not taken"
                monkeypatch.setattr(lora, "SGMV_MAX_ROWS", 0)
                ref = block.proj(x)
                monkeypatch.setattr(lora, "SGMV_MAX_ROWS", 4096)
                assert len(sgmv) == n + 1, "SGMV_MAX_ROWS = 0 did not switch the route off"
                assert y.shape == ref.shape == bare.shape and not torch.equal(ref, bare)
                check_bound(y, ref, torch.float16, f"module {tuple(x.shape)} select {which if isinstance(which, str) else 'ids'}")
            n = len(sgmv)
            bank.select(None)
            assert torch.equal(block.proj(x), bare) and len(sgmv) == n and not bgmv, "select(None) is not the bare layer"
        # the out-of-bank id leaves its rows to the base layer
        bank.select(row_ids)
        y = block.proj(x2)
        bare = base(x2)
        out = (row_ids == 2).cpu()
        assert torch.equal(y[out], bare[out]) and not torch.equal(y[~out], bare[~out])
        # per-sequence ids of a [B, S, K] input are broadcast over S on the device: the same rows with one id per row, bit for bit
        bank.select(seq_ids)
        y_seq = block.proj(x3)
        bank.select(torch.tensor([1] * 40 + [0] * 40, device=DEV))
        y_row = block.proj(x3.view(80, fin))
        assert y_seq.shape == (2, 40, fout) and torch.equal(y_seq.view(80, fout), y_row)
        # a 4-row call still goes to the BGMV launches
        n = len(sgmv)
        bank.select(torch.tensor([1, 0, 1, 0], device=DEV))
        block.proj(x2[:4])
        assert bgmv == [4] and len(sgmv) == n
    # a gradient is needed: the torch path
    bank.select(row_ids)
    block.proj.lora_A["a"].weight.requires_grad_(True)
    n = len(sgmv)
    y = block.proj(x2)
    assert len(sgmv) == n and y.requires_grad
    block.proj.lora_A["a"].weight.requires_grad_(False)
    lora.detach_adapters(block)
    assert block.proj is base


def test_captured_prefill_follows_ids_rewritten_in_place(sgmv_on):
    lora = sgmv_on
    fin, fout, rows = 1024, 256, 80
    base = _quantized(41, fin, fout)
    block = _Block({"proj": base})
    bank = lora.attach_adapters(block, {"a": _peft_pair(5, {"proj": (fin, fout)}, 16, 32), "b": _peft_pair(6, {"proj": (fin, fout)}, 24, 24)})
    x = torch.randn((rows, fin), generator=torch.Generator().manual_seed(6)).half().to(DEV)
    ids = torch.full((rows,), -1, dtype=torch.int64, device=DEV)
    bank.select(ids)
    with torch.no_grad():
        eager = {}
        for value in (-1, 0, 1):
            ids.fill_(value)
            eager[value] = block.proj(x).clone()
        assert torch.equal(eager[-1], base(x)) and not torch.equal(eager[0], eager[1]) and not torch.equal(eager[0], eager[-1])
        ids.fill_(-1)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(2):
                block.proj(x)
        torch.cuda.current_stream().wait_stream(s)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = block.proj(x)
        for value in (-1, 0, 1):  # base -> adapter 0 -> adapter 1
            ids.fill_(value)
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(out, eager[value]), f"replay with ids = {value}"
    lora.detach_adapters(block)
