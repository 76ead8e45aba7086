"""LoRA adapters per row of a decode batch, on the MI355X: the raw op ``torch.ops.aqlm.lora_bgmv_`` (aqlm_hip_lora_bgmv) against an
fp64 evaluation of its definition with ``y`` pre-filled, its bit-exact properties (a row's bits depend on its own x row, its own
y row and its adapter only), and ``aqlm.lora`` on a prepacked 1x16 g8 layer: BGMV route against torch path, ``select(None)``,
shared-input groups underneath the wrappers, hipGraph replay with the ids rewritten in place.

Bound: the project's per-element parity bound -- ``2e-3 * mean|y| + 4 ulp`` for fp16, ``1.6e-2 * mean|y| +
4 ulp`` for bf16 -- against the fp64 value of ``y_in + scaling * B (A x)``.  The share of elements bit-equal to the correctly
rounded fp64 value is printed, not asserted (DESIGN.md 4.8g records it).  The module tests set ``lora.BGMV_MAX_ROWS`` themselves:
the shipped value is a measured cross-over (profiles/lora_bgmv.json), not part of what is checked here."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
RANKS = (8, 24, 128)
SCALINGS = (2.0, 0.5, 1.25)
SHAPES = [(64, 16), (520, 300)]  # (in_features, out_features): 520 = one full 512-element wave step + an 8-element tail
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


def _adapters(seed, fin, fout, dtype, ranks=RANKS):
    gen = torch.Generator().manual_seed(seed)
    out = []
    for rank, scaling in zip(ranks, SCALINGS):
        a = (torch.randn((rank, fin), generator=gen) / fin ** 0.5).to(dtype).to(DEV)
        b = (torch.randn((fout, rank), generator=gen) / rank ** 0.5).to(dtype).to(DEV)
        out.append((a, b, scaling))
    return out


def _inputs(seed, rows, fin, fout, dtype):
    gen = torch.Generator().manual_seed(seed)
    return torch.randn((rows, fin), generator=gen).to(dtype).to(DEV), torch.randn((rows, fout), generator=gen).to(dtype).to(DEV)


def _mixed_ids(rows, n):
    """Every adapter, -1 and n, mixed over the rows; a single row takes the last (widest) adapter."""
    if rows == 1:
        return [n - 1]
    return [(-1, 0, n, 1, 2)[b % 5] if n == 3 else b % n for b in range(rows)]


def _ref64(y_in, x, ads, ids):
    y = y_in.double().cpu().clone()
    for b, a in enumerate(ids):
        if 0 <= a < len(ads):
            A, B, s = ads[a]
            y[b] += float(np.float32(s)) * (B.double().cpu() @ (A.double().cpu() @ x[b].double().cpu()))
    return y


def _run(y_in, x, ads, ids, ids_dtype=torch.int64, table=None):
    from aqlm_amd.inference_kernels import hip_kernel as hk

    table = hk.lora_table(ads, torch.device(DEV)) if table is None else table
    y = y_in.clone()
    idt = None if ids is None else torch.tensor(ids, dtype=ids_dtype, device=DEV)
    torch.ops.aqlm.lora_bgmv_(y, x, idt, table, [len(ads), max(a.shape[0] for a, _, _ in ads), y.shape[1], x.shape[1]])
    return y


@pytest.mark.parametrize("ids_dtype", [torch.int64, torch.int32], ids=["i64", "i32"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
@pytest.mark.parametrize("fin,fout", SHAPES)
def test_mixed_ranks_in_one_launch_match_fp64_and_hostile_ids_leave_their_rows(fin, fout, dtype, ids_dtype):
    ads = _adapters(1, fin, fout, dtype)
    for rows in (1, 5, 70):
        x, y_in = _inputs(10 + rows, rows, fin, fout, dtype)
        ids = _mixed_ids(rows, len(ads))
        y = _run(y_in, x, ads, ids, ids_dtype)
        check_bound(y, _ref64(y_in, x, ads, ids), dtype, f"in {fin} out {fout} {dtype} rows {rows}")
        for b, a in enumerate(ids):
            if not 0 <= a < len(ads):
                assert torch.equal(y[b], y_in[b]), f"row {b} with id {a} was written"
            else:
                assert not torch.equal(y[b], y_in[b])
    if fin == 520:
        # every single adapter alone at one row: ranks 8 and 24 leave rank groups of the grid (sized by 128) without work
        x, y_in = _inputs(3, 1, fin, fout, dtype)
        for a in range(len(ads)):
            check_bound(_run(y_in, x, ads, [a], ids_dtype), _ref64(y_in, x, ads, [a]), dtype, f"one row, adapter {a}")


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
def test_null_ids_mean_adapter_zero_for_every_row(dtype):
    fin, fout = 520, 300
    ads = _adapters(2, fin, fout, dtype)
    x, y_in = _inputs(4, 5, fin, fout, dtype)
    y = _run(y_in, x, ads, None)
    check_bound(y, _ref64(y_in, x, ads, [0] * 5), dtype, f"null ids {dtype}")
    assert torch.equal(y, _run(y_in, x, ads, [0] * 5))


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
def test_strided_rows_and_the_columns_past_out_features_stay_untouched(dtype):
    fin, fout, rows = 520, 300, 5
    ads = _adapters(5, fin, fout, dtype)
    x, y_in = _inputs(6, rows, fin, fout, dtype)
    xw = torch.full((rows, fin + 24), float("nan"), dtype=dtype, device=DEV)  # rows stay 16-byte aligned: 544 elements
    xw[:, :fin] = x
    yw = torch.full((rows, fout + 5), 7.0, dtype=dtype, device=DEV)
    yw[:, :fout] = y_in
    ids = _mixed_ids(rows, len(ads))
    from aqlm_amd.inference_kernels import hip_kernel as hk

    torch.ops.aqlm.lora_bgmv_(yw[:, :fout], xw[:, :fin], torch.tensor(ids, device=DEV), hk.lora_table(ads, torch.device(DEV)),
                              [len(ads), 128, fout, fin])
    assert torch.equal(yw[:, :fout], _run(y_in, x, ads, ids)), "strided rows change the result"
    assert bool((yw[:, fout:] == 7.0).all()), "columns past out_features were written"


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
def test_a_rows_bits_depend_on_that_row_alone(dtype):
    fin, fout, rows = 520, 300, 70
    ads = _adapters(7, fin, fout, dtype)
    x, y_in = _inputs(8, rows, fin, fout, dtype)
    ids = _mixed_ids(rows, len(ads))
    y = _run(y_in, x, ads, ids)
    assert torch.equal(y, _run(y_in, x, ads, ids)), "two runs differ"
    perm = torch.randperm(rows, generator=torch.Generator().manual_seed(9)).tolist()
    yp = _run(y_in[perm], x[perm], ads, [ids[p] for p in perm])
    assert torch.equal(yp, y[perm]), "permuting the rows does not permute the outputs"
    for subset in (list(range(0, 70, 2)), [3, 41, 69, 8, 13, 26, 27], [33]):
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
def small_prepack(monkeypatch):
    import aqlm_amd.inference as inf
    import aqlm_amd.lora as lora

    monkeypatch.setattr(inf, "PREPACK_MIN_CODES", 10_000)
    monkeypatch.setattr(lora, "BGMV_MAX_ROWS", 64)
    return lora


def test_module_bgmv_route_against_torch_path_and_select_none(small_prepack, monkeypatch):
    lora = small_prepack
    fin, fout = 1024, 256
    base = _quantized(21, fin, fout)
    block = _Block({"proj": base})
    bank = lora.attach_adapters(block, {"a": _peft_pair(1, {"proj": (fin, fout)}, 16, 32), "b": _peft_pair(2, {"proj": (fin, fout)}, 8, 4)})
    assert isinstance(block.proj, lora.LoraQuantizedLinear) and block.proj.base_layer is base
    calls = []
    from aqlm_amd.inference_kernels import hip_kernel as hk

    real = hk.lora_bgmv_
    monkeypatch.setattr(hk, "lora_bgmv_", lambda *a: (calls.append(a[0].shape[0]), real(*a))[1])
    with torch.no_grad():
        for rows in (1, 4):
            x = torch.randn((rows, fin), generator=torch.Generator().manual_seed(rows)).half().to(DEV)
            bare = base(x)
            assert base._packed_codes is not None, "the layer did not take the prepacked route"
            ids = torch.tensor([1, 0, 2, 1][:rows], device=DEV)
            for which in ("a", "b", ids):
                bank.select(which)
                n = len(calls)
                y = block.proj(x)
                assert len(calls) == n + 1, "the BGMV route was not taken"
                monkeypatch.setattr(lora, "BGMV_MAX_ROWS", 0)
                ref = block.proj(x)
                monkeypatch.setattr(lora, "BGMV_MAX_ROWS", 64)
                assert len(calls) == n + 1, "BGMV_MAX_ROWS = 0 did not switch the route off"
                assert not torch.equal(ref, bare)
                check_bound(y, ref, torch.float16, f"module rows {rows} select {which if isinstance(which, str) else 'ids'}")
            n = len(calls)
            bank.select(None)
            assert torch.equal(block.proj(x), bare) and len(calls) == n, "select(None) is not the bare layer"
        # per-sequence ids of a [B, S, K] input are broadcast over S on the device: the same rows with one id per row, bit for bit
        bank.select(torch.tensor([1, 1, 0, 0], device=DEV))
        y4 = block.proj(x)
        bank.select(torch.tensor([1, 0], device=DEV))
        n = len(calls)
        y3 = block.proj(x.view(2, 2, fin))
        assert len(calls) == n + 1 and y3.shape == (2, 2, fout) and torch.equal(y3.view(4, fout), y4)
        assert not torch.equal(y4[0], bare[0]) and not torch.equal(y4[2], bare[2])
    lora.detach_adapters(block)
    assert block.proj is base


def test_shared_input_groups_keep_one_base_launch_under_the_wrappers(small_prepack):
    import aqlm

    lora = small_prepack
    fin = 1024
    shapes = {"q_proj": (fin, 256), "k_proj": (fin, 128), "v_proj": (fin, 128)}
    mods = {n: _quantized(30 + i, fi, fo) for i, (n, (fi, fo)) in enumerate(shapes.items())}
    block = _Block(mods)
    x = torch.randn((2, fin), generator=torch.Generator().manual_seed(5)).half().to(DEV)
    with torch.no_grad():
        bare = {n: m(x) for n, m in mods.items()}
        (group,) = aqlm.fuse_shared_input_linears(block)
        bank = lora.attach_adapters(block, {"a": _peft_pair(3, shapes, 16, 16), "b": _peft_pair(4, shapes, 8, 16)})
        bank.select(torch.tensor([1, 0], device=DEV))
        before = group.launches
        out = {n: getattr(block, n)(x) for n in shapes}  # the same tensor object, one call after the other
        assert group.launches == before + 1 and group.served >= 2, "q / k / v no longer share one base launch"
        for n, (fi, fo) in shapes.items():
            w = getattr(block, n)
            ref = bare[n].double()
            for b, name in enumerate(("b", "a")):
                A, B, s = w._weights(name)
                ref[b] += s * (B.double() @ (A.double() @ x[b].double()))
            check_bound(out[n], ref, torch.float16, f"fused {n}")
            assert not torch.equal(out[n], bare[n])
    lora.detach_adapters(block)
    aqlm.unfuse_shared_input_linears(block)


def test_captured_step_follows_ids_rewritten_in_place_and_a_stale_table_raises(small_prepack):
    lora = small_prepack
    fin, fout = 1024, 256
    base = _quantized(41, fin, fout)
    block = _Block({"proj": base})
    bank = lora.attach_adapters(block, {"a": _peft_pair(5, {"proj": (fin, fout)}, 16, 32), "b": _peft_pair(6, {"proj": (fin, fout)}, 24, 24)})
    x = torch.randn((2, fin), generator=torch.Generator().manual_seed(6)).half().to(DEV)
    ids = torch.full((2,), -1, dtype=torch.int64, device=DEV)
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
        # an adapter written in place: its table is stale, and a capture cannot rebuild it
        block.proj.lora_A["a"].weight.mul_(1.0)
        stale = torch.cuda.CUDAGraph()
        with torch.cuda.graph(stale):
            with pytest.raises(RuntimeError, match="before capturing"):
                block.proj(x)
        block.proj(x)  # an eager call rebuilds it
        torch.cuda.synchronize()
    lora.detach_adapters(block)
