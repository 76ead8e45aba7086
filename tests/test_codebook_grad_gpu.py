"""Training codebooks and scales of 1x16 layers on the MI355X: aqlm_hip_codebook_grad_1x16 / aqlm_hip_scales_grad_1x16 and the
autograd route built on them.

The kernels accumulate in fp32, so integer-valued data makes every partial sum exact and the answer independent of the order: the
tests compare BITS against an fp64 numpy model rounded once -- a dropped, duplicated or misplaced term cannot hide behind a
tolerance.  Real-valued data (test 3) is a secondary check of the conversion paths, within the derived bound
``(n + 2) * 2^-24 * sum|terms| + u_out * |exact|`` (n terms per output, u_out the unit roundoff of the output dtype; plus half a
subnormal spacing of the output dtype for outputs that round below its normal range)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
ENTRIES = 65536
SHAPES = [(24, 64, 8), (40, 192, 16), (264, 520, 8)]  # (out, in, g); the last: 17160 codes, more than one workgroup of chunks
UNIT = {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8, torch.float32: 2.0 ** -24}
# half the spacing of the subnormals: the rounding error of an output below the normal range (fp16: |y| < 6.1e-5), which the
# relative term u_out * |exact| does not cover
TINY = {torch.float16: 2.0 ** -25, torch.bfloat16: 2.0 ** -134, torch.float32: 2.0 ** -150}


def _within(got, exact, bound, what):
    """|got - exact| <= bound everywhere; the message names the worst element."""
    excess = np.abs(got - exact) - bound
    i = np.unravel_index(np.argmax(excess), excess.shape)
    assert excess[i] <= 0, f"{what}: element {i}: got {got[i]!r}, exact {exact[i]!r}, bound {bound[i]!r}"


@pytest.fixture(scope="module")
def hk():
    from aqlm_amd.inference_kernels import hip_kernel

    return hip_kernel


def _codes(kind, out, nj, seed):
    rng = np.random.default_rng(seed)
    n = out * nj
    if kind == "uniform":
        v = rng.integers(0, ENTRIES, size=n)
        v[[0, 1, n // 2, n - 1]] = (32768, 65535, 0, 32767)  # the containers -32768, -1, 0, 32767
    elif kind == "equal":
        v = np.full(n, 40000)
    else:  # Zipf 1.2 over a shuffled alphabet: a few entries hold most positions
        v = rng.permutation(ENTRIES)[np.minimum(rng.zipf(1.2, size=n), ENTRIES) - 1]
    return v.astype(np.uint16).view(np.int16).reshape(out, nj, 1)


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _same_bits(got, want64, dtype):
    """``got`` equals the fp64 model rounded once to ``dtype``, bit for bit (signed zeros and NaN included)."""
    want = torch.from_numpy(np.ascontiguousarray(want64)).to(dtype)
    return torch.equal(_bits(got.cpu()), _bits(want))


@pytest.fixture(scope="module")
def raw_cases(hk):
    """Per (shape, kind): the codes, the index (built once, on the GPU) and the unsigned values."""
    cases = {}
    for si, (out, fin, g) in enumerate(SHAPES):
        for ki, kind in enumerate(("uniform", "equal", "zipf")):
            codes = _codes(kind, out, fin // g, 100 + 10 * si + ki)
            t = torch.from_numpy(codes).to(DEV)
            cases[(out, fin, g, kind)] = (codes, t, hk.build_codebook_grad_index(t, g), codes.reshape(out, -1).view(np.uint16).astype(np.int64))
    return cases


def _dw(out, fin, dtype, seed, padded, real=False):
    gen = torch.Generator().manual_seed(seed)
    dw = torch.randn((out, fin), generator=gen) if real else torch.randint(-8, 9, (out, fin), generator=gen).float()
    dw = dw.to(dtype)
    if not padded:
        return dw.to(DEV), dw.double().numpy()
    buf = torch.full((out, fin + 8), float("nan"), dtype=dtype, device=DEV)  # a row stride of in + 8 elements
    buf[:, :fin] = dw.to(DEV)
    return buf[:, :fin], dw.double().numpy()


def _model_dc(values, dw64, s64, g):
    out, nj = values.shape
    dc = np.zeros((ENTRIES, g))
    terms = dw64.reshape(out, nj, g) * s64.reshape(out, 1, 1)
    np.add.at(dc, values.reshape(-1), terms.reshape(-1, g))
    return dc, terms


# ---------------------------------------------------------------------------------------------------------------------------
# 1. raw dC, exact
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["uniform", "equal", "zipf"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_codebook_grad_is_exact_on_integer_data(hk, raw_cases, shape, kind):
    out, fin, g = shape
    codes, _, index, values = raw_cases[(out, fin, g, kind)]
    used = np.zeros(ENTRIES, dtype=bool)
    used[values.reshape(-1)] = True
    if kind == "equal" and shape == SHAPES[-1]:
        assert out * (fin // g) == 17160 > 60 * hk.CODEBOOK_GRAD_CHUNK  # one list across every chunk boundary
    gen = torch.Generator().manual_seed(7)
    for di, dw_dtype in enumerate((torch.float16, torch.bfloat16, torch.float32)):
        storage = torch.float16 if dw_dtype == torch.float32 else dw_dtype
        scales = torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (out,), generator=gen)].to(storage)
        for padded in (False, True):
            dw, dw64 = _dw(out, fin, dw_dtype, 20 + di, padded)
            for s in (scales, None):
                s64 = np.ones(out) if s is None else s.double().numpy()
                want, _ = _model_dc(values, dw64, s64, g)
                assert np.abs(want).max() * 2 < 2 ** 24  # every magnitude below 2^24 half-units: fp32 sums are exact
                for out_dtype in (torch.float32, storage):
                    got = hk.codebook_grad_1x16(dw, None if s is None else s.to(DEV), index, out_dtype=out_dtype)
                    assert got.shape == (ENTRIES, g) and got.dtype == out_dtype
                    assert not torch.isnan(got).any()
                    assert _same_bits(got, want, out_dtype), (dw_dtype, padded, s is None, out_dtype)
                    assert (_bits(got.cpu())[torch.from_numpy(~used)] == 0).all(), "unused entries are +0"


def test_codebook_grad_writes_every_output_whatever_out_and_workspace_held(hk, raw_cases):
    """The op allocates its output; here the raw entry gets an output and a workspace full of NaN."""
    from aqlm_amd import _native as nat

    out, fin, g = SHAPES[-1]
    for kind in ("equal", "zipf"):
        _, _, index, values = raw_cases[(out, fin, g, kind)]
        dw, dw64 = _dw(out, fin, torch.float16, 31, False)
        want, _ = _model_dc(values, dw64, np.ones(out), g)
        y = torch.full((ENTRIES, g), float("nan"), dtype=torch.float32, device=DEV)
        ws_bytes = nat.lib.aqlm_hip_codebook_grad_1x16_workspace_bytes(out, fin, g)
        ws = torch.full((ws_bytes // 4,), float("nan"), dtype=torch.float32, device=DEV)
        rc = nat.lib.aqlm_hip_codebook_grad_1x16(dw.data_ptr(), dw.stride(0), nat.F16, None, nat.F16, index.starts.data_ptr(),
                                                 index.order.data_ptr(), index.chunks.data_ptr(), index.chunk_starts.data_ptr(), out, fin,
                                                 g, y.data_ptr(), nat.F32, ws.data_ptr(), ws_bytes,
                                                 torch.cuda.current_stream(DEV).cuda_stream)
        assert rc == 0, nat.last_error()
        assert not torch.isnan(y).any() and _same_bits(y, want, torch.float32)


def test_positions_outside_the_layer_are_skipped(hk, raw_cases):
    """An index with positions outside [0, n_codes) -- the buffers come from Python -- contributes nothing through them."""
    out, fin, g = SHAPES[0]
    _, _, index, values = raw_cases[(out, fin, g, "uniform")]
    n = out * (fin // g)
    bad = hk.CodebookGradIndex(index.order.clone(), index.starts, index.chunks, index.chunk_starts, out, fin, g)
    drop = [3, 50, 101]
    bad.order[drop] = torch.tensor([n, -1, 2 ** 31 - 1], dtype=torch.int32, device=DEV)
    dw, dw64 = _dw(out, fin, torch.float16, 33, False)
    terms = dw64.reshape(out, fin // g, g).reshape(-1, g).copy()
    terms[index.order.cpu().numpy()[drop]] = 0
    want = np.zeros((ENTRIES, g))
    np.add.at(want, values.reshape(-1), terms)
    assert _same_bits(hk.codebook_grad_1x16(dw, None, bad, out_dtype=torch.float32), want, torch.float32)


# ---------------------------------------------------------------------------------------------------------------------------
# 2. raw ds, exact
# ---------------------------------------------------------------------------------------------------------------------------
def _model_ds(values, dw64, cb64, g):
    out, nj = values.shape
    terms = dw64.reshape(out, nj, g) * cb64[values]
    return terms.sum((1, 2)), terms


@pytest.mark.parametrize("kind", ["uniform", "equal", "zipf"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_scales_grad_is_exact_on_integer_data(hk, raw_cases, shape, kind):
    out, fin, g = shape
    _, codes, _, values = raw_cases[(out, fin, g, kind)]
    gen = torch.Generator().manual_seed(9)
    for di, dw_dtype in enumerate((torch.float16, torch.bfloat16, torch.float32)):
        storage = torch.float16 if dw_dtype == torch.float32 else dw_dtype
        cb = torch.randint(-4, 5, (1, ENTRIES, 1, g), generator=gen).to(storage)
        for padded in (False, True):
            dw, dw64 = _dw(out, fin, dw_dtype, 40 + di, padded)
            want, _ = _model_ds(values, dw64, cb.double().numpy().reshape(ENTRIES, g), g)
            assert np.abs(want).max() < 2 ** 24
            for out_dtype in (torch.float32, storage):
                got = hk.scales_grad_1x16(dw, codes, cb.to(DEV), out_dtype=out_dtype)
                assert got.shape == (out,) and got.dtype == out_dtype
                assert _same_bits(got, want, out_dtype), (dw_dtype, padded, out_dtype)


# ---------------------------------------------------------------------------------------------------------------------------
# 3. real-valued data, within the derived bound
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("kind", ["uniform", "equal", "zipf"])
def test_real_valued_data_within_the_fp32_bound(hk, raw_cases, kind, dtype):
    for out, fin, g in SHAPES[1:]:
        _, codes, index, values = raw_cases[(out, fin, g, kind)]
        gen = torch.Generator().manual_seed(13)
        dw, dw64 = _dw(out, fin, dtype, 50, True, real=True)
        scales = (torch.rand((out,), generator=gen) + 0.5).to(dtype)
        cb = torch.randn((1, ENTRIES, 1, g), generator=gen).to(dtype)
        exact, terms = _model_dc(values, dw64, scales.double().numpy(), g)
        mag = np.zeros((ENTRIES, g))
        np.add.at(mag, values.reshape(-1), np.abs(terms).reshape(-1, g))
        n = np.bincount(values.reshape(-1), minlength=ENTRIES).reshape(-1, 1)  # the list length of every entry
        for out_dtype in (torch.float32, dtype):
            got = hk.codebook_grad_1x16(dw, scales.to(DEV), index, out_dtype=out_dtype).double().cpu().numpy()
            _within(got, exact, (n + 2) * 2.0 ** -24 * mag + UNIT[out_dtype] * np.abs(exact) + TINY[out_dtype], f"dC {out_dtype}")
        exact, terms = _model_ds(values, dw64, cb.double().numpy().reshape(ENTRIES, g), g)
        mag = np.abs(terms).sum((1, 2))
        for out_dtype in (torch.float32, dtype):
            got = hk.scales_grad_1x16(dw, codes, cb.to(DEV), out_dtype=out_dtype).double().cpu().numpy()
            _within(got, exact, (fin + 2) * 2.0 ** -24 * mag + UNIT[out_dtype] * np.abs(exact) + TINY[out_dtype], f"ds {out_dtype}")


# ---------------------------------------------------------------------------------------------------------------------------
# 4. reproducibility
# ---------------------------------------------------------------------------------------------------------------------------
def test_two_calls_give_the_same_bits_whatever_the_workspace_held(hk, raw_cases):
    from aqlm_amd import _native as nat

    out, fin, g = SHAPES[-1]
    for kind in ("equal", "zipf"):
        _, _, index, _ = raw_cases[(out, fin, g, kind)]
        dw, _ = _dw(out, fin, torch.bfloat16, 60, False, real=True)
        scales = (torch.rand((out,), generator=torch.Generator().manual_seed(1)) + 0.5).to(torch.bfloat16).to(DEV)
        ws = hk._workspace(DEV, nat.lib.aqlm_hip_codebook_grad_1x16_workspace_bytes(out, fin, g))
        ws.fill_(float("nan"))
        a = hk.codebook_grad_1x16(dw, scales, index, out_dtype=torch.float32)
        assert hk._workspace(DEV, 16) is ws  # the cached workspace the call used
        ws.fill_(-3.0e38)
        b = hk.codebook_grad_1x16(dw, scales, index, out_dtype=torch.float32)
        assert torch.equal(_bits(a), _bits(b)) and not torch.isnan(a).any()


# ---------------------------------------------------------------------------------------------------------------------------
# 5. the module end to end
# ---------------------------------------------------------------------------------------------------------------------------
MODULE_CASES = [(8, 1024, 64, torch.float16), (8, 520, 64, torch.bfloat16), (16, 2048, 128, torch.bfloat16), (16, 1040, 40, torch.float16)]


def _integer_layer(g, fin, fout, dtype, seed, device=DEV):
    """Codebook integers in [-4, 4], scales in {0.5, 1, 2}, an integer bias: with integer inputs every gradient is exact in fp32."""
    import aqlm

    gen = torch.Generator().manual_seed(seed)
    m = aqlm.QuantizedLinear(fin, fout, g, 1, 1, 16, bias=True, device=device, dtype=dtype)
    with torch.no_grad():
        m.codes.copy_(torch.randint(-32768, 32768, m.codes.shape, generator=gen).to(torch.int16))
        m.codebooks.copy_(torch.randint(-4, 5, m.codebooks.shape, generator=gen).to(dtype))
        m.scales.copy_(torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (fout,), generator=gen)].reshape(m.scales.shape).to(dtype))
        m.bias.copy_(torch.randint(-3, 4, (fout,), generator=gen).to(dtype))
    return m


def _integer_inputs(rows, fin, fout, dtype, seed):
    """x and the loss weights: integers in [-2, 2]; at most 60 rows carry a loss weight, so |dW| <= 240 is exact in bf16 too."""
    gen = torch.Generator().manual_seed(seed)
    x = torch.randint(-2, 3, (rows, fin), generator=gen).to(dtype)
    wy = torch.randint(-2, 3, (rows, fout), generator=gen).to(dtype)
    wy[60:] = 0
    return x, wy


def _fp64_grads(layer, x, wy):
    from aqlm_amd.utils import _dequantize_weight

    leaves = [t.detach().double().cpu().requires_grad_(True) for t in (x, layer.codebooks, layer.scales, layer.bias)]
    codes = layer.codes.detach().cpu().to(torch.int64) % 65536
    y = torch.nn.functional.linear(leaves[0], _dequantize_weight(codes, leaves[1], leaves[2]), leaves[3])
    (y * wy.double().cpu()).sum().backward()
    return [t.grad for t in leaves]


@pytest.fixture(scope="module")
def module_layers():
    """Per case: the trainable layer, a frozen twin (the same tensors' values) and nothing else; never modified by the tests."""
    import copy

    out = {}
    for i, (g, fin, fout, dtype) in enumerate(MODULE_CASES):
        frozen = _integer_layer(g, fin, fout, dtype, 200 + i)
        train = copy.deepcopy(frozen)
        for p in (train.codebooks, train.scales, train.bias):
            p.requires_grad_(True)
        out[(g, fin, fout, dtype)] = (train, frozen)
    return out


@pytest.mark.parametrize("input_grad", [True, False], ids=["x_grad", "x_frozen"])
@pytest.mark.parametrize("rows", [3, 9, 300])
@pytest.mark.parametrize("case", MODULE_CASES, ids=lambda c: f"g{c[0]}_{c[1]}x{c[2]}_{str(c[3])[6:]}")
def test_module_gradients_equal_fp64_autograd_bit_for_bit(module_layers, case, rows, input_grad):
    from aqlm_amd.inference import _TrainableMatmul1x16

    g, fin, fout, dtype = case
    train, frozen = module_layers[case]
    x, wy = _integer_inputs(rows, fin, fout, dtype, rows)
    xt = x.to(DEV).requires_grad_(input_grad)
    for p in train.parameters():
        p.grad = None
    y = train(xt)
    assert y.grad_fn is not None and type(y.grad_fn).__name__ == _TrainableMatmul1x16.__name__ + "Backward"
    (y * wy.to(DEV)).sum().backward()
    with torch.no_grad():
        assert torch.equal(_bits(y.detach()), _bits(frozen(x.to(DEV)))), "y: the no-grad forward on the canonical codes"
        assert torch.equal(_bits(y.detach()), _bits(train(x.to(DEV))))
    want = _fp64_grads(train, x, wy)
    dw = wy.double().t() @ x.double()
    assert torch.equal(dw.to(dtype).double(), dw), "the data keeps dW exact in the storage dtype"
    for name, p, w in (("codebooks", train.codebooks, want[1]), ("scales", train.scales, want[2]), ("bias", train.bias, want[3])):
        assert p.grad is not None and p.grad.dtype == dtype and p.grad.shape == p.shape, name
        assert torch.equal(_bits(p.grad.cpu()), _bits(w.to(dtype))), name
    if input_grad:
        xf = x.to(DEV).requires_grad_(True)
        (frozen(xf) * wy.to(DEV)).sum().backward()
        assert torch.equal(_bits(xt.grad), _bits(xf.grad)), "grad_input: the frozen layer's"
    else:
        assert xt.grad is None
    assert all(p.grad is None for p in frozen.parameters())


# ---------------------------------------------------------------------------------------------------------------------------
# 6. a training step, then inference
# ---------------------------------------------------------------------------------------------------------------------------
def test_inference_after_a_training_step_reads_the_updated_parameters(monkeypatch):
    """prepack_model (the default drop) on a small layer (the packing threshold lowered for the whole test, as smoke() does: the
    layer is packed again whenever its derived state is rebuilt), one SGD step on codebooks and scales, then no-grad forwards of
    1, 9 and 300 rows: bit-identical to a freshly built and prepacked layer holding the updated parameters -- the codebook image
    and range of the packed buffer, the fast lane and every other derived copy were rebuilt."""
    import aqlm
    import aqlm_amd.inference as inf
    from aqlm_amd.checkpoint import prepack_model

    monkeypatch.setattr(inf, "PREPACK_MIN_CODES", 100_000)

    fin, fout, dtype = 2048, 512, torch.float16
    gen = torch.Generator().manual_seed(77)

    def build(codes, codebooks, scales, bias):
        m = aqlm.QuantizedLinear(fin, fout, 8, 1, 1, 16, bias=True, device=DEV, dtype=dtype)
        with torch.no_grad():
            m.codes.copy_(codes); m.codebooks.copy_(codebooks); m.scales.copy_(scales); m.bias.copy_(bias)  # noqa: E702
        rep = prepack_model(torch.nn.ModuleDict({"l": m}))
        assert rep["prepacked_layers"] == 1 and m._codes_dropped
        return m

    codes = torch.randint(-32768, 32768, (fout, fin // 8, 1), generator=gen).to(torch.int16)
    layer = build(codes, torch.randn((1, 65536, 1, 8), generator=gen) * 0.1, torch.rand((fout, 1, 1, 1), generator=gen) + 0.5,
                  torch.randn((fout,), generator=gen) * 0.1)
    xs = {rows: torch.randn((rows, fin), generator=gen).to(dtype).to(DEV) for rows in (1, 9, 300)}
    with torch.no_grad():
        # the derived state of the packed routes exists before the step (9 rows would take the canonical codes back: the training
        # call below meets the layer still dropped)
        before = {rows: layer(xs[rows]) for rows in (1, 300)}
    assert layer._codes_dropped
    params = aqlm.tuning.make_trainable(torch.nn.ModuleDict({"l": layer}))
    opt = torch.optim.SGD(params, lr=0.01)
    y = layer(xs[9])
    (y * torch.randn(y.shape, generator=gen).to(dtype).to(DEV)).sum().backward()
    assert layer.codebooks.grad is not None and layer.scales.grad is not None and layer.bias.grad is None
    old = layer.codebooks.detach().clone()
    opt.step()
    assert not torch.equal(old, layer.codebooks.detach())
    fresh = build(layer._canonical_codes().cpu(), layer.codebooks.detach().cpu(), layer.scales.detach().cpu(), layer.bias.detach().cpu())
    with torch.no_grad():
        for rows, x in xs.items():
            got, want = layer(x), fresh(x)
            assert rows > 6 or layer._packed_codes is not None
            assert torch.equal(_bits(got), _bits(want)), f"{rows} rows after the step"
            assert rows not in before or not torch.equal(_bits(got), _bits(before[rows])), f"{rows} rows: the step changed nothing?"


# ---------------------------------------------------------------------------------------------------------------------------
# 8. the switch
# ---------------------------------------------------------------------------------------------------------------------------
def test_switch_off_runs_the_torch_route(module_layers, monkeypatch):
    """With ``CODEBOOK_GRAD_KERNEL = False`` the reference's definition runs under autograd in the storage dtype: it rounds dW, the
    scaled dW and every step of its scatter-add to fp16 / bf16, so the fp32 bound of test 3 can only hold for it on data whose
    storage-dtype intermediates are exact -- the integer data of test 5 at 9 rows (|dW| <= 36, sums far below 2048 / 256)."""
    import copy

    import aqlm.tuning as tuning
    from aqlm_amd.inference import _TrainableMatmul1x16

    case = MODULE_CASES[0]
    g, fin, fout, dtype = case
    x, wy = _integer_inputs(9, fin, fout, dtype, 5)
    exact = _fp64_grads(module_layers[case][0], x, wy)
    magnitude = _fp64_grads_abs(module_layers[case][0], x, wy)
    grads = {}
    for on in (True, False):
        monkeypatch.setattr(tuning, "CODEBOOK_GRAD_KERNEL", on)
        layer = copy.deepcopy(module_layers[case][0])
        assert layer._takes_codebook_grad_kernel(x.to(DEV)) is on
        y = layer(x.to(DEV))
        assert (type(y.grad_fn).__name__ == _TrainableMatmul1x16.__name__ + "Backward") is on
        (y * wy.to(DEV)).sum().backward()
        grads[on] = [layer.codebooks.grad, layer.scales.grad, layer.bias.grad]
        assert all(t is not None and t.dtype == dtype for t in grads[on])
        n = 9 * fin  # terms per gradient element, at most
        for got, e, mag in zip(grads[on], exact[1:], magnitude[1:]):
            assert ((got.double().cpu() - e).abs() <= (n + 2) * 2.0 ** -24 * mag + UNIT[dtype] * e.abs()).all(), on
    for a, b in zip(grads[True], grads[False]):
        assert torch.equal(_bits(a), _bits(b))


def test_fp32_dw_gives_the_same_exact_gradients(module_layers, monkeypatch):
    """``CODEBOOK_GRAD_FP32_DW``: dW comes out of the library GEMM in fp32 and the two launches read it as such."""
    import copy

    import aqlm.tuning as tuning

    monkeypatch.setattr(tuning, "CODEBOOK_GRAD_FP32_DW", True)
    for case in MODULE_CASES[:2]:
        g, fin, fout, dtype = case
        layer = copy.deepcopy(module_layers[case][0])
        x, wy = _integer_inputs(300, fin, fout, dtype, 17)
        (layer(x.to(DEV)) * wy.to(DEV)).sum().backward()
        want = _fp64_grads(layer, x, wy)
        for p, w in ((layer.codebooks, want[1]), (layer.scales, want[2]), (layer.bias, want[3])):
            assert p.grad.dtype == dtype and torch.equal(_bits(p.grad.cpu()), _bits(w.to(dtype)))


def _fp64_grads_abs(layer, x, wy):
    """The gradients of the same expression on the absolute values: per gradient element the sum of its terms' magnitudes."""
    import copy

    m = copy.deepcopy(layer)
    with torch.no_grad():
        for p in (m.codebooks, m.scales, m.bias):
            p.abs_()
    return _fp64_grads(m, x.abs(), wy.abs())


# ---------------------------------------------------------------------------------------------------------------------------
# 7. capture (last: it ends with a capture that raises)
# ---------------------------------------------------------------------------------------------------------------------------
def test_forward_and_backward_replay_from_a_hip_graph(module_layers):
    import copy

    import aqlm.tuning as tuning

    case = MODULE_CASES[0]
    g, fin, fout, dtype = case
    layer = copy.deepcopy(module_layers[case][0])
    holder = torch.nn.ModuleDict({"l": layer})
    assert layer._grad_index is None
    assert tuning.prepare(holder) == layer._grad_index[1].nbytes() > 4 * layer.codes.numel()
    inputs = [_integer_inputs(9, fin, fout, dtype, 300 + i) for i in range(3)]
    sx, swy = inputs[0][0].to(DEV).clone().requires_grad_(True), inputs[0][1].to(DEV).clone()

    def step():
        y = layer(sx)
        (y * swy).sum().backward()

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # warm-up: library handles and workspaces exist before the capture
        step()
    torch.cuda.current_stream().wait_stream(side)
    for p in list(layer.parameters()) + [sx]:
        p.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    static = [layer.codebooks.grad, layer.scales.grad, layer.bias.grad, sx.grad]
    for x, wy in inputs[1:]:
        with torch.no_grad():
            sx.copy_(x.to(DEV)); swy.copy_(wy.to(DEV))  # noqa: E702
        graph.replay()
        torch.cuda.synchronize()
        replayed = [t.clone() for t in static]
        eager = copy.deepcopy(layer)
        for p in eager.parameters():
            p.grad = None
        ex = x.to(DEV).requires_grad_(True)
        (eager(ex) * wy.to(DEV)).sum().backward()
        for a, b in zip(replayed, [eager.codebooks.grad, eager.scales.grad, eager.bias.grad, ex.grad]):
            assert torch.equal(_bits(a), _bits(b))
        want = _fp64_grads(layer, x, wy)
        assert torch.equal(_bits(replayed[0].cpu()), _bits(want[1].to(dtype)))


def test_capture_without_the_index_raises_before_any_launch(module_layers):
    import copy

    case = MODULE_CASES[0]
    g, fin, fout, dtype = case
    layer = copy.deepcopy(module_layers[case][0])
    x = _integer_inputs(9, fin, fout, dtype, 1)[0].to(DEV)
    assert layer._grad_index is None
    graph = torch.cuda.CUDAGraph()
    with pytest.raises(RuntimeError, match="aqlm.tuning.prepare"):
        with torch.cuda.graph(graph):
            x * 2  # (the capture holds a node of its own, so that ending it is an ordinary capture end)
            layer(x)
    assert layer._grad_index is None
    torch.cuda.synchronize()
    y = layer(x)  # eager: the index is built now, and the call runs
    assert layer._grad_index is not None and y.requires_grad
