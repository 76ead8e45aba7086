"""Training codebooks and scales of K x 8 layers on the MI355X: aqlm_hip_codebook_grad_kx8 / aqlm_hip_scales_grad_kx8 and the
autograd route built on them.

The codebook gradient is a sum of fixed-point integers: its bits are a function of the arguments alone, so every test of it
compares BITS -- against the fp64 sum rounded once on integer data (where the quantisation is exact), against the numpy model of
the documented arithmetic (tests/kx8_grad_model.py) on real-valued data.  The scale gradient keeps the 1x16 entry's fp32 form and
its bound."""
import copy

import numpy as np
import pytest
import torch

from tests import kx8_grad_model as model

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
# (out, in, g, K): fewer rows than row blocks; g 16, one pass of four codebooks; 65 groups per row, rows not divisible by the blocks,
# 17160 positions; g 32, four passes of two codebooks; more rows than row blocks, uneven split (520 = 2 * 256 + 8)
SHAPES = [(24, 64, 8, 2), (40, 192, 16, 4), (264, 520, 8, 2), (72, 320, 32, 8), (520, 64, 8, 1)]
KINDS = ("uniform", "equal", "one_equal")
UNIT = {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8, torch.float32: 2.0 ** -24}
TINY = {torch.float16: 2.0 ** -25, torch.bfloat16: 2.0 ** -134, torch.float32: 2.0 ** -150}
DW_DTYPES = (torch.float16, torch.bfloat16, torch.float32)


def _name(dtype):
    return str(dtype)[6:]


def _storage(dw_dtype):
    return torch.float16 if dw_dtype == torch.float32 else dw_dtype


def _within(got, exact, bound, what):
    excess = np.abs(got - exact) - bound
    i = np.unravel_index(np.argmax(excess), excess.shape)
    assert excess[i] <= 0, f"{what}: element {i}: got {got[i]!r}, exact {exact[i]!r}, bound {bound[i]!r}"


@pytest.fixture(scope="module")
def hk():
    from aqlm_amd.inference_kernels import hip_kernel

    return hip_kernel


def _codes(kind, out, nj, K, seed):
    """int8 containers [out, nj, K].  uniform: every entry, the containers -128, -1, 0, 127 planted; equal: every position on one
    value (every lane on one LDS address); one_equal: codebook 0 on one value, the rest uniform."""
    rng = np.random.default_rng(seed)
    v = rng.integers(0, 256, size=(out, nj, K))
    if kind == "uniform":
        flat = v.reshape(-1)
        flat[[0, 1, flat.size // 2, flat.size - 1]] = (128, 255, 0, 127)
    elif kind == "equal":
        v[:] = 200
    else:
        v[:, :, 0] = 131
    return v.astype(np.uint8).view(np.int8)


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _same_bits(got, want, dtype):
    """``got`` equals ``want`` (fp64 or fp32 numpy) rounded once to ``dtype``, bit for bit (signed zeros and NaN included)."""
    w = torch.from_numpy(np.ascontiguousarray(want)).to(dtype)
    return torch.equal(_bits(got.cpu()), _bits(w))


@pytest.fixture(scope="module")
def raw_cases():
    """Per (shape, kind): the codes on the GPU and the unsigned values."""
    cases = {}
    for si, (out, fin, g, K) in enumerate(SHAPES):
        for ki, kind in enumerate(KINDS):
            codes = _codes(kind, out, fin // g, K, 100 + 10 * si + ki)
            cases[(out, fin, g, K, kind)] = (torch.from_numpy(codes).to(DEV), codes.view(np.uint8).astype(np.int64))
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


# ---------------------------------------------------------------------------------------------------------------------------
# 1. raw dC on integer data: the fp64 sum rounded once, bit for bit
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_codebook_grad_is_exact_on_integer_data(hk, raw_cases, shape, kind):
    out, fin, g, K = shape
    codes, values = raw_cases[(out, fin, g, K, kind)]
    unused = torch.from_numpy(model.counts(values) == 0)
    gen = torch.Generator().manual_seed(7)
    for di, dw_dtype in enumerate(DW_DTYPES):
        storage = _storage(dw_dtype)
        scales = torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (out,), generator=gen)].to(storage)
        for padded in (False, True):
            dw, dw64 = _dw(out, fin, dw_dtype, 20 + di, padded)
            for s in (scales, None):
                s64 = np.ones(out) if s is None else s.double().numpy()
                want, _ = model.exact_dc(values, dw64, s64, g)
                assert np.abs(want).max() * 2 < 2 ** 24  # the int64 -> fp32 conversion is exact
                for out_dtype in (torch.float32, storage):
                    got = hk.codebook_grad_kx8(dw, None if s is None else s.to(DEV), codes, g, out_dtype=out_dtype)
                    assert got.shape == (K, 256, g) and got.dtype == out_dtype
                    assert not torch.isnan(got).any()
                    assert _same_bits(got, want, out_dtype), (dw_dtype, padded, s is None, out_dtype)
                    assert (_bits(got.cpu())[unused] == 0).all(), "unused entries are +0"


# ---------------------------------------------------------------------------------------------------------------------------
# 2. real-valued dC: the numpy model of the fixed-point arithmetic bit for bit -- no schedule can change the bits
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dw_dtype", DW_DTYPES, ids=_name)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_real_valued_codebook_grad_equals_the_fixed_point_model_bit_for_bit(hk, raw_cases, shape, kind, dw_dtype):
    out, fin, g, K = shape
    codes, values = raw_cases[(out, fin, g, K, kind)]
    storage = _storage(dw_dtype)
    gen = torch.Generator().manual_seed(13)
    dw, dw64 = _dw(out, fin, dw_dtype, 50, True, real=True)
    scales = (torch.rand((out,), generator=gen) + 0.5).to(storage)
    s64 = scales.double().numpy()
    want32 = model.fixed_point_dc(values, dw64, s64, g)
    exact, _ = model.exact_dc(values, dw64, s64, g)
    for out_dtype in (torch.float32, storage):
        got = hk.codebook_grad_kx8(dw, scales.to(DEV), codes, g, out_dtype=out_dtype)
        assert _same_bits(got, want32, out_dtype), out_dtype
        _within(got.double().cpu().numpy(), exact, model.dc_bound(values, dw64, s64, g, _name(out_dtype)), f"dC {out_dtype}")


# ---------------------------------------------------------------------------------------------------------------------------
# 3. headroom: every position on one entry, maximal data
# ---------------------------------------------------------------------------------------------------------------------------
def test_headroom_at_maximal_data(hk):
    out, fin, g, K = SHAPES[2]
    codes = torch.full((out, fin // g, K), -56, dtype=torch.int8, device=DEV)  # the container of entry 200
    dw = torch.full((out, fin), 65504.0, dtype=torch.float16, device=DEV)
    s = torch.full((out,), 2.0, dtype=torch.float16, device=DEV)
    got = hk.codebook_grad_kx8(dw, s, codes, g, out_dtype=torch.float32).cpu()
    assert out * (fin // g) == 17160
    assert (got[:, 200, :] == 2248097280.0).all()
    got[:, 200, :] = 0
    assert (_bits(got) == 0).all()


# ---------------------------------------------------------------------------------------------------------------------------
# 4. zero and non-finite data
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[3]], ids=lambda s: "x".join(map(str, s)))
def test_zero_and_non_finite_data(hk, raw_cases, shape):
    out, fin, g, K = shape
    codes, values = raw_cases[(out, fin, g, K, "uniform")]
    dw, dw64 = _dw(out, fin, torch.float16, 61, False)
    s = torch.ones((out,), dtype=torch.float16, device=DEV)
    want, _ = model.exact_dc(values, dw64, np.ones(out), g)

    def finite_call_is_exact():
        assert _same_bits(hk.codebook_grad_kx8(dw, s, codes, g, out_dtype=torch.float32), want, torch.float32)

    finite_call_is_exact()
    zero = hk.codebook_grad_kx8(torch.zeros_like(dw), s, codes, g, out_dtype=torch.float32)
    assert (_bits(zero) == 0).all(), "dW == 0: every output is +0"
    finite_call_is_exact()
    for where, value in (("dw", float("inf")), ("dw", float("nan")), ("dw", float("-inf")), ("scales", float("inf"))):
        bad_dw, bad_s = dw.clone(), s.clone()
        if where == "dw":
            bad_dw[out - 1, fin - 3] = value
        else:
            bad_s[out // 2] = value
        for out_dtype in (torch.float32, torch.float16):
            got = hk.codebook_grad_kx8(bad_dw, bad_s, codes, g, out_dtype=out_dtype)
            assert torch.isnan(got).all(), (where, value, out_dtype)
        finite_call_is_exact()  # nothing sticks in the workspace


# ---------------------------------------------------------------------------------------------------------------------------
# 5. the raw entry on dirty buffers
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [SHAPES[2], SHAPES[3]], ids=lambda s: "x".join(map(str, s)))
def test_raw_entry_writes_every_output_whatever_out_and_workspace_held(hk, raw_cases, shape):
    from aqlm_amd import _native as nat

    out, fin, g, K = shape
    codes, values = raw_cases[(out, fin, g, K, "one_equal")]
    dw, dw64 = _dw(out, fin, torch.bfloat16, 60, False, real=True)
    scales = (torch.rand((out,), generator=torch.Generator().manual_seed(1)) + 0.5).to(torch.bfloat16)
    want32 = model.fixed_point_dc(values, dw64, scales.double().numpy(), g)
    scales = scales.to(DEV)
    ws_bytes = nat.lib.aqlm_hip_codebook_grad_kx8_workspace_bytes(out, fin, K, g)
    results = []
    for fill in ("nan", "ff", "ff"):
        if fill == "nan":
            y = torch.full((K, 256, g), float("nan"), dtype=torch.float32, device=DEV)
            ws = torch.full((ws_bytes // 4,), float("nan"), dtype=torch.float32, device=DEV)
        else:
            y = torch.full((K * 256 * g * 4,), 0xFF, dtype=torch.uint8, device=DEV).view(torch.float32).reshape(K, 256, g)
            ws = torch.full((ws_bytes,), 0xFF, dtype=torch.uint8, device=DEV)
        rc = nat.lib.aqlm_hip_codebook_grad_kx8(dw.data_ptr(), dw.stride(0), nat.BF16, scales.data_ptr(), nat.BF16, codes.data_ptr(), out,
                                                fin, K, g, y.data_ptr(), nat.F32, ws.data_ptr(), ws_bytes,
                                                torch.cuda.current_stream(DEV).cuda_stream)
        assert rc == 0, nat.last_error()
        assert not torch.isnan(y).any() and _same_bits(y, want32, torch.float32), fill
        results.append(y)
    a = hk.codebook_grad_kx8(dw, scales, codes, g, out_dtype=torch.float32)
    b = hk.codebook_grad_kx8(dw, scales, codes, g, out_dtype=torch.float32)
    for r in results + [b]:
        assert torch.equal(_bits(a), _bits(r))


# ---------------------------------------------------------------------------------------------------------------------------
# 6. the scale gradient
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_scales_grad_is_exact_on_integer_data(hk, raw_cases, shape, kind):
    out, fin, g, K = shape
    codes, values = raw_cases[(out, fin, g, K, kind)]
    gen = torch.Generator().manual_seed(9)
    for di, dw_dtype in enumerate(DW_DTYPES):
        storage = _storage(dw_dtype)
        cb = torch.randint(-4, 5, (K, 256, 1, g), generator=gen).to(storage)
        for padded in (False, True):
            dw, dw64 = _dw(out, fin, dw_dtype, 40 + di, padded)
            want, _ = model.exact_ds(values, dw64, cb.double().numpy().reshape(K, 256, g), g)
            assert np.abs(want).max() < 2 ** 24
            for out_dtype in (torch.float32, storage):
                got = hk.scales_grad_kx8(dw, codes, cb.to(DEV), out_dtype=out_dtype)
                assert got.shape == (out,) and got.dtype == out_dtype
                assert _same_bits(got, want, out_dtype), (dw_dtype, padded, out_dtype)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=_name)
@pytest.mark.parametrize("shape", SHAPES[1:], ids=lambda s: "x".join(map(str, s)))
def test_real_valued_scales_grad_within_the_fp32_bound(hk, raw_cases, shape, dtype):
    out, fin, g, K = shape
    codes, values = raw_cases[(out, fin, g, K, "uniform")]
    gen = torch.Generator().manual_seed(17)
    dw, dw64 = _dw(out, fin, dtype, 51, True, real=True)
    cb = torch.randn((K, 256, 1, g), generator=gen).to(dtype)
    exact, mag = model.exact_ds(values, dw64, cb.double().numpy().reshape(K, 256, g), g)
    for out_dtype in (torch.float32, dtype):
        got = hk.scales_grad_kx8(dw, codes, cb.to(DEV), out_dtype=out_dtype).double().cpu().numpy()
        _within(got, exact, (fin + K + 2) * 2.0 ** -24 * mag + UNIT[out_dtype] * np.abs(exact) + TINY[out_dtype], f"ds {out_dtype}")
    # a NaN in one row of dW poisons that row only
    bad = dw.clone()
    bad[out // 3, 5] = float("nan")
    got = hk.scales_grad_kx8(bad, codes, cb.to(DEV), out_dtype=torch.float32)
    clean = hk.scales_grad_kx8(dw, codes, cb.to(DEV), out_dtype=torch.float32)
    nan = torch.isnan(got).cpu()
    assert nan[out // 3] and int(nan.sum()) == 1
    keep = ~nan.to(DEV)
    assert torch.equal(_bits(got[keep]), _bits(clean[keep]))


# ---------------------------------------------------------------------------------------------------------------------------
# 7. the module end to end
# ---------------------------------------------------------------------------------------------------------------------------
MODULE_CASES = [(2, 8, 1024, 64, torch.float16), (1, 8, 520, 64, torch.bfloat16), (8, 32, 1024, 32, torch.bfloat16),
                (4, 16, 1040, 40, torch.float16), (2, 8, 1024, 64, torch.bfloat16), (8, 32, 1024, 32, torch.float16)]


def _case_id(c):
    return f"{c[0]}x8g{c[1]}_{c[2]}x{c[3]}_{_name(c[4])}"


def _integer_layer(K, g, fin, fout, dtype, seed, device=DEV):
    """Codebook integers in [-4, 4], scales in {0.5, 1, 2}, an integer bias: with integer inputs every gradient is exact in fp32."""
    import aqlm

    gen = torch.Generator().manual_seed(seed)
    m = aqlm.QuantizedLinear(fin, fout, g, 1, K, 8, bias=True, device=device, dtype=dtype)
    with torch.no_grad():
        m.codes.copy_(torch.randint(-128, 128, m.codes.shape, generator=gen).to(torch.int8))
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
    codes = layer._canonical_codes().detach().cpu().to(torch.int64) % 256
    y = torch.nn.functional.linear(leaves[0], _dequantize_weight(codes, leaves[1], leaves[2]), leaves[3])
    (y * wy.double().cpu()).sum().backward()
    return y.detach(), [t.grad for t in leaves]


def _fp64_grads_abs(layer, x, wy):
    m = copy.deepcopy(layer)
    with torch.no_grad():
        for p in (m.codebooks, m.scales, m.bias):
            p.abs_()
    return _fp64_grads(m, x.abs(), wy.abs())[1]


@pytest.fixture(scope="module")
def module_layers():
    """Per case: the trainable layer and a frozen twin; never modified by the tests."""
    out = {}
    for i, case in enumerate(MODULE_CASES):
        K, g, fin, fout, dtype = case
        frozen = _integer_layer(K, g, fin, fout, dtype, 200 + i)
        train = copy.deepcopy(frozen)
        for p in (train.codebooks, train.scales, train.bias):
            p.requires_grad_(True)
        out[case] = (train, frozen)
    return out


def _check_exact_gradients(train, x, wy, dtype, xt=None):
    _, want = _fp64_grads(train, x, wy)
    dw = wy.double().t() @ x.double()
    assert torch.equal(dw.to(dtype).double(), dw), "the data keeps dW exact in the storage dtype"
    for name, p, w in (("codebooks", train.codebooks, want[1]), ("scales", train.scales, want[2]), ("bias", train.bias, want[3])):
        assert p.grad is not None and p.grad.dtype == dtype and p.grad.shape == p.shape, name
        assert torch.equal(_bits(p.grad.cpu()), _bits(w.to(dtype))), name
    if xt is not None:
        assert torch.equal(_bits(xt.grad.cpu()), _bits(want[0].to(dtype))), "grad_input"


@pytest.mark.parametrize("input_grad", [True, False], ids=["x_grad", "x_frozen"])
@pytest.mark.parametrize("rows", [2, 9, 64])
@pytest.mark.parametrize("case", MODULE_CASES, ids=_case_id)
def test_module_gradients_equal_fp64_autograd_bit_for_bit(module_layers, case, rows, input_grad):
    K, g, fin, fout, dtype = case
    train, frozen = module_layers[case]
    x, wy = _integer_inputs(rows, fin, fout, dtype, rows)
    xt = x.to(DEV).requires_grad_(input_grad)
    for p in train.parameters():
        p.grad = None
    assert train._takes_codebook_grad_kernel_kx8(xt) and not train._takes_codebook_grad_kernel(xt)
    y = train(xt)
    assert y.grad_fn is not None and type(y.grad_fn).__name__ == "_TrainableMatmulKx8Backward"
    (y * wy.to(DEV)).sum().backward()
    with torch.no_grad():
        assert torch.equal(_bits(y.detach()), _bits(frozen(x.to(DEV)))), "y: the frozen layer's forward"
    _check_exact_gradients(train, x, wy, dtype, xt if input_grad else None)
    if not input_grad:
        assert xt.grad is None
    assert all(p.grad is None for p in frozen.parameters())
    assert train._grad_index is None, "no derived state"


def test_fp32_dw_gives_the_same_exact_gradients(module_layers, monkeypatch):
    import aqlm.tuning as tuning

    monkeypatch.setattr(tuning, "CODEBOOK_GRAD_FP32_DW", True)
    for case in MODULE_CASES[:4]:
        K, g, fin, fout, dtype = case
        layer = copy.deepcopy(module_layers[case][0])
        x, wy = _integer_inputs(64, fin, fout, dtype, 17)
        (layer(x.to(DEV)) * wy.to(DEV)).sum().backward()
        _check_exact_gradients(layer, x, wy, dtype)


# ---------------------------------------------------------------------------------------------------------------------------
# 8. the switch
# ---------------------------------------------------------------------------------------------------------------------------
def test_switch_off_runs_the_torch_route(module_layers, monkeypatch):
    """With ``CODEBOOK_GRAD_KERNEL = False`` the reference's definition runs under autograd in the storage dtype; on the integer
    data at 9 rows its storage-dtype intermediates are exact, so it meets the fp32 bound of the 1x16 test too."""
    import aqlm.tuning as tuning

    case = MODULE_CASES[0]
    K, g, fin, fout, dtype = case
    x, wy = _integer_inputs(9, fin, fout, dtype, 5)
    _, exact = _fp64_grads(module_layers[case][0], x, wy)
    magnitude = _fp64_grads_abs(module_layers[case][0], x, wy)
    grads = {}
    for on in (True, False):
        monkeypatch.setattr(tuning, "CODEBOOK_GRAD_KERNEL", on)
        layer = copy.deepcopy(module_layers[case][0])
        assert layer._takes_codebook_grad_kernel_kx8(x.to(DEV)) is on
        y = layer(x.to(DEV))
        assert (type(y.grad_fn).__name__ == "_TrainableMatmulKx8Backward") is on
        (y * wy.to(DEV)).sum().backward()
        grads[on] = [layer.codebooks.grad, layer.scales.grad, layer.bias.grad]
        assert all(t is not None and t.dtype == dtype for t in grads[on])
        n = 9 * fin * K
        for got, e, mag in zip(grads[on], exact[1:], magnitude[1:]):
            assert ((got.double().cpu() - e).abs() <= (n + 2) * 2.0 ** -24 * mag + UNIT[dtype] * e.abs()).all(), on
    for a, b in zip(grads[True], grads[False]):
        assert torch.equal(_bits(a), _bits(b))


# ---------------------------------------------------------------------------------------------------------------------------
# 9. a training step, then inference
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scheme", [(2, 8, 4096, 4096), (8, 32, 2048, 1024)], ids=["2x8g8_replicated_lds", "8x8g32_planar"])
def test_inference_after_an_optimizer_step_reads_the_stepped_parameters(scheme):
    """One SGD step on codebooks and scales, then a no-grad single-row forward -- the replicated-LDS matvec for 2x8 g8 at 4096 rows
    of W, the planar look-up-table kernel for 8x8 g32 -- against the definition on the live parameters."""
    import aqlm
    from aqlm_amd.utils import _dequantize_weight

    K, g, fin, fout = scheme
    dtype = torch.float16
    gen = torch.Generator().manual_seed(77)
    layer = aqlm.QuantizedLinear(fin, fout, g, 1, K, 8, bias=True, device=DEV, dtype=dtype)
    with torch.no_grad():
        layer.codes.copy_(torch.randint(-128, 128, layer.codes.shape, generator=gen).to(torch.int8))
        layer.codebooks.copy_(torch.randn(layer.codebooks.shape, generator=gen) * 0.1)
        layer.scales.copy_(torch.rand(layer.scales.shape, generator=gen) + 0.5)
        layer.bias.copy_(torch.randn(layer.bias.shape, generator=gen) * 0.1)
    x1 = torch.randn((1, fin), generator=gen).to(dtype).to(DEV)
    with torch.no_grad():
        before = layer(x1)  # the derived state of the decode route exists before the step
    if K == 8:
        from aqlm_amd.inference_kernels import hip_kernel

        assert isinstance(layer._packed_codes, hip_kernel.PlanarCodes)
    params = aqlm.tuning.make_trainable(torch.nn.ModuleDict({"l": layer}))
    opt = torch.optim.SGD(params, lr=1e-3)
    x9 = torch.randn((9, fin), generator=gen).to(dtype).to(DEV)
    y = layer(x9)
    assert type(y.grad_fn).__name__ == "_TrainableMatmulKx8Backward"
    (y * torch.randn(y.shape, generator=gen).to(dtype).to(DEV)).sum().backward()
    assert layer.codebooks.grad is not None and layer.scales.grad is not None and layer.bias.grad is None
    old = layer.codebooks.detach().clone()
    opt.step()
    assert not torch.equal(old, layer.codebooks.detach())
    with torch.no_grad():
        after = layer(x1)
        codes = layer._canonical_codes().to(torch.int64) % 256
        W = _dequantize_weight(codes, layer.codebooks.double(), layer.scales.double())
        want = torch.nn.functional.linear(x1.double(), W, layer.bias.double())
        absW = _dequantize_weight(codes, layer.codebooks.double().abs(), layer.scales.double().abs())
        mag = torch.nn.functional.linear(x1.double().abs(), absW, layer.bias.double().abs())
    # fp32 accumulation of fin * K + 1 products and one rounding to fp16
    bound = (fin * K + 4) * 2.0 ** -24 * mag + UNIT[dtype] * want.abs() + TINY[dtype]
    assert ((after.double() - want).abs() <= bound).all()
    assert not torch.equal(_bits(after), _bits(before)), "the step changed nothing?"
    stale = (before.double() - want).abs() > bound
    assert stale.any(), "the stale parameters would have met the bound: the test shows nothing"


# ---------------------------------------------------------------------------------------------------------------------------
# 10. dropped canonical codes
# ---------------------------------------------------------------------------------------------------------------------------
def test_dropped_planar_codes_train_with_the_same_bits(monkeypatch):
    import aqlm_amd.inference as inf
    from aqlm_amd.checkpoint import prepack_model

    monkeypatch.setattr(inf, "PREPACK_MIN_CODES", 1000)  # the small layer takes planar codes, whenever its derived state is built
    K, g, fin, fout, dtype = 8, 32, 2048, 32, torch.float16  # 64 input groups: the fewest the planar layout takes
    layer = _integer_layer(K, g, fin, fout, dtype, 301)
    x, wy = _integer_inputs(9, fin, fout, dtype, 3)

    def grads(m):
        for p in (m.codebooks, m.scales, m.bias):
            p.requires_grad_(True)
            p.grad = None
        y = m(x.to(DEV))
        assert type(y.grad_fn).__name__ == "_TrainableMatmulKx8Backward"
        (y * wy.to(DEV)).sum().backward()
        return [y.detach().clone(), m.codebooks.grad.clone(), m.scales.grad.clone(), m.bias.grad.clone()]

    before = grads(copy.deepcopy(layer))
    for p in layer.parameters():
        p.requires_grad_(False)
    rep = prepack_model(torch.nn.ModuleDict({"l": layer}), drop_canonical=True)
    if not layer._codes_dropped:
        pytest.fail(f"prepack_model did not drop the canonical codes of an 8x8 g32 layer: {rep}")
    after = grads(layer)
    for a, b in zip(before, after):
        assert torch.equal(_bits(a), _bits(b))
    _check_exact_gradients(layer, x, wy, dtype)


# ---------------------------------------------------------------------------------------------------------------------------
# 11. capture (last)
# ---------------------------------------------------------------------------------------------------------------------------
def test_forward_and_backward_replay_from_a_hip_graph(module_layers):
    import aqlm.tuning as tuning

    case = MODULE_CASES[0]
    K, g, fin, fout, dtype = case
    layer = copy.deepcopy(module_layers[case][0])
    assert tuning.prepare(torch.nn.ModuleDict({"l": layer})) == 0 and layer._grad_index is None  # nothing to build, nothing needed
    inputs = [_integer_inputs(9, fin, fout, dtype, 300 + i) for i in range(4)]
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
        _, want = _fp64_grads(layer, x, wy)
        assert torch.equal(_bits(replayed[0].cpu()), _bits(want[1].to(dtype)))
