"""GPU: the K x 9..16-bit g 8 kernels (2x16, 2x12, 4x16; 2x9 for the smallest codebook) against the float64 definition
utils._dequantize_weight + matmul -- the direct matvec (aqlm_hip_gemv_kx16) at 1 .. 9 rows and the fused dequantise-to-MFMA kernel
(aqlm_hip_gemm_kx16_rows) from 7 rows on, through the functions kernel_selector returns for these schemes."""
import functools

import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from aqlm_amd.utils import _dequantize_weight, unpack_int_data  # noqa: E402

F16, BF16 = torch.float16, torch.bfloat16
SCHEMES = [(2, 16), (2, 12), (4, 16), (2, 9)]
GEOMETRIES = [(512, 40), (544, 16)]   # out no multiple of 16 / of the rows of a block; 17 chunks: an uneven split over the waves
GEMV_ROWS, FUSED_ROWS = (1, 3, 6, 9), (7, 16, 17, 64, 65)   # 9: slabs of 8 + 1; 65: a second pass
EPS = {F16: 2.0 ** -11, BF16: 2.0 ** -8}


@pytest.fixture()
def hk(monkeypatch):
    assert torch.cuda.is_available(), "run with -m gpu on the MI355X box"
    from aqlm_amd.inference_kernels import hip_kernel

    monkeypatch.setattr(hip_kernel, "USE_KX16_GEMV", True)        # both routes open, whatever ships
    monkeypatch.setattr(hip_kernel, "FUSED_KX16_MAX_ROWS", 1 << 20)
    return hip_kernel


@functools.lru_cache(maxsize=None)
def layer(K, nbits, dtype, inf, out, exact, codes="plain"):
    """A seeded layer on the device, 65 rows of x and the float64 result.  exact: small integers, power-of-two scales, integer bias (every
    sum is exact in fp32).  codes: "high" sets the bits above nbits, "negative" makes every int16 code negative (nbits 16)."""
    g = torch.Generator().manual_seed(1000 * K + 10 * nbits + inf + (dtype == BF16))
    size = 1 << nbits
    idx = torch.randint(0, size, (out, inf // 8, K), generator=g)
    if codes == "negative":
        idx = idx | 0x8000
    stored = idx | (torch.randint(0, 1 << (16 - nbits), idx.shape, generator=g) << nbits) if codes == "high" else idx
    stored = torch.where(stored >= 32768, stored - 65536, stored).to(torch.int16)
    if exact:
        cb = torch.randint(-3, 4, (K, size, 1, 8), generator=g).double()
        scales = 2.0 ** torch.randint(-1, 2, (out, 1, 1, 1), generator=g).double()
        bias = torch.randint(-4, 5, (out,), generator=g).double()
        x = torch.randint(-2, 3, (65, inf), generator=g).double()
    else:
        cb = torch.randn(K, size, 1, 8, generator=g, dtype=torch.float64) * 0.05
        scales = torch.rand(out, 1, 1, 1, generator=g, dtype=torch.float64) + 0.5
        bias = torch.randn(out, generator=g, dtype=torch.float64)
        x = torch.randn(65, inf, generator=g, dtype=torch.float64)
    cb, scales, bias, x = (t.to(dtype) for t in (cb, scales, bias, x))   # the stored values are the operands of both sides
    assert torch.equal(unpack_int_data(stored, nbits), idx)
    W = _dequantize_weight(idx, cb.double(), None)
    y64 = (x.double() @ W.T) * scales.double().reshape(1, -1) + bias.double()
    slack = (x.double().abs() @ W.abs().T) * scales.double().abs().reshape(1, -1)
    dev = [t.cuda() for t in (stored, cb, scales, bias)]
    return dict(args=dev, x=x.cuda(), y64=y64, slack=slack, K=K, inf=inf)


def run(hk, L, rows, x=None):
    """The matvec below 7 rows and at 9, the fused kernel from 7 on."""
    x = L["x"][:rows] if x is None else x
    if rows in GEMV_ROWS:
        return hk.codekx16_matmat(x, *L["args"])
    y = hk.codekx16_matmat_dequant(x, *L["args"])
    direct = hk.codekx16_matmat_rows(x, *L["args"])
    assert direct is not None and torch.equal(y, direct)   # the window is open: the wrapper ran the entry
    return y


@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
@pytest.mark.parametrize("inf,out", GEOMETRIES)
@pytest.mark.parametrize("K,nbits", SCHEMES)
def test_exact_operands_give_the_float64_result(hk, K, nbits, inf, out, dtype):
    L = layer(K, nbits, dtype, inf, out, True)
    for rows in GEMV_ROWS + FUSED_ROWS:
        y = run(hk, L, rows)
        assert torch.equal(y.cpu(), L["y64"][:rows].to(dtype)), f"{rows} rows"


@pytest.mark.parametrize("K,nbits,codes", [(2, 12, "high"), (2, 9, "high"), (2, 16, "negative"), (4, 16, "negative")])
def test_codes_are_masked_and_read_unsigned(hk, K, nbits, codes):
    L = layer(K, nbits, F16, 512, 40, True, codes)
    for rows in (3, 16):
        assert torch.equal(run(hk, L, rows).cpu(), L["y64"][:rows].to(F16)), f"{rows} rows"


@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
@pytest.mark.parametrize("inf,out", GEOMETRIES)
@pytest.mark.parametrize("K,nbits", SCHEMES)
def test_random_operands_within_the_derived_bound(hk, K, nbits, inf, out, dtype):
    """|y - y64| <= eps_T |y64| + (K in + 2) 2^-24 |s| sum |w| |x|: exact products, K in fp32 additions, one scale fma, one rounding."""
    L = layer(K, nbits, dtype, inf, out, False)
    for rows in (1, 6, 7, 64):
        y = run(hk, L, rows).cpu().double()
        bound = EPS[dtype] * L["y64"][:rows].abs() + (K * inf + 2) * 2.0 ** -24 * L["slack"][:rows]
        excess = ((y - L["y64"][:rows]).abs() - bound).max().item()
        print(f"{K}x{nbits} {inf}->{out} {dtype} rows {rows}: max(|err| - bound) = {excess:.3e}")
        assert excess <= 0, f"{rows} rows"


@pytest.mark.parametrize("K,nbits", [(2, 12), (4, 16)])
def test_rows_are_independent_and_a_row_stride_is_honoured(hk, K, nbits):
    L = layer(K, nbits, F16, 544, 16, False)
    y = run(hk, L, 64)
    for first, rows in ((0, 7), (13, 16), (50, 11)):   # row b of the 64-row call == the same row in a call of 7 .. 16 rows
        assert torch.equal(run(hk, L, rows, L["x"][first:first + rows]), y[first:first + rows])
    wide = torch.zeros(64, 544 + 8, dtype=F16, device="cuda")
    wide[:, :544] = L["x"][:64]
    view = wide[:, :544]
    assert not view.is_contiguous()
    assert torch.equal(run(hk, L, 64, view), y) and torch.equal(run(hk, L, 6, view[:6]), run(hk, L, 6))


def test_module_runs_on_the_new_functions(hk, monkeypatch):
    import aqlm

    L = layer(2, 12, F16, 512, 40, False)
    calls = {"gemv": 0, "gemm": 0}
    gemv, gemm = hk.codekx16_matmat, hk.codekx16_matmat_dequant
    monkeypatch.setattr(hk, "codekx16_matmat", lambda *a: (calls.__setitem__("gemv", calls["gemv"] + 1), gemv(*a))[1])
    monkeypatch.setattr(hk, "codekx16_matmat_dequant", lambda *a: (calls.__setitem__("gemm", calls["gemm"] + 1), gemm(*a))[1])
    m = aqlm.QuantizedLinear(512, 40, 8, 1, 2, 12, bias=True, dtype=F16)
    m.load_state_dict(dict(zip(("codes", "codebooks", "scales", "bias"), L["args"])))
    m = m.cuda()
    y1, y16 = m(L["x"][:1]), m(L["x"][:16])
    assert calls == {"gemv": 1, "gemm": 1}
    assert torch.equal(y1, gemv(L["x"][:1], *L["args"])) and torch.equal(y16, hk.codekx16_matmat_rows(L["x"][:16], *L["args"]))
    x = L["x"][:16].clone().requires_grad_(True)
    m(x).sum().backward()   # the backward stays on generic_matmat_dequant_transposed
    W = _dequantize_weight(unpack_int_data(L["args"][0], 12), L["args"][1], L["args"][2])
    want = W.double().sum(0)
    assert x.grad is not None and (x.grad.double() - want).abs().max() <= 2.0 ** -8 * want.abs().max()
    monkeypatch.setattr(hk, "FUSED_KX16_MAX_ROWS", 0)   # outside the window: today's route, bit for bit
    assert torch.equal(m(L["x"][:16]), hk.generic_matmat_dequant(L["x"][:16], *L["args"]))
    assert calls == {"gemv": 1, "gemm": 3}
