"""The magnitude regimes of tests/magnitude.py on the host: the builder's conditions for every layer the GPU suite runs
(tests/test_magnitude_gpu.py), the twin statement on the numpy restatement of the arithmetic contract, and on the CPU kernels
of libaqlm_cpu.so.  Runs without a GPU.

The twin statement: (codebooks * 2**b, x * 2**-a, scales * 2**(a - b)) is the same real-valued layer, and arithmetic that forms
exact products, sums in fp32 and rounds once gives the same BITS for both, as long as nothing under- or overflows.  No tolerance."""
import numpy as np
import pytest

from oracle import aqlm_oracle as orc
from tests import magnitude as mg

torch = pytest.importorskip("torch")

from aqlm_amd.inference_kernels import cpu_kernel  # noqa: E402
from tests.test_hip_parity import check_close  # noqa: E402  (imports without a GPU; its tests are marked gpu)


@pytest.mark.parametrize("dtype", ["float16", "bfloat16"])
def test_the_restated_mean_bound_is_check_closes(dtype):
    """``magnitude.CHECK_CLOSE_MEAN`` (the builder's "ten times check_close's mean bound") against check_close itself: an output
    off by just less than the restated bound passes, one off by just more fails on the mean."""
    td = torch.float16 if dtype == "float16" else torch.bfloat16
    y64, b = np.ones(64), mg.CHECK_CLOSE_MEAN[dtype]
    check_close(y64 * (1 + 0.999 * b), y64, td, "just inside")
    with pytest.raises(AssertionError, match="mean-rel"):
        check_close(y64 * (1 + 1.001 * b), y64, td, "just outside")


def _fd(dtype):
    return np.float16 if dtype == "float16" else "bfloat16"


def _contract_bits(L, dtype):
    """The forward routes' contract in numpy: the selected entries of the codebooks added in fp32 in codebook order (W is never
    rounded: the matvec and fused-GEMM kernels do not materialise it), an fp32 dot with x, ``acc * scale + bias`` in fp32, one
    rounding into the storage type -> uint16 bit patterns."""
    cb = L["codebooks"].astype(np.float32)
    cu = L["codes_unsigned"]
    acc = np.zeros(cu.shape[:2] + cb.shape[2:], dtype=np.float32)
    for k in range(cb.shape[0]):
        acc += cb[k][cu[..., k]]
    W = acc.swapaxes(-3, -2).reshape(cu.shape[0] * cb.shape[2], cu.shape[1] * cb.shape[3])
    y = np.stack([(W * row[None, :]).sum(axis=1, dtype=np.float32) for row in L["x"].astype(np.float32)])   # exact products, fp32 sums
    y = y * L["scales"].reshape(1, -1).astype(np.float32)
    if L["bias"] is not None:
        y = y + L["bias"].astype(np.float32)
    assert y.dtype == np.float32
    return orc.round_to_storage_bits(y, _fd(dtype))


@pytest.mark.parametrize("name,regime,dtype", mg.cases())
def test_builder_conditions_and_the_contract_on_the_twin(name, regime, dtype):
    """``layer`` asserts the builder's conditions itself (round-trips, finite oracle below 6e4, subnormal share, the cost of a
    flush); here they are held for every case of the GPU suite, and the numpy contract gives equal bits on layer and twin."""
    K = mg.LAYERS[name][0]
    L, twin = mg.layer(name, regime, dtype)
    s = mg.regime_shifts(regime, K, dtype)
    assert L["shifts"] == s and (twin is None) == (regime == "outlier")
    if regime in ("sub_codebook", "sub_x"):
        assert L["subnormal_share"] >= mg.subnormal_share_floor(regime, K) and L["flush_cost"] >= 10 * mg.CHECK_CLOSE_MEAN[dtype]
    if regime == "outlier":
        # two outliers per row and nothing else out of the ordinary (builder sanity: N(0, 1) draws stay below 8, P = 1e-15 each)
        assert ((np.abs(L["x"]) == mg.OUTLIER).sum(axis=1) == 2).all() and ((np.abs(L["x"]) > 8).sum(axis=1) == 2).all()
        return
    assert np.array_equal(L["codes"], twin["codes"]) and np.array_equal(L["bias"], twin["bias"])
    for k in range(K):   # the twin is the layer moved by exact powers of two
        assert np.array_equal(np.ldexp(L["codebooks"][k], s["b"]), twin["codebooks"][k])
    assert np.array_equal(np.ldexp(twin["x"], s["a"]), L["x"]) and np.array_equal(np.ldexp(L["scales"], s["a"] - s["b"]), twin["scales"])
    assert np.array_equal(_contract_bits(L, dtype), _contract_bits(twin, dtype)), "the numpy contract is not magnitude-independent"
    if s["a"] == 0 and not mg.is_f16_subnormal(L["codebooks"]).any():
        # W itself (rounded into the storage type, as the dequantise kernels give it) is the same matrix where x is not moved and
        # no entry loses bits on the way down: W_twin = W * 2**a
        args = (L["codes_unsigned"], L["codebooks"], L["scales"]), (twin["codes_unsigned"], twin["codebooks"], twin["scales"])
        assert np.array_equal(orc.dequantize_weight_storage(*args[0], _fd(dtype)), orc.dequantize_weight_storage(*args[1], _fd(dtype)))


def test_a_flush_breaks_the_twin_statement():
    """What the suite is for: zero the subnormals of one side (what a flushing kernel computes with) and the bits differ."""
    for name, regime in (("1x16g8_512x64", "sub_codebook"), ("2x8g8_384x64", "sub_codebook"), ("8x8g32_2304x72", "sub_codebook"),
                         ("1x16g8_512x64", "sub_x"), ("8x8g32_2304x72", "sub_x")):
        L, twin = mg.layer(name, regime, "float16")
        flushed = _contract_bits(mg.flushed_copy(L, regime), "float16")
        # (a sanity floor, not a tolerance: a flush moves the result by 1e-2 .. 0.5 of its size -- `flush_cost` --, many fp16 ulps,
        # so nearly every output changes; half of them is a loose statement of "not a few")
        assert (flushed != _contract_bits(twin, "float16")).mean() > 0.5, (name, regime)


def _t(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dtype)


@pytest.mark.parametrize("name,regime", [(n, r) for n in ("1x16g8_512x64", "1x16g16_1024x64", "1x8g8_1024x128") for r in mg.REGIMES[:4]])
def test_cpu_gemv_1xn_on_the_twin(name, regime):
    """The direct CPU kernel (fp16 codebook table, fp32 arithmetic): close to the oracle and equal bits on layer and twin."""
    ys = []
    for D in mg.layer(name, regime, "float16"):
        y = cpu_kernel.cpu_gemv_1xn(_t(D["x"], torch.float16), torch.from_numpy(D["codes"]), _t(D["codebooks"], torch.float16),
                                    _t(D["scales"], torch.float16), _t(D["bias"], torch.float16), nthreads=1)
        check_close(y.double().numpy(), D["y64"], torch.float16, f"{name} {regime}")
        ys.append(y)
    assert torch.equal(ys[0], ys[1]), f"{name} {regime}: the CPU kernel is not magnitude-independent"


@pytest.mark.parametrize("name,regime", [(n, r) for n in ("1x8g8_1024x128", "2x8g8_1024x128", "8x8g32_2048x72", "8x8g8_1024x64")
                                         for r in mg.REGIMES[:4]])
def test_cpu_gemm_lut_on_the_twin(name, regime):
    """The CPU look-up-table kernel: per-row tables of x . codebook entry in fp32, summed over the codes."""
    ys = []
    for D in mg.layer(name, regime, "float16"):
        alt = cpu_kernel.permute_codes_for_lut(torch.from_numpy(D["codes"]))
        y = cpu_kernel.cpu_gemm_lut(_t(D["x"], torch.float16), alt, _t(D["codebooks"], torch.float16), _t(D["scales"], torch.float16),
                                    _t(D["bias"], torch.float16), nthreads=1)
        check_close(y.double().numpy(), D["y64"], torch.float16, f"{name} {regime}")
        ys.append(y)
    assert torch.equal(ys[0], ys[1]), f"{name} {regime}: the CPU kernel is not magnitude-independent"
