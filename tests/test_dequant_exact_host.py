"""The arithmetic contract of the dequantise kernels, pinned on the host before any kernel is held to it.

``orc.dequantize_weight_storage`` restates the contract: per weight, the selected codebook entries summed in
float32 in codebook order, times the float32 scale, ONE round-to-nearest-even into fp16 / bf16.  tests/test_dequant_exact_gpu.py
compares the kernels with it bit for bit; here it is tied to three independent anchors, none of which shares its code:

  * the fp32 C oracle (oracle/aqlm_oracle.c), rounded to storage: bit for bit, every scheme -- the 5-bit and 12-bit ones need the
    C oracle to mask its codes to ``nbits`` (an index >= 2**(nbits-1) sits negative in its container);
  * the fp64 oracle: for one codebook the fp32 product of two storage values is exact, so the result IS the correctly rounded fp64
    value; for several codebooks the fp32 sum adds at most K * 2**-24 * |scale| * sum_c |entry_c| before the one rounding;
  * the reference project's own fp32 weights (tests/golden, ``W_ref32``), rounded to storage.
"""
import numpy as np
import pytest

from oracle import aqlm_oracle as orc
from oracle import c_oracle
from tests.test_oracle_golden import meanrel, regen

SCHEMES = [(1, 16, 8), (1, 16, 16), (2, 8, 8), (1, 8, 8), (8, 8, 32), (4, 8, 16), (3, 5, 8), (1, 12, 8)]
DTYPES = ["float16", "bfloat16"]
OUT, IN_GROUPS = 37, 65   # rows and groups per row that are no multiple of anything


def np_dtype(dt):
    return np.float16 if dt == "float16" else "bfloat16"


def ulp_storage(a, dt):
    """Spacing of the storage type's values at |a| (subnormal spacing below the normal range)."""
    mant, emin = (10, -14) if dt == "float16" else (7, -126)
    _, e = np.frexp(np.abs(np.asarray(a, dtype=np.float64)))   # |a| = m * 2**e, 0.5 <= m < 1: floor(log2 |a|) = e - 1
    return np.ldexp(1.0, np.maximum(e - 1, emin) - mant)


def ordered(bits):
    """uint16 sign-magnitude patterns -> integers in the order of the values they denote (+0 and -0 coincide)."""
    b = bits.astype(np.int32)
    return np.where(b & 0x8000, -(b & 0x7FFF), b & 0x7FFF)


_layers = {}


def layer(K, nbits, g, dt):
    key = (K, nbits, g, dt)
    if key not in _layers:
        _layers[key] = orc.make_layer(4100 + 7 * K + nbits + g, g * IN_GROUPS, OUT, K, nbits, g, batch=1, bias=False,
                                      float_dtype=np_dtype(dt))
    return _layers[key]


@pytest.mark.parametrize("scaled", [True, False])
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("K,nbits,g", SCHEMES)
def test_restatement_equals_c_oracle_rounded_to_storage(K, nbits, g, dt, scaled):
    L = layer(K, nbits, g, dt)
    scales = L["scales"] if scaled else None
    bits = orc.dequantize_weight_storage(L["codes_unsigned"], L["codebooks"], scales, np_dtype(dt))
    assert bits.dtype == np.uint16 and bits.shape == (OUT, g * IN_GROUPS)
    Wc = c_oracle.dequant_weight(L["codebooks"], L["codes"], scales, nbits)   # fp32, from the signed containers
    assert Wc.dtype == np.float32
    want = orc.round_to_storage_bits(Wc, np_dtype(dt))
    diff = bits != want
    assert not diff.any(), f"{K}x{nbits}g{g} {dt}: {diff.sum()} of {diff.size} weights differ from the C oracle, first at {np.argwhere(diff)[0]}"


@pytest.mark.parametrize("K,nbits,g", [(3, 5, 8), (1, 12, 8)])
def test_c_oracle_gemv_entries_mask_their_codes(K, nbits, g):
    """``DequantGemv`` and ``LutGemv`` read the same signed containers as ``dequant_weight``: below the container's width they
    index past the codebook unless they mask to ``nbits``.  Bound: the one tests/test_oracle_golden.py holds them to at 8 / 16 bits."""
    L = layer(K, nbits, g, "float16")
    y64 = orc.dequantize_gemm(L["x"], L["codes"], L["codebooks"], L["scales"], None)[0]
    d = c_oracle.DequantGemv(L["codebooks"], L["codes"], L["scales"], None, nbits, nthreads=1)
    k = c_oracle.LutGemv(L["codebooks"], orc.permute_codes_for_lut(L["codes"]), L["scales"], nbits, nthreads=1)
    for what, y in (("DequantGemv", d(L["x"][0]).copy()), ("LutGemv", k(L["x"][0]).copy())):
        assert meanrel(y, y64) < 2e-5, what


@pytest.mark.parametrize("scaled", [True, False])
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("K,nbits,g", [s for s in SCHEMES if s[0] == 1])
def test_one_codebook_is_the_correctly_rounded_fp64_weight(K, nbits, g, dt, scaled):
    """entry * scale with 11-bit (fp16) or 8-bit (bf16) significands is exact in fp32: one rounding, the same as from fp64."""
    L = layer(K, nbits, g, dt)
    scales = L["scales"] if scaled else None
    bits = orc.dequantize_weight_storage(L["codes_unsigned"], L["codebooks"], scales, np_dtype(dt))
    W64 = orc.dequantize_weight(L["codes_unsigned"], L["codebooks"], scales)
    np.testing.assert_array_equal(bits, orc.round_to_storage_bits(W64, np_dtype(dt)))


@pytest.mark.parametrize("scaled", [True, False])
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("K,nbits,g", [s for s in SCHEMES if s[0] > 1])
def test_several_codebooks_within_the_derived_bound_of_fp64(K, nbits, g, dt, scaled):
    """One storage rounding plus the fp32 summation error: each of the K - 1 additions and the multiplication rounds a value of at
    most sum_c |entry_c| (times |scale|) by at most 2**-24 of it.  Cancellation can make that more than an ulp of a tiny result."""
    L = layer(K, nbits, g, dt)
    scales = L["scales"] if scaled else None
    bits = orc.dequantize_weight_storage(L["codes_unsigned"], L["codebooks"], scales, np_dtype(dt))
    W64 = orc.dequantize_weight(L["codes_unsigned"], L["codebooks"], scales)
    sum_abs = orc.dequantize_weight(L["codes_unsigned"], np.abs(L["codebooks"].astype(np.float64)), None)
    s = np.abs(L["scales"].astype(np.float64)).reshape(-1, 1) if scaled else 1.0
    bound = ulp_storage(W64, dt) + K * 2.0**-24 * s * sum_abs
    err = np.abs(orc.storage_bits_to_float64(bits, np_dtype(dt)) - W64)
    share = float(np.mean(bits == orc.round_to_storage_bits(W64, np_dtype(dt))))
    bad = err > bound
    assert not bad.any(), (f"{K}x{nbits}g{g} {dt}: {bad.sum()} weights outside the bound, worst excess {np.max(err - bound):.3g}; "
                           f"{share:.4%} of the weights equal the rounded fp64 value")


GOLDEN = ["c1x16g8_f16", "c1x16g8_f16_nobias", "c1x16g16_f16", "c1x16g8_bf16", "c2x8g8_f16", "c2x8g8_bf16",
          "c1x8g8_f16", "c8x8g32_f16", "c4x8g16_f16"]


@pytest.mark.parametrize("name", GOLDEN)
def test_restatement_against_the_reference_weights(golden, name):
    """``W_ref32`` is the reference project's own fp32 ``_dequantize_weight``; rounded to storage it is the restatement, up to the
    last place where the reference summed in another order, and exactly for one codebook."""
    L, cfg = regen(golden, name)
    dt = cfg["dtype"]
    bits = orc.dequantize_weight_storage(L["codes_unsigned"], L["codebooks"], L["scales"], np_dtype(dt))
    Wref = golden[f"{name}/W_ref32"]
    assert Wref.dtype == np.float32 and Wref.shape == bits.shape
    want = orc.round_to_storage_bits(Wref, np_dtype(dt))
    steps = np.abs(ordered(bits) - ordered(want))   # 1 = neighbouring storage values
    assert steps.max() <= 1, f"{name}: {np.sum(steps > 1)} weights more than one storage ulp from the reference's"
    if cfg["K"] == 1:
        np.testing.assert_array_equal(bits, want)


def test_rounding_helpers_on_known_patterns():
    """The two roundings the comparisons above lean on, on values whose result is known by hand."""
    f16 = lambda *v: orc.round_to_storage_bits(np.array(v, dtype=np.float64), np.float16).tolist()
    b16 = lambda *v: orc.round_to_storage_bits(np.array(v, dtype=np.float64), "bfloat16").tolist()
    assert f16(1.0, -0.0, 1 + 2.0**-11, 1 + 3 * 2.0**-11, 65520.0, 2.0**-24, 2.0**-25) == [0x3C00, 0x8000, 0x3C00, 0x3C02, 0x7C00, 1, 0]
    assert b16(1.0, -0.0, 1 + 2.0**-8, 1 + 3 * 2.0**-8, 2.0**-133, 2.0**-134, -(2.0**-134 + 2.0**-150)) == [0x3F80, 0x8000, 0x3F80, 0x3F82, 1, 0, 0x8001]
    assert b16(1 + 2.0**-8 + 2.0**-40) == [0x3F81]                    # a double rounding through float32 would give 0x3f80
    assert b16(float(np.float32(3.3895314e38)), 3.4e38) == [0x7F7F, 0x7F80]
    cb = np.zeros((1, 256, 1, 8), dtype=np.float32)
    cb[0, 1] = [np.inf, -np.inf, np.nan, -0.0, 0.0, 1.0, 65520.0, 2.0**-25]
    codes = np.array([[[1]]])
    for dt, want in (("float16", [0x7C00, 0xFC00, 0x7E00, 0x0000, 0x0000, 0x3C00, 0x7C00, 0x0000]),
                     ("bfloat16", [0x7F80, 0xFF80, 0x7FC0, 0x0000, 0x0000, 0x3F80, 0x4780, 0x3300])):
        assert orc.dequantize_weight_storage(codes, cb, None, np_dtype(dt))[0].tolist() == want, dt
    neg = orc.dequantize_weight_storage(codes, cb, np.full((1, 1, 1, 1), -1.0, dtype=np.float32), np.float16)[0].tolist()
    assert neg[3:5] == [0x8000, 0x8000]   # 0 + (-0) = +0, then +0 * -1 = -0
