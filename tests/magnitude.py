"""Layers at the magnitudes of real checkpoints, and at the bottom of the fp16 range, for the forward kernels.  Numpy only, no
device.  Test infrastructure.

``oracle.aqlm_oracle.make_layer`` draws codebooks, scales, x and bias from N(0, 1): every operand of every forward test sits at
exponent 0.  ``regime_layer`` starts from the same layer and moves each operand by a power of two (a *shift* of n multiplies
by 2**n), rounds it into the storage type where it lives, and returns it beside its TWIN:

    twin = (codebooks * 2**b, x * 2**-a, scales * 2**(a - b)), same codes, same bias

The real-valued result of layer and twin is the same number.  Every hand-written forward route forms exact fp16 / bf16
products, sums them in fp32 and rounds once, so as long as nothing under- or overflows every
intermediate of the two runs differs by an exact power of two and the outputs are equal BIT FOR BIT -- the fixed-point cells of
the fused finalizes included, whose unit comes from frexp of max|x| * max|codebook| and so moves by the same exponent.  A
kernel that flushes a subnormal operand, keeps an intermediate in half precision or carries an absolute constant breaks the
equality; no tolerance is involved.

Of each pair of values (layer, twin) the one of LOWER magnitude is rounded into the storage type first and the other is derived
from it by an exact up-shift: shifting up loses no bits below overflow, shifting down does.

The helper asserts its own preconditions (``_check``), so a test cannot pass on the wrong input."""
import functools

import numpy as np

from oracle import aqlm_oracle as orc

REGIMES = ("checkpoint", "small_normal", "sub_codebook", "sub_x", "outlier")
MIN_NORMAL_F16 = 2.0 ** -14
# the mean-relative bounds of tests/test_hip_parity.py::check_close, restated because this module imports neither torch nor a GPU
# test; tests/test_magnitude_host.py holds the restatement to check_close itself (it passes just below and fails just above)
CHECK_CLOSE_MEAN = {"float16": 1e-3, "bfloat16": 8e-3}
OUTLIER = 2048.0


def regime_dtypes(regime):
    """The storage types a regime exists in.  There is no bf16 subnormal regime: a bf16 subnormal is ~1e-38, no checkpoint
    reaches it."""
    return ("float16",) if regime in ("sub_codebook", "sub_x") else ("float16", "bfloat16")


def regime_shifts(regime, K, dtype):
    """-> dict(cb=[shift of codebook k], x=, sc=, b=, a=): the layer's shifts and the twin's (b, a); b = a = None without a twin.
    The twin's shifts are cb + b, x - a, sc + a - b."""
    assert regime in REGIMES and dtype in regime_dtypes(regime), (regime, dtype)
    if regime in ("checkpoint", "outlier"):
        # row-normalised weights: the scales carry the row norm, entries sit near 1 / sqrt(in_features); every further codebook
        # of a residual scheme is smaller again
        s = dict(cb=[-6 - k for k in range(K)] if K > 1 else [-6], x=0, sc=3 if K == 1 else 0, b=6, a=0)
        if regime == "outlier":
            s["b"] = s["a"] = None   # no twin beyond checkpoint's
        return s
    if regime == "small_normal":
        if dtype == "float16":
            return dict(cb=[-12] * K, x=6, sc=6, b=12, a=6)
        return dict(cb=[-40] * K, x=20, sc=20, b=40, a=20)   # every product and partial sum stays above 2**-100
    if regime == "sub_codebook":
        if K == 1:
            return dict(cb=[-14], x=7, sc=7, b=14, a=7)
        if K == 8:
            return dict(cb=[-8 - k for k in range(8)], x=4, sc=4, b=8, a=4)
        return dict(cb=[-13] * K, x=7, sc=7, b=13, a=7)
    if K == 8:  # sub_x
        return dict(cb=[4] * 8, x=-14, sc=10, b=-4, a=-14)
    return dict(cb=[6] * K, x=-14, sc=8, b=-6, a=-14)


def subnormal_share_floor(regime, K):
    """The least share of fp16 subnormals among the non-zero entries of the shifted operand of a ``sub_*`` regime: a half at a
    shift of -14 (P(|N(0,1)| < 1) = 0.68), a quarter for the K-codebook schemes' codebooks (0.38 at -13, 0.30 at -8 - k)."""
    return 0.5 if regime == "sub_x" or K == 1 else 0.25


def _round(a, dtype):
    a = np.ascontiguousarray(a, dtype=np.float32)
    if dtype == "bfloat16":
        return orc.round_to_bf16(a)
    with np.errstate(over="ignore"):
        return a.astype(np.float16).astype(np.float32)


def is_f16_subnormal(a):
    a = np.abs(np.asarray(a, dtype=np.float32))
    return (a > 0) & (a < MIN_NORMAL_F16)


def flush_f16_subnormals(a):
    """A copy with every fp16 subnormal set to +0: what a kernel that flushes the operand computes with."""
    a = np.array(a, dtype=np.float32, copy=True)
    a[is_f16_subnormal(a)] = 0.0
    return a


def _pair(base, lo, hi, dtype, no_subnormals):
    """-> (base * 2**lo rounded into the storage type, that times 2**(hi - lo)): the low side first, the high side by an exact
    up-shift."""
    assert lo <= hi
    low = _round(np.ldexp(np.asarray(base, dtype=np.float32), lo), dtype)
    if no_subnormals:
        low = flush_f16_subnormals(low)
    high = np.ldexp(low, hi - lo).astype(np.float32)
    return low, high


def _shifted(base, s_layer, s_twin, dtype, no_subnormals):
    """base at the layer's shift and at the twin's -> (layer values, twin values), float32 arrays of storage-type values."""
    if s_twin is None:
        return _pair(base, s_layer, s_layer, dtype, no_subnormals)[0], None
    low, high = _pair(base, min(s_layer, s_twin), max(s_layer, s_twin), dtype, no_subnormals)
    return (low, high) if s_layer <= s_twin else (high, low)


def oracle(L):
    return orc.dequantize_gemm(L["x"], L["codes"], L["codebooks"], L["scales"], L["bias"])


def flushed_copy(L, regime):
    """The layer a kernel sees that flushes the fp16 subnormals of the regime's shifted operand."""
    key = "codebooks" if regime == "sub_codebook" else "x"
    return dict(L, **{key: flush_f16_subnormals(L[key])})


def _check(regime, K, dtype, L, twin):
    """The builder's preconditions.  Conditions, not measurements: an input that misses one is the wrong input."""
    for D in (L, twin):
        if D is None:
            continue
        for k in ("codebooks", "scales", "x", "bias"):   # every value round-trips through the storage type exactly
            if D[k] is not None:
                assert D[k].dtype == np.float32 and np.isfinite(D[k]).all() and np.array_equal(_round(D[k], dtype), D[k]), (regime, k)
        y = D["y64"]
        assert np.isfinite(y).all() and (dtype != "float16" or np.abs(y).max() < 6e4), (regime, float(np.abs(y).max()))
    if twin is not None:
        # the same real number: the two fp64 oracles run the same operations on operands moved by exact powers of two, so they
        # agree to the round-off of an fp64 sum of in_features terms (in practice exactly).  A sanity check of the builder, not a
        # tolerance on any kernel.
        fin = L["x"].shape[1]
        assert np.abs(L["y64"] - twin["y64"]).max() <= fin * np.finfo(np.float64).eps * np.abs(L["y64"]).max(), regime
    if regime == "small_normal" and dtype == "float16":   # exponent handling alone: no subnormal operand on either side
        for D in (L, twin):
            assert not any(is_f16_subnormal(D[k]).any() for k in ("codebooks", "scales", "x")), regime
    if regime in ("sub_codebook", "sub_x"):
        op = L["codebooks" if regime == "sub_codebook" else "x"]
        share = float(is_f16_subnormal(op).sum()) / float((op != 0).sum())
        assert share >= subnormal_share_floor(regime, K), (regime, K, share)
        y, yf = L["y64"], oracle(flushed_copy(L, regime))
        cost = float(np.abs(y - yf).mean() / np.abs(y).mean())
        assert cost >= 10 * CHECK_CLOSE_MEAN[dtype], (regime, K, cost)   # a flush could not hide inside check_close
        L["subnormal_share"], L["flush_cost"] = share, cost


@functools.lru_cache(maxsize=None)
def regime_layer(regime, seed, fin, fout, K, nbits, g, rows, dtype, bias=True):
    """``make_layer(seed, fin, fout, K, nbits, g, batch=rows, bias=bias)`` at the magnitudes of ``regime`` in storage type ``dtype``
    ("float16" | "bfloat16") -> (layer, twin): dicts as ``make_layer`` returns them, fp32 arrays of exactly representable values,
    plus ``y64`` (the fp64 oracle on the stored values) and ``shifts``.  ``twin`` is None in ``outlier``.  Shared between the tests
    that ask for the same layer: leave both unchanged."""
    base = orc.make_layer(seed, fin, fout, K, nbits, g, batch=rows, bias=bias, float_dtype=np.float16 if dtype == "float16" else "bfloat16")
    s = regime_shifts(regime, K, dtype)
    has_twin = s["b"] is not None
    clean = regime == "small_normal" and dtype == "float16"   # there every |entry| < 2**-14 is set to +0
    xb = base["x"].copy()
    if regime == "outlier":   # massive activations: two entries per row thousands of times larger than the rest
        rng = np.random.default_rng(seed + 0x0071)
        for r in range(rows):
            i, j = rng.choice(fin, size=2, replace=False)
            xb[r, i], xb[r, j] = OUTLIER, -OUTLIER
    cbs = [_shifted(base["codebooks"][k], s["cb"][k], s["cb"][k] + s["b"] if has_twin else None, dtype, clean) for k in range(K)]
    x = _shifted(xb, s["x"], s["x"] - s["a"] if has_twin else None, dtype, clean)
    sc = _shifted(base["scales"], s["sc"], s["sc"] + s["a"] - s["b"] if has_twin else None, dtype, clean)
    out = []
    for side in (0, 1):
        if side == 1 and not has_twin:
            out.append(None)
            continue
        D = dict(base, codebooks=np.stack([c[side] for c in cbs]), x=x[side], scales=sc[side], shifts=s,
                 bias=None if base["bias"] is None else base["bias"].astype(np.float32))
        D["y64"] = oracle(D)
        out.append(D)
    L, twin = out
    _check(regime, K, dtype, L, twin)
    return L, twin


# The forward routes of tests/test_magnitude_gpu.py at their smallest shapes: name -> (K, nbits, g, fin, fout, rows).  The host
# test holds the builder's conditions on every one of them in every regime and storage type the GPU test runs.
LAYERS = {
    "1x16g8_512x64": (1, 16, 8, 512, 64, 8),
    "1x16g16_1024x64": (1, 16, 16, 1024, 64, 8),
    "1x16g8_1024x256": (1, 16, 8, 1024, 256, 8),
    "1x16g16_2048x256": (1, 16, 16, 2048, 256, 8),
    "1x8g8_1024x128": (1, 8, 8, 1024, 128, 1),
    "2x8g8_1024x128": (2, 8, 8, 1024, 128, 1),
    "8x8g32_2048x72": (8, 8, 32, 2048, 72, 8),
    "8x8g8_1024x64": (8, 8, 8, 1024, 64, 8),
    "1x16g8_512x48": (1, 16, 8, 512, 48, 32),
    "1x16g16_1024x64_b20": (1, 16, 16, 1024, 64, 20),
    "1x16g8_1024x64_b5": (1, 16, 8, 1024, 64, 5),
    "2x8g8_384x64": (2, 8, 8, 384, 64, 16),
    "2x8g8_640x48": (2, 8, 8, 640, 48, 100),
    "2x8g8_384x40": (2, 8, 8, 384, 40, 16),
    "8x8g32_2304x72": (8, 8, 32, 2304, 72, 3),
    "8x8g32_2048x200": (8, 8, 32, 2048, 200, 64),
    "3x5g8_512x40": (3, 5, 8, 512, 40, 2),
}
# One fixed seed per layer, so that adding a layer moves nobody else's input.  The (T) outcomes of the ``sub_*`` cases on the GPU
# depend on them (tests/test_magnitude_gpu.py: with subnormal operands a handful of outputs may sit one ulp from the twin's, by
# the seed's luck): changing a seed may flip such a case without any kernel having changed.
# The cost of a flush in the 8 x 8 schemes (codebook k at -8 - k) is 0.0095 .. 0.012 over the seeds, around the condition's
# 0.01: those four layers take a seed that meets it (the condition decides, `_check` asserts it).
SEEDS = {"1x16g8_512x64": 20256, "1x16g16_1024x64": 20250, "1x16g8_1024x256": 20253, "1x16g16_2048x256": 20252,
         "1x8g8_1024x128": 20257, "2x8g8_1024x128": 20258, "8x8g32_2048x72": 20261, "8x8g8_1024x64": 20259,
         "1x16g8_512x48": 20255, "1x16g16_1024x64_b20": 20251, "1x16g8_1024x64_b5": 20254, "2x8g8_384x64": 20260,
         "2x8g8_640x48": 20261, "2x8g8_384x40": 20259, "8x8g32_2304x72": 20259, "8x8g32_2048x200": 20251, "3x5g8_512x40": 20262}
assert set(SEEDS) == set(LAYERS)


def cases():
    """Every (layer name, regime, dtype) of the suite."""
    return [(n, r, d) for n in LAYERS for r in REGIMES for d in regime_dtypes(r)]


def layer(name, regime, dtype):
    K, nbits, g, fin, fout, rows = LAYERS[name]
    return regime_layer(regime, SEEDS[name], fin, fout, K, nbits, g, rows, dtype, True)
