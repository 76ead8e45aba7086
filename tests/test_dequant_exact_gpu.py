"""The dequantise kernels (aqlm_hip_dequant_1x16 / _kx8 / _generic, csrc/dequant.hip) held to their arithmetic contract on the
MI355X, bit for bit: W's bit patterns equal ``orc.dequantize_weight_storage`` -- the selected codebook entries summed in float32 in
codebook order, times the float32 scale, one round-to-nearest-even into fp16 / bf16 -- which tests/test_dequant_exact_host.py ties
to the C oracle, the fp64 oracle and the reference project's weights.  No tolerance is chosen anywhere in (a)-(e):

  (a) small shapes where indexing goes wrong, every entry point, every instance and the generic route;
  (b) one shape per instance just past its block cap, so that the grid-stride loop runs a second, partial pass;
  (c) ``force_generic`` on the tuned entries;
  (d) misaligned W / codebook / codes through the raw C ABI, with sentinels around W;
  (e) results on subnormals, signed zeros, infinities and exact ties.

(f) holds the ops built on W -- the transposed (backward) ops and the dequantise + library-GEMM forwards -- to the suite's
``check_close`` bounds against the fp64 product with the RESTATED storage W: what is left is the library GEMM's accumulation and
the output roundings.  The GEMM is the library's; nothing bit-exact is claimed about it."""
import numpy as np
import pytest

from oracle import aqlm_oracle as orc
from tests.test_hip_parity import DEV, check_close, tdtype, to_dev

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

DTYPES = ["float16", "bfloat16"]


@pytest.fixture(scope="module")
def hk():
    assert torch.cuda.is_available(), "run with -m gpu on the MI355X box"
    from aqlm_amd.inference_kernels import hip_kernel

    return hip_kernel


def np_dtype(dt):
    return np.float16 if dt == "float16" else "bfloat16"


def restated(L, dt, scaled=True):
    return orc.dequantize_weight_storage(L["codes_unsigned"], L["codebooks"], L["scales"] if scaled else None, np_dtype(dt))


def assert_bits(W, bits, what):
    """W (fp16 / bf16 on the device) has the bit patterns `bits` (uint16, host); a NaN must be a NaN, its payload is free."""
    assert tuple(W.shape) == bits.shape, (what, tuple(W.shape), bits.shape)
    got = W.contiguous().view(torch.int16)
    want = torch.from_numpy(bits.view(np.int16)).to(W.device)
    want_nan = torch.from_numpy((bits & 0x7FFF) > (0x7C00 if W.dtype == torch.float16 else 0x7F80)).to(W.device)
    nan = torch.isnan(W)
    assert torch.equal(nan, want_nan), f"{what}: NaNs at other places than the contract's"
    if bool(nan.any()):
        got, want = got.masked_fill(nan, 0), want.masked_fill(nan, 0)
    if not torch.equal(got, want):
        bad = (got != want).nonzero()
        r, c = [int(v) for v in bad[0]]
        raise AssertionError(f"{what}: {bad.shape[0]} of {got.numel()} weights differ from the contract, first at [{r}, {c}]: "
                             f"got 0x{int(got[r, c]) & 0xFFFF:04x}, want 0x{int(want[r, c]) & 0xFFFF:04x}")


def entries_for(hk, K, nbits):
    """The dequantise ops that take the scheme: its own entry and the generic one."""
    ops = [("generic_dequant", hk.generic_dequant)]
    if nbits == 16 and K == 1:
        ops.append(("code1x16_dequant", hk.code1x16_dequant))
    elif nbits == 8:
        ops.append(("code1x8_dequant", hk.code1x8_dequant) if K == 1 else ("code2x8_dequant", hk.code2x8_dequant))
    return ops


def check_layer(hk, L, K, nbits, dt, what, ops=None):
    T = to_dev(L, tdtype(dt))
    for scaled in (True, False):
        bits = restated(L, dt, scaled)
        for name, op in (ops or entries_for(hk, K, nbits)):
            W = op(T["codes"], T["codebooks"], T["scales"] if scaled else None)
            assert W.dtype == tdtype(dt)
            assert_bits(W, bits, f"{name} {what} {dt} scaled={scaled}")
    return T


# ------------------------------------------------------------------ (a) small shapes
TUNED = [(1, 16, 8), (1, 16, 16), (1, 8, 8), (2, 8, 8), (8, 8, 32)]         # L2-gather and LDS-codebook instances
UNTUNED = [(4, 8, 16), (2, 8, 16), (2, 8, 4), (3, 5, 8), (1, 12, 8)]        # the generic kernel, through the kx8 / generic entries
# (out, in_groups): one row; rows that end inside a wave (65 groups: t / in_groups changes within 64 lanes) with a partial last
# block; a single group per row
SMALL = [(1, 65), (37, 65), (37, 1)]


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("out,in_groups", SMALL)
@pytest.mark.parametrize("K,nbits,g", TUNED + UNTUNED)
def test_small_shapes_bit_exact(hk, K, nbits, g, out, in_groups, dt):
    L = orc.make_layer(300 + 11 * K + nbits + g + out + in_groups, g * in_groups, out, K, nbits, g, batch=1, bias=False,
                       float_dtype=np_dtype(dt))
    assert L["scales"].shape == (out, 1, 1, 1)   # the ops take the checkpoint's 4-D scales
    check_layer(hk, L, K, nbits, dt, f"{K}x{nbits}g{g} {g * in_groups}->{out}")


@pytest.mark.parametrize("dt", DTYPES)
def test_generic_dequant_scales_4d_and_flat(hk, dt):
    """`generic_dequant` flattens its scales: [out, 1, 1, 1] (a checkpoint's) and [out] give the same, contract, bits."""
    L = orc.make_layer(331, 8 * 65, 37, 3, 5, 8, batch=1, bias=False, float_dtype=np_dtype(dt))
    T = to_dev(L, tdtype(dt))
    bits = restated(L, dt)
    assert T["scales"].dim() == 4
    assert_bits(hk.generic_dequant(T["codes"], T["codebooks"], T["scales"]), bits, "4-D scales")
    assert_bits(hk.generic_dequant(T["codes"], T["codebooks"], T["scales"].reshape(-1)), bits, "flat scales")


# ------------------------------------------------------------------ (b) past the block cap: second, partial grid-stride pass
# launch_dequant / run_dequant_generic (csrc/dequant.hip): at most 256 * 32 blocks of 256 threads for the L2-gather instances and the
# generic kernel (2,097,152 groups per pass), 256 * 8 blocks of 256 for an LDS codebook of <= 48 KiB (524,288), 256 blocks of 1024
# above (262,144).  Every shape has a few rows more than one pass covers.
PAST_CAP = [
    (1, 16, 8, 4096, 4104, "float16", 256 * 32 * 256),
    (1, 16, 16, 8192, 4100, "bfloat16", 256 * 32 * 256),
    (1, 8, 8, 1024, 4200, "float16", 256 * 8 * 256),
    (2, 8, 8, 1024, 4200, "bfloat16", 256 * 8 * 256),
    (8, 8, 32, 2048, 4224, "float16", 256 * 1024),
    (1, 12, 8, 4096, 4104, "bfloat16", 256 * 32 * 256),
]


@pytest.mark.parametrize("K,nbits,g,fin,fout,dt,cap", PAST_CAP)
def test_second_grid_stride_pass_bit_exact(hk, K, nbits, g, fin, fout, dt, cap):
    groups = fout * (fin // g)
    assert cap < groups < 2 * cap, (groups, cap)   # the second pass is a partial one
    L = orc.make_layer(500 + K + nbits + g, fin, fout, K, nbits, g, batch=1, bias=False, float_dtype=np_dtype(dt))
    own = [e for e in entries_for(hk, K, nbits) if e[0] != "generic_dequant"] or entries_for(hk, K, nbits)
    check_layer(hk, L, K, nbits, dt, f"{K}x{nbits}g{g} {fin}->{fout} ({groups} groups, cap {cap})", ops=own)


# ------------------------------------------------------------------ (c) force_generic on the tuned entries
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("K,nbits,g", TUNED)
def test_force_generic_gives_the_tuned_bits(hk, K, nbits, g, dt):
    from aqlm_amd import _native

    L = orc.make_layer(700 + K + nbits + g, g * 65, 37, K, nbits, g, batch=1, bias=False, float_dtype=np_dtype(dt))
    T = to_dev(L, tdtype(dt))
    (name, op), = [e for e in entries_for(hk, K, nbits) if e[0] != "generic_dequant"]
    for scaled in (True, False):
        s = T["scales"] if scaled else None
        bits = restated(L, dt, scaled)
        tuned = op(T["codes"], T["codebooks"], s)
        _native.set_tuning("force_generic", 1)
        try:
            forced = op(T["codes"], T["codebooks"], s)
        finally:
            _native.set_tuning("force_generic", 0)
        assert_bits(tuned, bits, f"{name} tuned scaled={scaled}")
        assert_bits(forced, bits, f"{name} force_generic scaled={scaled}")


# ------------------------------------------------------------------ (d) misaligned pointers, raw C ABI
PAD = 24                   # sentinel elements on either side of W
SENTINEL = 0x5A5A


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("K,nbits,misaligned", [(1, 16, "W"), (1, 16, "codebook"), (2, 8, "W"), (2, 8, "codebook"), (2, 8, "codes")])
def test_misaligned_pointers_fall_back_and_stay_inside_w(hk, K, nbits, misaligned, dt):
    """A W, codebook or (kx8) code pointer that is not 16-byte aligned takes the generic kernel: the same bits, and nothing written
    outside W.  The 2-byte offsets are offsets inside larger buffers, so every access of the call stays inside an allocation."""
    from aqlm_amd import _native

    g, out, in_groups = 8, 37, 65
    fin = g * in_groups
    dtype = tdtype(dt)
    L = orc.make_layer(800 + K + nbits, fin, out, K, nbits, g, batch=1, bias=False, float_dtype=np_dtype(dt))
    T = to_dev(L, dtype)

    def inside(t, shift):
        """A copy of `t` that starts `shift` elements into a fresh (16-byte aligned) buffer."""
        flat = t.reshape(-1)
        buf = torch.zeros(flat.numel() + 16, dtype=t.dtype, device=t.device)
        assert buf.data_ptr() % 16 == 0
        buf[shift:shift + flat.numel()] = flat
        return buf, buf.data_ptr() + shift * t.element_size()

    n = out * fin
    w_shift = PAD + 1 if misaligned == "W" else PAD
    wbuf = torch.full((n + 2 * PAD + 8,), SENTINEL, dtype=torch.int16, device=DEV)
    w_ptr = wbuf.data_ptr() + 2 * w_shift
    cb_buf, cb_ptr = inside(T["codebooks"], 1 if misaligned == "codebook" else 0)
    codes_buf, codes_ptr = inside(T["codes"], 2 if misaligned == "codes" else 0)   # int8 codes: two elements = 2 bytes
    for name, ptr in (("W", w_ptr), ("codebook", cb_ptr), ("codes", codes_ptr)):
        assert (ptr % 16 != 0) == (name == misaligned) and ptr % 2 == 0, (name, ptr % 16)
    stream = torch.cuda.current_stream().cuda_stream
    for scaled in (True, False):
        wbuf.fill_(SENTINEL)
        s_ptr = T["scales"].data_ptr() if scaled else None
        if nbits == 16:
            rc = _native.lib.aqlm_hip_dequant_1x16(codes_ptr, cb_ptr, s_ptr, w_ptr, out, fin, g, _native.F16 if dt == "float16" else _native.BF16,
                                                   stream)
        else:
            rc = _native.lib.aqlm_hip_dequant_kx8(codes_ptr, cb_ptr, s_ptr, w_ptr, out, fin, K, g, _native.F16 if dt == "float16" else _native.BF16,
                                                  stream)
        assert rc == 0, _native.last_error()
        torch.cuda.synchronize()
        W = wbuf[w_shift:w_shift + n].clone().view(dtype).reshape(out, fin)
        assert_bits(W, restated(L, dt, scaled), f"{K}x{nbits} misaligned {misaligned} scaled={scaled}")
        assert bool((wbuf[:w_shift] == SENTINEL).all()) and bool((wbuf[w_shift + n:] == SENTINEL).all()), "wrote outside W"
    del cb_buf, codes_buf


# ------------------------------------------------------------------ (e) special values
def _f16(*v):
    a = np.array(v, dtype=np.float64)
    assert (a.astype(np.float16).astype(np.float64) == a).all(), "not an fp16 value"
    return a.astype(np.float32)


def _bf16(*v):
    a = np.array(v, dtype=np.float64).astype(np.float32)
    assert (np.array(v, dtype=np.float64) == a.astype(np.float64)).all() and (orc.round_to_bf16(a).view(np.uint32) == a.view(np.uint32)).all(), "not a bf16 value"
    return a


P = lambda e: 2.0**e   # noqa: E731

# One codebook (1x16 g8): the four rows that make_layer's edge codes select -- 0, 2**15 - 1, 2**15, 2**16 - 1 -- at the start of
# the first row of W (scale s_first) and, in reverse, at the end of the last row (scale s_last).  Every entry meets both scales and,
# in the unscaled run, none.
#   fp16, s_first = 2**-10: products in the subnormal range (spacing 2**-24), below it, and on ties of it
#         s_last  = -1025 = -(1 + 2**-10) * 2**10: 12-bit products that tie in the normal range, and products beyond 65504
ONE_CODEBOOK = {
    "float16": dict(
        s_first=P(-10), s_last=-1025.0,
        rows=[
            # * 2**-10: 1.5 * 2**-16 (a subnormal, exact) | 2**-16 + 2**-26 -> 2**-16 | 2**-24 + 3 * 2**-34 -> 2**-24 | 2**-26 -> +0
            # | -2**-26 -> -0 | 2**-25: tie, -> +0 (even) | 3 * 2**-25: tie, -> 2 * 2**-24 | -3 * 2**-25 -> -2 * 2**-24
            _f16(1.5 * P(-6), (1 + P(-10)) * P(-6), (1 + 3 * P(-10)) * P(-14), P(-16), -P(-16), P(-15), 3 * P(-15), -3 * P(-15)),
            # * -1025: 3 -> -3075: tie between 3074 and 3076, -> -3076 | 5 -> -5125: tie 5124 / 5128 is not one (5125 = 5124 + 1 of 4):
            # -> -5124 | 64 -> -65600 -> -inf | -64 -> +inf | 63.9375 -> -65535.9 -> -inf (>= 65520) | 63.875 -> -65471.9 -> -65472
            # | -0.0: 0 + -0 = +0, * -1025 = -0 (and * 2**-10 = +0) | 0.0 -> -0 (a negative scale times zero)
            _f16(3.0, 5.0, 64.0, -64.0, 63.9375, 63.875, -0.0, 0.0),
            # 5 * 2**-25 * ... further ties and near-ties of the subnormal range under 2**-10: 5 * 2**-15 -> 2.5 units -> 2 |
            # 7 * 2**-15 -> 3.5 -> 4 | (1 + 2**-9) * 2**-15 (itself a subnormal) -> just above half a unit -> 1 | the smallest subnormal itself, 2**-24
            # (-> 2**-34 -> 0) | the largest subnormal (1023 * 2**-24) | the smallest normal 2**-14 | 65504 | -65504
            _f16(5 * P(-15), 7 * P(-15), (1 + P(-9)) * P(-15), P(-24), 1023 * P(-24), P(-14), 65504.0, -65504.0),
            # infinities as entries keep their sign through both scales; 1.0 and 2**-14 * 1.5 as plain values
            _f16(np.inf, -np.inf, 1.0, -1.0, 1.5 * P(-14), 1025.0, 0.5, -0.5),
        ]),
    # bf16 (8-bit significands, fp32's exponent range), s_first = 2**-30: products that are fp32 subnormals -- representable bf16
    # subnormals (spacing 2**-133), ties of that spacing, and values that vanish; s_last = -(1 + 2**-7) * 2**30: 16-bit products
    # that tie in the normal range, products that are finite in fp32 but round to infinity in bf16, and fp32 overflow
    "bfloat16": dict(
        s_first=P(-30), s_last=-(1 + P(-7)) * P(30),
        rows=[
            # * 2**-30: 1.5 * 2**-130 = 12 units (an fp32-subnormal product, a bf16 subnormal, exact) | 2**-133 (one unit) | 2**-134:
            # tie, -> +0 | 3 * 2**-134: tie, -> 2 units | -3 * 2**-134 -> -2 units | 2**-140 -> +0 | -2**-140 -> -0 | 2**-155: below fp32 -> +0
            _bf16(1.5 * P(-100), P(-103), P(-104), 3 * P(-104), -3 * P(-104), P(-110), -P(-110), P(-125)),
            # * -(129/128) * 2**30: 3 -> tie in [2, 4) * 2**30 (3 + 3 * 2**-7: 1.5 spacings) | 5 -> 5 + 5 * 2**-7, no tie |
            # (254/128) * 2**97 -> -1.99987 * 2**127: finite in fp32, rounds to -inf in bf16 | its negative -> +inf |
            # 2**98 -> fp32 overflow -> -inf | (252/128) * 2**97 -> -1.98413 * 2**127 -> finite | -0.0 -> +0 then -0 | 0.0 -> -0
            _bf16(3.0, 5.0, (254 / 128) * P(97), -(254 / 128) * P(97), P(98), (252 / 128) * P(97), -0.0, 0.0),
            # 5 * 2**-134 -> 2.5 units -> 2 | 7 * 2**-134 -> 3.5 -> 4 | (1 + 2**-7) * 2**-134 -> 1 | the smallest bf16 subnormal 2**-133 as
            # an entry (-> 2**-163 -> 0 under 2**-30) | the largest subnormal | the smallest normal | the largest finite, both signs
            _bf16(5 * P(-104), 7 * P(-104), (1 + P(-7)) * P(-104), P(-133), 127 * P(-133), P(-126), (255 / 128) * P(127), -(255 / 128) * P(127)),
            _bf16(np.inf, -np.inf, 1.0, -1.0, 1.5 * P(-126), 129.0, 0.5, -0.5),
        ]),
}
# Two codebooks (2x8 g8): the edge codes pair rows (0, 127), (128, 255) of codebooks (0, 1) at the start of the first row of W and
# (255, 128), (127, 0) at the end of the last.  The fp32 SUM is what gets rounded: cancellation to +0, sums that need more bits
# than the storage type has (ties), sums beyond the largest finite value, inf - inf.
TWO_CODEBOOKS = {
    "float16": dict(
        s_first=0.5, s_last=-1025.0,
        pairs={
            # 2048 + 1: tie, -> 2048 | 2048 + 3: tie, -> 2052 | 1 - 1 = +0 | -0 + -0 (from f = +0) = +0 | 65504 + 16 = 65520: tie, -> inf
            # | 65504 + 15 -> 65504 | inf - inf = NaN | (1 + 2**-10) - 1 = 2**-10
            (0, 127): (_f16(2048.0, 2048.0, 1.0, -0.0, 65504.0, 65504.0, np.inf, 1 + P(-10)), _f16(1.0, 3.0, -1.0, -0.0, 16.0, 15.0, -np.inf, -1.0)),
            # subnormal sums: 2**-24 + 2**-24 | 3 units (halved by s_first: tie 1.5 -> 2) | 1 unit (halved: tie 0.5 -> 0) | -1 unit (-> -0)
            # | 1023 + 1 units = the smallest normal | 2**-14 - 2**-24 | -65504 - 16 -> -inf | 1 + 2**-11 (24-bit sum, tie -> 1)
            (128, 255): (_f16(P(-24), 2 * P(-24), P(-24), -P(-24), 1023 * P(-24), P(-14), -65504.0, 1.0),
                         _f16(P(-24), P(-24), 0.0, 0.0, P(-24), -P(-24), -16.0, P(-11))),
            # met by the last row (scale -1025): 3 = 1 + 2 -> -3075, tie -> -3076 | 32 + 32 = 64 -> -inf | 63 + 0.875 -> -65471.9 -> -65472 |
            # 0.5 - 0.5 = +0 -> -0 | -32 - 32 -> +inf | 2 + 3 = 5 -> -5125 -> -5124 | 1 + 2**-11: -1025.5004.. -> -1026 (spacing 1: not a tie) | 0 + 0
            (255, 128): (_f16(1.0, 32.0, 63.0, 0.5, -32.0, 2.0, 1.0, 0.0), _f16(2.0, 32.0, 0.875, -0.5, -32.0, 3.0, P(-11), 0.0)),
            (127, 0): (_f16(1.5, -1.5, P(-14), 100.0, 1000.0, 7.0, -7.0, 0.25), _f16(1.5, 1.5, P(-14), 0.0625, P(-10), -7.0, 7.0, 0.25)),
        }),
    "bfloat16": dict(
        s_first=0.5, s_last=-(1 + P(-7)) * P(30),
        pairs={
            # 256 + 1: tie (spacing 2), -> 256 | 256 + 3: tie, -> 260 | 1 - 1 = +0 | -0 + -0 = +0 | max + half a spacing (2**119): tie -> inf |
            # max + 2**118 -> max | inf - inf = NaN | (1 + 2**-7) - 1 = 2**-7
            (0, 127): (_bf16(256.0, 256.0, 1.0, -0.0, (255 / 128) * P(127), (255 / 128) * P(127), np.inf, 1 + P(-7)),
                       _bf16(1.0, 3.0, -1.0, -0.0, P(119), P(118), -np.inf, -1.0)),
            # sums of bf16 subnormals are fp32 subnormals: 2 units | 3 units (halved: tie -> 2) | 1 unit (halved: tie -> 0) | -1 unit (-> -0) |
            # 127 + 1 units = the smallest normal | 2**-126 - 2**-133 | -max - 2**119 -> -inf | 1 + 2**-8 (tie -> 1)
            (128, 255): (_bf16(P(-133), 2 * P(-133), P(-133), -P(-133), 127 * P(-133), P(-126), -(255 / 128) * P(127), 1.0),
                         _bf16(P(-133), P(-133), 0.0, 0.0, P(-133), -P(-133), -P(119), P(-8))),
            # met by the last row (scale -(129/128) * 2**30): 1 + 2 = 3: tie | 2**96 + 2**96 = 2**97 (finite) | (127/64 + 1/128 ...) * 2**97 ->
            # 254/128 * 2**97 -> -inf in bf16 | 0.5 - 0.5 = +0 -> -0 | -2**97 - 2**97 = -2**98 -> fp32 overflow -> +inf | 2 + 3 | 1 + 2**-8 | 0 + 0
            (255, 128): (_bf16(1.0, P(96), (127 / 64) * P(97), 0.5, -P(97), 2.0, 1.0, 0.0),
                         _bf16(2.0, P(96), 0.0, -0.5, -P(97), 3.0, P(-8), 0.0)),
            (127, 0): (_bf16(1.5, -1.5, P(-126), 100.0, 1000.0, 7.0, -7.0, 0.25), _bf16(1.5, 1.5, P(-126), 0.0625, P(-10), -7.0, 7.0, 0.25)),
        }),
}


def _patterns(dt):
    """(+inf pattern, number of mantissa bits) of the storage type."""
    return (0x7C00, 10) if dt == "float16" else (0x7F80, 7)


def _crafted(K, dt):
    nbits = 16 if K == 1 else 8
    out, in_groups = 5, 9
    L = orc.make_layer(900 + K, 8 * in_groups, out, K, nbits, 8, batch=1, bias=False, float_dtype=np_dtype(dt))
    cb, scales = L["codebooks"].astype(np.float32), L["scales"].astype(np.float32)
    spec = (ONE_CODEBOOK if K == 1 else TWO_CODEBOOKS)[dt]
    edges = [0, 2 ** (nbits - 1) - 1, 2 ** (nbits - 1), 2**nbits - 1]
    if K == 1:
        assert L["codes_unsigned"][0, :4, 0].tolist() == edges and L["codes_unsigned"][-1, -4:, 0].tolist() == edges[::-1]
        for code, row in zip(edges, spec["rows"]):
            cb[0, code, 0] = row
    else:
        assert L["codes_unsigned"][0, :2].tolist() == [edges[:2], edges[2:]] and L["codes_unsigned"][-1, -2:].tolist() == [edges[:1:-1], edges[1::-1]]
        for (c0, c1), (e0, e1) in spec["pairs"].items():
            cb[0, c0, 0], cb[1, c1, 0] = e0, e1
    scales[0], scales[-1] = spec["s_first"], spec["s_last"]
    _f16(float(scales[0, 0, 0, 0]), float(scales[-1, 0, 0, 0])) if dt == "float16" else _bf16(float(scales[0, 0, 0, 0]), float(scales[-1, 0, 0, 0]))
    return dict(L, codebooks=cb, scales=scales), 4 if K == 1 else 2


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("K", [1, 2])
def test_special_values_bit_exact(hk, K, dt):
    """Subnormal results, underflow to +/-0, overflow to +/-inf, exact ties, -0.0 entries, a negative scale times zero and (bf16)
    fp32-subnormal products: the kernel's bits are the contract's.  The crafted entries sit where make_layer's edge codes select them;
    the classes the expected patterns must contain are asserted first, so the case cannot go stale unnoticed."""
    L, ng = _crafted(K, dt)
    inf, mant = _patterns(dt)
    first = np.concatenate([restated(L, dt, s)[0, :8 * ng] for s in (True, False)])      # crafted entries under s_first / no scale
    last = np.concatenate([restated(L, dt, s)[-1, -8 * ng:] for s in (True, False)])     # ... under the negative s_last / no scale
    both = np.concatenate([first, last])
    mag = both & 0x7FFF
    assert ((mag > 0) & (mag < (1 << mant))).sum() >= 4, "no subnormal results"
    assert (first == 0x0000).any() and (first == 0x8000).any() and (last == 0x8000).any(), "no signed zeros"
    assert (last == inf).any() and (last == (inf | 0x8000)).any(), "no overflow to both infinities"
    assert (both == 0x0002).any(), "no tie between two subnormals (1.5 units -> 2)"
    if K == 2:
        assert (mag > inf).any(), "no inf - inf"
    ops = [("code1x16_dequant", hk.code1x16_dequant)] if K == 1 else [("code2x8_dequant", hk.code2x8_dequant)]
    check_layer(hk, L, K, 16 if K == 1 else 8, dt, f"special values {K} codebook(s)", ops=ops + [("generic_dequant", hk.generic_dequant)])


@pytest.mark.parametrize("dt", DTYPES)
def test_summation_follows_codebook_order(hk, dt):
    """Sums of eight fp16 / bf16 values of similar size are exact in fp32 in ANY order, so random layers cannot tell in which order a
    kernel adds its codebooks (on 8.6 M random weights two differ).  One crafted group of an 8x8 g32 layer can: every element adds
    +big, -big and six small values 3 * tiny, `big` so large that fp32 has no room for the small ones beside it.  Small values added
    while the sum is near +/-big are rounded to big's spacing (6 * 3 * tiny = 2.25 spacings -> 2), those added before +big or after
    -big survive; where +big and -big sit among the eight codebooks differs from element to element."""
    K, g, out, in_groups = 8, 32, 5, 3
    big, tiny = (2048.0, P(-16)) if dt == "float16" else (P(20), P(-7))    # fp32 spacing just below big: 2**-13 | 2**-4 = 8 * tiny
    L = orc.make_layer(950, g * in_groups, out, K, 8, g, batch=1, bias=False, float_dtype=np_dtype(dt))
    cu, cb = L["codes_unsigned"].copy(), L["codebooks"].astype(np.float32)
    cu[2, 1] = 100 + np.arange(K)                 # a group in the middle of W picks row 100 + c of codebook c
    for e in range(g):
        plus, minus = e % K, (e + 1 + e // K) % K
        for c in range(K):
            cb[c, 100 + c, 0, e] = big if c == plus else -big if c == minus else 3 * tiny
    (_f16 if dt == "float16" else _bf16)(big, 3 * tiny)
    L = dict(L, codes_unsigned=cu, codes=orc.pack_int_data(cu, 8), codebooks=cb)
    forward = restated(L, dt, False)[2, g:2 * g]
    backward = orc.dequantize_weight_storage(cu[..., ::-1], cb[::-1], None, np_dtype(dt))[2, g:2 * g]
    assert (forward != backward).sum() >= g // 2, "the crafted group does not depend on the order"
    check_layer(hk, L, K, 8, dt, "summation order 8x8g32")


# ------------------------------------------------------------------ (f) ops built on W
def _w64(L, dt, scaled):
    return orc.storage_bits_to_float64(restated(L, dt, scaled), np_dtype(dt))


TRANSPOSED = [
    # op, K, nbits, g, in, out, dtype, rows as, non-contiguous grad_output
    ("code1x16_matmat_dequant_transposed", 1, 16, 8, 512, 96, "float16", (2, 3), False),
    ("code1x16_matmat_dequant_transposed", 1, 16, 16, 1024, 40, "bfloat16", (8,), True),
    ("code2x8_matmat_dequant_transposed", 2, 8, 8, 512, 192, "float16", (12,), True),
    ("code2x8_matmat_dequant_transposed", 8, 8, 32, 1024, 64, "bfloat16", (2, 3), False),
    ("code1x8_matmat_dequant_transposed", 1, 8, 8, 512, 40, "bfloat16", (7,), False),
    ("code1x8_matmat_dequant_transposed", 1, 8, 8, 768, 120, "float16", (2, 3), True),
    ("generic_matmat_dequant_transposed", 3, 5, 8, 512, 72, "float16", (9,), True),
    ("generic_matmat_dequant_transposed", 4, 8, 16, 1024, 48, "bfloat16", (2, 3), False),
    ("generic_matmat_dequant_transposed", 1, 16, 16, 512, 40, "float16", (6,), False),
]


@pytest.mark.parametrize("op,K,nbits,g,fin,fout,dt,lead,noncontig", TRANSPOSED)
def test_transposed_ops_with_bias_against_the_restated_w(hk, op, K, nbits, g, fin, fout, dt, lead, noncontig):
    """grad_input = grad_output @ W + bias, W being the SCALED storage weight the dequantise kernel writes (scales folded into its
    rows).  Reference: fp64 with exactly that W; left over are the library GEMM's fp32 accumulation and two output roundings."""
    dtype = tdtype(dt)
    rows = int(np.prod(lead))
    L = orc.make_layer(1100 + K + nbits + g + fout, fin, fout, K, nbits, g, batch=rows, bias=False, float_dtype=np_dtype(dt))
    T = to_dev(L, dtype)
    gen = torch.Generator().manual_seed(fin + fout)
    gout = torch.randn(rows, fout, generator=gen).to(dtype)
    bias = torch.randn(fin, generator=gen).to(dtype)
    g_dev = gout.to(DEV)
    if noncontig:   # a column slice of a wider tensor
        wide = torch.zeros(rows, fout + 24, dtype=dtype, device=DEV)
        wide[:, 8:8 + fout] = g_dev
        g_dev = wide[:, 8:8 + fout]
        assert not g_dev.is_contiguous()
    g_dev = g_dev.reshape(*lead, fout) if len(lead) > 1 else g_dev
    got = getattr(hk, op)(g_dev, T["codes"], T["codebooks"], T["scales"], bias.to(DEV))
    assert got.shape == (*lead, fin) and got.dtype == dtype
    ref = gout.double().numpy() @ _w64(L, dt, True) + bias.double().numpy()
    check_close(got.float().cpu().numpy().reshape(rows, fin), ref, dtype, f"{op} {K}x{nbits}g{g} {fin}->{fout} {dt}", el_scale=1.0)


FORWARD = [
    ("generic_matmat_dequant", 4, 8, 16, 1024, 96, 9),
    ("generic_matmat_dequant", 1, 12, 8, 512, 160, 12),
    ("code1x8_matmat_dequant", 1, 8, 8, 448, 120, 7),    # in_features % 128 != 0: outside the fused kernel
]


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("op,K,nbits,g,fin,fout,rows", FORWARD)
def test_dequant_gemm_forwards_against_the_restated_w(hk, op, K, nbits, g, fin, fout, rows, dt):
    """y = (x @ W_unscaled.T) * scales + bias with the UNSCALED storage weight: these routes keep W unscaled and scale y in fp32."""
    dtype = tdtype(dt)
    L = orc.make_layer(1200 + K + nbits + g, fin, fout, K, nbits, g, batch=rows, bias=True, float_dtype=np_dtype(dt))
    T = to_dev(L, dtype)
    got = getattr(hk, op)(T["x"], T["codes"], T["codebooks"], T["scales"], T["bias"])
    assert got.shape == (rows, fout) and got.dtype == dtype
    ref = (L["x"].astype(np.float64) @ _w64(L, dt, False).T) * L["scales"].astype(np.float64).reshape(1, -1) + L["bias"].astype(np.float64)
    check_close(got.float().cpu().numpy(), ref, dtype, f"{op} {K}x{nbits}g{g} {fin}->{fout} rows={rows} {dt}", el_scale=1.0)
