"""CPU-only: which malformed call of the dense MFMA GEMM entries is refused with which code and which message, in which order,
and what aqlm_hip_workspace_bytes answers for the two ops that take a workspace.

Every call below carries at least one fault that its entry refuses in front of the first launch (read in gemm_mfma_entries.h,
gemm_8x8.hip, gemm_1x16_scan.hip), so none needs a GPU and none reaches one where there is one.  The codes, the message texts and
the byte counts were recorded from the library as it was before the entries' checks moved to the shared helpers of
aqlm_common.h and gemm_mfma.hip was split into parts; the whole text is compared, so a check that changes its wording, its code
or its place in the order fails here.
"""
import ctypes

import pytest


@pytest.fixture(scope="module")
def native():
    from aqlm_amd import _native

    return _native


# parameter names of each entry in ABI order (include/aqlm_hip.h); "P" in a default stands for 16-B aligned host memory
SIGNATURES = {
    "aqlm_hip_gemm_1x16_mfma": "codes codebook scales bias x y batch out inf g xs ys dtype ws ws_bytes stream",
    "aqlm_hip_gemm_kx8_mfma": "codes codebook scales bias x y batch out inf k g xs ys dtype stream",
    "aqlm_hip_gemm_kx8_mfma_ws": "codes codebook scales bias x y batch out inf k g xs ys dtype ws ws_bytes stream",
    "aqlm_hip_gemm_8x8_mfma": "codes codebook scales bias x y batch out inf g xs ys dtype stream",
    "aqlm_hip_gemm_1x16_scan": "codes codebook scales bias x y batch out inf xs ys dtype ws ws_bytes stream",
}
DEFAULTS = dict(codes="P", codebook="P", scales="P", bias=None, x="P", y="P", batch=8, out=4096, inf=4096, k=2, xs=4096, ys=4096,
                dtype=0, ws=None, ws_bytes=0, stream=None)
GROUP = {"aqlm_hip_gemm_1x16_mfma": 8, "aqlm_hip_gemm_kx8_mfma": 8, "aqlm_hip_gemm_kx8_mfma_ws": 8, "aqlm_hip_gemm_8x8_mfma": 32}

# the faults, one per check, named once; a case is a list of them
NULLS = [dict(codes=None), dict(codebook=None), dict(scales=None), dict(x=None), dict(y=None)]
SIZES = [dict(batch=0), dict(out=0), dict(inf=0), dict(batch=-3)]
DTYPE = dict(dtype=7)
NEG_STRIDE = dict(batch=2, xs=-4096)
X_MISALIGNED = dict(x="P+2")
XS_ODD = dict(xs=4100)
WS_NULL = dict(ws=None, ws_bytes=1 << 30)


def merged(*faults):
    out = {}
    for f in faults:
        out.update(f)
    return out


def common_cases(bad_group, bad_features, layout_faults):
    """The walk every entry shares: each single fault, then pairs of neighbours in the order of the checks (the earlier one must
    be the one reported).  `bad_group`: None for the entry without a group argument."""
    singles = NULLS + SIZES + ([bad_group] if bad_group else []) + [DTYPE, NEG_STRIDE] + bad_features + layout_faults
    order = [NULLS[0], SIZES[0]] + ([bad_group] if bad_group else []) + [DTYPE, NEG_STRIDE, X_MISALIGNED]
    pairs = [merged(b, a) for a, b in zip(order, order[1:])]            # the later fault is written first: its place in the
    pairs += [merged(DTYPE, NULLS[3]), merged(XS_ODD, SIZES[1])]         # argument list must not matter either
    return singles + pairs


def entry_cases(entry):
    """-> [overrides]: every call is refused in front of the first launch."""
    if entry == "aqlm_hip_gemm_1x16_mfma":
        # (the defaults carry no workspace: a call whose other arguments are good is refused for that)
        return common_cases(dict(g=4), [dict(inf=4100)], [dict(codes="P+8"), dict(codebook="P+8"), X_MISALIGNED, XS_ODD]) + [
            dict(g=32, ws="P", ws_bytes=1 << 30),
            WS_NULL,
            dict(ws="P", ws_bytes=0),
            dict(ws="P", ws_bytes=4194304 - 1),
            dict(batch=128, ws="P", ws_bytes=16777216 - 1),
            dict(batch=300, out=11008, ws="P", ws_bytes=1 << 20),
            dict(bias="P"),                                  # the bias is optional: the call gets as far as the workspace
            dict(batch=1, xs=-4096),                         # one row has no stride: not read, not refused
            merged(XS_ODD, dict(ws="P", ws_bytes=16)),
        ]
    if entry in ("aqlm_hip_gemm_kx8_mfma", "aqlm_hip_gemm_kx8_mfma_ws"):
        # (every call carries its fault and is otherwise good: 8 rows of 4096 features, so that a layout fault is the only reason
        # for its refusal; 256 features are too short for the X ring)
        return common_cases(dict(k=3), [dict(inf=4160), dict(inf=256), dict(inf=512, batch=32)], [dict(codebook="P+8"), X_MISALIGNED, XS_ODD]) + [
            dict(k=2, g=16),
            dict(k=0),
            merged(dict(k=4, g=32), DTYPE),
            # a tail slab of 2 rows plans steps of 4 chunks, of which 512 features hold two: refused after every slab is planned,
            # before any is launched (the first slab of 128 rows is inside the plans)
            dict(batch=130, inf=512),
            dict(batch=160, inf=512, xs=512),
        ] + ([] if entry == "aqlm_hip_gemm_kx8_mfma" else [   # a workspace changes no refusal (it only lets 49+ rows split K)
            dict(inf=256, ws="P", ws_bytes=1 << 30),
            dict(codes=None, ws="P", ws_bytes=1 << 30),
            dict(x="P+2", ws="P", ws_bytes=1 << 30),
            dict(batch=130, inf=512, ws="P+8", ws_bytes=1 << 30),
            dict(batch=130, inf=512, ws="P", ws_bytes=1 << 30),
        ])
    if entry == "aqlm_hip_gemm_8x8_mfma":
        # (as above: 4096 features are good, 1024 are fewer than the 8 waves' K shares)
        return common_cases(dict(g=8), [dict(inf=4224), dict(inf=1792), dict(inf=1024)], [dict(codes="P+8"), dict(codebook="P+8"), X_MISALIGNED, XS_ODD]) + [
            dict(g=16),
        ]
    assert entry == "aqlm_hip_gemm_1x16_scan"
    return common_cases(None, [dict(inf=4160)], [dict(codes="P+8"), dict(codebook="P+8"), X_MISALIGNED, XS_ODD]) + [
        dict(inf=133120, xs=133120, ws="P", ws_bytes=1 << 30),   # 520 units of 256 features: more than 32 K chunks of 2 units per wave
        WS_NULL,
        dict(ws="P", ws_bytes=1048576 - 1),
        dict(ws="P+8", ws_bytes=1 << 30),
        merged(X_MISALIGNED, dict(ws="P+8", ws_bytes=1 << 30)),
    ]


def describe(overrides):
    return ", ".join(f"{k}={v}" for k, v in overrides.items())


def run_case(native, entry, overrides, P):
    vals = dict(DEFAULTS, g=GROUP.get(entry))
    vals.update(overrides)

    def value(v):
        if isinstance(v, str):
            return P + int(v[2:] or 0)
        return v

    rc = getattr(native.lib, entry)(*[value(vals[name]) for name in SIGNATURES[entry].split()])
    return rc, native.last_error()


# entry -> case -> (return code, last_error() behind "<entry>: ")
KX8 = {
    "codes=None": (-1, "null pointer argument"),
    "codebook=None": (-1, "null pointer argument"),
    "scales=None": (-1, "null pointer argument"),
    "x=None": (-1, "null pointer argument"),
    "y=None": (-1, "null pointer argument"),
    "batch=0": (-1, "sizes must be positive"),
    "out=0": (-1, "sizes must be positive"),
    "inf=0": (-1, "sizes must be positive"),
    "batch=-3": (-1, "sizes must be positive"),
    "k=3": (-2, "1 or 2 codebooks of 256 x 8 only, got 3 codebooks, group 8"),
    "dtype=7": (-2, "AQLM HIP kernels only support float16 and bfloat16 (dtype id 7)"),
    "batch=2, xs=-4096": (-1, "negative x_row_stride -4096 (rows of x)"),
    "inf=4160": (-2, "needs in_features % 128 == 0, >= 384, and 16-B aligned codebooks / X rows"),
    "inf=256": (-2, "needs in_features % 128 == 0, >= 384, and 16-B aligned codebooks / X rows"),
    "inf=512, batch=32": (-2, "needs in_features % 128 == 0, >= 384, and 16-B aligned codebooks / X rows"),
    "codebook=P+8": (-2, "needs in_features % 128 == 0, >= 384, and 16-B aligned codebooks / X rows"),
    "x=P+2": (-2, "needs in_features % 128 == 0, >= 384, and 16-B aligned codebooks / X rows"),
    "xs=4100": (-2, "needs in_features % 128 == 0, >= 384, and 16-B aligned codebooks / X rows"),
    "batch=0, codes=None": (-1, "null pointer argument"),
    "k=3, batch=0": (-1, "sizes must be positive"),
    "dtype=7, k=3": (-2, "1 or 2 codebooks of 256 x 8 only, got 3 codebooks, group 8"),
    "batch=2, xs=-4096, dtype=7": (-2, "AQLM HIP kernels only support float16 and bfloat16 (dtype id 7)"),
    "x=P+2, batch=2, xs=-4096": (-1, "negative x_row_stride -4096 (rows of x)"),
    "dtype=7, x=None": (-1, "null pointer argument"),
    "xs=4100, out=0": (-1, "sizes must be positive"),
    "k=2, g=16": (-2, "1 or 2 codebooks of 256 x 8 only, got 2 codebooks, group 16"),
    "k=0": (-2, "1 or 2 codebooks of 256 x 8 only, got 0 codebooks, group 8"),
    "k=4, g=32, dtype=7": (-2, "1 or 2 codebooks of 256 x 8 only, got 4 codebooks, group 32"),
    "batch=130, inf=512": (-2, "a slab of 2 rows at in_features 512 is outside the kernel's plans"),
    "batch=160, inf=512, xs=512": (-2, "a slab of 32 rows at in_features 512 is outside the kernel's plans"),
}
EXPECTED = {
    "aqlm_hip_gemm_1x16_mfma": {
        "codes=None": (-1, "null pointer argument"),
        "codebook=None": (-1, "null pointer argument"),
        "scales=None": (-1, "null pointer argument"),
        "x=None": (-1, "null pointer argument"),
        "y=None": (-1, "null pointer argument"),
        "batch=0": (-1, "sizes must be positive"),
        "out=0": (-1, "sizes must be positive"),
        "inf=0": (-1, "sizes must be positive"),
        "batch=-3": (-1, "sizes must be positive"),
        "g=4": (-2, "only codebooks with 8 or 16 features are supported, got 4"),
        "dtype=7": (-2, "AQLM HIP kernels only support float16 and bfloat16 (dtype id 7)"),
        "batch=2, xs=-4096": (-1, "negative x_row_stride -4096 (rows of x)"),
        "inf=4100": (-2, "needs in_features % 64 == 0 and 16-B aligned codes/codebook/X rows"),
        "codes=P+8": (-2, "needs in_features % 64 == 0 and 16-B aligned codes/codebook/X rows"),
        "codebook=P+8": (-2, "needs in_features % 64 == 0 and 16-B aligned codes/codebook/X rows"),
        "x=P+2": (-2, "needs in_features % 64 == 0 and 16-B aligned codes/codebook/X rows"),
        "xs=4100": (-2, "needs in_features % 64 == 0 and 16-B aligned codes/codebook/X rows"),
        "batch=0, codes=None": (-1, "null pointer argument"),
        "g=4, batch=0": (-1, "sizes must be positive"),
        "dtype=7, g=4": (-2, "only codebooks with 8 or 16 features are supported, got 4"),
        "batch=2, xs=-4096, dtype=7": (-2, "AQLM HIP kernels only support float16 and bfloat16 (dtype id 7)"),
        "x=P+2, batch=2, xs=-4096": (-1, "negative x_row_stride -4096 (rows of x)"),
        "dtype=7, x=None": (-1, "null pointer argument"),
        "xs=4100, out=0": (-1, "sizes must be positive"),
        "g=32, ws=P, ws_bytes=1073741824": (-2, "only codebooks with 8 or 16 features are supported, got 32"),
        "ws=None, ws_bytes=1073741824": (-1, "workspace of 4194304 bytes required, got 1073741824"),
        "ws=P, ws_bytes=0": (-1, "workspace of 4194304 bytes required, got 0"),
        "ws=P, ws_bytes=4194303": (-1, "workspace of 4194304 bytes required, got 4194303"),
        "batch=128, ws=P, ws_bytes=16777215": (-1, "workspace of 16777216 bytes required, got 16777215"),
        "batch=300, out=11008, ws=P, ws_bytes=1048576": (-1, "workspace of 105676800 bytes required, got 1048576"),
        "bias=P": (-1, "workspace of 4194304 bytes required, got 0"),
        "batch=1, xs=-4096": (-1, "workspace of 4194304 bytes required, got 0"),
        "xs=4100, ws=P, ws_bytes=16": (-2, "needs in_features % 64 == 0 and 16-B aligned codes/codebook/X rows"),
    },
    "aqlm_hip_gemm_1x16_scan": {
        "codes=None": (-1, "null pointer argument"),
        "codebook=None": (-1, "null pointer argument"),
        "scales=None": (-1, "null pointer argument"),
        "x=None": (-1, "null pointer argument"),
        "y=None": (-1, "null pointer argument"),
        "batch=0": (-1, "sizes must be positive"),
        "out=0": (-1, "sizes must be positive"),
        "inf=0": (-1, "sizes must be positive"),
        "batch=-3": (-1, "sizes must be positive"),
        "dtype=7": (-2, "AQLM HIP kernels only support float16 and bfloat16 (dtype id 7)"),
        "batch=2, xs=-4096": (-1, "negative x_row_stride -4096 (rows of x)"),
        "inf=4160": (-2, "needs in_features % 256 == 0 (codebook vectors of 8) and 16-B aligned codes / codebook / X rows"),
        "codes=P+8": (-2, "needs in_features % 256 == 0 (codebook vectors of 8) and 16-B aligned codes / codebook / X rows"),
        "codebook=P+8": (-2, "needs in_features % 256 == 0 (codebook vectors of 8) and 16-B aligned codes / codebook / X rows"),
        "x=P+2": (-2, "needs in_features % 256 == 0 (codebook vectors of 8) and 16-B aligned codes / codebook / X rows"),
        "xs=4100": (-2, "needs in_features % 256 == 0 (codebook vectors of 8) and 16-B aligned codes / codebook / X rows"),
        "batch=0, codes=None": (-1, "null pointer argument"),
        "dtype=7, batch=0": (-1, "sizes must be positive"),
        "batch=2, xs=-4096, dtype=7": (-2, "AQLM HIP kernels only support float16 and bfloat16 (dtype id 7)"),
        "x=P+2, batch=2, xs=-4096": (-1, "negative x_row_stride -4096 (rows of x)"),
        "dtype=7, x=None": (-1, "null pointer argument"),
        "xs=4100, out=0": (-1, "sizes must be positive"),
        "inf=133120, xs=133120, ws=P, ws_bytes=1073741824": (-2, "no plan for 8 rows of 133120 -> 4096"),
        "ws=None, ws_bytes=1073741824": (-1, "16-B aligned workspace of 1048576 bytes required, got 1073741824"),
        "ws=P, ws_bytes=1048575": (-1, "16-B aligned workspace of 1048576 bytes required, got 1048575"),
        "ws=P+8, ws_bytes=1073741824": (-1, "16-B aligned workspace of 1048576 bytes required, got 1073741824"),
        "x=P+2, ws=P+8, ws_bytes=1073741824": (-2, "needs in_features % 256 == 0 (codebook vectors of 8) and 16-B aligned codes / codebook / X rows"),
    },
    "aqlm_hip_gemm_8x8_mfma": {
        "codes=None": (-1, "null pointer argument"),
        "codebook=None": (-1, "null pointer argument"),
        "scales=None": (-1, "null pointer argument"),
        "x=None": (-1, "null pointer argument"),
        "y=None": (-1, "null pointer argument"),
        "batch=0": (-1, "sizes must be positive"),
        "out=0": (-1, "sizes must be positive"),
        "inf=0": (-1, "sizes must be positive"),
        "batch=-3": (-1, "sizes must be positive"),
        "g=8": (-2, "8 codebooks of 256 x 32 only, got group 8"),
        "dtype=7": (-2, "AQLM HIP kernels only support float16 and bfloat16 (dtype id 7)"),
        "batch=2, xs=-4096": (-1, "negative x_row_stride -4096 (rows of x)"),
        "inf=4224": (-2, "needs in_features % 256 == 0, >= 2048, and 16-B aligned codes / codebooks / X rows"),
        "inf=1792": (-2, "needs in_features % 256 == 0, >= 2048, and 16-B aligned codes / codebooks / X rows"),
        "inf=1024": (-2, "needs in_features % 256 == 0, >= 2048, and 16-B aligned codes / codebooks / X rows"),
        "codes=P+8": (-2, "needs in_features % 256 == 0, >= 2048, and 16-B aligned codes / codebooks / X rows"),
        "codebook=P+8": (-2, "needs in_features % 256 == 0, >= 2048, and 16-B aligned codes / codebooks / X rows"),
        "x=P+2": (-2, "needs in_features % 256 == 0, >= 2048, and 16-B aligned codes / codebooks / X rows"),
        "xs=4100": (-2, "needs in_features % 256 == 0, >= 2048, and 16-B aligned codes / codebooks / X rows"),
        "batch=0, codes=None": (-1, "null pointer argument"),
        "g=8, batch=0": (-1, "sizes must be positive"),
        "dtype=7, g=8": (-2, "8 codebooks of 256 x 32 only, got group 8"),
        "batch=2, xs=-4096, dtype=7": (-2, "AQLM HIP kernels only support float16 and bfloat16 (dtype id 7)"),
        "x=P+2, batch=2, xs=-4096": (-1, "negative x_row_stride -4096 (rows of x)"),
        "dtype=7, x=None": (-1, "null pointer argument"),
        "xs=4100, out=0": (-1, "sizes must be positive"),
        "g=16": (-2, "8 codebooks of 256 x 32 only, got group 16"),
    },
    "aqlm_hip_gemm_kx8_mfma": KX8,
    "aqlm_hip_gemm_kx8_mfma_ws": {
        **KX8,
        "inf=256, ws=P, ws_bytes=1073741824": (-2, "needs in_features % 128 == 0, >= 384, and 16-B aligned codebooks / X rows"),
        "codes=None, ws=P, ws_bytes=1073741824": (-1, "null pointer argument"),
        "x=P+2, ws=P, ws_bytes=1073741824": (-2, "needs in_features % 128 == 0, >= 384, and 16-B aligned codebooks / X rows"),
        "batch=130, inf=512, ws=P+8, ws_bytes=1073741824": (-2, "a slab of 2 rows at in_features 512 is outside the kernel's plans"),
        "batch=130, inf=512, ws=P, ws_bytes=1073741824": (-2, "a slab of 2 rows at in_features 512 is outside the kernel's plans"),
    },
}


@pytest.mark.parametrize("entry", sorted(SIGNATURES))
def test_refusals_are_unchanged(native, entry):
    buf = ctypes.create_string_buffer(4096 + 16)
    P = (ctypes.addressof(buf) + 15) & ~15
    cases = entry_cases(entry)
    names = [describe(c) for c in cases]
    assert len(set(names)) == len(names) >= 20
    assert sorted(names) == sorted(EXPECTED[entry])
    who = "aqlm_hip_gemm_kx8_mfma" if entry == "aqlm_hip_gemm_kx8_mfma_ws" else entry   # (the two K x 8 entries are one function)
    for name, overrides in zip(names, cases):
        rc, text = EXPECTED[entry][name]
        assert run_case(native, entry, overrides, P) == (rc, f"{who}: {text}"), name


# (op, batch, out_features, in_features) -> bytes
WORKSPACE_BYTES = {
    ("kx8", 48, 4096, 4096): 0,
    ("kx8", 49, 4096, 4096): 3211264,
    ("kx8", 128, 4096, 4096): 8388608,
    ("kx8", 300, 4096, 4096): 8388608,
    ("1x16", 1, 4096, 4096): 4194304,
    ("1x16", 7, 4096, 4096): 4194304,
    ("1x16", 16, 4096, 4096): 4194304,
    ("1x16", 128, 4096, 4096): 16777216,
    ("1x16", 300, 4096, 4096): 39321600,
    ("kx8", 48, 11008, 4096): 0,
    ("kx8", 49, 11008, 4096): 8630272,
    ("kx8", 128, 11008, 4096): 22544384,
    ("kx8", 300, 11008, 4096): 22544384,
    ("1x16", 1, 11008, 4096): 2818048,
    ("1x16", 7, 11008, 4096): 2818048,
    ("1x16", 16, 11008, 4096): 5636096,
    ("1x16", 128, 11008, 4096): 45088768,
    ("1x16", 300, 11008, 4096): 105676800,
    ("1x16", 1, 4096, 11008): 4194304,
    ("1x16", 7, 4096, 11008): 4194304,
    ("1x16", 16, 4096, 11008): 6291456,
    ("1x16", 128, 4096, 11008): 50331648,
    ("1x16", 300, 4096, 11008): 117964800,
    ("1x16", 8, 4096, 4160): 4194304,
    ("1x16", 128, 4096, 4160): 16777216,
    ("1x16", 8, 4096, 4096): 4194304,
}


def test_workspace_bytes_are_unchanged(native):
    ops = {"kx8": native.OP_GEMM_KX8_MFMA, "1x16": native.OP_GEMM_1X16_MFMA}
    assert len(WORKSPACE_BYTES) >= 20
    for (op, batch, out, inf), want in WORKSPACE_BYTES.items():
        assert native.lib.aqlm_hip_workspace_bytes(ops[op], batch, out, inf) == want, (op, batch, out, inf)
