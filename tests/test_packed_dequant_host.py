"""W straight from packed 1x16 codes (aqlm_hip_dequant_1x16_packed), the parts that need no GPU: the entry is exported and bound as
the header declares it, it validates its arguments before touching the device, the route predicate of a dropped layer follows the
table of DESIGN section 7, and the dispatcher op has a fake implementation."""
import ctypes
import itertools
import re

import pytest

torch = pytest.importorskip("torch")

ENTRY = "aqlm_hip_dequant_1x16_packed"


@pytest.fixture(scope="module")
def native():
    from aqlm_amd import _native

    return _native


def _good_desc(native):
    """64 x 512, g8, uniform 16 x 16 geometry, 4 waves x 1 step (the descriptor tests/test_abi.py validates the matvec entry with)."""
    uniform = (ctypes.c_uint8 * 32)(*([16] * 16))
    return native.PackedDesc(0x37505141, 7, 64, 512, 4, 4, 1, 4, 1024 * (74 + 1024), 4, 1.5, 0, 4, uniform)


def test_entry_is_exported_and_bound_as_declared(native):
    import os

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "aqlm_hip.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+" + ENTRY + r"\s*\(([^;]*)\)\s*;", text)
    assert m, "the header does not declare the entry"
    params = [p.strip() for p in m.group(1).split(",")]
    assert len(params) == 7 and params[0].startswith("const aqlm_hip_packed_desc*") and params[5].startswith("int ")
    restype, argtypes = native.SIGNATURES[ENTRY]
    assert restype is ctypes.c_int and len(argtypes) == 7
    assert argtypes[0] is native._descp and argtypes[5] is ctypes.c_int
    assert all(a is ctypes.c_void_p for i, a in enumerate(argtypes) if i not in (0, 5))
    assert hasattr(ctypes.CDLL(native.LIB_PATH), ENTRY), "libaqlm_hip.so does not export the entry"
    assert native.lib.aqlm_hip_abi_version() == native.ABI_VERSION == 9   # additive: the ABI version stays


def test_argument_validation_without_gpu(native):
    fn = getattr(native.lib, ENTRY)
    buf = ctypes.create_string_buffer(4096 + 16)
    p = (ctypes.addressof(buf) + 15) & ~15
    good = _good_desc(native)
    for args in [(None, p, p, None, p), (ctypes.byref(good), None, p, None, p), (ctypes.byref(good), p, None, None, p),
                 (ctypes.byref(good), p, p, None, None)]:
        rc = fn(*args, native.F16, None)
        assert rc == native.E_INVALID and "null pointer" in native.last_error(), args
    zero = native.PackedDesc()
    rc = fn(ctypes.byref(zero), p, p, None, p, native.F16, None)
    assert rc == native.E_INVALID and "descriptor" in native.last_error()
    odd = native.PackedDesc.from_ints(good.as_ints())
    odd.slice_groups[3] = 17   # row groups that do not add up to the 256 workgroups
    rc = fn(ctypes.byref(odd), p, p, None, p, native.F16, None)
    assert rc == native.E_INVALID and "descriptor" in native.last_error()
    rc = fn(ctypes.byref(good), p, p, None, p + 2, native.F16, None)
    assert rc == native.E_INVALID and "16-byte aligned" in native.last_error()
    rc = fn(ctypes.byref(good), p, p, None, p, 7, None)
    assert rc == native.E_UNSUPPORTED and "float16 and bfloat16" in native.last_error()
    rc = fn(ctypes.byref(good), p, p, p, p, 7, None)
    assert rc == native.E_UNSUPPORTED
    # the 16-element twin validates the same way (a descriptor with 32 slices is forwarded to it)
    g16 = native.PackedDesc.from_ints(good.as_ints())
    g16.slices_log2 = 5
    rc = fn(ctypes.byref(g16), p, p, None, p, native.F16, None)
    assert rc == native.E_INVALID and "descriptor" in native.last_error()
    # relabelled: neither the codebook image nor its flag is asked for (the matvec entry refuses such a descriptor, tests/test_abi.py)
    relab = native.PackedDesc.from_ints(good.as_ints())
    relab.flags = native.PACKED_RELABELLED
    relab.used_bytes = 1024 * (74 + 1024) + 65536 * 2 + 65536 * 16
    rc = fn(ctypes.byref(relab), p, p, None, p, 7, None)
    assert rc == native.E_UNSUPPORTED and "float16 and bfloat16" in native.last_error()   # i.e. it passed the descriptor checks


def test_route_table_of_a_dropped_layer():
    """The table of DESIGN section 7, cell by cell, then exhaustively against its statement in words."""
    from aqlm_amd import inference as inf

    R = inf.dropped_layer_route
    assert inf.GEMV_MAX_ROWS == 6 and inf.PACKED_DEQUANT_ABOVE_ROWS == 256
    # (dropped, strict, rows_from_packed, rows, in % 64, grad) -> route
    table = [
        ((False, True, 0, 300, 0, False), inf.ROUTE_CANONICAL),
        ((False, False, 7, 9, 0, True), inf.ROUTE_CANONICAL),
        ((True, True, 0, 1, 0, False), inf.ROUTE_PACKED_MATVEC),            # <= 6 rows: unchanged
        ((True, False, 0, 6, 0, False), inf.ROUTE_PACKED_MATVEC),
        ((True, False, 7, 6, 8, False), inf.ROUTE_PACKED_MATVEC),
        ((True, False, 0, 7, 0, False), inf.ROUTE_RESTORE),                 # 7 .. 256 rows, in % 64 == 0, no opt-in: unchanged
        ((True, False, 0, 256, 0, False), inf.ROUTE_RESTORE),
        ((True, True, 0, 7, 0, False), inf.ROUTE_TRANSIENT_UNPACK),
        ((True, True, 0, 256, 0, False), inf.ROUTE_TRANSIENT_UNPACK),
        ((True, True, 0, 257, 0, False), inf.ROUTE_PACKED_DEQUANT),         # > 256 rows
        ((True, False, 0, 300, 0, False), inf.ROUTE_PACKED_DEQUANT),
        ((True, False, 0, 300, 0, True), inf.ROUTE_PACKED_DEQUANT),         # ... with a gradient too
        ((True, True, 0, 9, 8, False), inf.ROUTE_PACKED_DEQUANT),           # in % 64 != 0 at 7+ rows
        ((True, False, 0, 9, 8, True), inf.ROUTE_PACKED_DEQUANT),
        ((True, True, 7, 9, 0, False), inf.ROUTE_PACKED_DEQUANT),           # the opt-in: any no-grad forward of >= 7 rows
        ((True, True, 7, 7, 0, False), inf.ROUTE_PACKED_DEQUANT),
        ((True, True, 7, 64, 0, False), inf.ROUTE_PACKED_DEQUANT),
        ((True, True, 32, 31, 0, False), inf.ROUTE_TRANSIENT_UNPACK),       # below the layer's own threshold
        ((True, True, 7, 9, 0, True), inf.ROUTE_TRANSIENT_UNPACK),          # the opt-in is for no-grad forwards
        ((True, False, 7, 9, 0, True), inf.ROUTE_RESTORE),
        ((True, True, 0, 2, 0, True), inf.ROUTE_TRANSIENT_UNPACK),          # <= 6 rows with a gradient: the matvec op on the codes
        ((True, False, 0, 2, 0, True), inf.ROUTE_RESTORE),
        ((True, True, 1, 3, 0, False), inf.ROUTE_PACKED_MATVEC),            # a threshold below 7 never takes decode calls
    ]
    for args, want in table:
        assert R(*args) == want, args
    for dropped, strict, rfp, rows, mod, grad in itertools.product((False, True), (False, True), (0, 7, 100), (1, 6, 7, 99, 100, 256, 257, 4096),
                                                                   (0, 8), (False, True)):
        got = R(dropped, strict, rfp, rows, mod, grad)
        if not dropped:
            want = inf.ROUTE_CANONICAL
        elif rows <= 6 and not grad:
            want = inf.ROUTE_PACKED_MATVEC
        elif rows >= 7 and (rows > 256 or mod != 0 or (rfp and rows >= rfp and not grad)):
            want = inf.ROUTE_PACKED_DEQUANT
        else:
            want = inf.ROUTE_TRANSIENT_UNPACK if strict else inf.ROUTE_RESTORE
        assert got == want, (dropped, strict, rfp, rows, mod, grad)


def test_route_threshold_is_the_large_batch_ops_own():
    from aqlm_amd import inference as inf
    from aqlm_amd.inference_kernels import hip_kernel

    assert inf.PACKED_DEQUANT_ABOVE_ROWS == hip_kernel.FUSED_MFMA_MAX_ROWS
    m = inf.QuantizedLinear(512, 64, 8, 1, 1, 16, bias=False, device="meta", dtype=torch.float16)
    assert m.rows_from_packed == 0   # the opt-in is off unless asked for


def test_dispatcher_op_has_a_fake_implementation(native):
    from aqlm_amd.inference_kernels import hip_kernel  # noqa: F401  (registers the ops)

    ints = _good_desc(native).as_ints()
    for dtype in (torch.float16, torch.bfloat16):
        packed = torch.empty(4096, device="meta", dtype=torch.uint8)
        cb = torch.empty(1, 65536, 1, 8, device="meta", dtype=dtype)
        sc = torch.empty(64, 1, 1, 1, device="meta", dtype=dtype)
        for scales in (None, sc):
            for desc in (ints, ints + [0, -1]):   # with and without the codebook fingerprint `PackedCodes.op_ints()` appends
                w = torch.ops.aqlm.code1x16_dequant_packed(packed, cb, scales, desc)
                assert w.shape == (64, 512) and w.dtype == dtype and w.device.type == "meta"
