"""CPU-only checks of the C-ABI boundary: the library loads (no GPU needed), exports every symbol that
include/aqlm_hip.h declares, and rejects bad arguments before touching the device."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def native():
    from aqlm_amd import _native

    return _native


def header_symbols():
    text = open(os.path.join(ROOT, "include", "aqlm_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(aqlm_hip_[a-z0-9_]+)\s*\(", text)))


def test_header_and_binding_agree(native):
    syms = header_symbols()
    assert len(syms) >= 11
    assert sorted(native.SIGNATURES) == syms
    raw = ctypes.CDLL(native.LIB_PATH)
    for s in syms:
        assert hasattr(raw, s), f"libaqlm_hip.so does not export {s}"


def test_g16_twins_of_the_packed_entries_stay_hidden(native):
    """The packed 1x16 entries are built a second time for 16-element vectors as aqlm_hip_g16_*: reached through the public
    entries only, never exported."""
    packed = [s for s in native.SIGNATURES if "pack" in s]
    assert len(packed) >= 22
    raw = ctypes.CDLL(native.LIB_PATH)
    for s in packed:
        twin = "aqlm_hip_g16_" + s[len("aqlm_hip_"):]
        assert not hasattr(raw, twin), f"libaqlm_hip.so exports {twin}"


def test_abi_version_and_error_string(native):
    assert native.lib.aqlm_hip_abi_version() == native.ABI_VERSION == 9
    assert isinstance(native.last_error(), str)


def test_argument_validation_without_gpu(native):
    L = native.lib
    # null pointers
    rc = L.aqlm_hip_gemv_1x16(None, None, None, None, None, None, 64, 512, 8, 1, 512, 64, native.F16, None)
    assert rc == native.E_INVALID and "null pointer" in native.last_error()
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.addressof(buf)
    # sizes
    rc = L.aqlm_hip_gemv_1x16(p, p, p, None, p, p, 64, 500, 8, 1, 512, 64, native.F16, None)
    assert rc == native.E_INVALID and "multiple of in_group_size" in native.last_error()
    # batch too large for the gemv entry point
    rc = L.aqlm_hip_gemv_1x16(p, p, p, None, p, p, 64, 512, 8, 9, 512, 64, native.F16, None)
    assert rc == native.E_UNSUPPORTED
    # dtype: mirrors check_use_bfloat16 (reference cuda_kernel.cpp:9-25)
    rc = L.aqlm_hip_gemv_kx8(p, p, p, None, p, p, 64, 512, 2, 8, 1, 512, 64, 7, None)
    assert rc == native.E_UNSUPPORTED and "float16 and bfloat16" in native.last_error()
    # 1x16 group size: mirrors cuda_kernel.cpp:136-145
    rc = L.aqlm_hip_gemv_1x16(p, p, p, None, p, p, 64, 512, 4, 1, 512, 64, native.F16, None)
    assert rc == native.E_UNSUPPORTED and "8 or 16" in native.last_error()
    rc = L.aqlm_hip_dequant_1x16(p, p, None, p, 64, 512, 32, native.F16, None)
    assert rc == native.E_UNSUPPORTED
    rc = L.aqlm_hip_dequant_kx8(None, p, None, p, 64, 512, 2, 8, native.F16, None)
    assert rc == native.E_INVALID
    rc = L.aqlm_hip_gemm_1x16_mfma(p, p, p, None, p, p, 128, 4096, 4096, 8, 4096, 4096, native.F16, None, 0, None)
    assert rc == native.E_INVALID and "workspace" in native.last_error()
    with pytest.raises(NotImplementedError):
        native.check(native.E_UNSUPPORTED)
    with pytest.raises(ValueError):
        native.check(native.E_INVALID)


def good_packed_desc(native):
    """A valid descriptor of a 512 -> 64 layer: 4 waves x 1 step of 4-byte entries, 4 copies of x, |codebook| <= 1.5."""
    uniform = (ctypes.c_uint8 * 32)(*([16] * 16))
    return native.PackedDesc(0x37505141, 7, 64, 512, 4, 4, 1, 4, 1024 * (74 + 1024), 4, 1.5, 0, 4, uniform)


def test_segment_struct_and_multi_validation(native):
    # aqlm_hip_segment: 5 pointers + long + 2 ints, no padding surprises
    assert ctypes.sizeof(native.Segment) == 56
    assert native.Segment.y_row_stride.offset == 40 and native.Segment.out_features.offset == 48
    L = native.lib
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.addressof(buf)
    segs = (native.Segment * 2)()
    rc = L.aqlm_hip_gemv_1x16_multi(segs, 0, p, 512, 8, 1, 512, native.F16, None)
    assert rc == native.E_INVALID and "segments" in native.last_error()
    rc = L.aqlm_hip_gemv_1x16_multi(segs, native.MAX_SEGMENTS + 1, p, 512, 8, 1, 512, native.F16, None)
    assert rc == native.E_INVALID
    rc = L.aqlm_hip_gemv_1x16_multi(segs, 2, p, 512, 8, 1, 512, native.F16, None)  # null segment pointers
    assert rc == native.E_INVALID and "null pointer" in native.last_error()
    for s in segs:
        s.codes = s.codebook = s.scales = s.y = p
        s.out_features, s.y_row_stride = 64, 64
    rc = L.aqlm_hip_gemv_1x16_multi(segs, 2, p, 512, 4, 1, 512, native.F16, None)
    assert rc == native.E_UNSUPPORTED and "8 or 16" in native.last_error()
    rc = L.aqlm_hip_gemv_1x16_multi(segs, 2, p, 512, 8, 1, 512, 5, None)
    assert rc == native.E_UNSUPPORTED and "float16 and bfloat16" in native.last_error()
    # prepacked entry points: descriptors are validated before anything is launched
    assert ctypes.sizeof(native.PackedDesc) == 88
    assert L.aqlm_hip_prepack_1x16_bytes(4096, 4096, 8) > 2 * 4096 * 512 * 2
    assert L.aqlm_hip_prepack_1x16_bytes(4096, 4096, 16) > 2 * 4096 * 256 * 2   # 16-element vectors: the second instantiation
    assert L.aqlm_hip_prepack_1x16_bytes(4096, 4096, 32) == 0          # other group sizes are not packable
    assert L.aqlm_hip_prepack_1x16_bytes(64, 8 * 4095, 8) == 0         # in/8 > 4094: j does not fit 12 bits
    bad = native.PackedDesc()
    descs = (native._descp * 2)(ctypes.pointer(bad), ctypes.pointer(bad))
    rc = L.aqlm_hip_gemv_1x16_packed_multi(segs, descs, 2, p, 512, 1, 512, native.F16, p, 1 << 20, None)
    assert rc == native.E_INVALID and "descriptor" in native.last_error()
    rc = L.aqlm_hip_gemv_1x16_packed(ctypes.byref(bad), p, p, p, None, p, p, 1, 512, 64, native.F16, p, 1 << 20, None)
    assert rc == native.E_INVALID and "descriptor" in native.last_error()
    # 64 rows -> 4 per row group; winfo (sized for 16 waves) + row starts (256 x 5 u32) + the accumulator cells of the
    # fused finalize (8 x 64 u64) end at 74 KiB, then 256 x 4 x 1 KiB of entries
    good = good_packed_desc(native)
    back = native.PackedDesc.from_ints(good.as_ints())
    assert bytes(back) == bytes(good)
    rc = L.aqlm_hip_gemv_1x16_packed(ctypes.byref(good), p, p, p, None, p, p, 9, 512, 64, native.F16, p, 1 << 20, None)
    assert rc == native.E_INVALID and "batch" in native.last_error()
    rc = L.aqlm_hip_gemv_1x16_packed(ctypes.byref(good), p, p, p, None, p, p, 1, 512, 64, 7, p, 1 << 20, None)
    assert rc == native.E_UNSUPPORTED
    hdr = ctypes.create_string_buffer(bytes(good), 128)
    out = native.PackedDesc()
    assert L.aqlm_hip_packed_desc_read(ctypes.addressof(hdr), 128, ctypes.byref(out)) == 0 and bytes(out) == bytes(good)
    assert L.aqlm_hip_packed_desc_read(ctypes.addressof(hdr), 64, ctypes.byref(out)) == native.E_INVALID   # shorter than the descriptor
    assert L.aqlm_hip_packed_desc_read(ctypes.addressof(buf), 128, ctypes.byref(out)) == native.E_INVALID
    # format v7: a relabelled buffer refuses to run before its codebook image has been written
    relab = native.PackedDesc.from_ints(good.as_ints())
    relab.flags = native.PACKED_RELABELLED
    relab.used_bytes = 1024 * (74 + 1024) + 65536 * 2 + 65536 * 16
    rc = L.aqlm_hip_gemv_1x16_packed(ctypes.byref(relab), p, p, p, None, p, p, 1, 512, 64, native.F16, p, 1 << 20, None)
    assert rc == native.E_INVALID and "aqlm_hip_packed_set_codebook" in native.last_error()
    # ... and a descriptor whose row groups do not add up to the 256 workgroups is not a descriptor
    odd = native.PackedDesc.from_ints(good.as_ints())
    odd.slice_groups[3] = 17
    rc = L.aqlm_hip_gemv_1x16_packed(ctypes.byref(odd), p, p, p, None, p, p, 1, 512, 64, native.F16, p, 1 << 20, None)
    assert rc == native.E_INVALID and "descriptor" in native.last_error()


def packed_multi_malformed_calls(native, p):
    """-> [(name, call)]: malformed calls of aqlm_hip_gemv_1x16_packed_multi / _multi_cells of two segments; `p`: 16-B aligned host
    memory that stands for every buffer.  Every one of them is refused by a check that stands in front of the first launch (read
    in packed_gemv_entries.h), so none needs a GPU."""
    from tests import packed_model as pm

    L = native.lib

    def variant(out=64, entry_bytes=4, groups=None, flags=0, absmax=1.5):
        d = good_packed_desc(native)
        lay = pm.layout(out, 512 // 8, 4, 1, entry_bytes, groups, bool(flags & native.PACKED_RELABELLED))
        d.out_features, d.entry_bytes, d.flags, d.codebook_absmax = out, entry_bytes, flags, absmax
        d.rows_per_group, d.used_bytes = lay["RG"], lay["used"]
        if groups:
            d.slice_groups = (ctypes.c_uint8 * 32)(*groups)
        return d

    good = good_packed_desc(native)
    assert bytes(variant()) == bytes(good)
    norange = variant(absmax=0.0)                                   # no codebook range: two-kernel finalize, needs the workspace
    relab = variant(flags=native.PACKED_RELABELLED)                 # relabelled, codebook image never written
    three = variant(entry_bytes=3)
    vg = variant(out=512, groups=[17, 15] + [16] * 14, flags=native.PACKED_VARGEOM)   # 512 rows: the fewest with variable geometry

    def segs(*outs, **null):
        a = (native.Segment * len(outs))()
        for k, (s, out) in enumerate(zip(a, outs)):
            s.codes = s.codebook = s.scales = s.y = p
            s.out_features, s.y_row_stride = out, out
            if null.get("codes") == k:
                s.codes = None
        return a

    def descs(*ds):
        return (native._descp * len(ds))(*[ctypes.pointer(d) if d is not None else native._descp() for d in ds])

    def multi(sg, ds, n=2, x=p, in_features=512, batch=1, xs=512, dtype=native.F16, ws=p, ws_bytes=1 << 20):
        return lambda: L.aqlm_hip_gemv_1x16_packed_multi(sg, ds, n, x, in_features, batch, xs, dtype, ws, ws_bytes, None)

    def cells(sg, ds, c=p, c_bytes=1 << 20):
        return lambda: L.aqlm_hip_gemv_1x16_packed_multi_cells(sg, ds, 2, p, 512, 1, 512, native.F16, c, c_bytes, None)

    two, gg = segs(64, 64), descs(good, good)
    return [
        ("null segments", multi(None, gg)),
        ("null descs", multi(two, None)),
        ("0 segments", multi(two, gg, n=0)),
        ("MAX_SEGMENTS + 1 segments", multi(two, gg, n=native.MAX_SEGMENTS + 1)),
        ("dtype 7", multi(two, gg, dtype=7)),
        ("batch 0", multi(two, gg, batch=0)),
        ("batch 9", multi(two, gg, batch=9)),
        ("x misaligned by 2", multi(two, gg, x=p + 2)),
        ("batch 2, x_row_stride 12", multi(two, gg, batch=2, xs=12)),
        ("null descriptor in slot 1", multi(two, descs(good, None))),
        ("in_features differs from the argument", multi(two, gg, in_features=1024)),
        ("out_features differs from the segment's", multi(segs(64, 128), gg)),
        ("null codes in slot 1", multi(segs(64, 64, codes=1), gg)),
        ("null codes in slot 0, null descriptor in slot 1", multi(segs(64, 64, codes=0), descs(good, None))),
        ("null codes and null descriptor in slot 1", multi(segs(64, 64, codes=1), descs(good, None))),
        ("relabelled without its codebook image in slot 1", multi(two, descs(good, relab))),
        ("3- and 4-byte entries mixed", multi(two, descs(good, three))),
        ("no codebook range, workspace one byte short", multi(two, descs(norange, norange), ws_bytes=2 * 16 * 64 * 4 - 1)),
        ("cells: null cells", cells(two, gg, c=None)),
        ("cells: misaligned by 4", cells(two, gg, c=p + 4)),
        ("cells: descriptor without the range", cells(two, descs(good, norange))),
        ("cells: cells_bytes one short", cells(two, gg, c_bytes=2 * 64 * 8 - 1)),
        # a variable-geometry descriptor sends the call down the one-launch-per-segment path, which checks segment k only after
        # it has launched segment k - 1: the mismatch stands in slot 0, the descriptor that selects the path behind it
        ("variable geometry in slot 1, out_features mismatch in slot 0", multi(segs(128, 512), descs(good, vg))),
        ("variable geometry in slot 1, null descriptor in slot 0", multi(segs(64, 512), descs(None, vg))),
    ]


def test_packed_multi_rejections_are_unchanged(native):
    """Which malformed call of the shared-input packed entries is refused with which code and message: recorded from the library
    as it was before gemv_1x16_packed_multi_impl began to compute its segments' layouts once, up front."""
    multi, cells = "aqlm_hip_gemv_1x16_packed_multi: ", "aqlm_hip_gemv_1x16_packed_multi_cells: "
    expected = {
        "null segments": (-1, multi + "1..4 segments, their descriptors and a non-null x required (got 2)"),
        "null descs": (-1, multi + "1..4 segments, their descriptors and a non-null x required (got 2)"),
        "0 segments": (-1, multi + "1..4 segments, their descriptors and a non-null x required (got 0)"),
        "MAX_SEGMENTS + 1 segments": (-1, multi + "1..4 segments, their descriptors and a non-null x required (got 5)"),
        "dtype 7": (-2, multi + "AQLM HIP kernels only support float16 and bfloat16 (dtype id 7)"),
        "batch 0": (-1, multi + "batch must be 1..8 with 16-B aligned rows (batch 0)"),
        "batch 9": (-1, multi + "batch must be 1..8 with 16-B aligned rows (batch 9)"),
        "x misaligned by 2": (-1, multi + "batch must be 1..8 with 16-B aligned rows (batch 1)"),
        "batch 2, x_row_stride 12": (-1, multi + "batch must be 1..8 with 16-B aligned rows (batch 2)"),
        "null descriptor in slot 1": (-1, multi + "segment 1: invalid descriptor, or it does not match in_features 512 / out_features 64"),
        "in_features differs from the argument": (-1, multi + "segment 0: invalid descriptor, or it does not match in_features 1024 / out_features 64"),
        "out_features differs from the segment's": (-1, multi + "segment 1: invalid descriptor, or it does not match in_features 512 / out_features 128"),
        "null codes in slot 1": (-1, multi + "null pointer in segment 1"),
        "null codes in slot 0, null descriptor in slot 1": (-1, multi + "null pointer in segment 0"),
        "null codes and null descriptor in slot 1": (-1, multi + "null pointer in segment 1"),
        "relabelled without its codebook image in slot 1": (-1, multi + "segment 1: a relabelled buffer needs its codebook image (aqlm_hip_packed_set_codebook)"),
        "3- and 4-byte entries mixed": (-2, multi + "segments mix 3- and 4-byte entry formats"),
        "no codebook range, workspace one byte short": (-1, multi + "workspace of 8192 bytes required, got 8191"),
        "cells: null cells": (-1, cells + "needs 8-B aligned, zero-filled cells and the fused finalize switched on"),
        "cells: misaligned by 4": (-1, cells + "needs 8-B aligned, zero-filled cells and the fused finalize switched on"),
        "cells: descriptor without the range": (-1, cells + "every descriptor must carry the codebook range"),
        "cells: cells_bytes one short": (-1, cells + "1024 bytes of cells required, got 1023"),
        "variable geometry in slot 1, out_features mismatch in slot 0": (-1, multi + "segment 0: descriptor does not match in_features 512 / out_features 128"),
        "variable geometry in slot 1, null descriptor in slot 0": (-1, multi + "segment 0: descriptor does not match in_features 512 / out_features 64"),
    }
    buf = ctypes.create_string_buffer(4096 + 16)
    calls = packed_multi_malformed_calls(native, (ctypes.addressof(buf) + 15) & ~15)
    assert len(calls) == len(expected) >= 16
    for name, call in calls:
        rc = call()
        assert (rc, native.last_error()) == expected[name], name


def test_workspace_bytes(native):
    L = native.lib
    n = L.aqlm_hip_workspace_bytes(native.OP_GEMM_1X16_MFMA, 128, 4096, 4096)
    assert n > 0 and n % (4096 * 128 * 4) == 0
    assert L.aqlm_hip_workspace_bytes(99, 128, 4096, 4096) == 0
    assert L.aqlm_hip_workspace_bytes(native.OP_GEMM_1X16_MFMA, 7, 4096, 4096) < n
    assert L.aqlm_hip_workspace_bytes(native.OP_GEMV_1X16_PACKED, 1, 4096, 4096) == 16 * 4096 * 4
    assert L.aqlm_hip_workspace_bytes(native.OP_GEMV_1X16_PACKED, 4, 11008, 4096) == 16 * 4 * 11008 * 4
    assert L.aqlm_hip_workspace_bytes(native.OP_GEMV_1X16_G16_PACKED, 4, 11008, 4096) == 32 * 4 * 11008 * 4


def test_tuning_knobs(native):
    assert native.get_tuning("gemv_rows_per_wave") == 0
    native.set_tuning("gemv_rows_per_wave", 3)
    assert native.get_tuning("gemv_rows_per_wave") == 3
    native.set_tuning("gemv_rows_per_wave", 0)
    with pytest.raises(ValueError):
        native.set_tuning("no_such_knob", 1)


def test_scan_entry_validation_and_plan_without_gpu(native):
    """aqlm_hip_gemm_1x16_scan (round 6): argument checks and the plan behind the workspace size -- 8 codebook slices x the K chunks
    the x fragments' registers ask for (<= 3 units of 256 features per wave at <= 16 rows, <= 2 at 17+ rows)."""
    L = native.lib
    buf = ctypes.create_string_buffer(4096)
    p = (ctypes.addressof(buf) + 15) & ~15
    ws = L.aqlm_hip_gemm_1x16_scan_workspace_bytes
    assert ws(8, 4096, 4096) == 8 * 1 * 8 * 4096 * 4          # one chunk: 16 units over 8 waves x 2
    assert ws(16, 11008, 4096) == 8 * 1 * 16 * 11008 * 4
    assert ws(8, 4096, 11008) == 8 * 3 * 8 * 4096 * 4         # 43 units: 3 chunks of 15 / 14 / 14 units (8 waves x 2 units each)
    assert ws(32, 4096, 11008) == 8 * 3 * 32 * 4096 * 4       # the K chunking does not depend on the row count (batch invariance)
    assert ws(8, 4096, 14336) == 8 * 4 * 8 * 4096 * 4
    assert ws(8, 4096, 4096 + 64) == 0 and ws(0, 4096, 4096) == 0   # in_features % 256 != 0: no plan
    assert L.aqlm_hip_workspace_bytes(native.OP_GEMM_1X16_MFMA, 16, 11008, 4096) >= ws(16, 11008, 4096)
    rc = L.aqlm_hip_gemm_1x16_scan(None, p, p, None, p, p, 8, 4096, 4096, 4096, 4096, native.F16, p, 1 << 30, None)
    assert rc == native.E_INVALID and "null pointer" in native.last_error()
    rc = L.aqlm_hip_gemm_1x16_scan(p, p, p, None, p, p, 8, 4096, 4160, 4160, 4096, native.F16, p, 1 << 30, None)
    assert rc == native.E_UNSUPPORTED and "256" in native.last_error()
    rc = L.aqlm_hip_gemm_1x16_scan(p, p, p, None, p, p, 8, 4096, 4096, 4096, 4096, 7, p, 1 << 30, None)
    assert rc == native.E_UNSUPPORTED and "float16 and bfloat16" in native.last_error()
    rc = L.aqlm_hip_gemm_1x16_scan(p, p, p, None, p, p, 8, 4096, 4096, 4096, 4096, native.F16, p, 64, None)
    assert rc == native.E_INVALID and "workspace" in native.last_error()
    assert native.get_tuning("scan_max_rows") == 0              # not on a default route (measured slower: gemm_1x16_scan.hip)
    native.set_tuning("scan_max_rows", 64)
    assert native.get_tuning("scan_max_rows") == 64
    native.set_tuning("scan_max_rows", 0)
