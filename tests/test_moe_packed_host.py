"""Mixtral decode on prepacked experts, the parts that need no GPU: the C ABI of the routed packed launch
(aqlm_hip_gemv_1x16_routed_packed and its helpers) against header and bindings, its argument checks, the entry / geometry helpers
on a hand-made descriptor, the launch's LDS size on the Mixtral-8x7B shapes, the route predicate as a table, that
``prepack_model`` still leaves experts alone, and the resource report of the new kernel (no scratch)."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
ISA_FLAGS = ["-O3", "-std=c++17", "--offload-arch=gfx950", "-fPIC", "-ffp-contract=fast", "-mllvm",
             "-amdgpu-kernarg-preload-count=14", "--cuda-device-only", "-S"]
NEW_ENTRIES = ["aqlm_hip_gemv_1x16_routed_packed", "aqlm_hip_gemv_1x16_routed_packed_geometry",
               "aqlm_hip_gemv_1x16_routed_packed_supported", "aqlm_hip_gemv_1x16_routed_packed_lds_bytes",
               "aqlm_hip_routed_packed_entry_fill"]


def _good_desc(nat, waves=4, steps=1):
    """The 64 x 512 g8 descriptor of tests/test_abi.py: 4 rows per row group, 4 waves x 1 step, |codebook| <= 1.5."""
    uniform = (ctypes.c_uint8 * 32)(*([16] * 16))
    return nat.PackedDesc(0x37505141, 7, 64, 512, 4, waves, steps, 4, 1024 * (74 + 256 * waves * steps), 4, 1.5, 0, 4, uniform)


def test_header_exports_and_bindings_agree_and_abi_stays_9():
    from aqlm_amd import _native as nat

    text = open(os.path.join(ROOT, "include", "aqlm_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(aqlm_hip_[a-z0-9_]+)\s*\(", text))
    raw = ctypes.CDLL(nat.LIB_PATH)
    for name in NEW_ENTRIES:
        assert name in declared, f"include/aqlm_hip.h does not declare {name}"
        assert name in nat.SIGNATURES, f"_native.SIGNATURES lacks {name}"
        assert hasattr(raw, name), f"libaqlm_hip.so does not export {name}"
    assert nat.lib.aqlm_hip_abi_version() == nat.ABI_VERSION == 9
    assert "#define AQLM_HIP_ABI_VERSION 9" in open(os.path.join(ROOT, "include", "aqlm_hip.h")).read()
    # the structs: 6 pointers + 8 words, and 8 words -- what the header declares
    assert ctypes.sizeof(nat.RoutedPackedEntry) == 80 and nat.ROUTED_PACKED_ENTRY_WORDS == 10
    assert nat.RoutedPackedEntry.out_features.offset == 48 and nat.RoutedPackedEntry.codebook_absmax.offset == 72
    assert ctypes.sizeof(nat.RoutedPackedGeometry) == 32


def test_entry_fill_and_geometry_on_a_descriptor_without_a_gpu():
    from aqlm_amd import _native as nat

    L = nat.lib
    buf = ctypes.create_string_buffer(1 << 16)
    p = (ctypes.addressof(buf) + 15) // 16 * 16
    good = _good_desc(nat)
    ent = nat.RoutedPackedEntry()
    assert L.aqlm_hip_routed_packed_entry_fill(ctypes.byref(good), p, p + 4096, p + 8192, None, ctypes.byref(ent)) == 0
    # offsets of format v6 / v7 (tests/test_abi.py): winfo at 256, row starts behind the 16-wave info, 256 KiB of entries at 74 KiB
    assert ent.wave_info == p + 256 and ent.row_starts == p + 256 + 256 * 16 * 16 and ent.entries == p + 74 * 1024
    assert ent.codebook == p + 4096 and ent.scales == p + 8192 and not ent.bias
    assert (ent.out_features, ent.rows_per_group, ent.waves, ent.steps, ent.x_copies) == (64, 4, 4, 1, 4)
    assert ent.entry_stream_bytes == 256 * 4 * 1024 and ent.codebook_absmax == 1.5
    assert L.aqlm_hip_routed_packed_entry_fill(ctypes.byref(good), None, p, p, None, ctypes.byref(ent)) == nat.E_INVALID
    assert "null pointer" in nat.last_error()
    assert L.aqlm_hip_routed_packed_entry_fill(ctypes.byref(good), p + 8, p, p, None, ctypes.byref(ent)) == nat.E_INVALID
    assert "aligned" in nat.last_error()
    # what the launch declines: no codebook range, a relabelled buffer without its image, garbage
    norange = nat.PackedDesc.from_ints(good.as_ints())
    norange.codebook_absmax = 0.0
    assert L.aqlm_hip_routed_packed_entry_fill(ctypes.byref(norange), p, p, p, None, ctypes.byref(ent)) == nat.E_UNSUPPORTED
    assert "codebook range" in nat.last_error()
    relab = nat.PackedDesc.from_ints(good.as_ints())
    relab.flags = nat.PACKED_RELABELLED
    relab.used_bytes = int(good.used_bytes) + 65536 * 2 + 65536 * 16
    assert L.aqlm_hip_routed_packed_entry_fill(ctypes.byref(relab), p, p, p, None, ctypes.byref(ent)) == nat.E_INVALID
    assert "aqlm_hip_packed_set_codebook" in nat.last_error()
    bad = nat.PackedDesc()
    assert L.aqlm_hip_routed_packed_entry_fill(ctypes.byref(bad), p, p, p, None, ctypes.byref(ent)) == nat.E_INVALID
    assert "descriptor" in nat.last_error()

    # geometry: the launch-wide maximum of the wave counts; one table holds one shape
    other = _good_desc(nat, waves=6, steps=2)
    descs = (nat._descp * 2)(ctypes.pointer(good), ctypes.pointer(other))
    geom = nat.RoutedPackedGeometry()
    assert L.aqlm_hip_gemv_1x16_routed_packed_geometry(descs, 2, ctypes.byref(geom)) == 0
    assert (geom.out_features, geom.in_features, geom.in_group_size, geom.rows_per_group, geom.max_waves) == (64, 512, 8, 4, 6)
    assert 0 < geom.lds_bytes <= 160 * 1024 and geom.lds_bytes == L.aqlm_hip_gemv_1x16_routed_packed_lds_bytes(64, 512, 8)
    assert L.aqlm_hip_gemv_1x16_routed_packed_supported(descs, 2) == 1
    descs = (nat._descp * 2)(ctypes.pointer(good), ctypes.pointer(norange))
    assert L.aqlm_hip_gemv_1x16_routed_packed_supported(descs, 2) == 0
    assert L.aqlm_hip_gemv_1x16_routed_packed_geometry(descs, 2, ctypes.byref(geom)) == nat.E_UNSUPPORTED
    assert L.aqlm_hip_gemv_1x16_routed_packed_geometry(descs, 0, ctypes.byref(geom)) == nat.E_INVALID
    descs = (nat._descp * 2)(ctypes.pointer(good), ctypes.pointer(bad))
    assert L.aqlm_hip_gemv_1x16_routed_packed_geometry(descs, 2, ctypes.byref(geom)) == nat.E_INVALID


def test_routed_packed_entry_rejects_bad_arguments_without_a_gpu():
    from aqlm_amd import _native as nat

    L = nat.lib
    buf = ctypes.create_string_buffer(1 << 16)
    p = (ctypes.addressof(buf) + 15) // 16 * 16
    good = _good_desc(nat)
    descs = (nat._descp * 1)(ctypes.pointer(good))
    geom = nat.RoutedPackedGeometry()
    assert L.aqlm_hip_gemv_1x16_routed_packed_geometry(descs, 1, ctypes.byref(geom)) == 0
    need = 2 * 2 * 64 * 8  # pairs x segments x out_features cells
    args = lambda **kw: [kw.get(n, d) for n, d in (  # noqa: E731
        ("table", p), ("geom", ctypes.byref(geom)), ("E", 8), ("S", 2), ("ids", p), ("i64", 1), ("pairs", 2), ("k", 2), ("x", p),
        ("xs", 512), ("per_pair", 0), ("y", p), ("dt", nat.F16), ("cells", p), ("cells_bytes", need), ("stream", None))]
    call = L.aqlm_hip_gemv_1x16_routed_packed
    assert call(*args(table=None)) == nat.E_INVALID and "null pointer" in nat.last_error()
    assert call(*args(geom=None)) == nat.E_INVALID and "null pointer" in nat.last_error()
    assert call(*args(cells=None)) == nat.E_INVALID and "null pointer" in nat.last_error()
    assert call(*args(pairs=0)) == nat.E_INVALID and "pairs" in nat.last_error()
    assert call(*args(pairs=nat.MAX_ROUTED_PAIRS + 2)) == nat.E_INVALID and "pairs" in nat.last_error()
    assert call(*args(pairs=3)) == nat.E_INVALID  # not a multiple of top_k
    assert call(*args(E=nat.MAX_ROUTED_EXPERTS + 1)) == nat.E_INVALID and "experts" in nat.last_error()
    assert call(*args(S=3)) == nat.E_INVALID
    assert call(*args(ids=p + 4)) == nat.E_INVALID and "misaligned" in nat.last_error()
    assert call(*args(x=p + 8)) == nat.E_INVALID and "16-byte aligned" in nat.last_error()
    assert call(*args(xs=516)) == nat.E_INVALID and "16-byte aligned" in nat.last_error()
    assert call(*args(cells=p + 4)) == nat.E_INVALID and "cells" in nat.last_error()
    assert call(*args(cells_bytes=need - 8)) == nat.E_INVALID and f"{need} bytes" in nat.last_error()
    assert call(*args(dt=2)) == nat.E_UNSUPPORTED and "float16 and bfloat16" in nat.last_error()
    zero = nat.RoutedPackedGeometry()
    assert call(*args(geom=ctypes.byref(zero))) == nat.E_INVALID and "geometry" in nat.last_error()


def test_launch_lds_fits_a_cu_on_the_mixtral_shapes():
    """Dynamic LDS is sized at launch from the table's common shape: the library's own size function at Mixtral-8x7B's row
    counts, both group sizes, stays within the 160 KiB of a CU (x window + 64 KiB slice + the row tables of a row group)."""
    from aqlm_amd import _native as nat

    size = nat.lib.aqlm_hip_gemv_1x16_routed_packed_lds_bytes
    worst = 0
    for g in (8, 16):
        for out_features, in_features in ((14336, 4096), (4096, 14336)):
            n = size(out_features, in_features, g)
            assert 64 * 1024 < n <= 160 * 1024, (g, out_features, in_features, n)
            worst = max(worst, n)
    assert worst <= 160 * 1024
    assert size(4096, 4096, 32) == 0 and size(64, 8 * 4095, 8) == 0  # shapes the packed format refuses


def test_route_predicate_is_a_pure_table(monkeypatch):
    import aqlm_amd.moe as moe

    monkeypatch.setattr(moe, "ROUTED_PACKED_MAX_PAIRS", 8)
    table = [  # prepacked, grad needed, pairs, supported -> taken
        ((True, False, 1, True), True), ((True, False, 8, True), True), ((True, False, 9, True), False),
        ((True, False, 0, True), False), ((False, False, 2, True), False), ((True, True, 2, True), False),
        ((True, False, 2, False), False), ((False, True, 64, False), False)]
    for args, want in table:
        assert moe.takes_routed_packed_route(*args) is want, args
    monkeypatch.setattr(moe, "ROUTED_PACKED_MAX_PAIRS", 1000)  # never beyond what one routed launch sequence is measured for
    assert moe.takes_routed_packed_route(True, False, moe.MAX_ROUTED_PAIRS, True)
    assert not moe.takes_routed_packed_route(True, False, moe.MAX_ROUTED_PAIRS + 1, True)
    monkeypatch.setattr(moe, "ROUTED_PACKED_MAX_PAIRS", 0)  # 0 switches the route off
    assert not moe.takes_routed_packed_route(True, False, 1, True)


def test_prepack_model_still_leaves_experts_alone_and_prepack_experts_is_opt_in(tmp_path, monkeypatch):
    pytest.importorskip("transformers")
    import aqlm_amd.moe as moe
    from aqlm_amd.moe import QuantizedMixtralExperts, prepack_experts
    from tests import moe_checkpoint as mc

    mc.build(tmp_path / "ckpt")
    model, _ = mc.load(str(tmp_path / "ckpt"), "cpu")
    blocks = [m for m in model.modules() if isinstance(m, QuantizedMixtralExperts)]
    assert blocks and all(b._prepack is None and b._packed_tables is None for b in blocks)
    for b in blocks:  # a block that was never prepacked never asks for packed tables
        monkeypatch.setattr(b, "routed_packed_tables", lambda device: pytest.fail("not prepacked: no packed tables"))
    x = torch.randn(3, mc.HID)
    ids = torch.tensor([[0, 1], [2, 3], [1, 2]])
    w = torch.full((3, 2), 0.5)
    with torch.no_grad():
        blocks[0](x.half(), ids, w)
    with pytest.raises(NotImplementedError, match="MI355X"):
        prepack_experts(model)  # host modules: there is no packed path to opt into
    assert all(b._prepack is None for b in blocks)
    assert "4.8 resident bits" in prepack_experts.__doc__ and "27 GB" in prepack_experts.__doc__
    assert isinstance(moe.ROUTED_PACKED_MAX_PAIRS, int) and 0 <= moe.ROUTED_PACKED_MAX_PAIRS <= moe.MAX_ROUTED_PAIRS


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
@pytest.mark.parametrize("src,ns", [("gemv_packed.hip", "pk_g8"), ("gemv_packed_g16.hip", "pk_g16")])
def test_routed_packed_kernel_isa_uses_no_scratch_and_counts_its_fill_loads(src, ns, tmp_path):
    """Zero scratch, and the body's invariant (tests/test_isa_invariants.py) inside the new wrapper: the first ``s_waitcnt vmcnt(N)``
    behind the last LDS-DMA of a pass waits for exactly the loads issued behind it (the entry ring + scale + bias) -- the wrapper
    calls the body in a loop, where a hoisted scale / bias load would leave the count two too high."""
    out = tmp_path / (src + ".s")
    subprocess.run([HIPCC] + ISA_FLAGS + [os.path.join(ROOT, "aqlm_amd", "csrc", src), "-o", str(out)], check=True,
                   stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=900)
    text = out.read_text()
    pattern = rf"_ZN4aqlm\d+{ns}\d+gemv_1x16_packed_routed_kernel\w+"
    names = set(re.findall(rf"^\s+\.name:\s+({pattern})", text, re.M))
    assert len(names) == 4, names  # fp16 / bf16 x the two LDS maps
    for m in re.finditer(rf"\.name:\s+({pattern})(.*?)(?=\n  - |\Z)", text, re.S):
        assert re.search(r"\.private_segment_fixed_size:\s+0\b", m.group(2)), m.group(1)
    checked = 0
    for name in names:
        body = re.split(rf"^{name}:", text, maxsplit=1, flags=re.M)[1].split(".Lfunc_end", 1)[0]
        assert not re.search(r"\b(scratch_|flat_)(load|store)", body), f"{name}: scratch or FLAT access"
        loads, seen_dma, waits = 0, False, []
        for line in body.split("\n"):
            if "global_load_lds" in line:
                loads, seen_dma = 0, True
            elif seen_dma and re.search(r"\b(global_load|buffer_load)_", line):
                loads += 1
            else:
                w = re.search(r"s_waitcnt vmcnt\((\d+)\)", line)
                if w and seen_dma:
                    waits.append((loads, int(w.group(1))))
                    seen_dma = False
        assert waits, f"{name}: no LDS fill found"
        assert all(a == b for a, b in waits), f"{name}: fill wait does not match the loads behind the LDS-DMA: {waits}"
        checked += 1
    assert checked == 4
