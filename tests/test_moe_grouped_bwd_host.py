"""The transposed grouped launch (the backward of the expert-grouped 1x16 GEMM) without a GPU: the two C entries in the header, the
prototype table and the built library, argument validation before any device call, the op's fake implementation, the module's
route predicate as a truth table, and the kernels' ISA (no scratch, MFMA, the transposed LDS read)."""
import ctypes
import itertools
import os
import re
import subprocess

import pytest
import torch

from tests.test_moe_gpu import HIPCC, ISA_FLAGS, ROOT

ENTRIES = ("aqlm_hip_gemm_1x16_grouped_transposed", "aqlm_hip_gemm_1x16_grouped_transposed_supported")


def test_entries_in_header_prototypes_and_library():
    from aqlm_amd import _native

    header = open(os.path.join(ROOT, "include", "aqlm_hip.h")).read()
    lib = _native.lib
    for name in ENTRIES:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), f"{name} is not declared in aqlm_hip.h"
        assert name in _native.SIGNATURES, f"{name} has no prototype in _native.py"
        assert getattr(lib, name) is not None
    assert "cuda_kernel.cpp" in header[header.index("Input gradient of aqlm_hip_gemm_1x16_grouped"):header.index("int " + ENTRIES[1] + "(")]
    assert lib.aqlm_hip_abi_version() == 9


def test_supported_shapes():
    from aqlm_amd.inference_kernels import hip_kernel as hk

    for g in (8, 16):
        for out_f, in_f in ((14336, 4096), (4096, 14336), (2048, 1024), (1024, 2048), (2064, 1088), (1088, 2064), (16, 64)):
            assert hk.grouped_transposed_supported(out_f, in_f, g), (out_f, in_f, g)
    assert not hk.grouped_transposed_supported(2048, 1024, 32)
    assert not hk.grouped_transposed_supported(2040, 1024, 8)
    assert not hk.grouped_transposed_supported(0, 1024, 8)


def test_argument_validation_without_gpu():
    from aqlm_amd import _native

    lib = _native.lib
    buf = (ctypes.c_char * 4096)()
    p = ctypes.addressof(buf)
    p += -p % 16

    def call(table=p, E=8, S=2, bucket=p + 1024, tp=16, P=32, gy=p + 2048, stride=2 * 64, gx=p + 3072, out_f=64, in_f=64, g=8, dt=0):
        return lib.aqlm_hip_gemm_1x16_grouped_transposed(table, E, S, bucket, tp, P, gy, stride, gx, out_f, in_f, g, dt, None)

    for bad in (dict(table=None), dict(bucket=None), dict(gy=None), dict(gx=None), dict(bucket=p + 1028), dict(E=0), dict(E=257),
                dict(S=0), dict(S=3), dict(P=0), dict(P=(1 << 18) + 1), dict(tp=48), dict(out_f=0), dict(in_f=60)):
        assert call(**bad) == _native.E_INVALID, bad
    for declined in (dict(dt=7), dict(g=32, in_f=64), dict(out_f=72), dict(gy=p + 2056), dict(gx=p + 3080), dict(stride=2 * 64 + 4),
                     dict(stride=64)):
        assert call(**declined) == _native.E_UNSUPPORTED, declined


def test_op_is_registered_with_a_fake_impl():
    gy = torch.empty((10, 2, 64), dtype=torch.bfloat16, device="meta")
    bucket = torch.empty((64,), dtype=torch.int32, device="meta")
    table = torch.empty((64,), dtype=torch.int64, device="meta")
    gx = torch.ops.aqlm.code1x16_moe_matmat_grouped_transposed(gy, bucket, table, [8, 2, 64, 128, 8, 2, 16, 10])
    assert gx.device.type == "meta" and gx.dtype == torch.float32 and tuple(gx.shape) == (10, 128)
    schema = str(torch.ops.aqlm.code1x16_moe_matmat_grouped_transposed.default._schema)
    assert "Tensor grad_output, Tensor bucket, Tensor table, int[] geometry" in schema and schema.endswith("-> Tensor")


def test_route_predicate_truth_table():
    from aqlm_amd import moe

    assert moe.GROUPED_BACKWARD is True
    for enabled, supported in itertools.product((False, True), repeat=2):
        assert moe.takes_grouped_backward(enabled, supported) is (enabled and supported)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_transposed_kernels_isa(tmp_path):
    out = tmp_path / "moe_grouped_bwd.s"
    subprocess.run([HIPCC] + ISA_FLAGS + [os.path.join(ROOT, "aqlm_amd", "csrc", "moe_grouped_bwd.hip"), "-o", str(out)], check=True,
                   stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=600)
    text = out.read_text()
    pat = r"_ZN4aqlm\w*gemm_1x16_grouped_transposed_kernel\w+"
    names = set(re.findall(r"^\s+\.name:\s+(%s)" % pat, text, re.M))
    assert len(names) == 16, names  # fp16 / bf16 x g 8 / 16 x tiles of 16 / 32 / 64 / 128
    for m in re.finditer(r"\.name:\s+(%s)(.*?)(?=\n  - |\Z)" % pat, text, re.S):
        assert re.search(r"\.private_segment_fixed_size:\s+0\b", m.group(2)), m.group(1)
    code = text.split(".amdgpu_metadata")[0]
    assert not re.search(r"\bscratch_(load|store)", code)
    for name in names:
        body = code[code.index(f"\n{name}:"):]
        body = body[:body.index("s_endpgm")]
        assert "v_mfma_f32_16x16x32" in body, name
        assert "ds_read_b64_tr_b16" in body, name
        assert "flat_load" not in body, name  # the table's pointers are global memory: flat loads would wait with the LDS reads
