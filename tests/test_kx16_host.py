"""CPU-only: the K x 9..16-bit entries (aqlm_hip_gemv_kx16, aqlm_hip_gemm_kx16_rows, its _supported) refuse bad arguments before they
touch the device, and kernel_selector routes 2 / 4 codebooks of 512 .. 65536 entries with g 8 to the new functions and nothing else."""
import ctypes
from types import SimpleNamespace

import pytest
import torch


@pytest.fixture(scope="module")
def native():
    from aqlm_amd import _native

    return _native


def call(native, entry, p, **kw):
    """One call of `entry` ("gemv" / "rows") on a valid 2x12 layer of 512 -> 64 with the arguments in `kw` replaced; host memory `p`
    stands for every buffer (no valid call is made: each case is refused by a check in front of the launch)."""
    a = dict(codes=p, codebooks=p, scales=p, bias=None, x=p, y=p, out=64, inf=512, K=2, nbits=12, g=8, rows=1, dtype=native.F16)
    a.update(kw)
    if entry == "gemv":
        rc = native.lib.aqlm_hip_gemv_kx16(a["codes"], a["codebooks"], a["scales"], a["bias"], a["x"], a["y"], a["out"], a["inf"], a["K"],
                                           a["nbits"], a["g"], a["rows"], a["inf"], a["out"], a["dtype"], None)
    else:
        rc = native.lib.aqlm_hip_gemm_kx16_rows(a["codes"], a["codebooks"], a["scales"], a["bias"], a["x"], a["y"], a["rows"], a["out"],
                                                a["inf"], a["K"], a["nbits"], a["g"], a["inf"], a["out"], a["dtype"], None)
    return rc, native.last_error()


COMMON = [(dict(codes=None), -1, "null pointer"), (dict(inf=508), -1, "in"), (dict(dtype=7), -2, "float16 and bfloat16"),
          (dict(nbits=8), -2, "nbits 8"), (dict(nbits=17), -2, "nbits 17"), (dict(K=1), -2, "num_codebooks 1"), (dict(K=9), -2, "num_codebooks 9")]


@pytest.mark.parametrize("entry,kw,code,text", [(e,) + c for e in ("gemv", "rows") for c in COMMON] + [("gemv", dict(rows=9), -2, "batch 9")])
def test_entries_validate_before_touching_the_device(native, entry, kw, code, text):
    buf = ctypes.create_string_buffer(4096 + 16)
    rc, msg = call(native, entry, (ctypes.addressof(buf) + 15) & ~15, **kw)
    if "inf" in kw:
        text = "multiple of in_group_size" if entry == "gemv" else "in=508"   # (the matvec entries' wording / check_sizes')
    assert rc == code and text in msg and msg.startswith("aqlm_hip_gemv_kx16" if entry == "gemv" else "aqlm_hip_gemm_kx16_rows")


def test_supported_names_the_schemes(native):
    ok = native.lib.aqlm_hip_gemm_kx16_rows_supported
    for K in (2, 4):
        for nbits in (12, 16):
            assert ok(40, 512, K, nbits, 8, 7) == 1 and ok(4096, 14336, K, nbits, 8, 1024) == 1
    assert ok(40, 512, 3, 12, 8, 7) == 0      # K 3
    assert ok(40, 512, 2, 12, 16, 7) == 0     # g 16
    assert ok(40, 512, 2, 8, 8, 7) == 0       # 8-bit codebooks are the K x 8 kernels'
    assert ok(40, 520, 2, 12, 8, 7) == 0      # in / 8 no multiple of the 4 groups of a chunk
    assert ok(40, 512, 2, 12, 8, 0) == 0


def test_selector_routes_only_the_new_schemes(native):
    from aqlm_amd.inference_kernels import cpu_kernel, hip_kernel, kernel_selector as ks

    def on_gpu(*shape):  # what the selector reads of a device tensor: no device needed
        return SimpleNamespace(device=SimpleNamespace(type="cuda"), shape=shape)

    ops = torch.ops.aqlm
    for shape in ((2, 65536, 1, 8), (2, 4096, 1, 8), (4, 65536, 1, 8), (2, 512, 1, 8)):
        assert ks.get_forward_pass_kernel(on_gpu(*shape), False) is hip_kernel.codekx16_matmat
        assert ks.get_forward_pass_kernel(on_gpu(*shape), True) is hip_kernel.codekx16_matmat_dequant
    for shape in ((3, 4096, 1, 8), (2, 4096, 1, 16), (1, 4096, 1, 8), (3, 32, 1, 8)):   # K 3, g 16, 1x12 and 3x5 stay generic
        assert ks.get_forward_pass_kernel(on_gpu(*shape), False) is ops.generic_matmat
        assert ks.get_forward_pass_kernel(on_gpu(*shape), True) is ops.generic_matmat_dequant
    # the tuned schemes return what they returned before
    assert ks.get_forward_pass_kernel(on_gpu(1, 65536, 1, 8), False) is ops.code1x16_matmat
    assert ks.get_forward_pass_kernel(on_gpu(1, 65536, 1, 16), True) is ops.code1x16_matmat_dequant
    assert ks.get_forward_pass_kernel(on_gpu(2, 256, 1, 8), False) is ops.code2x8_matmat
    assert ks.get_forward_pass_kernel(on_gpu(1, 256, 1, 8), True) is ops.code1x8_matmat_dequant
    assert ks.get_forward_pass_kernel(on_gpu(8, 256, 1, 32), False) is ops.codekx8_matmat
    assert ks.get_forward_pass_kernel(on_gpu(2, 65536, 2, 8), False) is ks._torch_forward
    # host tensors keep the CPU branch
    assert ks.get_forward_pass_kernel(torch.zeros(2, 65536, 1, 8), False) is ks._torch_forward
    assert ks.get_forward_pass_kernel(torch.zeros(2, 256, 1, 8), False) is cpu_kernel.cpu_gemm_lut
    # both routes ship as measured (profiles/kx16.json)
    assert set(hip_kernel.USE_KX16_GEMV) == {(2, 16), (2, 12), (4, 16), None} and hip_kernel.USE_KX16_GEMV[None] is False
    assert isinstance(hip_kernel.FUSED_KX16_MAX_ROWS, int) and hip_kernel.FUSED_KX16_MAX_ROWS >= 0
