"""The fused transposed K x 8 GEMM without a GPU: which layers the entry takes, its workspace size, argument validation before any
device call, and the selector's CPU branch."""
import ctypes

import pytest
import torch


@pytest.mark.parametrize("out_f,in_f,K,g,taken", [
    (4096, 4096, 1, 8, True), (14336, 4096, 2, 8, True), (40, 192, 4, 16, True), (4096, 14336, 8, 32, True), (1, 8, 3, 8, True),
    (4096, 4096, 16, 8, False),   # 16 codebooks
    (4096, 4096, 2, 4, False),    # g = 4
    (4096, 4104, 4, 16, False),   # in_features not a multiple of g
    (0, 4096, 2, 8, False),
])
def test_supported_table(out_f, in_f, K, g, taken):
    from aqlm_amd import _native

    assert bool(_native.lib.aqlm_hip_gemm_kx8_transposed_supported(out_f, in_f, K, g)) is taken


def test_a_1x16_layer_is_declined():
    from aqlm_amd.inference_kernels import hip_kernel as hk

    gy = torch.zeros(8, 64, dtype=torch.float16)
    codes = torch.zeros(64, 16, 1, dtype=torch.int16)
    assert hk.codekx8_matmat_transposed(gy, codes, torch.zeros(1, 65536, 1, 8, dtype=torch.float16), torch.ones(64, 1, 1, 1, dtype=torch.float16)) is None


@pytest.mark.parametrize("rows,out_f,in_f", [(1, 40, 192), (17, 96, 256), (256, 4096, 14336)])
def test_workspace_bytes(rows, out_f, in_f):
    from aqlm_amd import _native

    ws = _native.lib.aqlm_hip_gemm_kx8_transposed_workspace_bytes
    assert ws(rows, out_f, in_f, 1) == 0
    for splits in (2, 3, 16):
        assert ws(rows, out_f, in_f, splits) == splits * rows * in_f * 4
    assert ws(rows, out_f, in_f, 0) * 4 <= out_f * in_f * 2  # the entry's own choice: within a quarter of the W it replaces


def test_argument_validation_without_gpu():
    from aqlm_amd import _native

    buf = (ctypes.c_char * 8192)()
    p = ctypes.addressof(buf)
    p += -p % 16

    def call(codes=p, books=p + 1024, scales=p + 2048, gy=p + 3072, gx=p + 4096, rows=2, out_f=64, in_f=64, K=2, g=8, gys=64, gxs=64, dt=0,
             splits=1, ws=None, ws_bytes=0):
        return _native.lib.aqlm_hip_gemm_kx8_transposed(codes, books, scales, gy, gx, rows, out_f, in_f, K, g, gys, gxs, dt, splits, ws, ws_bytes, None)

    for bad in (dict(codes=None), dict(books=None), dict(scales=None), dict(gy=None), dict(gx=None), dict(rows=0),
                dict(splits=2), dict(splits=2, ws=p + 5120, ws_bytes=2 * 2 * 64 * 4 - 1)):
        assert call(**bad) == _native.E_INVALID, bad
        assert "aqlm_hip_gemm_kx8_transposed" in _native.last_error()
    for declined in (dict(dt=7), dict(K=16), dict(g=4), dict(in_f=68), dict(gy=p + 3080), dict(gx=p + 4104), dict(gys=68), dict(gxs=60),
                     dict(gys=56), dict(rows=65537), dict(splits=17)):
        assert call(**declined) == _native.E_UNSUPPORTED, declined


def test_cpu_backward_kernel_is_untouched():
    from aqlm_amd.inference_kernels import kernel_selector

    books = torch.zeros(2, 256, 1, 8)
    assert kernel_selector.get_backward_pass_kernel(books, True) is kernel_selector._torch_backward
    assert kernel_selector.get_backward_pass_kernel(books, False) is kernel_selector._torch_backward
