"""The fused transposed 1x16 GEMM without a GPU: its symbols, which layers the entry takes, its workspace size, where the Python
wrapper declines, and the selector's row window."""
import os

import pytest
import torch

SYMBOLS = ["aqlm_hip_gemm_1x16_transposed_supported", "aqlm_hip_gemm_1x16_transposed_workspace_bytes", "aqlm_hip_gemm_1x16_transposed"]


def test_symbols_declared_bound_and_exported():
    from aqlm_amd import _native

    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "aqlm_hip.h")) as f:
        header = f.read()
    for name in SYMBOLS:
        assert f" {name}(" in header and name in _native.SIGNATURES and callable(getattr(_native.lib, name))
    assert _native.lib.aqlm_hip_abi_version() == _native.ABI_VERSION == 9


@pytest.mark.parametrize("out_f,in_f,g,taken", [
    (4096, 4096, 8, True), (14336, 4096, 16, True), (40, 192, 8, True), (40, 208, 16, True), (8, 8, 8, True),
    (4096, 4096, 32, False),  # g = 32
    (4096, 4104, 16, False),  # in_features not a multiple of g
    (44, 192, 8, False),      # out_features not a multiple of 8: the rows of gy could not be read in whole 16-byte pieces
    (0, 4096, 8, False), (4096, 0, 8, False),
])
def test_supported_table(out_f, in_f, g, taken):
    from aqlm_amd import _native

    assert bool(_native.lib.aqlm_hip_gemm_1x16_transposed_supported(out_f, in_f, g)) is taken


@pytest.mark.parametrize("rows,out_f,in_f", [(1, 40, 192), (17, 96, 256), (16, 4096, 4096), (256, 4096, 14336), (4096, 14336, 4096)])
def test_workspace_bytes(rows, out_f, in_f):
    from aqlm_amd import _native

    ws = _native.lib.aqlm_hip_gemm_1x16_transposed_workspace_bytes
    assert ws(rows, out_f, in_f, 1) == 0
    for splits in (2, 3, 16):
        assert ws(rows, out_f, in_f, splits) == splits * rows * in_f * 4
    assert ws(rows, out_f, in_f, 0) <= out_f * in_f * 2 // 4  # the entry's own choice: within a quarter of the W it replaces
    assert ws(rows, out_f, in_f, 0) % (rows * in_f * 4) == 0
    for bad in ((0, out_f, in_f, 2), (rows, 0, in_f, 2), (rows, out_f, 0, 2), (65537, out_f, in_f, 2), (rows, out_f, in_f, 17)):
        assert ws(*bad) == 0


def test_wrapper_declines():
    from aqlm_amd.inference_kernels import hip_kernel as hk

    gy, scales = torch.zeros(8, 64, dtype=torch.float16), torch.ones(64, 1, 1, 1, dtype=torch.float16)
    codes, books = torch.zeros(64, 16, 1, dtype=torch.int16), torch.zeros(1, 65536, 1, 8, dtype=torch.float16)
    assert hk.code1x16_matmat_transposed(gy, codes.to(torch.int8), books, scales) is None     # int8 codes
    assert hk.code1x16_matmat_transposed(gy.bfloat16(), codes, books, scales) is None          # mismatched dtypes
    assert hk.code1x16_matmat_transposed(gy, codes, books, scales) is None                     # host tensors


@pytest.mark.parametrize("g", [8, 16])
def test_selector_window(monkeypatch, g):
    from aqlm_amd.inference_kernels import hip_kernel as hk
    from aqlm_amd.inference_kernels import kernel_selector

    calls = []
    monkeypatch.setattr(hk, "code1x16_matmat_transposed", lambda gy, *rest: calls.append("fused") or "fused")
    monkeypatch.setattr(torch.ops.aqlm, "code1x16_matmat_dequant_transposed", lambda *args: calls.append("named") or "named", raising=False)
    monkeypatch.setattr(kernel_selector, "_require_gpu", lambda books: None)
    monkeypatch.setattr(hk, "FUSED_1X16_TRANSPOSED_ROWS", {g: (16, 64), None: hk.FUSED_1X16_TRANSPOSED_NEVER})
    assert hk.fused_1x16_transposed_rows(g) == (16, 64) and hk.fused_1x16_transposed_rows(24 - g) == hk.FUSED_1X16_TRANSPOSED_NEVER
    backward = kernel_selector.get_backward_pass_kernel(torch.zeros(1, 65536, 1, g, device="meta"), True)
    got = [backward(torch.zeros(rows, 64), None, None, None, None) for rows in (15, 16, 64, 65)]
    assert got == ["named", "fused", "fused", "named"] == calls
    monkeypatch.setattr(hk, "USE_FUSED_1X16_TRANSPOSED", False)
    assert backward(torch.zeros(16, 64), None, None, None, None) == "named"
