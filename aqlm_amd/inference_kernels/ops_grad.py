"""The training launches of codebooks and scales and their ``aqlm::`` ops: the indexed gradients of a 1x16 layer, the one-pass
gradients of the K x 8 schemes, and the calibrated step on fp32 masters (``aqlm_amd/tuning.py`` is the module-level interface).
Every name here is re-exported by ``hip_kernel``, which is where callers and tests reach it."""
from __future__ import annotations

from typing import Optional

import torch

from .. import _native
from .._native import lib as _lib
from ._launch import _GRAD_DT, _GRAD_TORCH_DT, _c, _device_guard, _dtype_id, _ptr, _stream_ptr, _workspace, register_op


# ------------------------------------------------------------------------------------------------------
# gradients of the codebook and the scales of a 1x16 layer (aqlm_hip_codebook_grad_1x16, aqlm_hip_scales_grad_1x16)
# ------------------------------------------------------------------------------------------------------
CODEBOOK_GRAD_CHUNK = int(_lib.aqlm_hip_codebook_grad_chunk())  # positions per chunk of an entry's list (a constant of the library)
CODEBOOK_GRAD_ENTRIES = 65536


def codebook_grad_supported(out_features: int, in_features: int, in_group_size: int) -> bool:
    return bool(_lib.aqlm_hip_codebook_grad_1x16_supported(int(out_features), int(in_features), int(in_group_size))
                and _lib.aqlm_hip_scales_grad_1x16_supported(int(out_features), int(in_features), int(in_group_size)))


def codebook_grad_max_chunks(out_features: int, in_features: int, in_group_size: int) -> int:
    return int(_lib.aqlm_hip_codebook_grad_1x16_max_chunks(int(out_features), int(in_features), int(in_group_size)))


class CodebookGradIndex:
    """The inverted index of a 1x16 layer's codes (include/aqlm_hip.h, aqlm_hip_codebook_grad_1x16): per codebook entry the
    ascending list of the positions ``o * (in_features / g) + j`` that use it (``order`` int32 [n_codes], ``starts`` int32 [65537]),
    every list cut into chunks of at most ``CODEBOOK_GRAD_CHUNK`` positions (``chunks`` int32 [max_chunks, 3]: entry, begin, end;
    rows past the last chunk hold entry -1; ``chunk_starts`` int32 [65537]).  4 bytes per code plus ~0.5 MB of tables."""

    __slots__ = ("order", "starts", "chunks", "chunk_starts", "out_features", "in_features", "in_group_size")

    def __init__(self, order, starts, chunks, chunk_starts, out_features, in_features, in_group_size):
        self.order, self.starts, self.chunks, self.chunk_starts = order, starts, chunks, chunk_starts
        self.out_features, self.in_features, self.in_group_size = int(out_features), int(in_features), int(in_group_size)

    def nbytes(self) -> int:
        return sum(t.numel() * t.element_size() for t in (self.order, self.starts, self.chunks, self.chunk_starts))

    def geometry(self):
        return [self.out_features, self.in_features, self.in_group_size]


def build_codebook_grad_index(codes: torch.Tensor, in_group_size: int) -> CodebookGradIndex:
    """The index from canonical ``codes`` [out, in / g, 1] int16, with torch ops on the codes' device: one stable sort by the
    unsigned code value and binary searches for the tables.  No host synchronisation (the chunk table has its upper bound
    ``min(n_codes, 65536) + n_codes // CHUNK`` of rows, the unused ones marked -1) and no kernel of this library: it runs once per
    layer.  Works on host tensors too (the tests model it in numpy)."""
    if codes.dim() != 3 or codes.shape[2] != 1 or codes.dtype != torch.int16:
        raise ValueError(f"codes must be int16 [out, in / g, 1], got {codes.dtype} {tuple(codes.shape)}")
    out_features, nj = int(codes.shape[0]), int(codes.shape[1])
    g, n, chunk = int(in_group_size), out_features * nj, CODEBOOK_GRAD_CHUNK
    max_chunks = codebook_grad_max_chunks(out_features, nj * g, g)
    if max_chunks == 0:
        raise NotImplementedError(f"no codebook-gradient index for a layer of {out_features} x {nj * g}, g = {g}")
    dev = codes.device
    with torch.inference_mode(False), torch.no_grad():
        values = codes.detach().reshape(-1).to(torch.int32) & 0xFFFF  # the unsigned index a two's-complement container holds
        sorted_values, order = torch.sort(values, stable=True)        # stable: every entry's list ascends
        entries = torch.arange(CODEBOOK_GRAD_ENTRIES + 1, dtype=torch.int32, device=dev)
        starts = torch.searchsorted(sorted_values, entries)           # [65537]; starts[65536] == n
        counts = starts[1:] - starts[:-1]
        chunk_starts = torch.zeros_like(starts)
        chunk_starts[1:] = torch.cumsum((counts + (chunk - 1)) // chunk, 0)
        k = torch.arange(max_chunks, dtype=torch.int64, device=dev)
        entry = torch.searchsorted(chunk_starts[1:], k, right=True)   # the entry whose chunk rows hold k; 65536: past the last chunk
        valid = entry < CODEBOOK_GRAD_ENTRIES
        e = entry.clamp(max=CODEBOOK_GRAD_ENTRIES - 1)
        begin = starts[e] + (k - chunk_starts[e]) * chunk
        end = torch.minimum(begin + chunk, starts[e + 1])
        zero = torch.zeros_like(k)
        chunks = torch.stack((torch.where(valid, entry, zero - 1), torch.where(valid, begin, zero), torch.where(valid, end, zero)), 1)
        return CodebookGradIndex(order.to(torch.int32), starts.to(torch.int32), chunks.to(torch.int32).contiguous(),
                                 chunk_starts.to(torch.int32), out_features, nj * g, g)


def _check_dw(dw, out_features, in_features, what):
    if dw.dim() != 2 or tuple(dw.shape) != (out_features, in_features) or dw.stride(1) != 1 or dw.dtype not in _GRAD_DT or not dw.is_cuda:
        raise ValueError(f"{what}: dW must be a GPU fp16 / bf16 / fp32 [{out_features}, {in_features}] with a unit inner stride, got "
                         f"{dw.dtype} {tuple(dw.shape)} strides {tuple(dw.stride())} on {dw.device}")


def _check_scales(scales, out_features, device, what):
    if scales.numel() != out_features or scales.device != device:
        raise ValueError(f"{what}: scales must hold {out_features} elements on {device}")


def _codebook_grad_op(dw, scales, starts, order, chunks, chunk_starts, geometry):
    out_features, in_features, g, out_dt = (int(x) for x in geometry)
    _check_dw(dw, out_features, in_features, "codebook_grad_1x16")
    n = out_features * (in_features // max(g, 1))
    max_chunks = codebook_grad_max_chunks(out_features, in_features, g)
    want = ((starts, (CODEBOOK_GRAD_ENTRIES + 1,)), (order, (n,)), (chunks, (max_chunks, 3)), (chunk_starts, (CODEBOOK_GRAD_ENTRIES + 1,)))
    for t, shape in want:
        if t.dtype != torch.int32 or tuple(t.shape) != shape or not t.is_contiguous() or t.device != dw.device:
            raise ValueError(f"codebook_grad_1x16: index tensors must be contiguous int32 {[s for _, s in want]} on {dw.device} "
                             "(build_codebook_grad_index)")
    dt = _native.F16
    if scales is not None:
        _check_scales(scales, out_features, dw.device, "codebook_grad_1x16")
        dt = _dtype_id(scales)
        scales = _c(scales)
    out = torch.empty((CODEBOOK_GRAD_ENTRIES, g), dtype=_GRAD_TORCH_DT[out_dt], device=dw.device)
    ws_bytes = int(_lib.aqlm_hip_codebook_grad_1x16_workspace_bytes(out_features, in_features, g))
    ws = _workspace(dw.device, max(ws_bytes, 16))
    with _device_guard(dw.device):
        rc = _lib.aqlm_hip_codebook_grad_1x16(dw.data_ptr(), dw.stride(0), _GRAD_DT[dw.dtype], _ptr(scales), dt, starts.data_ptr(),
                                              order.data_ptr(), chunks.data_ptr(), chunk_starts.data_ptr(), out_features, in_features,
                                              g, out.data_ptr(), out_dt, ws.data_ptr(), ws.numel() * 4, _stream_ptr(dw.device))
    if rc:
        _native.check(rc, "aqlm codebook grad")
    return out


# geometry = [out_features, in_features, g, output dtype id]
register_op("codebook_grad_1x16", "(Tensor dw, Tensor? scales, Tensor starts, Tensor order, Tensor chunks, Tensor chunk_starts, "
            "int[] geometry) -> Tensor", _codebook_grad_op,
            lambda dw, scales, starts, order, chunks, chunk_starts, geometry: dw.new_empty(
                (CODEBOOK_GRAD_ENTRIES, int(geometry[2])), dtype=_GRAD_TORCH_DT[int(geometry[3])]))


def codebook_grad_1x16(dw, scales, index: CodebookGradIndex, out_dtype: Optional[torch.dtype] = None):
    """dC [65536, g] (``out_dtype``, default dW's dtype) = for every entry the sum of ``scales[o] * dW[o, j*g : j*g + g]`` over the
    positions of its list, fp32, in the fixed order of the index (include/aqlm_hip.h); ``scales`` None = 1.  Every element is
    written (+0 for unused entries).  Two launches on the current stream, the fp32 partials in the cached per-stream workspace (a
    fresh one inside a hipGraph capture)."""
    out_dt = _GRAD_DT[dw.dtype if out_dtype is None else out_dtype]
    return _codebook_grad_op(dw, scales, index.starts, index.order, index.chunks, index.chunk_starts, index.geometry() + [out_dt])


def _scales_grad_op(dw, codes, codebooks, geometry):
    out_features, in_features, g, out_dt = (int(x) for x in geometry)
    _check_dw(dw, out_features, in_features, "scales_grad_1x16")
    if (codes.dtype != torch.int16 or codes.numel() != out_features * (in_features // max(g, 1)) or not codes.is_contiguous()
            or codes.device != dw.device):
        raise ValueError(f"scales_grad_1x16: codes must be contiguous int16 [{out_features}, {in_features // max(g, 1)}, 1] on {dw.device}")
    if tuple(codebooks.shape) != (1, CODEBOOK_GRAD_ENTRIES, 1, g) or codebooks.device != dw.device:
        raise ValueError(f"scales_grad_1x16: codebooks must be [1, 65536, 1, {g}] on {dw.device}, got {tuple(codebooks.shape)}")
    dt = _dtype_id(codebooks)
    codebooks = _c(codebooks)
    out = torch.empty((out_features,), dtype=_GRAD_TORCH_DT[out_dt], device=dw.device)
    with _device_guard(dw.device):
        rc = _lib.aqlm_hip_scales_grad_1x16(dw.data_ptr(), dw.stride(0), _GRAD_DT[dw.dtype], codes.data_ptr(), codebooks.data_ptr(), dt,
                                            out_features, in_features, g, out.data_ptr(), out_dt, _stream_ptr(dw.device))
    if rc:
        _native.check(rc, "aqlm scales grad")
    return out


register_op("scales_grad_1x16", "(Tensor dw, Tensor codes, Tensor codebooks, int[] geometry) -> Tensor", _scales_grad_op,
            lambda dw, codes, codebooks, geometry: dw.new_empty((int(geometry[0]),), dtype=_GRAD_TORCH_DT[int(geometry[3])]))


def scales_grad_1x16(dw, codes, codebooks, out_dtype: Optional[torch.dtype] = None):
    """ds [out] (``out_dtype``, default dW's dtype): ``sum over j, t of dW[o, j*g + t] * codebooks[0, code(o, j), 0, t]`` -- the
    unscaled codebook, the canonical codes; fp32 in a fixed order, one rounding (include/aqlm_hip.h)."""
    g = int(codebooks.shape[3])
    out_dt = _GRAD_DT[dw.dtype if out_dtype is None else out_dtype]
    return _scales_grad_op(dw, codes, codebooks, [int(codes.shape[0]), int(codes.shape[1]) * g, g, out_dt])


# ------------------------------------------------------------------------------------------------------
# the same gradients for the K x 8 schemes (aqlm_hip_codebook_grad_kx8, aqlm_hip_scales_grad_kx8): no index
# ------------------------------------------------------------------------------------------------------
def codebook_grad_kx8_supported(out_features: int, in_features: int, num_codebooks: int, in_group_size: int) -> bool:
    args = (int(out_features), int(in_features), int(num_codebooks), int(in_group_size))
    return bool(_lib.aqlm_hip_codebook_grad_kx8_supported(*args) and _lib.aqlm_hip_scales_grad_kx8_supported(*args))


def _check_kx8_codes(codes, dw, out_features, in_features, K, g, what):
    if (codes.dtype != torch.int8 or codes.numel() != out_features * (in_features // max(g, 1)) * K or not codes.is_contiguous()
            or codes.device != dw.device):
        raise ValueError(f"{what}: codes must be contiguous int8 [{out_features}, {in_features // max(g, 1)}, {K}] on {dw.device}")


def _codebook_grad_kx8_op(dw, scales, codes, geometry):
    out_features, in_features, K, g, out_dt = (int(x) for x in geometry)
    _check_dw(dw, out_features, in_features, "codebook_grad_kx8")
    _check_kx8_codes(codes, dw, out_features, in_features, K, g, "codebook_grad_kx8")
    dt = _native.F16
    if scales is not None:
        _check_scales(scales, out_features, dw.device, "codebook_grad_kx8")
        dt = _dtype_id(scales)
        scales = _c(scales)
    out = torch.empty((K, 256, g), dtype=_GRAD_TORCH_DT[out_dt], device=dw.device)
    ws_bytes = int(_lib.aqlm_hip_codebook_grad_kx8_workspace_bytes(out_features, in_features, K, g))
    ws = _workspace(dw.device, max(ws_bytes, 16))
    with _device_guard(dw.device):
        rc = _lib.aqlm_hip_codebook_grad_kx8(dw.data_ptr(), dw.stride(0), _GRAD_DT[dw.dtype], _ptr(scales), dt, codes.data_ptr(),
                                             out_features, in_features, K, g, out.data_ptr(), out_dt, ws.data_ptr(), ws.numel() * 4,
                                             _stream_ptr(dw.device))
    if rc:
        _native.check(rc, "aqlm codebook grad kx8")
    return out


# geometry = [out_features, in_features, K, g, output dtype id]
register_op("codebook_grad_kx8", "(Tensor dw, Tensor? scales, Tensor codes, int[] geometry) -> Tensor", _codebook_grad_kx8_op,
            lambda dw, scales, codes, geometry: dw.new_empty((int(geometry[2]), 256, int(geometry[3])),
                                                             dtype=_GRAD_TORCH_DT[int(geometry[4])]))


def codebook_grad_kx8(dw, scales, codes, in_group_size: int, out_dtype: Optional[torch.dtype] = None):
    """dC [K, 256, g] (``out_dtype``, default dW's dtype) of a K x 8 layer from ``dw`` [out, in], ``scales`` ([out] elements or None =
    1) and the canonical ``codes`` [out, in / g, K] int8: per entry the sum of ``scales[o] * dW[o, j*g : j*g + g]`` over the positions
    that use it, taken as fixed-point integers (include/aqlm_hip.h has the arithmetic) -- exact in the quantised terms and the same
    bits under any schedule.  Every element is written (+0 for unused entries; NaN everywhere when dW or the scales hold a
    non-finite value).  Three launches on the current stream, the int64 partials in the cached per-stream workspace (a fresh one
    inside a hipGraph capture)."""
    g = int(in_group_size)
    out_dt = _GRAD_DT[dw.dtype if out_dtype is None else out_dtype]
    return _codebook_grad_kx8_op(dw, scales, codes, [int(codes.shape[0]), int(codes.shape[1]) * g, int(codes.shape[2]), g, out_dt])


def _scales_grad_kx8_op(dw, codes, codebooks, geometry):
    out_features, in_features, K, g, out_dt = (int(x) for x in geometry)
    _check_dw(dw, out_features, in_features, "scales_grad_kx8")
    _check_kx8_codes(codes, dw, out_features, in_features, K, g, "scales_grad_kx8")
    if tuple(codebooks.shape) != (K, 256, 1, g) or codebooks.device != dw.device:
        raise ValueError(f"scales_grad_kx8: codebooks must be [{K}, 256, 1, {g}] on {dw.device}, got {tuple(codebooks.shape)}")
    dt = _dtype_id(codebooks)
    codebooks = _c(codebooks)
    out = torch.empty((out_features,), dtype=_GRAD_TORCH_DT[out_dt], device=dw.device)
    with _device_guard(dw.device):
        rc = _lib.aqlm_hip_scales_grad_kx8(dw.data_ptr(), dw.stride(0), _GRAD_DT[dw.dtype], codes.data_ptr(), codebooks.data_ptr(), dt,
                                           out_features, in_features, K, g, out.data_ptr(), out_dt, _stream_ptr(dw.device))
    if rc:
        _native.check(rc, "aqlm scales grad kx8")
    return out


register_op("scales_grad_kx8", "(Tensor dw, Tensor codes, Tensor codebooks, int[] geometry) -> Tensor", _scales_grad_kx8_op,
            lambda dw, codes, codebooks, geometry: dw.new_empty((int(geometry[0]),), dtype=_GRAD_TORCH_DT[int(geometry[4])]))


def scales_grad_kx8(dw, codes, codebooks, out_dtype: Optional[torch.dtype] = None):
    """ds [out] (``out_dtype``, default dW's dtype): ``sum over j, t of dW[o, j*g + t] * sum over c of codebooks[c, code(o, j, c), 0,
    t]`` -- the unscaled codebooks [K, 256, 1, g], the canonical codes [out, in / g, K] int8; fp32 in a fixed order, one rounding
    (include/aqlm_hip.h)."""
    K, g = int(codebooks.shape[0]), int(codebooks.shape[3])
    out_dt = _GRAD_DT[dw.dtype if out_dtype is None else out_dtype]
    return _scales_grad_kx8_op(dw, codes, codebooks, [int(codes.shape[0]), int(codes.shape[1]) * g, K, g, out_dt])


# ------------------------------------------------------------------------------------------------------
# one step of the calibrated training of codebooks and scales on fp32 masters (aqlm_hip_calib_*; tuning.calibrated_loss_and_grads)
# ------------------------------------------------------------------------------------------------------
def calib_supported(out_features: int, in_features: int, num_codebooks: int, nbits_per_codebook: int, in_group_size: int) -> bool:
    """All entries of the calibrated step take this layer (out_group_size 1: 1x16 with g 8 / 16, K x 8 with K 1..8 and g 8 / 16 / 32)."""
    o, i, K, nbits, g = int(out_features), int(in_features), int(num_codebooks), int(nbits_per_codebook), int(in_group_size)
    if not (_lib.aqlm_hip_calib_delta_supported(o, i, K, nbits, g) and _lib.aqlm_hip_calib_rows_supported(o, i, K, nbits, g)):
        return False
    if nbits == 16:
        return bool(_lib.aqlm_hip_calib_codebook_grad_1x16_supported(o, i, g))
    return bool(_lib.aqlm_hip_calib_codebook_grad_kx8_supported(o, i, K, g))


def _calib_scales(who, scales, out_features, device):
    """The checked fp32 ``scales`` as a contiguous [out]."""
    if scales.numel() != out_features or scales.dtype != torch.float32 or scales.device != device:
        raise ValueError(f"{who}: scales must hold {out_features} fp32 elements on {device}")
    return _c(scales.detach()).reshape(-1)


def _calib_layer(who, codes, codebooks, scales):
    """(codes, codebooks [K, S, g] fp32, scales [out] fp32 or None, out, in, K, nbits, g) of checked operands on one GPU."""
    if codebooks.dim() != 4 or codebooks.shape[2] != 1 or codebooks.dtype != torch.float32 or not codebooks.is_cuda:
        raise ValueError(f"{who}: codebooks must be GPU fp32 [K, S, 1, g], got {codebooks.dtype} {tuple(codebooks.shape)} on {codebooks.device}")
    K, size, _, g = (int(v) for v in codebooks.shape)
    nbits = {256: 8, 65536: 16}.get(size, 0)
    want = torch.int16 if nbits == 16 else torch.int8
    if codes.dim() != 3 or codes.shape[2] != K or codes.dtype != want or not codes.is_contiguous() or codes.device != codebooks.device:
        raise ValueError(f"{who}: codes must be contiguous {want} [out, in / g, {K}] on {codebooks.device}, got {codes.dtype} {tuple(codes.shape)}")
    out_features, in_features = int(codes.shape[0]), int(codes.shape[1]) * g
    if scales is not None:
        scales = _calib_scales(who, scales, out_features, codebooks.device)
    return codes, _c(codebooks.detach()), scales, out_features, in_features, K, nbits, g


def _check_calib_matrix(who, name, m, out_features, in_features, device, dtypes=(torch.float32,)):
    if m.dim() != 2 or tuple(m.shape) != (out_features, in_features) or m.stride(1) != 1 or m.dtype not in dtypes or m.device != device:
        raise ValueError(f"{who}: {name} must be a {' / '.join(str(d) for d in dtypes)} [{out_features}, {in_features}] with a unit inner "
                         f"stride on {device}, got {m.dtype} {tuple(m.shape)} strides {tuple(m.stride())} on {m.device}")


def calib_delta(codes, codebooks, scales, reference_weight, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """D [out, in] fp32 = ``scales * sum_c codebooks[c][codes[..., c]] - reference_weight``: every operation one fp32 operation, the bits of
    torch's fp32 ``_dequantize_weight(...) - reference_weight`` (include/aqlm_hip.h, aqlm_hip_calib_delta).  ``reference_weight`` fp32 / fp16
    / bf16 with any row stride; ``out``: an fp32 [out, in] to write (rows 16-byte aligned), default a new one.  One launch."""
    codes, books, scales, o, i, K, nbits, g = _calib_layer("calib_delta", codes, codebooks, scales)
    if scales is None:
        raise ValueError("calib_delta: scales are required")
    _check_calib_matrix("calib_delta", "reference_weight", reference_weight, o, i, books.device, tuple(_GRAD_DT))
    if out is None:
        out = torch.empty((o, i), dtype=torch.float32, device=books.device)
    _check_calib_matrix("calib_delta", "out", out, o, i, books.device)
    with _device_guard(books.device):
        rc = _lib.aqlm_hip_calib_delta(codes.data_ptr(), books.data_ptr(), scales.data_ptr(), reference_weight.data_ptr(),
                                       _GRAD_DT[reference_weight.dtype], reference_weight.stride(0), o, i, K, nbits, g, out.data_ptr(),
                                       out.stride(0), _stream_ptr(books.device))
    if rc:
        _native.check(rc, "aqlm calib delta")
    return out


def calib_rows(g_matrix, delta, codes, codebooks):
    """``(ds_raw [out], rowloss [out])`` fp32 of ``G = D @ XTX`` and the stored ``D``: ``ds_raw[o] = sum G[o] * w[o]`` (w: the UNSCALED
    dequantised row), ``rowloss[o] = sum G[o] * D[o]``; one wave per row in the fixed order of ``scales_grad_1x16`` (include/aqlm_hip.h,
    aqlm_hip_calib_rows).  One launch."""
    codes, books, _, o, i, K, nbits, g = _calib_layer("calib_rows", codes, codebooks, None)
    _check_calib_matrix("calib_rows", "G", g_matrix, o, i, books.device)
    _check_calib_matrix("calib_rows", "D", delta, o, i, books.device)
    out = torch.empty((2, o), dtype=torch.float32, device=books.device)
    with _device_guard(books.device):
        rc = _lib.aqlm_hip_calib_rows(g_matrix.data_ptr(), g_matrix.stride(0), delta.data_ptr(), delta.stride(0), codes.data_ptr(),
                                      books.data_ptr(), o, i, K, nbits, g, out[0].data_ptr(), out[1].data_ptr(), _stream_ptr(books.device))
    if rc:
        _native.check(rc, "aqlm calib rows")
    return out[0], out[1]


def calib_codebook_grad_1x16(g_matrix, scales, index: CodebookGradIndex) -> torch.Tensor:
    """dC [65536, g] fp32: per entry the sum of ``scales[o] * G[o, j*g : j*g + g]`` over the positions of its list -- the launches and the
    order of ``codebook_grad_1x16`` with fp32 scales (aqlm_hip_calib_codebook_grad_1x16).  Every element is written."""
    o, i, g = index.geometry()
    _check_calib_matrix("calib_codebook_grad_1x16", "G", g_matrix, o, i, index.order.device)
    scales = _calib_scales("calib_codebook_grad_1x16", scales, o, g_matrix.device)
    out = torch.empty((CODEBOOK_GRAD_ENTRIES, g), dtype=torch.float32, device=g_matrix.device)
    ws_bytes = int(_lib.aqlm_hip_calib_codebook_grad_1x16_workspace_bytes(o, i, g))
    ws = _workspace(g_matrix.device, max(ws_bytes, 16))
    with _device_guard(g_matrix.device):
        rc = _lib.aqlm_hip_calib_codebook_grad_1x16(g_matrix.data_ptr(), g_matrix.stride(0), scales.data_ptr(), index.starts.data_ptr(),
                                                    index.order.data_ptr(), index.chunks.data_ptr(), index.chunk_starts.data_ptr(), o, i, g,
                                                    out.data_ptr(), ws.data_ptr(), ws.numel() * 4, _stream_ptr(g_matrix.device))
    if rc:
        _native.check(rc, "aqlm calib codebook grad")
    return out


def calib_codebook_grad_kx8(g_matrix, scales, codes, in_group_size: int) -> torch.Tensor:
    """dC [K, 256, g] fp32 of a K x 8 layer: the fixed-point sums of ``codebook_grad_kx8`` with fp32 scales
    (aqlm_hip_calib_codebook_grad_kx8); NaN everywhere when ``G`` or the scales hold a non-finite value."""
    g = int(in_group_size)
    o, i, K = int(codes.shape[0]), int(codes.shape[1]) * g, int(codes.shape[2])
    _check_calib_matrix("calib_codebook_grad_kx8", "G", g_matrix, o, i, codes.device)
    _check_kx8_codes(codes, g_matrix, o, i, K, g, "calib_codebook_grad_kx8")
    scales = _calib_scales("calib_codebook_grad_kx8", scales, o, g_matrix.device)
    out = torch.empty((K, 256, g), dtype=torch.float32, device=g_matrix.device)
    ws_bytes = int(_lib.aqlm_hip_calib_codebook_grad_kx8_workspace_bytes(o, i, K, g))
    ws = _workspace(g_matrix.device, max(ws_bytes, 16))
    with _device_guard(g_matrix.device):
        rc = _lib.aqlm_hip_calib_codebook_grad_kx8(g_matrix.data_ptr(), g_matrix.stride(0), scales.data_ptr(), codes.data_ptr(), o, i, K, g,
                                                   out.data_ptr(), ws.data_ptr(), ws.numel() * 4, _stream_ptr(g_matrix.device))
    if rc:
        _native.check(rc, "aqlm calib codebook grad kx8")
    return out
