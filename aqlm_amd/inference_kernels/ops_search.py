"""The code-update launches and their ``aqlm::`` ops: the nearest-codeword search of the 1x16 schemes, the beam search of the
K x 8 schemes, the calibrated (XTX) step of either, and one Lloyd iteration of the k-means initialisation (``aqlm_amd/tuning.py``
is the module-level interface).  Every name here is re-exported by ``hip_kernel``, which is where callers and tests reach it --
tests replace the public searches there, so nothing in this module calls one of them by its bare name."""
from __future__ import annotations

import ctypes
from typing import NamedTuple, Optional

import torch

from .. import _native
from .._native import lib as _lib
from ._launch import _GRAD_DT, _c, _device_guard, _dtype_id, _ptr, _stream_ptr, _workspace, register_op
from .ops_grad import CODEBOOK_GRAD_ENTRIES  # the 65536 entries of a 1x16 codebook


# ------------------------------------------------------------------------------------------------------
# nearest-codeword search of the 1x16 schemes (the V step of PV-tuning; aqlm_hip_code_search_1x16)
# ------------------------------------------------------------------------------------------------------
CODE_SEARCH_EPS = _native.CODE_SEARCH_EPS  # the accuracy contract of include/aqlm_hip.h: computed scores within eps * (|r|^2 + max|C|^2)


def code_search_1x16_supported(out_features: int, in_features: int, in_group_size: int) -> bool:
    return bool(_lib.aqlm_hip_code_search_1x16_supported(int(out_features), int(in_features), int(in_group_size)))


def _code_search_1x16_impl(reference, scales, codebook, group_ids, codes_out, geometry):
    out_features, in_features, g = (int(x) for x in geometry)
    if (reference.dim() != 2 or tuple(reference.shape) != (out_features, in_features) or reference.dtype not in _GRAD_DT
            or not reference.is_cuda):
        raise ValueError(f"code_search_1x16: reference must be fp16 / bf16 / fp32 [{out_features}, {in_features}] on the GPU, got "
                         f"{reference.dtype} {tuple(reference.shape)}")
    if reference.stride(1) != 1 or reference.stride(0) < in_features:  # a transposed or expanded view: the kernel walks rows
        reference = reference.contiguous()
    if codebook.numel() != CODEBOOK_GRAD_ENTRIES * g or codebook.device != reference.device:
        raise ValueError(f"code_search_1x16: the codebook must hold 65536 x {g} elements on {reference.device}")
    dt = _dtype_id(codebook)
    codebook = _c(codebook)
    if scales is not None:
        if scales.numel() != out_features or scales.device != reference.device or scales.dtype != codebook.dtype:
            raise ValueError(f"code_search_1x16: scales must hold {out_features} elements of {codebook.dtype} on {reference.device}")
        scales = _c(scales)
    total = out_features * (in_features // max(g, 1))
    if group_ids is not None:
        if group_ids.dtype not in (torch.int32, torch.int64) or group_ids.dim() != 1 or group_ids.device != reference.device:
            raise ValueError("code_search_1x16: group_ids must be a 1-d int32 / int64 tensor on the reference's device")
        group_ids = _c(group_ids)
        n = int(group_ids.numel())
    else:
        n = total
    if codes_out is None:
        codes_out = torch.empty((n,), dtype=torch.int16, device=reference.device)
    elif codes_out.dtype != torch.int16 or codes_out.numel() != n or not codes_out.is_contiguous() or codes_out.device != reference.device:
        raise ValueError(f"code_search_1x16: codes_out must be contiguous int16 [{n}] on {reference.device}")
    if n == 0:
        return codes_out
    ws_bytes = int(_lib.aqlm_hip_code_search_1x16_workspace_bytes(n, g))
    ws = _workspace(reference.device, max(ws_bytes, 16))
    with _device_guard(reference.device):
        rc = _lib.aqlm_hip_code_search_1x16(reference.data_ptr(), _GRAD_DT[reference.dtype], reference.stride(0), _ptr(scales),
                                            codebook.data_ptr(), dt, out_features, in_features, g, _ptr(group_ids),
                                            int(group_ids is not None and group_ids.dtype == torch.int64), n, codes_out.data_ptr(),
                                            ws.data_ptr(), ws.numel() * 4, _stream_ptr(reference.device))
    if rc:
        _native.check(rc, "aqlm code search")
    return codes_out


def _code_search_1x16_op(reference, scales, codebook, group_ids, geometry):
    return _code_search_1x16_impl(reference, scales, codebook, group_ids, None, geometry)


# geometry = [out_features, in_features, g]
register_op("code_search_1x16", "(Tensor reference, Tensor? scales, Tensor codebook, Tensor? group_ids, int[] geometry) -> Tensor",
            _code_search_1x16_op, lambda reference, scales, codebook, group_ids, geometry: reference.new_empty(
                (int(group_ids.numel()) if group_ids is not None else int(geometry[0]) * (int(geometry[1]) // int(geometry[2])),),
                dtype=torch.int16))


def code_search_1x16(reference, scales, codebook, in_group_size: int, group_ids=None, codes_out=None):
    """int16 codes: for every group of ``in_group_size`` weights of ``reference`` [out, in] (fp32 / fp16 / bf16, any row stride; a view
    with another column stride is copied first) --
    or for the flat groups ``group_ids`` (int32 / int64, ``o * (in / g) + j``), in their order -- the codeword of ``codebook`` (65536
    x g elements, fp16 / bf16) that minimises ``|C_c|^2 - 2 <reference_group / scales[o], C_c>``; ``scales`` ([out] elements in the
    codebook dtype) None = 1.  Equal computed scores give the smallest index; the accuracy contract is in include/aqlm_hip.h
    (``CODE_SEARCH_EPS``).  ``codes_out`` (int16, one entry per group searched): written in place when given -- an id outside the
    layer leaves its entry as it was.  Two launches on the current stream, |C|^2 in the cached per-stream workspace."""
    g = int(in_group_size)
    return _code_search_1x16_impl(reference, scales, codebook, group_ids, codes_out, [int(reference.shape[0]), int(reference.shape[1]), g])


# ------------------------------------------------------------------------------------------------------
# k-means initialisation: one Lloyd iteration (aqlm_hip_kmeans_assign, aqlm_hip_kmeans_update)
# ------------------------------------------------------------------------------------------------------
KMEANS_EPS = _native.KMEANS_EPS  # the accuracy contract of include/aqlm_hip.h: computed scores within eps * (|x|^2 + max|C|^2)


def kmeans_supported(n: int, k: int, d: int) -> bool:
    return bool(_lib.aqlm_hip_kmeans_supported(int(n), int(k), int(d)))


def _kmeans_operands(who, data, centroids):
    if data.dim() != 2 or data.dtype != torch.float32 or not data.is_cuda:
        raise ValueError(f"{who}: data must be fp32 [n, d] on the GPU, got {data.dtype} {tuple(data.shape)} on {data.device}")
    if centroids.dim() != 2 or centroids.dtype != torch.float32 or centroids.device != data.device or centroids.shape[1] != data.shape[1]:
        raise ValueError(f"{who}: centroids must be fp32 [k, {data.shape[1]}] on {data.device}, got {centroids.dtype} "
                         f"{tuple(centroids.shape)} on {centroids.device}")
    n, d, k = int(data.shape[0]), int(data.shape[1]), int(centroids.shape[0])
    if not kmeans_supported(n, k, d):
        raise NotImplementedError(f"{who}: n={n} k={k} d={d} is outside the kernel (d 8 or 16, k a multiple of 128 up to 65536, "
                                  "1 <= n < 2^31)")
    return n, k, d


def _aligned16(t: torch.Tensor) -> torch.Tensor:
    t = _c(t)
    return t if t.data_ptr() % 16 == 0 else t.clone()


def _kmeans_assign_op(data, centroids, data_absmax, with_sums):
    n, k, d = _kmeans_operands("kmeans_assign", data, centroids)
    data, centroids = _aligned16(data), _aligned16(centroids)
    codes = torch.empty((n,), dtype=torch.int32, device=data.device)
    sums = torch.empty((k, d) if with_sums else (0, d), dtype=torch.int64, device=data.device)
    counts = torch.empty((k,) if with_sums else (0,), dtype=torch.int32, device=data.device)
    ws_bytes = int(_lib.aqlm_hip_kmeans_workspace_bytes(n, k, d))
    ws = _workspace(data.device, ws_bytes)
    with _device_guard(data.device):
        rc = _lib.aqlm_hip_kmeans_assign(data.data_ptr(), n, centroids.data_ptr(), k, d, float(data_absmax), codes.data_ptr(),
                                         sums.data_ptr() if with_sums else None, counts.data_ptr() if with_sums else None,
                                         ws.data_ptr(), ws.numel() * 4, _stream_ptr(data.device))
    if rc:
        _native.check(rc, "aqlm kmeans assign")
    return codes, sums, counts


def _fake_kmeans_assign(data, centroids, data_absmax, with_sums):
    k, d = (int(centroids.shape[0]), int(centroids.shape[1])) if with_sums else (0, int(centroids.shape[1]))
    return (data.new_empty((data.shape[0],), dtype=torch.int32), data.new_empty((k, d), dtype=torch.int64),
            data.new_empty((k,), dtype=torch.int32))


register_op("kmeans_assign", "(Tensor data, Tensor centroids, float data_absmax, bool with_sums) -> (Tensor, Tensor, Tensor)",
            _kmeans_assign_op, _fake_kmeans_assign)


def kmeans_assign(data, centroids, data_absmax: float, with_sums: bool = True):
    """-> (codes int32 [n], sums int64 [k, d], counts int32 [k]): per row of ``data`` [n, d] (fp32, d 8 / 16) the index of the row of
    ``centroids`` [k, d] (fp32, k a multiple of 128 up to 65536) that minimises ``|C_c|^2 - 2 <x_n, C_c>`` -- equal computed scores
    give the smallest index, the accuracy contract is in include/aqlm_hip.h (``KMEANS_EPS``) -- and the fixed-point sums and counts of
    every cluster's points in the unit that ``data_absmax`` (>= every |element| of ``data``) and n set (tests/kmeans_model.py restates
    it); a point with a non-finite element or one above ``data_absmax`` adds nothing.  ``with_sums=False``: the codes alone (the other two
    tensors are empty).  Memsets and three launches on the current stream, the centroids' split image in the cached workspace."""
    return _kmeans_assign_op(data, centroids, float(data_absmax), bool(with_sums))


def kmeans_update_(centroids, sums, counts, n: int, data_absmax: float) -> None:
    """``centroids[c] = sums[c] * 2^-s / counts[c]`` in place where ``counts[c] > 0`` (double arithmetic, one rounding to fp32); an empty
    cluster keeps its centroid bit for bit.  ``n`` and ``data_absmax``: those of the ``kmeans_assign`` call that made the sums."""
    if centroids.dim() != 2 or centroids.dtype != torch.float32 or not centroids.is_cuda or not centroids.is_contiguous():
        raise ValueError(f"kmeans_update_: centroids must be contiguous fp32 [k, d] on the GPU, got {centroids.dtype} {tuple(centroids.shape)}")
    k, d = int(centroids.shape[0]), int(centroids.shape[1])
    if (sums.dtype != torch.int64 or tuple(sums.shape) != (k, d) or not sums.is_contiguous() or sums.device != centroids.device
            or counts.dtype != torch.int32 or tuple(counts.shape) != (k,) or not counts.is_contiguous() or counts.device != centroids.device):
        raise ValueError(f"kmeans_update_: sums must be contiguous int64 [{k}, {d}] and counts int32 [{k}] on {centroids.device}")
    with _device_guard(centroids.device):
        rc = _lib.aqlm_hip_kmeans_update(sums.data_ptr(), counts.data_ptr(), int(n), k, d, float(data_absmax), centroids.data_ptr(),
                                         _stream_ptr(centroids.device))
    if rc:
        _native.check(rc, "aqlm kmeans update")


register_op("kmeans_update_", "(Tensor(a!) centroids, Tensor sums, Tensor counts, int n, float data_absmax) -> ()", kmeans_update_,
            lambda centroids, sums, counts, n, data_absmax: None)


def kmeans_update(centroids, sums, counts, n: int, data_absmax: float) -> torch.Tensor:
    """``kmeans_update_`` on a copy: the new centroids."""
    out = centroids.detach().clone(memory_format=torch.contiguous_format)
    kmeans_update_(out, sums, counts, n, data_absmax)
    return out


# ------------------------------------------------------------------------------------------------------
# beam search over the codebooks of the K x 8 schemes (the V step of PV-tuning; aqlm_hip_code_search_kx8)
# ------------------------------------------------------------------------------------------------------
CODE_SEARCH_KX8_MAX_BEAM = 16  # AQLM_HIP_CODE_SEARCH_KX8_MAX_BEAM


def code_search_kx8_supported(out_features: int, in_features: int, num_codebooks: int, in_group_size: int, beam_size: int) -> bool:
    return bool(_lib.aqlm_hip_code_search_kx8_supported(int(out_features), int(in_features), int(num_codebooks), int(in_group_size),
                                                        int(beam_size)))


def _dim_order(who: str, dim_order, K: int):
    """``dim_order`` as a list of ints (None stays None); anything but a permutation of 0 .. K - 1 is a ValueError in ``who``'s name."""
    if dim_order is None:
        return None
    order = [int(c) for c in dim_order]
    if sorted(order) != list(range(K)):
        raise ValueError(f"{who}: dim_order must be a permutation of 0 .. {K - 1}, got {order}")
    return order


def _code_search_kx8_impl(reference, scales, codebooks, prev_codes, group_ids, codes_out, geometry, want_scores):
    out_features, in_features, K, g, beam_size = (int(x) for x in geometry[:5])
    if (reference.dim() != 2 or tuple(reference.shape) != (out_features, in_features) or reference.dtype not in _GRAD_DT
            or not reference.is_cuda):
        raise ValueError(f"code_search_kx8: reference must be fp16 / bf16 / fp32 [{out_features}, {in_features}] on the GPU, got "
                         f"{reference.dtype} {tuple(reference.shape)}")
    if reference.stride(1) != 1 or reference.stride(0) < in_features:  # a transposed or expanded view: the kernel walks rows
        reference = reference.contiguous()
    if codebooks.numel() != K * 256 * g or codebooks.device != reference.device:
        raise ValueError(f"code_search_kx8: the codebooks must hold {K} x 256 x {g} elements on {reference.device}")
    dt = _dtype_id(codebooks)
    codebooks = _c(codebooks)
    if scales is not None:
        if scales.numel() != out_features or scales.device != reference.device or scales.dtype != codebooks.dtype:
            raise ValueError(f"code_search_kx8: scales must hold {out_features} elements of {codebooks.dtype} on {reference.device}")
        scales = _c(scales)
    total = out_features * (in_features // max(g, 1))
    if prev_codes.dtype != torch.int8 or prev_codes.numel() != total * K or prev_codes.device != reference.device:
        raise ValueError(f"code_search_kx8: prev_codes must hold {total} x {K} int8 codes (the whole layer) on {reference.device}")
    prev_codes = _c(prev_codes)
    order = _dim_order("code_search_kx8", geometry[5:] or None, K)  # (the geometry ends after beam_size: no dim_order)
    if group_ids is not None:
        if group_ids.dtype not in (torch.int32, torch.int64) or group_ids.dim() != 1 or group_ids.device != reference.device:
            raise ValueError("code_search_kx8: group_ids must be a 1-d int32 / int64 tensor on the reference's device")
        group_ids = _c(group_ids)
        n = int(group_ids.numel())
    else:
        n = total
    if codes_out is None:
        codes_out = torch.empty((n, K), dtype=torch.int8, device=reference.device)
    elif codes_out.dtype != torch.int8 or codes_out.numel() != n * K or not codes_out.is_contiguous() or codes_out.device != reference.device:
        raise ValueError(f"code_search_kx8: codes_out must be contiguous int8 [{n}, {K}] on {reference.device}")
    scores = torch.empty((n,), dtype=torch.float32, device=reference.device) if want_scores else None
    if n == 0:
        return codes_out, scores
    dim_order = (ctypes.c_int * K)(*order) if order else None
    with _device_guard(reference.device):
        rc = _lib.aqlm_hip_code_search_kx8(reference.data_ptr(), _GRAD_DT[reference.dtype], reference.stride(0), _ptr(scales),
                                           codebooks.data_ptr(), dt, prev_codes.data_ptr(), out_features, in_features, K, g, beam_size,
                                           dim_order, _ptr(group_ids), int(group_ids is not None and group_ids.dtype == torch.int64), n,
                                           codes_out.data_ptr(), _ptr(scores), None, 0, _stream_ptr(reference.device))
    if rc:
        _native.check(rc, "aqlm code search kx8")
    return codes_out, scores


def _code_search_kx8_op(reference, scales, codebooks, prev_codes, group_ids, geometry):
    return _code_search_kx8_impl(reference, scales, codebooks, prev_codes, group_ids, None, geometry, True)


def _fake_code_search_kx8(reference, scales, codebooks, prev_codes, group_ids, geometry):
    n = int(group_ids.numel()) if group_ids is not None else int(geometry[0]) * (int(geometry[1]) // int(geometry[3]))
    return reference.new_empty((n, int(geometry[2])), dtype=torch.int8), reference.new_empty((n,), dtype=torch.float32)


# geometry = [out_features, in_features, K, g, beam_size] + dim_order (or nothing); -> the codes [n, K] int8 and the fp32 score of
# every returned hypothesis [n]
register_op("code_search_kx8", "(Tensor reference, Tensor? scales, Tensor codebooks, Tensor prev_codes, Tensor? group_ids, "
            "int[] geometry) -> (Tensor, Tensor)", _code_search_kx8_op, _fake_code_search_kx8)


def code_search_kx8(reference, scales, codebooks, prev_codes, in_group_size: int, beam_size: int, dim_order=None, group_ids=None,
                    codes_out=None, return_scores: bool = False):
    """int8 codes [n, K]: for every group of ``in_group_size`` weights of ``reference`` [out, in] (fp32 / fp16 / bf16, any row stride; a
    view with another column stride is copied first) -- or for the flat groups ``group_ids`` (int32 / int64, ``o * (in / g) + j``), in
    their order -- the codes the reference's beam search over the ``K`` codebooks (``codebooks``: K x 256 x g elements, fp16 / bf16)
    reaches from ``prev_codes`` (int8, the WHOLE layer's [out * in / g, K], read at the group's id) with ``beam_size`` hypotheses,
    revisiting the codebooks in ``dim_order`` (default 0 .. K - 1); ``scales`` ([out] elements in the codebook dtype) None = 1.  The
    arithmetic is fixed operation for operation in include/aqlm_hip.h (tests/kx8_search_model.py is its numpy restatement): equal
    scores go to the smaller flat index ``position * 256 + code``.  ``codes_out`` (int8, K entries per group searched): written in
    place when given -- an id outside the layer leaves its entries as they were.  ``return_scores``: also the fp32 score of the
    returned hypothesis on the last step, [n].  One launch on the current stream, no workspace."""
    g, K = int(in_group_size), int(codebooks.shape[0])
    order = _dim_order("code_search_kx8", dim_order, K) or []
    codes, scores = _code_search_kx8_impl(reference, scales, codebooks, prev_codes, group_ids, codes_out,
                                          [int(reference.shape[0]), int(reference.shape[1]), K, g, int(beam_size)] + order, return_scores)
    return (codes, scores) if return_scores else codes


# ------------------------------------------------------------------------------------------------------
# the calibrated beam search of the K x 8 schemes, one input group per launch (aqlm_hip_code_search_kx8_xtx)
# ------------------------------------------------------------------------------------------------------
def code_search_kx8_xtx_supported(out_features: int, num_codebooks: int, in_group_size: int, beam_size: int, positions_in: int = 1) -> bool:
    return bool(_lib.aqlm_hip_code_search_kx8_xtx_supported(int(out_features), int(num_codebooks), int(in_group_size), int(beam_size),
                                                            int(positions_in)))


class XtxStep(NamedTuple):
    """What one launch of aqlm_hip_code_search_kx8_xtx returns, every tensor [beam_size, out, ...] with rank 0 the best."""

    loss: torch.Tensor     # fp32 [beam, out]
    codes: torch.Tensor    # int8 [beam, out, K]
    source: torch.Tensor   # uint8 [beam, out]: the position at entry
    delta: torch.Tensor    # fp32 [beam, out, g]
    t: Optional[torch.Tensor]  # fp32 [beam, out, g] when asked for


def code_search_kx8_xtx_step(t, loss, codes_in, H, q, codebooks, scales, beam_size: int, dim_order=None, return_t: bool = False) -> XtxStep:
    """One launch of aqlm_hip_code_search_kx8_xtx: all K codebook steps of the calibrated beam search for ONE input group and every
    output row (include/aqlm_hip.h has the definition and the arithmetic, tests/kx8_xtx_model.py its numpy restatement).  ``t`` fp32
    [positions, out, g] -- the group's slice of ``T = (W_ref - W_position) XTX``, any position / row stride with g contiguous (a view
    into a wider buffer is read in place) --, ``loss`` fp32 [positions, out], ``codes_in`` int8 [positions, out, K], ``H`` fp32 [g, g] =
    ``XTX[group, group]``, ``q`` fp32 [K, 256] = ``C H C^T`` unscaled, ``codebooks`` K x 256 x g elements fp16 / bf16, ``scales`` [out]
    elements in the same dtype or None.  One launch on the current stream; no workspace, no synchronisation."""
    if t.dim() != 3 or t.dtype != torch.float32 or not t.is_cuda:
        raise ValueError(f"code_search_kx8_xtx_step: t must be fp32 [positions, out, g] on the GPU, got {t.dtype} {tuple(t.shape)}")
    positions, out_features, g = (int(x) for x in t.shape)
    K, beam_size = int(codebooks.shape[0]), int(beam_size)
    dev = t.device
    if t.stride(2) != 1 or t.stride(1) < g or (positions > 1 and t.stride(0) < g):
        t = t.contiguous()
    if codebooks.numel() != K * 256 * g or codebooks.device != dev:
        raise ValueError(f"code_search_kx8_xtx_step: the codebooks must hold {K} x 256 x {g} elements on {dev}")
    dt = _dtype_id(codebooks)
    codebooks = _c(codebooks)
    for name, x, shape, dtype in (("loss", loss, (positions, out_features), torch.float32), ("codes_in", codes_in, (positions, out_features, K), torch.int8),
                                  ("H", H, (g, g), torch.float32), ("q", q, (K, 256), torch.float32)):
        if tuple(x.shape) != shape or x.dtype != dtype or x.device != dev:
            raise ValueError(f"code_search_kx8_xtx_step: {name} must be {dtype} {list(shape)} on {dev}, got {x.dtype} {tuple(x.shape)}")
    loss, codes_in, H, q = _c(loss), _c(codes_in), _c(H), _c(q)
    if scales is not None:
        if scales.numel() != out_features or scales.device != dev or scales.dtype != codebooks.dtype:
            raise ValueError(f"code_search_kx8_xtx_step: scales must hold {out_features} elements of {codebooks.dtype} on {dev}")
        scales = _c(scales)
    order = _dim_order("code_search_kx8_xtx_step", dim_order, K)
    if not code_search_kx8_xtx_supported(out_features, K, g, beam_size, positions):
        raise NotImplementedError(f"code_search_kx8_xtx_step: K={K} g={g} beam_size={beam_size} positions={positions} is outside the kernel")
    out = XtxStep(torch.empty((beam_size, out_features), dtype=torch.float32, device=dev),
                  torch.empty((beam_size, out_features, K), dtype=torch.int8, device=dev),
                  torch.empty((beam_size, out_features), dtype=torch.uint8, device=dev),
                  torch.empty((beam_size, out_features, g), dtype=torch.float32, device=dev),
                  torch.empty((beam_size, out_features, g), dtype=torch.float32, device=dev) if return_t else None)
    with _device_guard(dev):
        rc = _lib.aqlm_hip_code_search_kx8_xtx(t.data_ptr(), t.stride(0), t.stride(1), loss.data_ptr(), codes_in.data_ptr(), H.data_ptr(),
                                               q.data_ptr(), codebooks.data_ptr(), dt, _ptr(scales), out_features, K, g, beam_size, positions,
                                               None if order is None else (ctypes.c_int * K)(*order), out.loss.data_ptr(),
                                               out.codes.data_ptr(), out.source.data_ptr(), out.delta.data_ptr(), _ptr(out.t), None, 0,
                                               _stream_ptr(dev))
    if rc:
        _native.check(rc, "aqlm code search kx8 xtx")
    return out


# ------------------------------------------------------------------------------------------------------
# the calibrated search of the 1x16 schemes, one input group per call (aqlm_hip_code_search_1x16_xtx)
# ------------------------------------------------------------------------------------------------------
CODE_SEARCH_1X16_XTX_MAX_BEAM = 8  # AQLM_HIP_CODE_SEARCH_1X16_XTX_MAX_BEAM


def code_search_1x16_xtx_supported(out_features: int, in_group_size: int, beam_size: int, positions_in: int = 1) -> bool:
    return bool(_lib.aqlm_hip_code_search_1x16_xtx_supported(int(out_features), int(in_group_size), int(beam_size), int(positions_in)))


def code_search_1x16_xtx_step(t, loss, codes_in, H, q, codebook, scales, beam_size: int, return_t: bool = False) -> XtxStep:
    """One call of aqlm_hip_code_search_1x16_xtx: the calibrated search of ONE input group of a 1x16 layer for every output row
    (include/aqlm_hip.h has the definition and the arithmetic, tests/x16_xtx_model.py its numpy restatement).  ``t`` fp32 [positions, out,
    g] -- any position / row stride with g contiguous (a view into a wider buffer is read in place) --, ``loss`` fp32 [positions, out],
    ``codes_in`` int16 [positions, out, 1], ``H`` fp32 [g, g] = ``XTX[group, group]``, ``q`` fp32 [65536] (or [1, 65536]) = ``C H C^T``
    unscaled, ``codebook`` 65536 x g elements fp16 / bf16, ``scales`` [out] elements in the same dtype or None.  Returns an ``XtxStep``
    with int16 codes [beam_size, out, 1].  Three launches on the current stream through a workspace allocated on the current device;
    no synchronisation."""
    if t.dim() != 3 or t.dtype != torch.float32 or not t.is_cuda:
        raise ValueError(f"code_search_1x16_xtx_step: t must be fp32 [positions, out, g] on the GPU, got {t.dtype} {tuple(t.shape)}")
    positions, out_features, g = (int(x) for x in t.shape)
    beam_size = int(beam_size)
    dev = t.device
    if t.stride(2) != 1 or t.stride(1) < g or (positions > 1 and t.stride(0) < g):
        t = t.contiguous()
    if codebook.numel() != 65536 * g or codebook.device != dev:
        raise ValueError(f"code_search_1x16_xtx_step: the codebook must hold 65536 x {g} elements on {dev}")
    dt = _dtype_id(codebook)
    codebook = _c(codebook)
    if q.dim() == 2 and q.shape[0] == 1:
        q = q[0]
    for name, x, shape, dtype in (("loss", loss, (positions, out_features), torch.float32), ("codes_in", codes_in, (positions, out_features, 1), torch.int16),
                                  ("H", H, (g, g), torch.float32), ("q", q, (65536,), torch.float32)):
        if tuple(x.shape) != shape or x.dtype != dtype or x.device != dev:
            raise ValueError(f"code_search_1x16_xtx_step: {name} must be {dtype} {list(shape)} on {dev}, got {x.dtype} {tuple(x.shape)}")
    loss, codes_in, H, q = _c(loss), _c(codes_in), _c(H), _c(q)
    if scales is not None:
        if scales.numel() != out_features or scales.device != dev or scales.dtype != codebook.dtype:
            raise ValueError(f"code_search_1x16_xtx_step: scales must hold {out_features} elements of {codebook.dtype} on {dev}")
        scales = _c(scales)
    if not code_search_1x16_xtx_supported(out_features, g, beam_size, positions):
        raise NotImplementedError(f"code_search_1x16_xtx_step: g={g} beam_size={beam_size} positions={positions} is outside the kernel")
    out = XtxStep(torch.empty((beam_size, out_features), dtype=torch.float32, device=dev),
                  torch.empty((beam_size, out_features, 1), dtype=torch.int16, device=dev),
                  torch.empty((beam_size, out_features), dtype=torch.uint8, device=dev),
                  torch.empty((beam_size, out_features, g), dtype=torch.float32, device=dev),
                  torch.empty((beam_size, out_features, g), dtype=torch.float32, device=dev) if return_t else None)
    need = int(_lib.aqlm_hip_code_search_1x16_xtx_workspace_bytes(out_features, g, beam_size, positions))
    with _device_guard(dev):
        workspace = torch.empty((need,), dtype=torch.uint8, device=dev)
        rc = _lib.aqlm_hip_code_search_1x16_xtx(t.data_ptr(), t.stride(0), t.stride(1), loss.data_ptr(), codes_in.data_ptr(), H.data_ptr(),
                                                q.data_ptr(), codebook.data_ptr(), dt, _ptr(scales), out_features, g, beam_size, positions,
                                                out.loss.data_ptr(), out.codes.data_ptr(), out.source.data_ptr(), out.delta.data_ptr(),
                                                _ptr(out.t), workspace.data_ptr(), need, _stream_ptr(dev))
    if rc:
        _native.check(rc, "aqlm code search 1x16 xtx")
    return out
