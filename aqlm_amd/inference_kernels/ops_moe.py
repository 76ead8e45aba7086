"""The mixture-of-experts launches and their ``aqlm::`` ops: the routed 1x16 matvec, the routed matvec on prepacked experts, and
the expert-grouped GEMM with its transposed twin (``aqlm_amd/moe.py`` is the module-level interface).  Every name here is
re-exported by ``hip_kernel``, which is where callers and tests reach it."""
from __future__ import annotations

import ctypes

import torch

from .. import _native
from .._native import lib as _lib
from ._launch import _c, _device_guard, _dtype_id, _flat_rows, _ptr, _stream_ptr, register_op


# ------------------------------------------------------------------------------------------------------
# expert-routed 1x16 matvec (mixture-of-experts decode; aqlm_hip_gemv_1x16_routed)
# ------------------------------------------------------------------------------------------------------
def routed_table(layers, device) -> torch.Tensor:
    """The device-resident table of aqlm_hip_gemv_1x16_routed: ``layers[e][s] = (codes, codebooks, scales, bias or None)``
    -> int64 [E * S * 4] of device pointers, entry [e * S + s].  The table holds raw addresses: the caller keeps the tensors
    alive and rebuilds it when one of them moves (``aqlm_amd.moe.QuantizedMixtralExperts`` keys it on data_ptr + version).
    A host-to-device copy: never while a hipGraph is being captured."""
    words = []
    for per_expert in layers:
        for codes, codebooks, scales, bias in per_expert:
            for t in (codes, codebooks, scales):
                if not t.is_contiguous() or t.data_ptr() % 16:
                    raise ValueError("routed table: codes / codebooks / scales must be contiguous and 16-byte aligned")
            if bias is not None and not bias.is_contiguous():
                raise ValueError("routed table: bias must be contiguous")
            words += [codes.data_ptr(), codebooks.data_ptr(), scales.data_ptr(), 0 if bias is None else bias.data_ptr()]
    return torch.tensor(words, dtype=torch.int64).to(device)


def routed_chunks(tokens: int, top_k: int):
    """Token ranges [t0, t1) of the routed launches that serve ``tokens`` tokens: at most MAX_ROUTED_PAIRS (token, expert) pairs
    per launch, whole tokens only."""
    per = max(1, _native.MAX_ROUTED_PAIRS // max(1, top_k))
    return [(t0, min(tokens, t0 + per)) for t0 in range(0, tokens, per)]


def _check_routed_args(input, expert_ids, table, E, S, in_features, top_k, x_per_pair, entry_words, words) -> int:
    """The id, input and table checks of the two routed ops (``words``: the table length the caller was told) -> tokens."""
    if expert_ids.dim() != 2 or expert_ids.shape[1] != top_k or expert_ids.dtype not in (torch.int64, torch.int32):
        raise ValueError(f"expert_ids must be [T, {top_k}] int64 / int32, got {tuple(expert_ids.shape)} {expert_ids.dtype}")
    T = expert_ids.shape[0]
    rows = T * top_k if x_per_pair else T
    if input.dim() != 2 or tuple(input.shape) != (rows, in_features):
        raise ValueError(f"input must be [{rows}, {in_features}], got {tuple(input.shape)}")
    if table.dtype != torch.int64 or table.numel() != words or words != E * S * entry_words or table.device != input.device:
        raise ValueError(f"table must be int64 [{E * S * entry_words}] on {input.device}")
    if expert_ids.device != input.device:
        raise ValueError("expert_ids must be on the input's device")
    return T


def _routed_launches(x, ids, y, top_k, x_per_pair, what, launch) -> None:
    """One ``launch(ids pointer, ids_int64, pairs, x pointer, y pointer) -> rc`` per chunk of ``routed_chunks``."""
    esz = ids.element_size()
    with _device_guard(x.device):
        for t0, t1 in routed_chunks(ids.shape[0], top_k):
            p0 = t0 * top_k
            rc = launch(ids.data_ptr() + p0 * esz, int(esz == 8), (t1 - t0) * top_k,
                        x.data_ptr() + (p0 if x_per_pair else t0) * x.stride(0) * 2, y.data_ptr() + p0 * y.stride(0) * 2)
            if rc:
                _native.check(rc, what)


def code1x16_moe_matmat(input, expert_ids, table, geometry, x_per_pair):
    """Every (token, expert) pair of one or two 1x16 projections of a mixture-of-experts block in one launch per 64 pairs.
    geometry = [num_experts, num_segments, out_features, in_features, in_group_size, top_k]; ``expert_ids`` [T, top_k] int64 /
    int32 on the device (what the router's topk returns; read on the device only, any values are safe: ids outside
    [0, num_experts) give zero rows); ``input`` [T, in] (token rows, ``x_per_pair`` False) or [T * top_k, in] (pair rows);
    ``table`` from ``routed_table``.  -> [T * top_k, num_segments, out_features]; row (t * top_k + j, s) is projection s of
    expert expert_ids[t, j] applied to its x row, bit-identical to code1x16_matmat of that expert on that row."""
    E, S, out_features, in_features, g, top_k = (int(v) for v in geometry)
    dt = _dtype_id(input)
    T = _check_routed_args(input, expert_ids, table, E, S, in_features, top_k, x_per_pair, _native.ROUTED_ENTRY_WORDS,
                           E * S * _native.ROUTED_ENTRY_WORDS)
    x = _flat_rows(input)
    ids = _c(expert_ids)
    y = torch.empty((T * top_k, S, out_features), dtype=input.dtype, device=input.device)
    if T == 0:
        return y
    stream = _stream_ptr(input.device)
    _routed_launches(x, ids, y, top_k, x_per_pair, "aqlm routed gemv", lambda idp, i64, npairs, xp, yp: _lib.aqlm_hip_gemv_1x16_routed(
        table.data_ptr(), E, S, idp, i64, npairs, top_k, xp, x.stride(0), int(bool(x_per_pair)), yp, out_features, in_features, g, dt,
        stream))
    return y


def _fake_moe(input, expert_ids, table, geometry, x_per_pair):
    return input.new_empty((expert_ids.shape[0] * expert_ids.shape[1], int(geometry[1]), int(geometry[2])))


_MOE_SCHEMA = "(Tensor input, Tensor expert_ids, Tensor table, int[] geometry, bool x_per_pair) -> Tensor"
register_op("code1x16_moe_matmat", _MOE_SCHEMA, code1x16_moe_matmat, _fake_moe)


# ------------------------------------------------------------------------------------------------------
# expert-routed matvec on PREPACKED experts (mixture-of-experts decode; aqlm_hip_gemv_1x16_routed_packed)
# ------------------------------------------------------------------------------------------------------
ROUTED_PACKED_GEOMETRY_INTS = 11  # [E, S, out, in, g, top_k] + rows_per_group, max_waves, slice_first, lds_bytes, table words


def _desc_array(packed_list):
    return (_native._descp * len(packed_list))(*[ctypes.pointer(p.desc) for p in packed_list])


def routed_packed_supported(packed_list) -> bool:
    """Will aqlm_hip_gemv_1x16_routed_packed serve a table of these ``PackedCodes`` (one shape; 4-byte entries, uniform geometry, a
    codebook range each)?  A host query on the descriptors."""
    from .hip_kernel import PackedCodes  # at call time: hip_kernel imports this module, and this is load-time code

    if not packed_list or any(p is None or not isinstance(p, PackedCodes) for p in packed_list):
        return False
    return bool(_lib.aqlm_hip_gemv_1x16_routed_packed_supported(_desc_array(packed_list), len(packed_list)))


def routed_packed_table(layers, device):
    """The device-resident table of aqlm_hip_gemv_1x16_routed_packed and its launch geometry: ``layers[e][s] = (packed,
    codebooks, scales, bias or None)`` with ``packed`` the layer's ``PackedCodes`` -> (int64 table on ``device``, entry [e * S + s]
    as filled by aqlm_hip_routed_packed_entry_fill; geometry tail for ``code1x16_moe_matmat_packed``).  Every expert's codebook
    range -- and the codebook image of a relabelled buffer -- is brought up to date first (``refresh_range``): the table bakes in
    the bound and the image's address.  The table holds raw addresses: the caller keeps the tensors alive and rebuilds it when one
    of them moves or is rewritten.  A host-to-device copy (and, for a stale range, a read-back): never while a hipGraph is being
    captured.  NotImplementedError when the launch declines the table (the caller keeps the routed launch on the canonical
    codes)."""
    from .hip_kernel import refresh_range  # at call time: hip_kernel imports this module, and this is load-time code

    if torch.cuda.is_current_stream_capturing():
        raise RuntimeError("routed_packed_table: the table is built by a host-to-device copy; build it before capturing")
    entries, packs = [], []
    for per_expert in layers:
        for packed, codebooks, scales, bias in per_expert:
            for t in (codebooks, scales):
                if not t.is_contiguous() or t.data_ptr() % 16:
                    raise ValueError("routed packed table: codebooks / scales must be contiguous and 16-byte aligned")
            if bias is not None and not bias.is_contiguous():
                raise ValueError("routed packed table: bias must be contiguous")
            refresh_range(packed, codebooks)
            ent = _native.RoutedPackedEntry()
            rc = _lib.aqlm_hip_routed_packed_entry_fill(ctypes.byref(packed.desc), packed.data_ptr(), codebooks.data_ptr(),
                                                        scales.data_ptr(), _ptr(bias), ctypes.byref(ent))
            if rc:
                _native.check(rc, "aqlm routed_packed_entry_fill")
            entries.append(ent)
            packs.append(packed)
    geom = _native.RoutedPackedGeometry()
    rc = _lib.aqlm_hip_gemv_1x16_routed_packed_geometry(_desc_array(packs), len(packs), ctypes.byref(geom))
    if rc:
        _native.check(rc, "aqlm routed_packed_geometry")
    raw = b"".join(bytes(e) for e in entries)
    table = torch.frombuffer(bytearray(raw), dtype=torch.int64).clone().to(device)
    tail = [int(geom.rows_per_group), int(geom.max_waves), int(geom.slice_first), int(geom.lds_bytes), int(table.numel())]
    return table, tail


# Accumulator cells of the routed packed launch: [pairs][segments][out_features] u64, zero at rest.  One zero-filled buffer per
# table (= per block and projection launch) and size class, allocated at the first eager call and reused by every later call,
# captured ones included -- a capture runs on a stream of its own, so a per-stream registry would find nothing there, and
# nothing can be allocated for good inside a capture.  The kernel leaves every cell it touched at zero.  Like the cells inside a
# packed buffer, a set serves one stream at a time: one block must not run on two streams at once.  A hipGraph may have captured
# an address, so a buffer is never resized or freed behind its back: sizes are rounded up to a power of two and each size class
# is allocated once (release_routed_packed_cells frees them when the caller knows no such graph is alive).
_ROUTED_PACKED_CELLS = {}


def routed_packed_cells(device: torch.device, owner: int, nbytes: int):
    size = 1 << max(16, (int(nbytes) - 1).bit_length())
    key = (device.index, owner, size)
    cells = _ROUTED_PACKED_CELLS.get(key)
    if cells is None:
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("code1x16_moe_matmat_packed: the accumulator cells are allocated at the first eager call; run one "
                               "eager forward of this size before capturing")
        with torch.cuda.device(device):
            cells = torch.zeros((size // 8,), dtype=torch.int64, device=device)
        _ROUTED_PACKED_CELLS[key] = cells
    return cells


def release_routed_packed_cells() -> int:
    """Free every cell buffer of the routed packed launch (the caller knows that no hipGraph that captured one is alive)."""
    n = len(_ROUTED_PACKED_CELLS)
    _ROUTED_PACKED_CELLS.clear()
    return n


def code1x16_moe_matmat_packed(input, expert_ids, table, geometry, x_per_pair):
    """``code1x16_moe_matmat`` on prepacked experts: every (token, expert) pair of one or two 1x16 projections of a
    mixture-of-experts block in one launch per 64 pairs, each pair a batch-1 pass of the packed matvec on its expert's buffer.
    geometry = [num_experts, num_segments, out_features, in_features, in_group_size, top_k] + the tail ``routed_packed_table``
    returned with ``table``.  ``expert_ids`` [T, top_k] int64 / int32 on the device (read there only; ids outside
    [0, num_experts) give zero rows); ``input`` [T, in] (token rows) or [T * top_k, in] (``x_per_pair``).
    -> [T * top_k, num_segments, out_features]; row (t * top_k + j, s) is bit-identical to ``code1x16_matmat_packed`` of expert
    expert_ids[t, j], projection s, on that row alone."""
    if len(geometry) != ROUTED_PACKED_GEOMETRY_INTS:
        raise ValueError(f"geometry must hold {ROUTED_PACKED_GEOMETRY_INTS} ints (shape + the tail of routed_packed_table)")
    E, S, out_features, in_features, g, top_k, rpg, max_waves, slice_first, lds_bytes, words = (int(v) for v in geometry)
    dt = _dtype_id(input)
    T = _check_routed_args(input, expert_ids, table, E, S, in_features, top_k, x_per_pair, _native.ROUTED_PACKED_ENTRY_WORDS, words)
    x = _flat_rows(input)
    if x.data_ptr() % 16 or (x.stride(0) * 2) % 16:
        x = x.clone(memory_format=torch.contiguous_format)
    ids = _c(expert_ids)
    y = torch.empty((T * top_k, S, out_features), dtype=input.dtype, device=input.device)
    if T == 0:
        return y
    geom = _native.RoutedPackedGeometry(out_features, in_features, g, rpg, max_waves, slice_first, lds_bytes, 0)
    stream = _stream_ptr(input.device)
    max_pairs = max(t1 - t0 for t0, t1 in routed_chunks(T, top_k)) * top_k
    cells = routed_packed_cells(input.device, table.data_ptr(), max_pairs * S * out_features * 8)
    _routed_launches(x, ids, y, top_k, x_per_pair, "aqlm routed packed gemv",
                     lambda idp, i64, npairs, xp, yp: _lib.aqlm_hip_gemv_1x16_routed_packed(
                         table.data_ptr(), ctypes.byref(geom), E, S, idp, i64, npairs, top_k, xp, x.stride(0), int(bool(x_per_pair)),
                         yp, dt, cells.data_ptr(), cells.numel() * 8, stream))
    return y


register_op("code1x16_moe_matmat_packed", _MOE_SCHEMA, code1x16_moe_matmat_packed, _fake_moe)


# ------------------------------------------------------------------------------------------------------
# expert-grouped 1x16 GEMM (mixture-of-experts prefill / training; aqlm_hip_moe_bucket + aqlm_hip_gemm_1x16_grouped)
# ------------------------------------------------------------------------------------------------------
def grouped_tile_pairs(num_pairs: int, num_experts: int) -> int:
    """Pairs per tile of the grouped launches: the mean pairs per expert rounded up to a power of two, 16 .. 128.  A function of
    the sizes only, never of the routing, so a captured graph serves every routing."""
    mean = -(-int(num_pairs) // max(1, int(num_experts)))
    t = _native.GROUPED_TILE_PAIRS[0]
    while t < mean and t < _native.GROUPED_TILE_PAIRS[-1]:
        t *= 2
    return t


def grouped_supported(out_features: int, in_features: int, in_group_size: int) -> bool:
    """Whether aqlm_hip_gemm_1x16_grouped takes a layer of this shape (a host query: decide before a capture)."""
    return bool(_lib.aqlm_hip_gemm_1x16_grouped_supported(int(out_features), int(in_features), int(in_group_size)))


def _bucket_words(num_pairs: int, num_experts: int, tile_pairs: int) -> int:
    n = _lib.aqlm_hip_moe_bucket_bytes(int(num_pairs), int(num_experts), int(tile_pairs))
    if n == 0:
        raise ValueError(f"moe_bucket: {num_pairs} pairs, {num_experts} experts, tiles of {tile_pairs} are outside the entry "
                         f"(1..{_native.MAX_GROUPED_PAIRS} pairs, 1..{_native.MAX_ROUTED_EXPERTS} experts, tiles of "
                         f"{'/'.join(map(str, _native.GROUPED_TILE_PAIRS))})")
    return n // 4


def moe_bucket(expert_ids, num_experts, tile_pairs):
    """The router's ids [T, top_k] (int64 / int32, device) grouped by expert on the device (aqlm_hip_moe_bucket): an int32
    buffer whose size depends on T * top_k, num_experts and tile_pairs only.  No host synchronisation."""
    if expert_ids.dim() != 2 or expert_ids.dtype not in (torch.int64, torch.int32):
        raise ValueError(f"expert_ids must be [T, top_k] int64 / int32, got {tuple(expert_ids.shape)} {expert_ids.dtype}")
    ids = _c(expert_ids)
    bucket = torch.empty((_bucket_words(ids.numel(), num_experts, tile_pairs),), dtype=torch.int32, device=ids.device)
    with _device_guard(ids.device):
        rc = _lib.aqlm_hip_moe_bucket(ids.data_ptr(), int(ids.element_size() == 8), ids.numel(), int(num_experts), int(tile_pairs),
                                      bucket.data_ptr(), _stream_ptr(ids.device))
    if rc:
        _native.check(rc, "aqlm moe bucket")
    return bucket


def _fake_bucket(expert_ids, num_experts, tile_pairs):
    return expert_ids.new_empty((_bucket_words(expert_ids.shape[0] * expert_ids.shape[1], num_experts, tile_pairs),),
                                dtype=torch.int32)


register_op("moe_bucket", "(Tensor expert_ids, int num_experts, int tile_pairs) -> Tensor", moe_bucket, _fake_bucket)


def _check_grouped_args(table, bucket, E, S, P, tile_pairs, device) -> None:
    """The table and bucket checks of the grouped forward and its transposed op."""
    if table.dtype != torch.int64 or table.numel() != E * S * _native.ROUTED_ENTRY_WORDS or table.device != device:
        raise ValueError(f"table must be int64 [{E * S * _native.ROUTED_ENTRY_WORDS}] on {device}")
    if bucket.dtype != torch.int32 or bucket.numel() != _bucket_words(P, E, tile_pairs) or bucket.device != device:
        raise ValueError("bucket must come from moe_bucket with the same pairs, experts and tile size")


def code1x16_moe_matmat_grouped(input, bucket, table, geometry, x_per_pair):
    """``code1x16_moe_matmat`` for any number of pairs, on the expert-grouped 16-row MFMA kernel.  geometry = [num_experts,
    num_segments, out_features, in_features, in_group_size, top_k, tile_pairs, num_pairs]; ``bucket`` from ``moe_bucket`` with
    the same num_pairs / num_experts / tile_pairs; ``table`` from ``routed_table``; ``input`` [num_pairs / top_k, in] (token rows)
    or [num_pairs, in] (``x_per_pair``).  -> [num_pairs, num_segments, out_features]; pairs whose id lies outside [0,
    num_experts) get zero rows.  No host synchronisation."""
    E, S, out_features, in_features, g, top_k, tile_pairs, P = (int(v) for v in geometry)
    dt = _dtype_id(input)
    if top_k < 1 or P % top_k != 0:
        raise ValueError(f"{P} pairs is not a multiple of top_k {top_k}")
    rows = P if x_per_pair else P // top_k
    if input.dim() != 2 or tuple(input.shape) != (rows, in_features):
        raise ValueError(f"input must be [{rows}, {in_features}], got {tuple(input.shape)}")
    _check_grouped_args(table, bucket, E, S, P, tile_pairs, input.device)
    y = torch.empty((P, S, out_features), dtype=input.dtype, device=input.device)
    if P == 0:
        return y
    x = _flat_rows(input)
    with _device_guard(input.device):
        rc = _lib.aqlm_hip_gemm_1x16_grouped(table.data_ptr(), E, S, bucket.data_ptr(), tile_pairs, P, top_k, x.data_ptr(), x.stride(0),
                                             int(bool(x_per_pair)), y.data_ptr(), out_features, in_features, g, dt,
                                             _stream_ptr(input.device))
    if rc:
        _native.check(rc, "aqlm grouped gemm")
    return y


def _fake_grouped(input, bucket, table, geometry, x_per_pair):
    return input.new_empty((int(geometry[7]), int(geometry[1]), int(geometry[2])))


register_op("code1x16_moe_matmat_grouped", "(Tensor input, Tensor bucket, Tensor table, int[] geometry, bool x_per_pair) -> Tensor",
            code1x16_moe_matmat_grouped, _fake_grouped)


def grouped_transposed_supported(out_features: int, in_features: int, in_group_size: int) -> bool:
    """Whether aqlm_hip_gemm_1x16_grouped_transposed takes a layer of this shape (a host query: decide before a capture)."""
    return bool(_lib.aqlm_hip_gemm_1x16_grouped_transposed_supported(int(out_features), int(in_features), int(in_group_size)))


def code1x16_moe_matmat_grouped_transposed(grad_output, bucket, table, geometry):
    """The input gradient of ``code1x16_moe_matmat_grouped``: ``grad_output`` [num_pairs, num_segments, out_features] (fp16 / bf16),
    ``bucket``, ``table`` and ``geometry`` those of the forward call -> fp32 [num_pairs, in_features],
    gx[p] = sum_s (grad_output[p, s] * scales[e_p, s]) @ Wq[e_p, s]; pairs whose id lies outside [0, num_experts) get zero rows.
    One launch, W never leaves the chip, no host synchronisation."""
    E, S, out_features, in_features, g, top_k, tile_pairs, P = (int(v) for v in geometry)
    dt = _dtype_id(grad_output)
    if grad_output.dim() != 3 or tuple(grad_output.shape) != (P, S, out_features):
        raise ValueError(f"grad_output must be [{P}, {S}, {out_features}], got {tuple(grad_output.shape)}")
    _check_grouped_args(table, bucket, E, S, P, tile_pairs, grad_output.device)
    gx = torch.empty((P, in_features), dtype=torch.float32, device=grad_output.device)
    if P == 0:
        return gx
    gy = _c(grad_output)
    if gy.data_ptr() % 16 != 0:
        gy = gy.clone()
    with _device_guard(gy.device):
        rc = _lib.aqlm_hip_gemm_1x16_grouped_transposed(table.data_ptr(), E, S, bucket.data_ptr(), tile_pairs, P, gy.data_ptr(),
                                                        gy.stride(0), gx.data_ptr(), out_features, in_features, g, dt,
                                                        _stream_ptr(gy.device))
    if rc:
        _native.check(rc, "aqlm grouped transposed gemm")
    return gx


def _fake_grouped_transposed(grad_output, bucket, table, geometry):
    return grad_output.new_empty((int(geometry[7]), int(geometry[3])), dtype=torch.float32)


register_op("code1x16_moe_matmat_grouped_transposed", "(Tensor grad_output, Tensor bucket, Tensor table, int[] geometry) -> Tensor",
            code1x16_moe_matmat_grouped_transposed, _fake_grouped_transposed)
