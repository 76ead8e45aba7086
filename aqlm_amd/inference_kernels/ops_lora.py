"""The LoRA adapter launches and their ``aqlm::`` ops: per-row adapters at decode (bgmv) and at prefill (sgmv), the same two on the
routed experts of a mixture-of-experts block, and the backward of the routed adapters (``aqlm_amd/lora.py`` is the module-level
interface).  Every name here is re-exported by ``hip_kernel``, which is where callers and tests reach it."""
from __future__ import annotations

import torch

from .. import _native
from .._native import lib as _lib
from ._launch import _DT, _c, _device_guard, _dtype_id, _flat_rows, _ptr, _stream_ptr, _workspace, register_op
from .ops_moe import _bucket_words  # the routed launches read the expert bucket of the grouped MoE ops


# ------------------------------------------------------------------------------------------------------
# LoRA adapters per row of a decode batch (aqlm_hip_lora_bgmv; aqlm_amd/lora.py is the module-level interface)
# ------------------------------------------------------------------------------------------------------
def lora_table(adapters, device) -> torch.Tensor:
    """The device-resident table of aqlm_hip_lora_bgmv: ``adapters[a] = (A [rank, in], B [out, rank], scaling)`` -> int64
    [num_adapters * 3] holding the aqlm_hip_lora_entry structs, entry a = adapter id a.  Filled on the host and copied once, like
    ``routed_table``: the table holds raw addresses, so the caller keeps the tensors alive and rebuilds it when one of them moves
    or is written (``aqlm_amd.lora`` keys it on data_ptr + version).  Never while a hipGraph is being captured."""
    entries = (_native.LoraEntry * len(adapters))()
    for ent, (a, b, scaling) in zip(entries, adapters):
        if a.dim() != 2 or b.dim() != 2 or a.shape[0] != b.shape[1] or a.dtype != b.dtype:
            raise ValueError(f"lora table: A must be [rank, in] and B [out, rank] of one dtype, got {tuple(a.shape)} / {tuple(b.shape)}")
        for t in (a, b):
            if not t.is_contiguous() or t.data_ptr() % 16:
                raise ValueError("lora table: A and B must be contiguous and 16-byte aligned")
        ent.a, ent.b, ent.rank, ent.scaling = a.data_ptr(), b.data_ptr(), int(a.shape[0]), float(scaling)
    words = torch.frombuffer(bytearray(bytes(entries)), dtype=torch.int64) if len(adapters) else torch.empty(0, dtype=torch.int64)
    return words.to(device)


def lora_bgmv_supported(out_features: int, in_features: int, max_rank: int, rows: int) -> bool:
    return bool(_lib.aqlm_hip_lora_bgmv_supported(int(out_features), int(in_features), int(max_rank), int(rows)))


def _lora_gmv_(y, x, ids, table, geometry, entry, workspace_bytes, what, y_groups_of_4) -> None:
    """The checks, the workspace and the call of ``lora_bgmv_`` / ``lora_sgmv_``: ``entry`` the native launch,
    ``workspace_bytes(rows, max_rank, in_features)`` its workspace size."""
    n, max_rank, out_features, in_features = (int(v) for v in geometry)
    dt = _dtype_id(y)
    if y.dim() != 2 or x.dim() != 2 or y.shape[0] != x.shape[0] or y.shape[1] != out_features or x.shape[1] != in_features:
        raise ValueError(f"y must be [rows, {out_features}] and x [rows, {in_features}], got {tuple(y.shape)} / {tuple(x.shape)}")
    if x.dtype != y.dtype or x.device != y.device or table.device != y.device:
        raise ValueError("x, y and the table must share dtype and device")
    if y.stride(1) != 1:
        raise ValueError("y must have a unit inner stride (it is written in place)")
    rows = y.shape[0]
    if y_groups_of_4 and (y.data_ptr() % 8 or (rows > 1 and y.stride(0) % 4)):
        raise ValueError("y must be 8-byte aligned with a row stride that is a multiple of 4 elements (it is written in groups of 4)")
    if table.dtype != torch.int64 or table.numel() != n * _native.LORA_ENTRY_WORDS:
        raise ValueError(f"table must be int64 [{n * _native.LORA_ENTRY_WORDS}]")
    if ids is not None:
        if ids.dim() != 1 or ids.shape[0] != rows or ids.dtype not in (torch.int64, torch.int32) or ids.device != y.device:
            raise ValueError(f"ids must be [{rows}] int64 / int32 on {y.device}, got {tuple(ids.shape)} {ids.dtype} on {ids.device}")
        ids = _c(ids)
    if rows == 0:
        return
    x = _flat_rows(x)
    ws = _workspace(y.device, max(workspace_bytes(rows, max_rank, in_features), 16))
    with _device_guard(y.device):
        rc = entry(table.data_ptr(), n, max_rank, _ptr(ids), int(ids is not None and ids.element_size() == 8), rows, x.data_ptr(),
                   x.stride(0) if rows > 1 else in_features, y.data_ptr(), y.stride(0) if rows > 1 else out_features, out_features,
                   in_features, dt, ws.data_ptr(), ws.numel() * 4, _stream_ptr(y.device))
    if rc:
        _native.check(rc, what)


def lora_bgmv_(y, x, ids, table, geometry) -> None:
    """``y[b] += scaling_a * B_a (A_a x[b])`` with a = ids[b], in place, for every row of a decode batch in two launches
    (include/aqlm_hip.h, aqlm_hip_lora_bgmv: fp32 sums, the rank-sized intermediate is never rounded, y is rounded once).
    geometry = [num_adapters, max_rank, out_features, in_features]; ``y`` [rows, out] and ``x`` [rows, in] fp16 / bf16 with unit
    inner strides; ``ids`` [rows] int64 / int32 on the device (read there only; a row whose id lies outside [0, num_adapters) is
    left as it is) or None = adapter 0 for every row; ``table`` from ``lora_table``.  The fp32 workspace comes from the caching
    allocator, so the call can be captured."""
    _lora_gmv_(y, x, ids, table, geometry, _lib.aqlm_hip_lora_bgmv,
               lambda rows, max_rank, in_features: _lib.aqlm_hip_lora_workspace_bytes(rows, max_rank),
               "aqlm lora bgmv", y_groups_of_4=False)


def _fake_lora_bgmv(y, x, ids, table, geometry):  # mutates y, returns nothing
    return None


_LORA_GMV_SCHEMA = "(Tensor(a!) y, Tensor x, Tensor? ids, Tensor table, int[] geometry) -> ()"
register_op("lora_bgmv_", _LORA_GMV_SCHEMA, lora_bgmv_, _fake_lora_bgmv)


def lora_sgmv_supported(out_features: int, in_features: int, max_rank: int, rows: int) -> bool:
    return bool(_lib.aqlm_hip_lora_sgmv_supported(int(out_features), int(in_features), int(max_rank), int(rows)))


def lora_sgmv_(y, x, ids, table, geometry) -> None:
    """``lora_bgmv_`` at any row count (prefill, large batches): the segmented adapter GEMM on the matrix unit
    (include/aqlm_hip.h, aqlm_hip_lora_sgmv), two launches, one pass per distinct adapter of every 16-row tile.  Same arguments
    as ``lora_bgmv_``; in addition ``y`` must be 8-byte aligned with a row stride that is a multiple of 4 elements (it is written
    in groups of 4 outputs).  Not bit-equal to ``lora_bgmv_``: the sums run in another order, and the rank-sized intermediate
    enters the second product as a pair of storage-type values."""
    _lora_gmv_(y, x, ids, table, geometry, _lib.aqlm_hip_lora_sgmv, _lib.aqlm_hip_lora_sgmv_workspace_bytes, "aqlm lora sgmv",
               y_groups_of_4=True)


register_op("lora_sgmv_", _LORA_GMV_SCHEMA, lora_sgmv_, _fake_lora_bgmv)


# ------------------------------------------------------------------------------------------------------
# LoRA adapters on the routed experts of a mixture-of-experts block (aqlm_hip_lora_bgmv_routed; aqlm_amd/lora.py
# LoraQuantizedMixtralExperts is the module-level interface)
# ------------------------------------------------------------------------------------------------------
def lora_routed_table(entries, device) -> torch.Tensor:
    """The device-resident table of aqlm_hip_lora_bgmv_routed: ``entries[a][e][s]`` is ``(A [rank, in], B [out, rank], scaling)`` or
    ``None`` (adapter a has no weights for projection s of expert e: a zero entry, "no adapter") -> int64 [A * E * S * 3] holding
    the aqlm_hip_lora_entry structs, entry [(a * E + e) * S + s].  Same checks, same ownership rules as ``lora_table``: raw
    addresses, the caller keeps the tensors alive and rebuilds the table when one moves or is written.  Never while a hipGraph
    is being captured."""
    flat = [ent for per_adapter in entries for per_expert in per_adapter for ent in per_expert]
    E = len(entries[0]) if entries else 0
    S = len(entries[0][0]) if E else 0
    if any(len(pa) != E or any(len(pe) != S for pe in pa) for pa in entries):
        raise ValueError("lora routed table: entries must be [adapters][experts][segments]")
    structs = (_native.LoraEntry * len(flat))()
    for ent, item in zip(structs, flat):
        if item is None:
            continue  # ctypes zero-fills: rank 0, null pointers
        a, b, scaling = item
        if a.dim() != 2 or b.dim() != 2 or a.shape[0] != b.shape[1] or a.dtype != b.dtype:
            raise ValueError(f"lora table: A must be [rank, in] and B [out, rank] of one dtype, got {tuple(a.shape)} / {tuple(b.shape)}")
        for t in (a, b):
            if not t.is_contiguous() or t.data_ptr() % 16:
                raise ValueError("lora table: A and B must be contiguous and 16-byte aligned")
        ent.a, ent.b, ent.rank, ent.scaling = a.data_ptr(), b.data_ptr(), int(a.shape[0]), float(scaling)
    words = torch.frombuffer(bytearray(bytes(structs)), dtype=torch.int64) if len(flat) else torch.empty(0, dtype=torch.int64)
    return words.to(device)


def lora_bgmv_routed_supported(out_features: int, in_features: int, max_rank: int, num_pairs: int, num_experts: int,
                               num_segments: int) -> bool:
    return bool(_lib.aqlm_hip_lora_bgmv_routed_supported(int(out_features), int(in_features), int(max_rank), int(num_pairs),
                                                         int(num_experts), int(num_segments)))


def _check_lora_routed(y, x, adapter_ids, expert_ids, table, geometry, x_per_pair):
    """The argument checks of ``lora_bgmv_routed_`` / ``lora_sgmv_routed_`` -> (P, rows, dtype id, contiguous adapter ids)."""
    n, E, S, max_rank, out_features, in_features, top_k = (int(v) for v in geometry)
    dt = _dtype_id(y)
    if expert_ids.dim() != 2 or expert_ids.shape[1] != top_k or expert_ids.dtype not in (torch.int64, torch.int32):
        raise ValueError(f"expert_ids must be [T, {top_k}] int64 / int32, got {tuple(expert_ids.shape)} {expert_ids.dtype}")
    T = expert_ids.shape[0]
    P = T * top_k
    rows = P if x_per_pair else T
    if tuple(y.shape) not in ((P, S, out_features),) + (((P, out_features),) if S == 1 else ()) or not y.is_contiguous():
        raise ValueError(f"y must be contiguous [{P}, {S}, {out_features}], got {tuple(y.shape)} with strides {y.stride()}")
    if x.dim() != 2 or tuple(x.shape) != (rows, in_features):
        raise ValueError(f"x must be [{rows}, {in_features}], got {tuple(x.shape)}")
    if x.dtype != y.dtype or x.device != y.device or table.device != y.device or expert_ids.device != y.device:
        raise ValueError("x, y, expert_ids and the table must share a device, x and y a dtype")
    if table.dtype != torch.int64 or table.numel() != n * E * S * _native.LORA_ENTRY_WORDS:
        raise ValueError(f"table must be int64 [{n * E * S * _native.LORA_ENTRY_WORDS}]")
    if adapter_ids is not None:
        if (adapter_ids.dim() != 1 or adapter_ids.shape[0] != T or adapter_ids.dtype not in (torch.int64, torch.int32)
                or adapter_ids.device != y.device):
            raise ValueError(f"adapter_ids must be [{T}] int64 / int32 on {y.device}, got {tuple(adapter_ids.shape)} "
                             f"{adapter_ids.dtype} on {adapter_ids.device}")
        adapter_ids = _c(adapter_ids)
    return P, rows, dt, adapter_ids


def lora_bgmv_routed_(y, x, adapter_ids, expert_ids, table, geometry, x_per_pair) -> None:
    """``y[p, s] += scaling * B (A x_row(p))`` with the adapter of ``table`` entry (adapter_ids[p // top_k], expert_ids[p], s), in
    place, for every (token, expert) pair and projection of a mixture-of-experts launch in two launches (include/aqlm_hip.h,
    aqlm_hip_lora_bgmv_routed; bit-identical per row to ``lora_bgmv_`` with that entry as a one-slot table).
    geometry = [num_adapters, num_experts, num_segments, max_rank, out_features, in_features, top_k]; ``y`` contiguous
    [T * top_k, num_segments, out] (or [T * top_k, out] with one segment), the output of the routed / grouped ops; ``x`` [T, in]
    (token rows, ``x_per_pair`` False) or [T * top_k, in] (pair rows) with a unit inner stride; ``adapter_ids`` [T] int64 / int32 on
    the device or None = adapter 0; ``expert_ids`` [T, top_k] int64 / int32 on the device; both are read on the device only, and a
    pair with either id out of range is left as it is.  ``table`` from ``lora_routed_table``.  At most MAX_LORA_ROWS pairs per
    call.  The fp32 workspace comes from the caching allocator, so the call can be captured."""
    n, E, S, max_rank, out_features, in_features, top_k = (int(v) for v in geometry)
    P, rows, dt, adapter_ids = _check_lora_routed(y, x, adapter_ids, expert_ids, table, geometry, x_per_pair)
    if P == 0:
        return
    x = _flat_rows(x)
    eids = _c(expert_ids)
    ws = _workspace(y.device, max(_lib.aqlm_hip_lora_bgmv_routed_workspace_bytes(P, S, max_rank), 16))
    with _device_guard(y.device):
        rc = _lib.aqlm_hip_lora_bgmv_routed(
            table.data_ptr(), n, E, S, max_rank, _ptr(adapter_ids), int(adapter_ids is not None and adapter_ids.element_size() == 8),
            eids.data_ptr(), int(eids.element_size() == 8), P, top_k, x.data_ptr(), x.stride(0) if rows > 1 else in_features,
            int(bool(x_per_pair)), y.data_ptr(), out_features, in_features, dt, ws.data_ptr(), ws.numel() * 4, _stream_ptr(y.device))
    if rc:
        _native.check(rc, "aqlm lora bgmv routed")


register_op("lora_bgmv_routed_", "(Tensor(a!) y, Tensor x, Tensor? adapter_ids, Tensor expert_ids, Tensor table, int[] geometry, "
            "bool x_per_pair) -> ()", lora_bgmv_routed_, lambda y, x, adapter_ids, expert_ids, table, geometry, x_per_pair: None)


SGMV_ROUTED_TILE_PAIRS = 16  # pairs per tile of the bucket aqlm_hip_lora_sgmv_routed reads: the rows of one matrix instruction


def lora_sgmv_routed_supported(out_features: int, in_features: int, max_rank: int, num_pairs: int, num_experts: int,
                               num_segments: int) -> bool:
    return bool(_lib.aqlm_hip_lora_sgmv_routed_supported(int(out_features), int(in_features), int(max_rank), int(num_pairs),
                                                         int(num_experts), int(num_segments)))


def lora_sgmv_routed_(y, x, adapter_ids, expert_ids, bucket, table, geometry, x_per_pair, workspace=None) -> None:
    """``lora_bgmv_routed_`` at any number of pairs (prefill, large batches): the segmented adapter GEMM on the matrix unit over
    row tiles gathered through the expert bucket (include/aqlm_hip.h, aqlm_hip_lora_sgmv_routed; bit-identical per row to
    ``lora_sgmv_`` with that entry as a one-slot table).  Same arguments as ``lora_bgmv_routed_`` plus ``bucket``:
    ``moe_bucket(expert_ids, num_experts, 16)`` of the same ``expert_ids``.  ``out_features`` must be a multiple of 4 (y rows are
    written in groups of 4 outputs).  At most MAX_LORA_SGMV_ROUTED_PAIRS pairs per call.  ``workspace``: a contiguous fp32 tensor
    of at least ``lora_sgmv_routed_workspace_floats`` elements that the caller owns -- after the call it holds the rank-sized
    intermediate t [P][S][splits][max_rank] of every served pair (the backward reads it) --; default: the cached workspace."""
    n, E, S, max_rank, out_features, in_features, top_k = (int(v) for v in geometry)
    P, rows, dt, adapter_ids = _check_lora_routed(y, x, adapter_ids, expert_ids, table, geometry, x_per_pair)
    if P == 0:
        return
    if (bucket.dtype != torch.int32 or bucket.device != y.device or not bucket.is_contiguous()
            or bucket.numel() != _bucket_words(P, E, SGMV_ROUTED_TILE_PAIRS)):
        raise ValueError(f"bucket must come from moe_bucket(expert_ids, {E}, {SGMV_ROUTED_TILE_PAIRS}) on {y.device}")
    x = _flat_rows(x)
    eids = _c(expert_ids)
    need = max(_lib.aqlm_hip_lora_sgmv_routed_workspace_bytes(P, S, max_rank, in_features), 16)
    if workspace is None:
        ws = _workspace(y.device, need)
    else:
        ws = workspace
        if (ws.dtype != torch.float32 or ws.device != y.device or not ws.is_contiguous() or ws.numel() * 4 < need
                or ws.data_ptr() % 16):
            raise ValueError(f"workspace must be a contiguous, 16-byte aligned float32 tensor of at least {need // 4} elements on "
                             f"{y.device}")
    with _device_guard(y.device):
        rc = _lib.aqlm_hip_lora_sgmv_routed(
            table.data_ptr(), n, E, S, max_rank, _ptr(adapter_ids), int(adapter_ids is not None and adapter_ids.element_size() == 8),
            eids.data_ptr(), int(eids.element_size() == 8), bucket.data_ptr(), P, top_k, x.data_ptr(),
            x.stride(0) if rows > 1 else in_features, int(bool(x_per_pair)), y.data_ptr(), out_features, in_features, dt,
            ws.data_ptr(), ws.numel() * 4, _stream_ptr(y.device))
    if rc:
        _native.check(rc, "aqlm lora sgmv routed")


register_op("lora_sgmv_routed_", "(Tensor(a!) y, Tensor x, Tensor? adapter_ids, Tensor expert_ids, Tensor bucket, Tensor table, "
            "int[] geometry, bool x_per_pair) -> ()", lora_sgmv_routed_,
            lambda y, x, adapter_ids, expert_ids, bucket, table, geometry, x_per_pair: None)


def lora_sgmv_splits(in_features: int) -> int:
    """K slices of the shrink launch of ``lora_sgmv_`` / ``lora_sgmv_routed_``: a function of in_features alone."""
    return _lib.aqlm_hip_lora_sgmv_routed_workspace_bytes(1, 1, 8, int(in_features)) // 32


def lora_sgmv_routed_workspace_floats(num_pairs: int, num_segments: int, max_rank: int, in_features: int) -> int:
    """fp32 elements of the workspace of one ``lora_sgmv_routed_`` call: [P][S][splits][max_rank]; 0 when unsupported."""
    return _lib.aqlm_hip_lora_sgmv_routed_workspace_bytes(int(num_pairs), int(num_segments), int(max_rank), int(in_features)) // 4


# ------------------------------------------------------------------------------------------------------
# the backward of the adapters on the routed experts (aqlm_hip_lora_transpose_routed, aqlm_hip_lora_grad_routed; aqlm_amd/lora.py
# is the module-level interface)
# ------------------------------------------------------------------------------------------------------
def lora_routed_transposed_layout(ranks, scalings, out_features: int, in_features: int, base: int, element_size: int = 2):
    """The transposed table of the grad_x launch and the layout of the buffer behind it, a pure function (no device):
    ``ranks[a][e][s]`` the rank of entry (a, e, s) or 0 / None for none, ``scalings[a][e][s]`` its factor, ``base`` the address of
    the buffer.  -> (the aqlm_hip_lora_entry structs laid out [s][a][e], offsets, elements): entry (s, a, e) is
    ``{a: B^T [rank, out], b: A^T [in, rank], rank, scaling}``, its two copies back to back in the buffer in table order --
    ``offsets[(a, e, s)] = (element offset of B^T, element offset of A^T)`` -- and an entry without weights or with a rank that is
    no multiple of 8 is a zero entry that owns no part of the buffer."""
    n = len(ranks)
    E = len(ranks[0]) if n else 0
    S = len(ranks[0][0]) if E else 0
    structs = (_native.LoraEntry * (n * E * S))()
    offsets, at = {}, 0
    for s in range(S):
        for a in range(n):
            for e in range(E):
                r = int(ranks[a][e][s] or 0)
                if r <= 0 or r % 8:
                    continue
                ent = structs[(s * n + a) * E + e]
                offsets[(a, e, s)] = (at, at + r * out_features)
                ent.a, ent.b = base + at * element_size, base + (at + r * out_features) * element_size
                ent.rank, ent.scaling = r, float(scalings[a][e][s])
                at += r * (out_features + in_features)
    return structs, offsets, at


def lora_routed_transposed_table(entries, device):
    """``entries[a][e][s]`` as for ``lora_routed_table`` -> (buffer, table, offsets): the storage-type buffer of the transposed
    copies (filled by ``lora_transpose_routed_``, not here), the device table [S][A][E] of ``lora_routed_transposed_layout``
    whose segment s is the one-segment table ``table[s * A * E * 3:(s + 1) * A * E * 3]``, and the element offsets of the copies.
    Never while a hipGraph is being captured."""
    live = [ent for pa in entries for pe in pa for ent in pe if ent is not None]
    if not live:
        raise ValueError("lora routed transposed table: no entry has weights")
    a0, b0, _ = live[0]
    out_features, in_features = int(b0.shape[0]), int(a0.shape[1])
    for a, b, _ in live:
        if a.dim() != 2 or b.dim() != 2 or a.shape[0] != b.shape[1] or a.dtype != a0.dtype or b.dtype != a0.dtype \
                or a.shape[1] != in_features or b.shape[0] != out_features:
            raise ValueError(f"lora table: A must be [rank, {in_features}] and B [{out_features}, rank] of one dtype, got "
                             f"{tuple(a.shape)} / {tuple(b.shape)}")
    if out_features % 8 or in_features % 8:
        raise NotImplementedError("lora routed transposed table: in_features and out_features must be multiples of 8")
    ranks = [[[0 if ent is None else int(ent[0].shape[0]) for ent in pe] for pe in pa] for pa in entries]
    scalings = [[[0.0 if ent is None else float(ent[2]) for ent in pe] for pe in pa] for pa in entries]
    _, _, elements = lora_routed_transposed_layout(ranks, scalings, out_features, in_features, 0)
    buffer = torch.zeros((max(elements, 8),), dtype=a0.dtype, device=device)
    structs, offsets, _ = lora_routed_transposed_layout(ranks, scalings, out_features, in_features, buffer.data_ptr(),
                                                        buffer.element_size())
    words = torch.frombuffer(bytearray(bytes(structs)), dtype=torch.int64)
    return buffer, words.to(device), offsets


def lora_transpose_routed_supported(out_features: int, in_features: int, max_rank: int, num_experts: int, num_segments: int) -> bool:
    return bool(_lib.aqlm_hip_lora_transpose_routed_supported(int(out_features), int(in_features), int(max_rank), int(num_experts),
                                                              int(num_segments)))


def lora_transpose_routed_(buffer, table, transposed, geometry) -> None:
    """Fill ``buffer`` with B^T and A^T of every live entry of the forward ``table`` (``lora_routed_table``) at the places the
    ``transposed`` table (``lora_routed_transposed_table``) names, in ONE launch (include/aqlm_hip.h,
    aqlm_hip_lora_transpose_routed).  geometry = [num_adapters, num_experts, num_segments, max_rank, out_features, in_features].
    An entry that is not live, whose transposed entry has another rank, or whose copies would not lie inside ``buffer`` leaves
    the buffer as it is."""
    n, E, S, max_rank, out_features, in_features = (int(v) for v in geometry)
    words = n * E * S * _native.LORA_ENTRY_WORDS
    for t in (table, transposed):
        if t.dtype != torch.int64 or t.numel() != words or t.device != buffer.device or not t.is_contiguous():
            raise ValueError(f"table and transposed must be contiguous int64 [{words}] on {buffer.device}")
    if buffer.dtype not in _DT or not buffer.is_contiguous() or buffer.dim() != 1:
        raise ValueError("buffer must be a contiguous 1-D float16 / bfloat16 tensor")
    with _device_guard(buffer.device):
        rc = _lib.aqlm_hip_lora_transpose_routed(table.data_ptr(), transposed.data_ptr(), n, E, S, max_rank, out_features, in_features,
                                                 buffer.data_ptr(), buffer.numel() * buffer.element_size(), _stream_ptr(buffer.device))
    if rc:
        _native.check(rc, "aqlm lora transpose routed")


register_op("lora_transpose_routed_", "(Tensor(a!) buffer, Tensor table, Tensor transposed, int[] geometry) -> ()",
            lora_transpose_routed_, lambda buffer, table, transposed, geometry: None)


def lora_grad_routed_supported(dim: int, max_rank: int, num_pairs: int, num_experts: int, num_segments: int) -> bool:
    return bool(_lib.aqlm_hip_lora_grad_routed_supported(int(dim), int(max_rank), int(num_pairs), int(num_experts), int(num_segments)))


def lora_grad_routed(v, w, adapter_ids, expert_ids, bucket, table, geometry, layout, out=None):
    """The reduction over pairs that both weight gradients of the routed adapters are (include/aqlm_hip.h,
    aqlm_hip_lora_grad_routed), for ONE adapter: -> fp32 ``G [E, S, max_rank, dim]``,
    ``G[e, s, r, i] = scaling * sum over the pairs p of expert e with adapter `adapter`, ascending, of w[p, s][r] * V[p, s][i]``.
    geometry = [num_adapters, num_experts, num_segments, max_rank, dim, top_k, adapter]; ``v`` the fp16 / bf16 tensor that holds
    the V rows and ``w`` the fp32 tensor that holds the rank-sized rows, both addressed through
    layout = [v_row_stride, v_seg_stride, v_per_pair, w_pair_stride, w_seg_stride, w_splits, w_split_stride] (elements; every
    address it can form is checked against the two tensors here).  ``adapter_ids`` [T] or None = adapter 0 for every pair,
    ``expert_ids`` [T, top_k], ``bucket`` = ``moe_bucket(expert_ids, num_experts, 16)``, ``table`` from ``lora_routed_table``.
    Entries that are not live keep what ``out`` held (a new ``G`` is zero there)."""
    n, E, S, max_rank, dim, top_k, adapter = (int(x) for x in geometry)
    vrs, vss, vpp, wps, wss, wsplits, wsp = (int(x) for x in layout)
    dt = _dtype_id(v)
    if expert_ids.dim() != 2 or expert_ids.shape[1] != top_k or expert_ids.dtype not in (torch.int64, torch.int32):
        raise ValueError(f"expert_ids must be [T, {top_k}] int64 / int32, got {tuple(expert_ids.shape)} {expert_ids.dtype}")
    T = expert_ids.shape[0]
    P = T * top_k
    if P == 0:
        raise ValueError("lora_grad_routed: no pairs")
    if w.dtype != torch.float32 or v.stride(-1) != 1:
        raise ValueError("w must be float32 and v must have a unit inner stride")
    if any(t.device != v.device for t in (w, expert_ids, bucket, table)):
        raise ValueError("v, w, expert_ids, bucket and table must share a device")
    if table.dtype != torch.int64 or table.numel() != n * E * S * _native.LORA_ENTRY_WORDS:
        raise ValueError(f"table must be int64 [{n * E * S * _native.LORA_ENTRY_WORDS}]")
    if (bucket.dtype != torch.int32 or not bucket.is_contiguous() or bucket.numel() != _bucket_words(P, E, SGMV_ROUTED_TILE_PAIRS)):
        raise ValueError(f"bucket must come from moe_bucket(expert_ids, {E}, {SGMV_ROUTED_TILE_PAIRS})")
    if adapter_ids is not None:
        if (adapter_ids.dim() != 1 or adapter_ids.shape[0] != T or adapter_ids.dtype not in (torch.int64, torch.int32)
                or adapter_ids.device != v.device):
            raise ValueError(f"adapter_ids must be [{T}] int64 / int32 on {v.device}")
        adapter_ids = _c(adapter_ids)
    if min(vrs, wps, wsplits) < 1 or min(vss, wss, wsp) < 0 or S < 1 or max_rank < 1 or dim < 1:
        raise ValueError("lora_grad_routed: strides and sizes must be positive")
    # the furthest element either operand can be asked for, against what the tensors hold (from their data_ptr on)
    v_rows = P if vpp else T
    v_span = v.untyped_storage().nbytes() // v.element_size() - v.storage_offset()
    w_span = w.untyped_storage().nbytes() // 4 - w.storage_offset()
    if (v_rows - 1) * vrs + (S - 1) * vss + dim > v_span:
        raise ValueError(f"v holds {v_span} elements, the layout reaches {(v_rows - 1) * vrs + (S - 1) * vss + dim}")
    if (P - 1) * wps + (S - 1) * wss + (wsplits - 1) * wsp + max_rank > w_span:
        raise ValueError(f"w holds {w_span} elements, the layout reaches {(P - 1) * wps + (S - 1) * wss + (wsplits - 1) * wsp + max_rank}")
    if out is None:
        out = torch.zeros((E, S, max_rank, dim), dtype=torch.float32, device=v.device)
    elif out.dtype != torch.float32 or tuple(out.shape) != (E, S, max_rank, dim) or not out.is_contiguous() or out.device != v.device:
        raise ValueError(f"out must be contiguous float32 [{E}, {S}, {max_rank}, {dim}] on {v.device}")
    eids = _c(expert_ids)
    with _device_guard(v.device):
        rc = _lib.aqlm_hip_lora_grad_routed(
            table.data_ptr(), n, E, S, max_rank, adapter, _ptr(adapter_ids),
            int(adapter_ids is not None and adapter_ids.element_size() == 8), eids.data_ptr(), int(eids.element_size() == 8),
            bucket.data_ptr(), P, top_k, v.data_ptr(), vrs, vss, int(bool(vpp)), dim, w.data_ptr(), wps, wss, wsplits, wsp,
            out.data_ptr(), out.numel() * 4, dt, _stream_ptr(v.device))
    if rc:
        _native.check(rc, "aqlm lora grad routed")
    return out


register_op("lora_grad_routed", "(Tensor v, Tensor w, Tensor? adapter_ids, Tensor expert_ids, Tensor bucket, Tensor table, "
            "int[] geometry, int[] layout) -> Tensor", lora_grad_routed,
            lambda v, w, adapter_ids, expert_ids, bucket, table, geometry, layout: v.new_empty(
                (int(geometry[1]), int(geometry[2]), int(geometry[3]), int(geometry[4])), dtype=torch.float32))
