"""torch.ops.aqlm.* backed by libaqlm_hip.so (MI355X / gfx950).

Host-side mirror of the reference's op registration + host glue
(inference_lib/src/aqlm/inference_kernels/cuda_kernel.py:13-132 and cuda_kernel.cpp:148-182, 249-354 and the
2x8 / 1x8 copies): same op names, same schemas, same output shapes, same error conventions -- but each op is a
thin shim: flatten, allocate the output, call the C ABI (include/aqlm_hip.h) on torch's current stream.

Differences from the reference, all deliberate:
  * one launch for up to 8 rows instead of a per-row loop; scale+bias fused (no epilogue launches, no clone);
  * the ``*_matmat_dequant`` ops run a fused dequant-tile -> MFMA kernel for 1x16 (W never reaches HBM); other
    schemes dequantise with our kernel and call F.linear (hipBLASLt) like the reference;
  * ``*_dequant_transposed`` applies the scales for every scheme and honours in_group_size (the reference drops
    the scales for 2x8/1x8 and hard-codes g=8 for 1x16).

Layout.  This module is the forward path -- the gemv ops, the packed / planar / look-up-table formats with their cell
registries, the raw-op prepack cache and compiled front end, dequantisation and the large-batch ops -- and the one namespace
callers and tests use.  The launch helpers live in ``_launch``; the mixture-of-experts, LoRA, gradient and search / k-means ops
live in ``ops_moe``, ``ops_lora``, ``ops_grad`` and ``ops_search``, each registering its own ``aqlm::`` ops, and are re-exported
at the end of this file, name by name and as the same objects.  The forward path stays here on purpose: its knobs
(``RAW_OP_PREPACK*``, ``RAW_OP_CHECK_EVERY``, ``FUSED_MFMA_MAX_ROWS``, ``FUSED_8X8_MFMA_MAX_ROWS``, ``USE_FUSED_8X8_MFMA``) and
``tensor_checksum`` / ``unpack_1x16`` are rebound as attributes of this module by tests and benchmarks and read here as module
globals, so moving that code would silently disconnect a knob or a test's patch.  The family modules never import this module at
module scope; it imports them after its own definitions.
"""
from __future__ import annotations

import contextlib  # noqa: F401  (not used here since the split; still a name of this namespace, like NamedTuple below)
import ctypes
import os
from types import SimpleNamespace
from typing import NamedTuple, Optional  # noqa: F401

import torch
import torch.nn.functional as F

from .. import _native
from .._native import lib as _lib
from ..derived import tensor_checksum, tensor_version
from ._launch import (  # noqa: F401  (by name: the decode path keeps plain global look-ups)
    _DT,
    _GRAD_DT,
    _GRAD_TORCH_DT,
    _LIB,
    _NO_GUARD,
    _WORKSPACES,
    _c,
    _device_guard,
    _dtype_id,
    _flat_rows,
    _ptr,
    _stream_ptr,
    _workspace,
    register_op,
)

_version = tensor_version  # the name the tests reach

HIP_FOLDER = os.path.dirname(os.path.abspath(_native.LIB_PATH))
CUDA_FOLDER = HIP_FOLDER  # reference name (cuda_kernel.py:6); ROCm reports device type "cuda"


# ------------------------------------------------------------------------------------------------------
# gemv ops (decode; the hot path)
# ------------------------------------------------------------------------------------------------------
def _gemv(input, codes, codebooks, scales, bias, kind):
    dt = _dtype_id(input)
    num_codebooks, codebook_size, out_group_size, in_group_size = codebooks.shape
    if out_group_size != 1:
        raise NotImplementedError("AQLM HIP kernels require out_group_size == 1")
    if codebooks.dtype != input.dtype or scales.dtype != input.dtype:
        raise NotImplementedError(f"input dtype {input.dtype} must match codebooks/scales dtype {codebooks.dtype}")
    out_features = codes.shape[0]
    in_features = codes.shape[1] * in_group_size
    if input.shape[-1] != in_features:
        raise ValueError(f"input has {input.shape[-1]} features, layer expects {in_features}")
    x = _flat_rows(input)
    codes, codebooks, scales = _c(codes), _c(codebooks), _c(scales)
    if bias is not None:
        bias = _c(bias)
    B = x.shape[0]
    if kind == "kx8" and B > _native.MAX_GEMV_BATCH:
        # more rows than one matvec launch takes: ONE launch of the fused MFMA op (W never materialised) instead of slabs of 8 that
        # each re-read all the codes -- inside aqlm_hip_gemv_kx8 every slab of >= 3 rows would take that kernel half empty anyway
        y = _fused_kx8_mfma(input, codes, codebooks, scales, bias, dt)
        if y is not None:
            return y
    y = torch.empty((B, out_features), dtype=input.dtype, device=input.device)
    stream = _stream_ptr(input.device)
    with _device_guard(input.device):
        for b0 in range(0, B, _native.MAX_GEMV_BATCH):
            nb = min(_native.MAX_GEMV_BATCH, B - b0)
            xp = x.data_ptr() + b0 * x.stride(0) * 2
            yp = y.data_ptr() + b0 * out_features * 2
            if kind == "1x16":
                rc = _lib.aqlm_hip_gemv_1x16(codes.data_ptr(), codebooks.data_ptr(), scales.data_ptr(), _ptr(bias),
                                             xp, yp, out_features, in_features, in_group_size, nb,
                                             x.stride(0), out_features, dt, stream)
            elif kind == "kx8":
                rc = _lib.aqlm_hip_gemv_kx8(codes.data_ptr(), codebooks.data_ptr(), scales.data_ptr(), _ptr(bias),
                                            xp, yp, out_features, in_features, num_codebooks, in_group_size, nb,
                                            x.stride(0), out_features, dt, stream)
            else:
                nbits = int(codebook_size).bit_length() - 1
                rc = _lib.aqlm_hip_gemv_generic(codes.data_ptr(), codebooks.data_ptr(), scales.data_ptr(), _ptr(bias),
                                                xp, yp, out_features, in_features, num_codebooks, nbits,
                                                in_group_size, nb, x.stride(0), out_features, dt, stream)
            if rc:
                _native.check(rc, "aqlm gemv")
    return y.reshape(input.shape[:-1] + (out_features,))


# ------------------------------------------------------------------------------------------------------
# prepacked 1x16 path, g8 and g16 (format v6): 1..8 input rows per launch on slice-bucketed codes
# ------------------------------------------------------------------------------------------------------
class _DerivedCodes:
    """What both packed formats of the codes share: the device buffer and the codebook range -- max |codebook entry|, the bound
    the single-kernel finalize scales its fixed-point cells by (include/aqlm_hip.h) -- with the fingerprint (data pointer,
    version) of the codebook tensor it was taken from and the checksum of that tensor's bytes at that moment (writes through
    ``.data``: ``verify_range``).  Each format says where the bound is stored (``_store_range``)."""

    __slots__ = ("buf", "out_features", "in_features", "in_group_size", "_range_of", "_range_checksum")

    def set_codebook_range(self, codebooks: torch.Tensor) -> None:
        """Take the range of ``codebooks``.  One small reduction + a host read-back: load-time work, never issued while a hipGraph
        is being captured."""
        absmax = float(codebooks.detach().abs().max().float().item())
        self._store_range(absmax if absmax == absmax and absmax != float("inf") else 0.0, codebooks)
        self._range_of = (codebooks.data_ptr(), tensor_version(codebooks))
        self._range_checksum = tensor_checksum(codebooks)

    def range_is_current(self, codebooks: torch.Tensor) -> bool:
        return self._range_of == (codebooks.data_ptr(), tensor_version(codebooks))

    def verify_range(self, codebooks: torch.Tensor) -> bool:
        """Was the codebook written behind the version counter's back (``codebooks.data.copy_()``)?  Compares the checksum taken
        with the range; on a mismatch the range is forgotten and taken again at the next eager call.  Synchronises: not for use
        while a hipGraph is being captured."""
        if self._range_of is None or not self.range_is_current(codebooks) or self._range_checksum is None:
            return True
        if tensor_checksum(codebooks) == self._range_checksum:
            return True
        self.forget_range()
        return False

    def forget_range(self) -> None:
        """No range: the bound is 0 (the two-kernel form) until ``refresh_range`` takes it again."""
        self._store_range(0.0, None)
        self._range_of = self._range_checksum = None

    def numel(self) -> int:  # bytes held
        return self.buf.numel()

    @property
    def device(self):
        return self.buf.device

    def data_ptr(self) -> int:
        return self.buf.data_ptr()


def refresh_range(packed: _DerivedCodes, codebooks: torch.Tensor) -> None:
    """Keep a packed buffer's codebook range in step with the codebook tensor the op is called with (first use, or the codebook
    was retrained / rebound).  While a hipGraph is being captured or a graph traced nothing can be read back: a range that is not
    current is not trusted, and the two-kernel form serves that call."""
    if packed.range_is_current(codebooks):
        return
    if torch.cuda.is_current_stream_capturing() or torch.compiler.is_compiling():
        packed.forget_range()
        return
    packed.set_codebook_range(codebooks)


class PackedCodes(_DerivedCodes):
    """A prepacked 1x16 code buffer (``aqlm_hip_prepack_1x16``; g8: 16 codebook slices, g16: 32): device bytes + the
    host-side descriptor the kernels are launched with.  Derived from ``codes`` (lossless: ``unpack_1x16`` gives them
    back); never saved."""

    __slots__ = ("desc", "slices", "_ints")

    def __init__(self, buf: torch.Tensor, desc: "_native.PackedDesc"):
        self.buf, self.desc = buf, desc
        self.out_features, self.in_features = int(desc.out_features), int(desc.in_features)
        self.slices = 1 << int(desc.slices_log2)
        self.in_group_size = 16 if self.slices == 32 else 8  # the two instantiations of csrc/gemv_packed.hip
        self._ints = desc.as_ints()
        self._range_of = self._range_checksum = None

    def _store_range(self, absmax: float, codebooks: Optional[torch.Tensor]) -> None:
        """The bound goes into the descriptor.  A relabelled buffer (format v7) also gets its permuted codebook image here
        (aqlm_hip_packed_set_codebook): the kernels read the image, so it is rewritten whenever the codebook tensor changes --
        same fingerprint, same moment.  Without a codebook the image is not trusted either: the entry then refuses the call with
        a message that says what to do (one eager forward after the codebook changed rewrites it)."""
        self.desc.codebook_absmax = absmax
        if codebooks is None:
            self.desc.flags &= ~_native.PACKED_HAS_CODEBOOK
        elif self.desc.relabelled:
            cb = _c(codebooks.detach())
            with torch.cuda.device(self.buf.device):
                rc = _lib.aqlm_hip_packed_set_codebook(ctypes.byref(self.desc), self.buf.data_ptr(), cb.data_ptr(),
                                                       _stream_ptr(self.buf.device))
            if rc:
                _native.check(rc, "aqlm packed_set_codebook")
        self._ints = self.desc.as_ints()

    def op_ints(self):
        """What the dispatcher op `aqlm::code1x16_matmat_packed` takes: the descriptor + the fingerprint (data pointer, version) of the
        codebook tensor its range -- and, for a relabelled buffer, its codebook IMAGE -- was taken from.  A traced graph bakes these
        ints in; the op compares the fingerprint with the codebook it is called with and refreshes on a mismatch (a codebook updated
        in place between two calls of a compiled model must not be served from the stale image: ADVICE r05)."""
        fp = self._range_of if self._range_of is not None else (0, -1)
        return list(self._ints) + [int(fp[0]), int(fp[1])]

    def padding_fraction(self) -> float:
        """Share of the entry slots that hold no code: every (row, slice) bucket is rounded up to lane-steps of 4 entries and every
        stream to whole wave-steps.  Short rows pay most (a 1024-wide shard of a row-split layer has 8 codes per row and slice =
        2 lane-steps, mostly padding: VERDICT r05 weak #2)."""
        d = self.desc
        streams = sum(int(v) for v in list(d.slice_groups)[:self.slices])
        slots = streams * int(d.waves) * int(d.steps) * 64 * 4
        codes = self.out_features * (self.in_features // self.in_group_size)
        return 1.0 - codes / slots if slots else 0.0

    def unpack(self) -> torch.Tensor:
        return unpack_1x16(self)

    @classmethod
    def from_buffer(cls, buf: torch.Tensor) -> "PackedCodes":
        """Re-attach a descriptor to a packed buffer (e.g. one that was saved / moved): it is stored in its first bytes."""
        head = bytes(buf[:128].cpu().numpy().tobytes())
        desc = _native.PackedDesc()
        raw = (ctypes.c_char * len(head)).from_buffer_copy(head)
        _native.check(_lib.aqlm_hip_packed_desc_read(ctypes.addressof(raw), len(head), ctypes.byref(desc)), "packed_desc_read")
        return cls(buf, desc)


_UNPACKABLE_WARNED = set()


def prepack_1x16(codes: torch.Tensor, in_group_size: int = 8, codebooks: Optional[torch.Tensor] = None, *,
                 relabel: bool = True, uniform_only: bool = False) -> Optional[PackedCodes]:
    """Repack 1x16 codes [out, in/g, 1] (int16; g = 8 or 16) into the slice-bucketed buffer of aqlm_hip_gemv_1x16_packed.
    Returns None when the packed path does not cover the layer.  One-off, at load / first use (the counterpart of the
    reference's load-time code permutation for its CPU kernel, inference.py:78-83).  With ``codebooks`` the descriptor
    also gets the layer's codebook range (``PackedCodes.set_codebook_range``): single-kernel matvecs.

    The repack balances the codebook slices whatever the code histogram is (format v7: relabelling, and for entries that
    outweigh a whole slice a variable row-group geometry; include/aqlm_hip.h).  ``relabel=False`` keeps the checkpoint's
    labels, ``uniform_only=True`` keeps the 16 x 16 geometry (what the publish form of row-parallel shards needs)."""
    out_features, in_features = codes.shape[0], codes.shape[1] * in_group_size
    cap = _lib.aqlm_hip_prepack_1x16_bytes(out_features, in_features, in_group_size)
    if cap == 0:
        return None
    codes = _c(codes)
    scratch = torch.empty((cap,), dtype=torch.uint8, device=codes.device)
    desc = _native.PackedDesc()
    flags = (0 if relabel else _native.PREPACK_NO_RELABEL) | (_native.PREPACK_UNIFORM_ONLY if uniform_only else 0)
    with torch.cuda.device(codes.device):
        rc = _lib.aqlm_hip_prepack_1x16_ex(codes.data_ptr(), out_features, in_features, in_group_size, scratch.data_ptr(),
                                           cap, ctypes.byref(desc), flags, _stream_ptr(codes.device))
    if rc == _native.E_UNSUPPORTED:
        # even the balanced streams do not fit (rows that differ wildly from one another): the direct kernel serves this layer,
        # 2-3x slower -- say so once per shape instead of degrading silently
        key = (out_features, in_features, in_group_size)
        if key not in _UNPACKABLE_WARNED:
            _UNPACKABLE_WARNED.add(key)
            import warnings

            warnings.warn(f"aqlm_amd: 1x16 g{in_group_size} layer {in_features} -> {out_features} cannot take the prepacked matvec "
                          f"({_native.last_error()}); it runs on the direct kernel (about 2-3x slower at batch 1)", RuntimeWarning, stacklevel=2)
        return None
    if rc:
        _native.check(rc, "aqlm prepack_1x16")
    packed = PackedCodes(scratch[: int(desc.used_bytes)].clone(), desc)  # keep only the bytes in use
    if codebooks is not None:
        packed.set_codebook_range(codebooks)
    return packed


def unpack_1x16(packed: PackedCodes) -> torch.Tensor:
    """The canonical codes [out, in/g, 1] (int16) of a prepacked buffer (aqlm_hip_unpack_1x16; lossless)."""
    codes = torch.empty((packed.out_features, packed.in_features // packed.in_group_size, 1), dtype=torch.int16, device=packed.device)
    with torch.cuda.device(packed.device):
        rc = _lib.aqlm_hip_unpack_1x16(ctypes.byref(packed.desc), packed.data_ptr(), codes.data_ptr(),
                                       _stream_ptr(packed.device))
    if rc:
        _native.check(rc, "aqlm unpack_1x16")
    return codes


def dequant_1x16_packed(packed: PackedCodes, codebooks: torch.Tensor, scales: Optional[torch.Tensor] = None) -> torch.Tensor:
    """W [out, in] in the codebook dtype straight from a prepacked buffer (aqlm_hip_dequant_1x16_packed): the bits of
    ``code1x16_dequant(unpack_1x16(packed), codebooks, scales)`` without the int16 codes in between.  Reads the entries, the
    permutation inside the buffer and ``codebooks`` as passed -- never the buffer's codebook image or range, so it needs no
    ``refresh_range`` and is stream-ordered (no allocation beyond W, no synchronisation: it can be captured in a hipGraph)."""
    dt = _dtype_id(codebooks)
    if tuple(codebooks.shape) != (1, 65536, 1, packed.in_group_size):
        raise NotImplementedError(f"dequant_1x16_packed needs codebooks [1, 65536, 1, {packed.in_group_size}], got {tuple(codebooks.shape)}")
    if codebooks.device != packed.device:
        raise ValueError(f"codebooks on {codebooks.device}, packed codes on {packed.device}")
    if scales is not None:
        if scales.dtype != codebooks.dtype or scales.numel() != packed.out_features:
            raise ValueError(f"scales must hold {packed.out_features} values of {codebooks.dtype}")
        scales = _c(scales)
    codebooks = _c(codebooks)
    W = torch.empty((packed.out_features, packed.in_features), dtype=codebooks.dtype, device=codebooks.device)
    with _device_guard(codebooks.device):
        rc = _lib.aqlm_hip_dequant_1x16_packed(ctypes.byref(packed.desc), packed.data_ptr(), codebooks.data_ptr(), _ptr(scales),
                                               W.data_ptr(), dt, _stream_ptr(codebooks.device))
    if rc:
        _native.check(rc, "aqlm dequant_1x16_packed")
    return W


# Accumulator cells of the single-kernel finalize, one zero-at-rest set per (device, stream): the prepacked buffers are then
# only read, so one layer may run on several streams at once (weight sharing, overlapped graphs) -- the reference's
# launcher is stateless in the same way (cuda_kernel.cu:505-509).  Launches on one stream are ordered, so all layers of a
# stream share the set.  Sized once and never freed or resized (a hipGraph may have captured the pointer); calls that
# need more, and captures on a stream that has no set yet, use the cells inside the layer's packed buffer (one stream at
# a time per layer, include/aqlm_hip.h).
PACKED_CELLS_BYTES = _native.MAX_GEMV_BATCH * 131072 * 8
_PACKED_CELLS = {}


def _shared_cells(device: torch.device, stream: int, nbytes: int):
    """The per-(device, stream) set kept by the compiled front end, when it is loaded: ONE registry for the module lanes, the
    compiled ops and the Python ops (False: no extension, the dictionaries below are the registry)."""
    from .. import _front

    if not _front.available() or not hasattr(_front.ext, "stream_cells"):
        return False
    like = _CELLS_LIKE.get(device.index)
    if like is None:
        like = _CELLS_LIKE[device.index] = torch.empty((0,), dtype=torch.float16, device=device)
    return _front.ext.stream_cells(like, stream, nbytes)


_CELLS_LIKE = {}


def accumulator_cells(device: Optional[torch.device] = None, stream: Optional[int] = None):
    """Every accumulator-cell tensor that exists for (device, stream) -- defaults: the current ones -- whichever registry holds
    it.  Diagnostics and tests: all of them must read zero whenever the stream is idle."""
    device = torch.device("cuda", torch.cuda.current_device()) if device is None else device
    stream = torch.cuda.current_stream(device).cuda_stream if stream is None else stream
    found = []
    shared = _shared_cells(device, stream, 8)
    if shared is not False and shared is not None:
        found.append(shared)
    for reg in (_PACKED_CELLS, _LUT_CELLS):
        if (device.index, stream) in reg:
            found.append(reg[(device.index, stream)])
    return found


def release_accumulator_cells(device: Optional[torch.device] = None, stream: Optional[int] = None) -> int:
    """Free the accumulator-cell sets (8 MiB each) of ``(device, stream)`` -- ``None`` = every device / every stream -- in all
    registries.  The library cannot know whether a hipGraph that captured a launch on the stream is still alive (it holds the
    cells' address), so this is the caller's decision: call it when the streams / graphs of a finished phase are gone (a serving
    process that retires a capture pool, a test suite).  A later call on a released stream allocates a fresh zero-filled set.
    Returns the number of sets freed."""
    from .. import _front

    n = 0
    dev_index = None if device is None else torch.device(device).index
    for reg in (_PACKED_CELLS, _LUT_CELLS):
        for key in [k for k in reg if (dev_index is None or k[0] == dev_index) and (stream is None or k[1] == stream)]:
            del reg[key]
            n += 1
    if device is None and stream is None:
        _LUT_CELLS_RETIRED.clear()
    if _front.available() and hasattr(_front.ext, "release_stream_cells"):
        n += int(_front.ext.release_stream_cells(-1 if dev_index is None else dev_index, 0 if stream is None else stream, stream is None))
    return n


def _packed_cells(device: torch.device, stream: int, nbytes: int):
    if nbytes > PACKED_CELLS_BYTES:
        return None
    shared = _shared_cells(device, stream, nbytes)
    if shared is not False:
        return shared
    key = (device.index, stream)
    cells = _PACKED_CELLS.get(key)
    if cells is None:
        if torch.cuda.is_current_stream_capturing():
            return None
        with torch.cuda.device(device):
            cells = torch.zeros((PACKED_CELLS_BYTES // 8,), dtype=torch.int64, device=device)
        _PACKED_CELLS[key] = cells
    return cells


FUSED_FINALIZE = True  # mirror of the library knob `packed_fused_finalize` (set both through set_fused_finalize)


def set_fused_finalize(on: bool) -> None:
    """A/B switch: finalize inside the prepacked kernel (default) or in a second kernel through an fp32 workspace."""
    global FUSED_FINALIZE
    _native.set_tuning("packed_fused_finalize", 1 if on else 0)
    FUSED_FINALIZE = bool(on)
    _raw_sync_config()  # the compiled raw ops launch the single-kernel form only: off with the switch


def _check_packed_args(input, packed, codebooks, scales):
    dt = _dtype_id(input)
    if codebooks.dtype != input.dtype or scales.dtype != input.dtype:
        raise NotImplementedError(f"input dtype {input.dtype} must match codebooks/scales dtype {codebooks.dtype}")
    if input.shape[-1] != packed.in_features:
        raise ValueError(f"input has {input.shape[-1]} features, layer expects {packed.in_features}")
    if input.device != packed.device or codebooks.device != input.device:
        raise ValueError(f"input on {input.device}, layer on {packed.device}")
    return dt


def code1x16_matmat_packed(input, packed: PackedCodes, codebooks, scales, bias=None):
    """1x16 g8 matvec on prepacked codes (aqlm_hip_gemv_1x16_packed): up to 8 input rows per launch share the codes and
    the gathered codebook vectors (the reference relaunches its matvec per row, cuda_kernel.cpp:165-175)."""
    dt = _check_packed_args(input, packed, codebooks, scales)
    out_features = packed.out_features
    x = _flat_rows(input)
    codebooks, scales = _c(codebooks), _c(scales)
    if bias is not None:
        bias = _c(bias)
    B = x.shape[0]
    y = torch.empty((B, out_features), dtype=input.dtype, device=input.device)
    nb_max = min(B, _native.MAX_GEMV_BATCH)
    stream = _stream_ptr(input.device)
    refresh_range(packed, codebooks)
    cells = None
    if FUSED_FINALIZE and packed.desc.codebook_absmax > 0.0:   # single kernel: fixed-point cells, per stream where possible
        ws_ptr, ws_len = None, 0
        cells = _packed_cells(input.device, stream, nb_max * out_features * 8)
    else:                                   # two kernels: fp32 slice partials in a workspace
        ws = _workspace(input.device, packed.slices * nb_max * out_features * 4, stream)
        ws_ptr, ws_len = ws.data_ptr(), ws.numel() * 4
    with _device_guard(input.device):
        for b0 in range(0, B, _native.MAX_GEMV_BATCH):
            nb = min(_native.MAX_GEMV_BATCH, B - b0)
            if cells is not None:
                rc = _lib.aqlm_hip_gemv_1x16_packed_cells(ctypes.byref(packed.desc), packed.data_ptr(), codebooks.data_ptr(),
                                                          scales.data_ptr(), _ptr(bias), x.data_ptr() + b0 * x.stride(0) * 2,
                                                          y.data_ptr() + b0 * out_features * 2, nb, x.stride(0), out_features,
                                                          dt, cells.data_ptr(), cells.numel() * 8, stream)
            else:
                rc = _lib.aqlm_hip_gemv_1x16_packed(ctypes.byref(packed.desc), packed.data_ptr(), codebooks.data_ptr(),
                                                    scales.data_ptr(), _ptr(bias), x.data_ptr() + b0 * x.stride(0) * 2,
                                                    y.data_ptr() + b0 * out_features * 2, nb, x.stride(0), out_features, dt,
                                                    ws_ptr, ws_len, stream)
            if rc:
                _native.check(rc, "aqlm gemv_1x16_packed")
    return y.reshape(input.shape[:-1] + (out_features,))


def _gemv_multi(input, codes, codebooks, scales, bias, kind):
    n = len(codes)
    if not (1 <= n <= _native.MAX_SEGMENTS) or not (len(codebooks) == len(scales) == len(bias) == n):
        raise ValueError(f"shared-input ops take 1..{_native.MAX_SEGMENTS} layers with one entry per list")
    dt = _dtype_id(input)
    num_codebooks, codebook_size, out_group_size, in_group_size = codebooks[0].shape
    if out_group_size != 1:
        raise NotImplementedError("AQLM HIP kernels require out_group_size == 1")
    in_features = codes[0].shape[1] * in_group_size
    if input.shape[-1] != in_features:
        raise ValueError(f"input has {input.shape[-1]} features, layers expect {in_features}")
    keep = []
    segs = (_native.Segment * n)()
    x = _flat_rows(input)
    B = x.shape[0]
    outs = []
    for k in range(n):
        cb = codebooks[k]
        if tuple(cb.shape) != (num_codebooks, codebook_size, 1, in_group_size):
            raise NotImplementedError(f"all layers of a shared-input launch must use one scheme; got codebooks "
                                      f"{tuple(cb.shape)} next to {tuple(codebooks[0].shape)}")
        if codes[k].shape[1] * in_group_size != in_features or codes[k].shape[2] != num_codebooks:
            raise ValueError("all layers of a shared-input launch must have the same in_features and num_codebooks")
        if cb.dtype != input.dtype or scales[k].dtype != input.dtype:
            raise NotImplementedError(f"input dtype {input.dtype} must match codebooks/scales dtype {cb.dtype}")
        c, cb, sc = _c(codes[k]), _c(cb), _c(scales[k])
        bi = None if bias[k] is None else _c(bias[k])
        out_features = c.shape[0]
        y = torch.empty((B, out_features), dtype=input.dtype, device=input.device)
        keep += [c, cb, sc, bi]
        outs.append(y)
        segs[k].codes, segs[k].codebook, segs[k].scales, segs[k].bias = c.data_ptr(), cb.data_ptr(), sc.data_ptr(), _ptr(bi)
        segs[k].y, segs[k].y_row_stride, segs[k].out_features = y.data_ptr(), out_features, out_features
    stream = _stream_ptr(input.device)
    with _device_guard(input.device):
        for b0 in range(0, B, _native.MAX_GEMV_BATCH):
            nb = min(_native.MAX_GEMV_BATCH, B - b0)
            for k in range(n):
                segs[k].y = outs[k].data_ptr() + b0 * outs[k].shape[1] * 2
            xp = x.data_ptr() + b0 * x.stride(0) * 2
            if kind == "1x16":
                rc = _lib.aqlm_hip_gemv_1x16_multi(segs, n, xp, in_features, in_group_size, nb, x.stride(0), dt, stream)
            else:
                rc = _lib.aqlm_hip_gemv_kx8_multi(segs, n, xp, in_features, num_codebooks, in_group_size, nb,
                                                  x.stride(0), dt, stream)
            if rc:
                _native.check(rc, "aqlm shared-input gemv")
    return [y.reshape(input.shape[:-1] + (y.shape[1],)) for y in outs]


def code1x16_matmat_multi(input, codes, codebooks, scales, bias):
    """Several 1x16 layers applied to the SAME input in one launch (aqlm_hip_gemv_1x16_multi): the q/k/v or gate/up
    projections of a decoder layer.  Lists of per-layer tensors in, list of outputs out; each output is bit-identical
    to code1x16_matmat on that layer.  Up to 8 input rows per launch like the single-layer op."""
    for cb in codebooks:
        if cb.shape[0] != 1 or cb.shape[1] != 65536:
            raise NotImplementedError(f"code1x16_matmat_multi needs codebooks [1, 65536, 1, g], got {tuple(cb.shape)}")
    return _gemv_multi(input, codes, codebooks, scales, bias, "1x16")


# Zero-at-rest accumulator cells of the single-kernel look-up-table matvec (aqlm_hip_gemv_8x8_lut_fused): one persistent
# int64 buffer per (device, stream) -- launches on one stream are ordered, so consecutive layers can share it; every launch
# leaves it zero.  Never allocated while a hipGraph is being captured (a captured torch.zeros would replay a memset per
# call): a capture whose stream has not run the op before takes the two-kernel form.
USE_8X8_LUT_FUSED = True
_LUT_CELLS = {}
_LUT_CELLS_RETIRED = []


def _lut_cells(device: torch.device, stream: int, rows: int) -> Optional[torch.Tensor]:
    if not USE_8X8_LUT_FUSED:
        return None
    if rows * 8 <= PACKED_CELLS_BYTES:  # both kernels leave their cells zero and launches of a stream are ordered: one set serves both
        shared = _shared_cells(device, stream, rows * 8)
        if shared is not False and shared is not None:
            return shared
    key = (device.index, stream)
    cells = _LUT_CELLS.get(key)
    if cells is None or cells.numel() < rows:
        if torch.cuda.is_current_stream_capturing():
            return None
        if cells is not None:
            _LUT_CELLS_RETIRED.append(cells)  # a hipGraph may have captured its address: never freed
        cells = torch.zeros((max(rows, 1 << 17),), dtype=torch.int64, device=device)
        _LUT_CELLS[key] = cells
    return cells


def _gemv_8x8_lut_multi(input, codes, codebooks, scales, bias):
    """Several 8-codebook layers times one single input row through per-token look-up tables in ONE launch
    (aqlm_hip_gemv_8x8_lut_multi); bit-identical to _gemv_8x8_lut per layer."""
    n = len(codes)
    dt = _dtype_id(input)
    g = codebooks[0].shape[3]
    in_features = codes[0].shape[1] * g
    if input.shape[-1] != in_features:
        raise ValueError(f"input has {input.shape[-1]} features, layers expect {in_features}")
    x = _flat_rows(input)
    segs = (_native.Segment * n)()
    keep, outs = [], []
    ws_bytes = 0
    for k in range(n):
        if tuple(codebooks[k].shape) != tuple(codebooks[0].shape) or codes[k].shape[1] * g != in_features:
            raise ValueError("all layers of a shared-input launch must have the same scheme and in_features")
        c, cb, sc = _c(codes[k]), _c(codebooks[k]), _c(scales[k])
        bi = None if bias[k] is None else _c(bias[k])
        out_features = c.shape[0]
        y = torch.empty((1, out_features), dtype=input.dtype, device=input.device)
        keep += [c, cb, sc, bi]
        outs.append(y)
        segs[k].codes, segs[k].codebook, segs[k].scales, segs[k].bias = c.data_ptr(), cb.data_ptr(), sc.data_ptr(), _ptr(bi)
        segs[k].y, segs[k].y_row_stride, segs[k].out_features = y.data_ptr(), out_features, out_features
        ws_bytes += _lib.aqlm_hip_workspace_bytes(_native.OP_GEMV_8X8_LUT, g, out_features, in_features)
    stream = _stream_ptr(input.device)
    cells = _lut_cells(input.device, stream, sum(y.shape[1] for y in outs))
    if cells is not None:
        with _device_guard(input.device):
            rc = _lib.aqlm_hip_gemv_8x8_lut_multi_fused(segs, n, x.data_ptr(), in_features, g, dt, cells.data_ptr(),
                                                        cells.numel() * 8, stream)
        if rc:
            _native.check(rc, "aqlm gemv_8x8_lut_multi_fused")
        return [y.reshape(input.shape[:-1] + (y.shape[1],)) for y in outs]
    ws = torch.empty((ws_bytes // 4,), dtype=torch.float32, device=input.device)
    with _device_guard(input.device):
        rc = _lib.aqlm_hip_gemv_8x8_lut_multi(segs, n, x.data_ptr(), in_features, g, dt, ws.data_ptr(), ws_bytes,
                                              _stream_ptr(input.device))
    if rc:
        _native.check(rc, "aqlm gemv_8x8_lut_multi")
    return [y.reshape(input.shape[:-1] + (y.shape[1],)) for y in outs]


def codekx8_matmat_multi(input, codes, codebooks, scales, bias):
    """Several K x 8-bit layers of one scheme applied to the same input: one launch for 1x8 / 2x8 g8
    (aqlm_hip_gemv_kx8_multi) and for single rows of 8-codebook schemes (look-up tables, aqlm_hip_gemv_8x8_lut_multi),
    one launch per layer otherwise.  Outputs agree with codekx8_matmat to fp32 rounding (8x8: bit for bit)."""
    for cb in codebooks:
        if cb.shape[1] != 256:
            raise NotImplementedError(f"codekx8_matmat_multi needs codebooks [K, 256, 1, g], got {tuple(cb.shape)}")
    cb0 = codebooks[0]
    if (USE_8X8_LUT and 1 <= len(codes) <= _native.MAX_SEGMENTS and cb0.shape[0] == 8 and cb0.shape[2] == 1
            and cb0.shape[3] in (8, 16, 32) and input.dtype == cb0.dtype and 1 <= _lut_rows(input) <= LUT_MAX_ROWS):
        if _lut_rows(input) > 1:  # the shared-input kernel takes one row of x: one multi-row launch per layer
            return [_gemv_8x8_lut(input, codes[k], codebooks[k], scales[k], bias[k]) for k in range(len(codes))]
        return _gemv_8x8_lut_multi(input, codes, codebooks, scales, bias)
    return _gemv_multi(input, codes, codebooks, scales, bias, "kx8")


def code1x16_matmat_packed_multi(input, packed, codebooks, scales, bias):
    """Several prepacked 1x16 g8 layers applied to the same input (up to 8 rows) in one launch
    (aqlm_hip_gemv_1x16_packed_multi); outputs bit-identical to code1x16_matmat_packed per layer."""
    n = len(packed)
    if not (1 <= n <= _native.MAX_SEGMENTS) or not (len(codebooks) == len(scales) == len(bias) == n):
        raise ValueError(f"code1x16_matmat_packed_multi takes 1..{_native.MAX_SEGMENTS} layers with one entry per list")
    x = _flat_rows(input)
    B = x.shape[0]
    if B > _native.MAX_GEMV_BATCH:
        return [code1x16_matmat_packed(input, packed[k], codebooks[k], scales[k], bias[k]) for k in range(n)]
    segs = (_native.Segment * n)()
    descs = (_native._descp * n)()
    keep, outs = [], []
    total = sum(pk.out_features for pk in packed)
    dt = None
    for k in range(n):
        dt = _check_packed_args(input, packed[k], codebooks[k], scales[k])
        refresh_range(packed[k], codebooks[k])
        cb, sc = _c(codebooks[k]), _c(scales[k])
        bi = None if bias[k] is None else _c(bias[k])
        of = packed[k].out_features
        y = torch.empty((B, of), dtype=input.dtype, device=input.device)
        keep += [cb, sc, bi]
        outs.append(y)
        segs[k].codes, segs[k].codebook, segs[k].scales, segs[k].bias = packed[k].data_ptr(), cb.data_ptr(), sc.data_ptr(), _ptr(bi)
        segs[k].y, segs[k].y_row_stride, segs[k].out_features = y.data_ptr(), of, of
        descs[k] = ctypes.pointer(packed[k].desc)
    stream = _stream_ptr(input.device)
    cells = None
    if FUSED_FINALIZE and all(pk.desc.codebook_absmax > 0.0 for pk in packed):  # single kernel, no workspace
        ws_ptr, ws_len = None, 0
        cells = _packed_cells(input.device, stream, B * total * 8)
    else:
        ws = _workspace(input.device, packed[0].slices * B * total * 4, stream)
        ws_ptr, ws_len = ws.data_ptr(), ws.numel() * 4
    with _device_guard(input.device):
        if cells is not None:
            rc = _lib.aqlm_hip_gemv_1x16_packed_multi_cells(segs, descs, n, x.data_ptr(), packed[0].in_features, B, x.stride(0),
                                                            dt, cells.data_ptr(), cells.numel() * 8, stream)
        else:
            rc = _lib.aqlm_hip_gemv_1x16_packed_multi(segs, descs, n, x.data_ptr(), packed[0].in_features, B, x.stride(0), dt,
                                                      ws_ptr, ws_len, stream)
    if rc == _native.E_UNSUPPORTED and B > 1:
        # the rows do not fit one LDS image next to the codebook slice (very wide inputs): per-layer launches split the
        # rows themselves; same kernels, same bits
        return [code1x16_matmat_packed(input, packed[k], codebooks[k], scales[k], bias[k]) for k in range(n)]
    if rc:
        _native.check(rc, "aqlm gemv_1x16_packed_multi")
    return [y.reshape(input.shape[:-1] + (y.shape[1],)) for y in outs]


# Transparent prepack for the RAW op.  `aqlm::code1x16_matmat` is stateless in the reference (cuda_kernel.cpp:148-182); here
# the fast kernel needs the slice-bucketed layout of the codes (1.2-5x faster on layers of >= 0.5 M codes).  `QuantizedLinear`
# keeps that derived buffer itself; callers of the raw op -- the reference's own benchmark/matmul_benchmark.py:103, vLLM-style
# integrations -- get it from this cache: keyed by the identity of the `codes` tensor object (a weak reference drops the
# entry when the tensor dies, so an address reused by a new tensor can never alias it), validated on every hit against
# (data_ptr, _version, shape), bounded in bytes (RAW_OP_PREPACK_MAX_BYTES, 1 GiB, least recently used evicted).  A caller that passes a fresh view object on every call never hits: after
# RAW_OP_PREPACK_MAX_MISSES packs without a single hit the cache switches itself off.  Nothing is packed while a hipGraph is
# being captured (the pack synchronises); outputs equal the direct kernel's up to fp32 summation order.
MATMAT_GEMM_MIN_ROWS = 7              # rows (batch x sequence) from which aqlm::code1x16_matmat runs the MFMA kernel (= the module's gemv rule + 1)
RAW_OP_PREPACK = True                 # set False to keep the raw op on the direct kernel
RAW_OP_PREPACK_MIN_CODES = 500_000  # same threshold as QuantizedLinear (inference.PREPACK_MIN_CODES)
RAW_OP_PREPACK_MAX_BYTES = 1 << 30  # of packed buffers held for callers of the raw op (modules keep their own); least recently used go first
RAW_OP_PREPACK_MAX_MISSES = 8
RAW_OP_CHECK_EVERY = 256            # hits of a cached layer between two checksum verifications of its codes (0 = never): a write through `.data` changes neither identity nor version
_RAW_PACKED = {}                      # id(codes) -> _RawEntry


class _RawEntry:
    """One layer of the raw op's cache (packed is None: a layer the packed path does not cover, cached so that it is not retried)."""

    __slots__ = ("ref", "fingerprint", "packed", "checksum", "hits")

    def __init__(self, ref, fingerprint, packed, checksum):
        self.ref, self.fingerprint, self.packed, self.checksum = ref, fingerprint, packed, checksum
        self.hits = 0  # since the last verification: the calls served here + those the compiled op served

    def __getitem__(self, i):  # positional access, in the order of the fields (what callers of the former tuple index)
        return getattr(self, self.__slots__[i])


_RAW_STATS = {"bytes": 0, "packs_without_hit": 0, "hits": 0, "packs": 0}
# Compiled kernels of the three reference ops (csrc_front/front.cpp, installed at the end of this file when the extension is
# built): calls through torch.ops.aqlm.* of <= 6 rows are launched from C++; this module stays their fallback and the owner of
# the cache above -- a packed layer is REGISTERED with the extension (key below) and forgotten there when it is dropped here.
_RAW_FAST = None                      # the extension once its kernels are installed
_RAW_FAST_KEYS = {}                   # id(codes) -> (key of the extension's entry, (id, version, data pointer) of the codebooks it was registered with)


def _raw_sync_config():
    """Push the knobs the compiled raw ops mirror (call after changing RAW_OP_PREPACK*, MATMAT_GEMM_MIN_ROWS, FUSED_FINALIZE;
    clear_raw_op_prepack_cache() does)."""
    if _RAW_FAST is not None:
        _RAW_FAST.raw_config(bool(FUSED_FINALIZE), bool(RAW_OP_PREPACK), int(RAW_OP_PREPACK_MIN_CODES), int(MATMAT_GEMM_MIN_ROWS),
                             int(RAW_OP_CHECK_EVERY))


def _raw_register_fast(codes, packed, codebooks):
    if _RAW_FAST is None or not FUSED_FINALIZE or packed.desc.codebook_absmax <= 0.0:
        return
    have = _RAW_FAST_KEYS.get(id(codes))
    mark = (id(codebooks), tensor_version(codebooks), codebooks.data_ptr())
    if have is not None and have[1] == mark:
        return
    key = _RAW_FAST.raw_register(codes, packed.buf, bytes(packed.desc), codebooks)
    if key:
        _RAW_FAST_KEYS[id(codes)] = (key, mark)


def _raw_fingerprint(codes):
    return (codes.data_ptr(), tensor_version(codes), tuple(codes.shape), tuple(codes.stride()), codes.dtype, codes.device)


def _raw_drop(key):
    entry = _RAW_PACKED.pop(key, None)
    if entry is not None and entry.packed is not None:
        _RAW_STATS["bytes"] -= entry.packed.numel()
    fast = _RAW_FAST_KEYS.pop(key, None)
    if fast is not None and _RAW_FAST is not None:
        _RAW_FAST.raw_forget(fast[0])


def clear_raw_op_prepack_cache():
    """Forget every buffer the raw op packed on its own (frees the device memory they hold)."""
    for key in list(_RAW_PACKED):
        _raw_drop(key)
    _RAW_STATS["packs_without_hit"] = 0
    if _RAW_FAST is not None:
        _RAW_FAST.raw_clear()
        _RAW_FAST_KEYS.clear()
    _raw_sync_config()


def _raw_packed_for(codes, codebooks, input):
    """The cached packed form of `codes`, packing it at first sight; None = use the direct kernel."""
    if not RAW_OP_PREPACK or not codes.is_cuda or codes.dtype != torch.int16 or codes.dim() != 3 or codes.shape[2] != 1:
        return None
    if codebooks.shape[3] not in (8, 16) or codes.shape[0] * codes.shape[1] < RAW_OP_PREPACK_MIN_CODES:
        return None
    if input.dtype != codebooks.dtype or input.numel() // input.shape[-1] > _native.MAX_GEMV_BATCH:
        return None
    key = id(codes)
    entry = _RAW_PACKED.get(key)
    fp = _raw_fingerprint(codes)
    if entry is not None:
        ok = entry.ref() is codes and entry.fingerprint == fp
        if ok and entry.packed is not None and not torch.cuda.is_current_stream_capturing() and not torch.compiler.is_compiling():
            # unversioned writes (`codes.data.copy_()`): re-check the checksum taken at pack time once per RAW_OP_CHECK_EVERY hits
            # of THIS layer -- served here or by the compiled op (its count for this entry is taken over below; it hands the call
            # that completes a period to this function).  The calls it declines for other reasons (grad mode, strided x) come
            # here too and must not pay a checksum + host sync each: other layers' hits do not count.
            fast = _RAW_FAST_KEYS.get(key)
            entry.hits += 1 + (_RAW_FAST.raw_take_hits(fast[0]) if fast is not None else 0)
            if RAW_OP_CHECK_EVERY and entry.hits >= RAW_OP_CHECK_EVERY:
                entry.hits = 0
                ok = entry.checksum is None or tensor_checksum(codes) == entry.checksum
                entry.packed.verify_range(codebooks)  # ... and the codebook image / range against the codebook's
        if ok:
            if entry.packed is not None:
                _RAW_STATS["hits"] += 1
                _RAW_STATS["packs_without_hit"] = 0
                _RAW_PACKED[key] = _RAW_PACKED.pop(key)  # most recently used last (dicts keep insertion order)
            return entry.packed
        _raw_drop(key)  # the tensor was modified in place / rebound: pack again
    if _RAW_FAST is not None:  # hits served by the compiled op never pass through here: read its counter
        fast_hits = _RAW_FAST.raw_hits()
        if fast_hits != _RAW_STATS.get("fast_hits_seen", 0):
            _RAW_STATS["fast_hits_seen"] = fast_hits
            _RAW_STATS["packs_without_hit"] = 0
    if (_RAW_STATS["packs_without_hit"] >= RAW_OP_PREPACK_MAX_MISSES or torch.cuda.is_current_stream_capturing()
            or torch.compiler.is_compiling()):
        return None
    import weakref

    packed = None
    g = int(codebooks.shape[3])
    cap = _lib.aqlm_hip_prepack_1x16_bytes(codes.shape[0], codes.shape[1] * g, g)
    est = cap * 3 // 10  # what the packed buffer will hold, roughly (the capacity covers the 3-byte form's working copy, unbalanced streams and scratch)
    if cap and est <= RAW_OP_PREPACK_MAX_BYTES:
        # bounded: the least recently used packed buffers make room (a caller cycling through more layers than fit keeps
        # repacking -- `packs_without_hit` then switches the cache off -- and should hold PackedCodes itself, like the module)
        for old in list(_RAW_PACKED):
            if _RAW_STATS["bytes"] + est <= RAW_OP_PREPACK_MAX_BYTES:
                break
            if _RAW_PACKED[old].packed is not None:
                _raw_drop(old)
        packed = prepack_1x16(codes, g)
    try:
        ref = weakref.ref(codes, lambda _r, k=key: _raw_drop(k))
    except TypeError:
        return None
    _RAW_PACKED[key] = _RawEntry(ref, fp, packed, tensor_checksum(codes) if packed is not None and RAW_OP_CHECK_EVERY else None)
    if packed is not None:
        _RAW_STATS["bytes"] += packed.numel()
        _RAW_STATS["packs"] += 1
        _RAW_STATS["packs_without_hit"] += 1
    return packed


def code1x16_matmat(input, codes, codebooks, scales, bias=None):
    """aqlm::code1x16_matmat (cuda_kernel.py:13-22, cuda_kernel.cpp:148-182)."""
    if codebooks.shape[0] != 1 or codebooks.shape[1] != 65536:
        raise NotImplementedError(f"code1x16_matmat needs codebooks [1, 65536, 1, g], got {tuple(codebooks.shape)}")
    rows = input.numel() // input.shape[-1] if input.shape[-1] else 0
    if rows >= MATMAT_GEMM_MIN_ROWS and input.shape[-1] % 64 == 0 and input.dtype == codebooks.dtype and codebooks.shape[2] == 1:
        # the matvec kernels pay one more LDS gather + 4 dot products per code and input row (prepacked 4096->11008:
        # 9 / 18 / 35 us for 1 / 4 / 8 rows); from 7 rows on the MFMA kernel (~16 / 28 us for up to 16 rows at
        # 4096->4096 / 4096->11008, one gather per code whatever the batch) is the faster way through the same op.  The
        # reference relaunches its matvec once per row here (cuda_kernel.cpp:165-175).
        return code1x16_matmat_dequant(input, codes, codebooks, scales, bias)
    packed = _raw_packed_for(codes, codebooks, input)
    if packed is not None and scales.dtype == input.dtype and input.device == codes.device:
        y = code1x16_matmat_packed(input, packed, codebooks, scales, bias)
        _raw_register_fast(codes, packed, codebooks)  # (after the call: it brought the codebook range up to date)
        return y
    return _gemv(input, codes, codebooks, scales, bias, "1x16")


def code2x8_matmat(input, codes, codebooks, scales, bias=None):
    """aqlm::code2x8_matmat (cuda_kernel.py:58-67, cuda_kernel.cpp:387-421)."""
    if codebooks.shape[0] != 2 or codebooks.shape[1] != 256:
        raise NotImplementedError(f"code2x8_matmat needs codebooks [2, 256, 1, g], got {tuple(codebooks.shape)}")
    return _gemv(input, codes, codebooks, scales, bias, "kx8")


def code1x8_matmat(input, codes, codebooks, scales, bias=None):
    """aqlm::code1x8_matmat (cuda_kernel.py:100-109, cuda_kernel.cpp:552-586)."""
    if codebooks.shape[0] != 1 or codebooks.shape[1] != 256:
        raise NotImplementedError(f"code1x8_matmat needs codebooks [1, 256, 1, g], got {tuple(codebooks.shape)}")
    return _gemv(input, codes, codebooks, scales, bias, "kx8")


# 8 x 8-bit matvecs of up to LUT_MAX_ROWS rows use per-token look-up tables in LDS (aqlm_hip_gemv_8x8_lut*) instead of LDS
# gathers: one row = one set of workgroups, 2+ rows = one launch of rows x that set (aqlm_hip_gemv_8x8_lut_batch; round 5 -- before,
# the second row sent the call to the plain LDS kernel: 16-37 us for what the table kernel does in 6 per row)
USE_8X8_LUT = True
LUT_MAX_ROWS = _native.MAX_GEMV_BATCH


def _lut_rows(input) -> int:
    return input.numel() // input.shape[-1] if input.shape[-1] else 0


def _gemv_8x8_lut_rows(input, x, codes_ptr, codebooks, scales, bias, out_features, in_features, g, dt, planar, absmax):
    """2..LUT_MAX_ROWS rows: ONE launch when the stream's cells hold rows x out_features (else None: the caller loops the rows)."""
    B = x.shape[0]
    stream = _stream_ptr(input.device)
    cells = _lut_cells(input.device, stream, B * out_features)
    if cells is None or (planar and not absmax > 0.0):
        return None
    y = torch.empty((B, out_features), dtype=input.dtype, device=input.device)
    with _device_guard(input.device):
        rc = _lib.aqlm_hip_gemv_8x8_lut_batch(codes_ptr, codebooks.data_ptr(), scales.data_ptr(), _ptr(bias), x.data_ptr(), y.data_ptr(),
                                              out_features, in_features, g, B, x.stride(0), out_features, dt, 1 if planar else 0,
                                              float(absmax), cells.data_ptr(), cells.numel() * 8, stream)
    if rc:
        _native.check(rc, "aqlm gemv_8x8_lut_batch")
    return y.reshape(input.shape[:-1] + (out_features,))


def _gemv_8x8_lut(input, codes, codebooks, scales, bias):
    dt = _dtype_id(input)
    g = codebooks.shape[3]
    out_features, in_features = codes.shape[0], codes.shape[1] * g
    if input.shape[-1] != in_features:
        raise ValueError(f"input has {input.shape[-1]} features, layer expects {in_features}")
    x = _flat_rows(input)
    codes, codebooks, scales = _c(codes), _c(codebooks), _c(scales)
    if bias is not None:
        bias = _c(bias)
    if x.shape[0] > 1:
        y = _gemv_8x8_lut_rows(input, x, codes.data_ptr(), codebooks, scales, bias, out_features, in_features, g, dt, False, 0.0)
        if y is not None:
            return y
        return torch.cat([_gemv_8x8_lut(x[b:b + 1], codes, codebooks, scales, bias) for b in range(x.shape[0])]).reshape(
            input.shape[:-1] + (out_features,))
    y = torch.empty((1, out_features), dtype=input.dtype, device=input.device)
    stream = _stream_ptr(input.device)
    cells = _lut_cells(input.device, stream, out_features)
    if cells is not None:  # one kernel
        with _device_guard(input.device):
            rc = _lib.aqlm_hip_gemv_8x8_lut_fused(codes.data_ptr(), codebooks.data_ptr(), scales.data_ptr(), _ptr(bias),
                                                  x.data_ptr(), y.data_ptr(), out_features, in_features, g, dt,
                                                  cells.data_ptr(), cells.numel() * 8, stream)
        if rc:
            _native.check(rc, "aqlm gemv_8x8_lut_fused")
        return y.reshape(input.shape[:-1] + (out_features,))
    ws_bytes = _lib.aqlm_hip_workspace_bytes(_native.OP_GEMV_8X8_LUT, g, out_features, in_features)
    ws = torch.empty((ws_bytes // 4,), dtype=torch.float32, device=input.device)
    with _device_guard(input.device):
        rc = _lib.aqlm_hip_gemv_8x8_lut(codes.data_ptr(), codebooks.data_ptr(), scales.data_ptr(), _ptr(bias),
                                        x.data_ptr(), y.data_ptr(), out_features, in_features, g, dt, ws.data_ptr(),
                                        ws_bytes, stream)
    if rc:
        _native.check(rc, "aqlm gemv_8x8_lut")
    return y.reshape(input.shape[:-1] + (out_features,))


# ------------------------------------------------------------------------------------------------------
# planar 8 x 8-bit codes (aqlm_hip_8x8_planar_pack): [8][out][in_groups rounded up to 4] bytes, the checkpoint's
# [out][in_groups][8] transposed.  A workgroup of the look-up-table matvec then serves ONE codebook x 128 input groups: 16 KiB
# of codebook instead of 128 KiB through its L1, its codes as 128 contiguous bytes per row.  Same size as the canonical codes,
# lossless; derived at load time like the prepacked 1x16 buffer (the reference permutes its codes for the CPU look-up kernel
# in the same place, inference.py:78-83).
# ------------------------------------------------------------------------------------------------------
PLANAR_8X8_MIN_GROUPS = 64  # input groups below which a 128-group slab would be mostly empty: canonical layout


class PlanarCodes(_DerivedCodes):
    """8x8 codes in the planar layout + the codebook bound the single-kernel finalize needs."""

    __slots__ = ("codebook_absmax",)

    def __init__(self, buf: torch.Tensor, out_features: int, in_features: int, in_group_size: int):
        self.buf = buf
        self.out_features, self.in_features, self.in_group_size = out_features, in_features, in_group_size
        self.codebook_absmax = 0.0
        self._range_of = self._range_checksum = None

    def _store_range(self, absmax: float, codebooks: Optional[torch.Tensor]) -> None:
        self.codebook_absmax = absmax

    def unpack(self) -> torch.Tensor:
        return planar_8x8_unpack(self)


def planar_8x8_pack(codes: torch.Tensor, in_group_size: int, codebooks: Optional[torch.Tensor] = None) -> Optional[PlanarCodes]:
    """Planar copy of 8x8 codes [out, in/g, 8] (int8); None when the layout does not pay (few input groups)."""
    if codes.dim() != 3 or codes.shape[2] != 8 or codes.dtype != torch.int8 or not codes.is_cuda:
        return None
    out_features, in_groups = codes.shape[0], codes.shape[1]
    if in_groups < PLANAR_8X8_MIN_GROUPS:
        return None
    in_features = in_groups * in_group_size
    nbytes = _lib.aqlm_hip_8x8_planar_bytes(out_features, in_features, in_group_size)
    if nbytes == 0:
        return None
    codes = _c(codes)
    buf = torch.empty((nbytes,), dtype=torch.uint8, device=codes.device)
    with torch.cuda.device(codes.device):
        rc = _lib.aqlm_hip_8x8_planar_pack(codes.data_ptr(), out_features, in_features, in_group_size, buf.data_ptr(), nbytes,
                                           _stream_ptr(codes.device))
    if rc:
        _native.check(rc, "aqlm 8x8_planar_pack")
    planar = PlanarCodes(buf, out_features, in_features, in_group_size)
    if codebooks is not None and not torch.cuda.is_current_stream_capturing():
        planar.set_codebook_range(codebooks)
    return planar


def planar_8x8_unpack(planar: PlanarCodes) -> torch.Tensor:
    """The canonical codes [out, in/g, 8] (int8) of a planar buffer (aqlm_hip_8x8_planar_unpack; lossless)."""
    codes = torch.empty((planar.out_features, planar.in_features // planar.in_group_size, 8), dtype=torch.int8, device=planar.device)
    with torch.cuda.device(planar.device):
        rc = _lib.aqlm_hip_8x8_planar_unpack(planar.data_ptr(), planar.out_features, planar.in_features, planar.in_group_size,
                                             codes.data_ptr(), _stream_ptr(planar.device))
    if rc:
        _native.check(rc, "aqlm 8x8_planar_unpack")
    return codes


def _check_planar_args(input, planar, codebooks, scales):
    if codebooks.dtype != input.dtype or scales.dtype != input.dtype:
        raise NotImplementedError(f"input dtype {input.dtype} must match codebooks/scales dtype {codebooks.dtype}")
    if tuple(codebooks.shape) != (8, 256, 1, planar.in_group_size):
        raise NotImplementedError(f"planar codes of an 8x8 g{planar.in_group_size} layer need codebooks [8, 256, 1, {planar.in_group_size}], got {tuple(codebooks.shape)}")
    if input.shape[-1] != planar.in_features:
        raise ValueError(f"input has {input.shape[-1]} features, layer expects {planar.in_features}")
    if input.device != planar.device or codebooks.device != input.device:
        raise ValueError(f"input on {input.device}, layer on {planar.device}")
    return _dtype_id(input)


def code8x8_matmat_planar(input, planar: PlanarCodes, codebooks, scales, bias=None):
    """8x8 matvec of 1..LUT_MAX_ROWS rows on planar codes (aqlm_hip_gemv_8x8_lut_planar / _batch); same contract as codekx8_matmat."""
    dt = _check_planar_args(input, planar, codebooks, scales)
    x = _flat_rows(input)
    codebooks, scales = _c(codebooks), _c(scales)
    if bias is not None:
        bias = _c(bias)
    out_features, in_features, g = planar.out_features, planar.in_features, planar.in_group_size
    refresh_range(planar, codebooks)
    if x.shape[0] > 1:
        if x.shape[0] > LUT_MAX_ROWS:
            raise ValueError(f"code8x8_matmat_planar takes 1..{LUT_MAX_ROWS} rows, got {x.shape[0]}")
        y = _gemv_8x8_lut_rows(input, x, planar.data_ptr(), codebooks, scales, bias, out_features, in_features, g, dt, True,
                               planar.codebook_absmax)
        if y is not None:
            return y
        return torch.cat([code8x8_matmat_planar(x[b:b + 1], planar, codebooks, scales, bias) for b in range(x.shape[0])]).reshape(
            input.shape[:-1] + (out_features,))
    y = torch.empty((1, out_features), dtype=input.dtype, device=input.device)
    stream = _stream_ptr(input.device)
    cells = _lut_cells(input.device, stream, out_features) if planar.codebook_absmax > 0.0 else None
    with _device_guard(input.device):
        if cells is not None:
            rc = _lib.aqlm_hip_gemv_8x8_lut_planar(planar.data_ptr(), codebooks.data_ptr(), scales.data_ptr(), _ptr(bias), x.data_ptr(),
                                                   y.data_ptr(), out_features, in_features, g, dt, planar.codebook_absmax,
                                                   cells.data_ptr(), cells.numel() * 8, 1, stream)
        else:
            ws_bytes = _lib.aqlm_hip_workspace_bytes(_native.OP_GEMV_8X8_LUT, g, out_features, in_features)
            ws = torch.empty((ws_bytes // 4,), dtype=torch.float32, device=input.device)
            rc = _lib.aqlm_hip_gemv_8x8_lut_planar(planar.data_ptr(), codebooks.data_ptr(), scales.data_ptr(), _ptr(bias), x.data_ptr(),
                                                   y.data_ptr(), out_features, in_features, g, dt, 0.0, ws.data_ptr(), ws_bytes, 0, stream)
    if rc:
        _native.check(rc, "aqlm gemv_8x8_lut_planar")
    return y.reshape(input.shape[:-1] + (out_features,))


def code8x8_matmat_planar_multi(input, planar, codebooks, scales, bias):
    """Several planar 8x8 layers times one input row in ONE launch (aqlm_hip_gemv_8x8_lut_planar_multi); bit-identical to
    code8x8_matmat_planar per layer."""
    n = len(planar)
    if not (1 <= n <= _native.MAX_SEGMENTS) or not (len(codebooks) == len(scales) == len(bias) == n):
        raise ValueError(f"code8x8_matmat_planar_multi takes 1..{_native.MAX_SEGMENTS} layers with one entry per list")
    if _lut_rows(input) > 1:  # the shared-input kernel takes one row of x: 2+ rows run one (multi-row) launch per layer
        return [code8x8_matmat_planar(input, planar[k], codebooks[k], scales[k], bias[k]) for k in range(n)]
    x = _flat_rows(input)
    segs = (_native.Segment * n)()
    absmax = (ctypes.c_float * n)()
    keep, outs = [], []
    dt, ws_bytes = None, 0
    g, in_features = planar[0].in_group_size, planar[0].in_features
    for k in range(n):
        dt = _check_planar_args(input, planar[k], codebooks[k], scales[k])
        if planar[k].in_group_size != g or planar[k].in_features != in_features:
            raise ValueError("all layers of a shared-input launch must have the same scheme and in_features")
        refresh_range(planar[k], codebooks[k])
        cb, sc = _c(codebooks[k]), _c(scales[k])
        bi = None if bias[k] is None else _c(bias[k])
        of = planar[k].out_features
        y = torch.empty((1, of), dtype=input.dtype, device=input.device)
        keep += [cb, sc, bi]
        outs.append(y)
        segs[k].codes, segs[k].codebook, segs[k].scales, segs[k].bias = planar[k].data_ptr(), cb.data_ptr(), sc.data_ptr(), _ptr(bi)
        segs[k].y, segs[k].y_row_stride, segs[k].out_features = y.data_ptr(), of, of
        absmax[k] = planar[k].codebook_absmax
        ws_bytes += _lib.aqlm_hip_workspace_bytes(_native.OP_GEMV_8X8_LUT, g, of, in_features)
    stream = _stream_ptr(input.device)
    cells = _lut_cells(input.device, stream, sum(y.shape[1] for y in outs)) if all(a > 0.0 for a in absmax) else None
    with _device_guard(input.device):
        if cells is not None:
            rc = _lib.aqlm_hip_gemv_8x8_lut_planar_multi(segs, absmax, n, x.data_ptr(), in_features, g, dt, cells.data_ptr(),
                                                         cells.numel() * 8, 1, stream)
        else:
            ws = torch.empty((ws_bytes // 4,), dtype=torch.float32, device=input.device)
            rc = _lib.aqlm_hip_gemv_8x8_lut_planar_multi(segs, absmax, n, x.data_ptr(), in_features, g, dt, ws.data_ptr(), ws_bytes, 0,
                                                         stream)
    if rc:
        _native.check(rc, "aqlm gemv_8x8_lut_planar_multi")
    return [y.reshape(input.shape[:-1] + (y.shape[1],)) for y in outs]


def codekx8_matmat(input, codes, codebooks, scales, bias=None):
    """Any K x 8-bit scheme (e.g. 8x8 g32): the HIP replacement for the reference's Triton fallback
    (kernel_selector.py:91-94, triton_kernel.py:187-205)."""
    if codebooks.shape[1] != 256:
        raise NotImplementedError(f"codekx8_matmat needs 256-entry codebooks, got {tuple(codebooks.shape)}")
    if (codebooks.shape[0] == 8 and codebooks.shape[3] == 32 and input.dtype == codebooks.dtype and input.dtype in _DT and codes.dim() == 3
            and _lut_rows(input) >= fused_8x8_min_rows(codes.shape[0], codes.shape[1] * 32)):
        y = _fused_8x8_mfma(input, codes, codebooks, scales, bias, _DT[input.dtype])  # one MFMA per codebook, rows (<= 16) for free
        if y is not None:
            return y
    if (USE_8X8_LUT and codebooks.shape[0] == 8 and codebooks.shape[2] == 1 and codebooks.shape[3] in (8, 16, 32)
            and 1 <= _lut_rows(input) <= LUT_MAX_ROWS and input.dtype == codebooks.dtype):
        return _gemv_8x8_lut(input, codes, codebooks, scales, bias)
    return _gemv(input, codes, codebooks, scales, bias, "kx8")


def generic_matmat(input, codes, codebooks, scales, bias=None):
    """Any scheme with out_group_size == 1 (slow generic kernel)."""
    return _gemv(input, codes, codebooks, scales, bias, "generic")


# ------------------------------------------------------------------------------------------------------
# dequantisation
# ------------------------------------------------------------------------------------------------------
def _dequant(codes, codebooks, scales, kind):
    dt = _dtype_id(codebooks)
    num_codebooks, codebook_size, out_group_size, in_group_size = codebooks.shape
    if out_group_size != 1:
        raise NotImplementedError("AQLM HIP kernels require out_group_size == 1")
    out_features = codes.shape[0]
    in_features = codes.shape[1] * in_group_size
    codes, codebooks = _c(codes), _c(codebooks)
    if scales is not None:
        scales = _c(scales)
    W = torch.empty((out_features, in_features), dtype=codebooks.dtype, device=codebooks.device)
    with torch.cuda.device(codebooks.device):
        if kind == "1x16":
            rc = _lib.aqlm_hip_dequant_1x16(codes.data_ptr(), codebooks.data_ptr(), _ptr(scales), W.data_ptr(),
                                            out_features, in_features, in_group_size, dt, _stream_ptr(codebooks.device))
        elif kind == "generic":
            nbits = int(codebook_size).bit_length() - 1
            rc = _lib.aqlm_hip_dequant_generic(codes.data_ptr(), codebooks.data_ptr(), _ptr(scales), W.data_ptr(),
                                               out_features, in_features, num_codebooks, nbits, in_group_size, dt,
                                               _stream_ptr(codebooks.device))
        else:
            rc = _lib.aqlm_hip_dequant_kx8(codes.data_ptr(), codebooks.data_ptr(), _ptr(scales), W.data_ptr(),
                                           out_features, in_features, num_codebooks, in_group_size, dt, _stream_ptr(codebooks.device))
    if rc:
        _native.check(rc, "aqlm dequant")
    return W


def code1x16_dequant(codes, codebooks, scales):
    """pybind ``code1x16_dequant`` (cuda_kernel.cpp:184-227): scaled weight [out, in]."""
    return _dequant(codes, codebooks, scales, "1x16")


def code2x8_dequant(codes, codebooks, scales):
    """pybind ``code2x8_dequant`` (cuda_kernel.cpp:423-448)."""
    return _dequant(codes, codebooks, scales, "kx8")


def code1x8_dequant(codes, codebooks, scales):
    """pybind ``code1x8_dequant`` (cuda_kernel.cpp:588-613)."""
    return _dequant(codes, codebooks, scales, "kx8")


# ------------------------------------------------------------------------------------------------------
# large-batch ops
# ------------------------------------------------------------------------------------------------------
# Rows (batch x sequence) up to which the large-batch 1x16 op runs the fused dequant->MFMA kernel.  The fused kernel
# re-gathers the codebook entries for every slab of 128 rows (~21 us per slab at 4096x4096 since round 3), whereas
# dequantising W once costs 14 us and lets hipBLASLt run the GEMM at matrix-core speed.  Measured (bench.py detail,
# hipGraph, 4096x4096): 128 rows 23.3 vs 38.9 us, 256 rows 42.8 vs 54.1 us, 1024 rows 167 vs 72 us -- two slabs still win,
# long prefills take the dequant + GEMM route like the reference does (cuda_kernel.cpp:249-301).
FUSED_MFMA_MAX_ROWS = 256


def _scale_bias_fp32(y, scales, bias):
    """y * scales + bias for the dequant + library-GEMM routes, in fp32 with one final rounding (the fused kernels do
    the same in registers; the reference does it in the output dtype, cuda_kernel.cpp:95-111)."""
    out = y.float() * scales.reshape(1, -1).float()
    if bias is not None:
        out = out + bias.float()
    return out.to(y.dtype)


def _fused_mfma_ok(x, in_features):
    return in_features % 64 == 0 and x.shape[0] <= FUSED_MFMA_MAX_ROWS


def code1x16_matmat_scan(input, codes, codebooks, scales, bias=None):
    """1x16 g8 at 2+ rows on the slice-scan MFMA kernel (aqlm_hip_gemm_1x16_scan, round 6): codebook slices in LDS, canonical codes,
    no gathers from L2.  Returns None when the kernel does not take the layer (codebook vectors other than 8, in_features % 256 != 0,
    misaligned rows) -- callers then use `code1x16_matmat_dequant`, which also routes here by default."""
    if codebooks.shape[0] != 1 or codebooks.shape[1] != 65536 or codebooks.shape[2] != 1 or codebooks.shape[3] != 8:
        return None
    out_features, in_features = codes.shape[0], codes.shape[1] * 8
    if input.shape[-1] != in_features:
        raise ValueError(f"input has {input.shape[-1]} features, layer expects {in_features}")
    x = _flat_rows(input)
    B = x.shape[0]
    if B == 0 or in_features % 256 != 0 or x.stride(0) % 8 != 0 or x.data_ptr() % 16 != 0:
        return None
    dt = _dtype_id(input)
    ws_bytes = _lib.aqlm_hip_gemm_1x16_scan_workspace_bytes(B, out_features, in_features)
    if ws_bytes == 0:
        return None
    codes, codebooks, scales = _c(codes), _c(codebooks), _c(scales)
    if bias is not None:
        bias = _c(bias)
    y = torch.empty((B, out_features), dtype=input.dtype, device=input.device)
    ws = torch.empty((ws_bytes // 4,), dtype=torch.float32, device=input.device)
    with _device_guard(input.device):
        rc = _lib.aqlm_hip_gemm_1x16_scan(codes.data_ptr(), codebooks.data_ptr(), scales.data_ptr(), _ptr(bias), x.data_ptr(), y.data_ptr(),
                                          B, out_features, in_features, x.stride(0), out_features, dt, ws.data_ptr(), ws.numel() * 4,
                                          _stream_ptr(input.device))
    if rc:
        _native.check(rc, "aqlm gemm_1x16_scan")
    return y.reshape(input.shape[:-1] + (out_features,))


def code1x16_matmat_dequant(input, codes, codebooks, scales, bias=None):
    """aqlm::code1x16_matmat_dequant (cuda_kernel.py:24-35, cuda_kernel.cpp:249-301) -- fused MFMA kernel."""
    dt = _dtype_id(input)
    if codebooks.shape[0] != 1 or codebooks.shape[1] != 65536 or codebooks.shape[2] != 1:
        raise NotImplementedError(f"code1x16_matmat_dequant needs codebooks [1, 65536, 1, g], got {tuple(codebooks.shape)}")
    in_group_size = codebooks.shape[3]
    out_features, in_features = codes.shape[0], codes.shape[1] * in_group_size
    if input.shape[-1] != in_features:
        raise ValueError(f"input has {input.shape[-1]} features, layer expects {in_features}")
    x = _flat_rows(input)
    B = x.shape[0]
    if not _fused_mfma_ok(x, in_features):
        # unscaled W is exact in the storage dtype (it IS the codebook entries); scaling W instead of y would round it
        W = _dequant(codes, codebooks, None, "1x16")
        return _scale_bias_fp32(F.linear(x, W), scales, bias).reshape(input.shape[:-1] + (out_features,))
    codes, codebooks, scales = _c(codes), _c(codebooks), _c(scales)
    if bias is not None:
        bias = _c(bias)
    y = torch.empty((B, out_features), dtype=input.dtype, device=input.device)
    ws_bytes = _lib.aqlm_hip_workspace_bytes(_native.OP_GEMM_1X16_MFMA, B, out_features, in_features)
    ws = torch.empty((max(ws_bytes, 16) // 4,), dtype=torch.float32, device=input.device)
    with _device_guard(input.device):
        rc = _lib.aqlm_hip_gemm_1x16_mfma(codes.data_ptr(), codebooks.data_ptr(), scales.data_ptr(), _ptr(bias),
                                          x.data_ptr(), y.data_ptr(), B, out_features, in_features, in_group_size,
                                          x.stride(0), out_features, dt, ws.data_ptr(), ws.numel() * 4, _stream_ptr(input.device))
    if rc:
        _native.check(rc, "aqlm gemm_1x16_mfma")
    return y.reshape(input.shape[:-1] + (out_features,))


def _matmat_dequant_kx8(input, codes, codebooks, scales, bias):
    """Reference pipeline for the 8-bit schemes (cuda_kernel.cpp:450-484, 615-649): dequantise (our kernel), one
    library GEMM, scale + bias."""
    dt = _dtype_id(input)
    y = _fused_kx8_mfma(input, codes, codebooks, scales, bias, dt)
    if y is None and codebooks.shape[0] == 8:
        y = _fused_8x8_mfma(input, codes, codebooks, scales, bias, dt)
    if y is not None:
        return y
    # W without the scales: exact for one codebook, one rounding of the K-term sum otherwise (as in the reference, which
    # also scales y after the GEMM, cuda_kernel.cpp:478-483); folding the scales into W would round every weight again
    W = _dequant(codes, codebooks, None, "kx8")
    return _scale_bias_fp32(F.linear(input, W), scales, bias)


# Rows up to which the 8-bit schemes' large-batch ops run the fused kernel (aqlm_hip_gemm_kx8_mfma: one launch per 128 rows, every
# 16-row block streams all of X); beyond, W is dequantised once and hipBLASLt runs the GEMM, as the reference does.  Measured
# (profiles/r04_gemm_kx8_shapes.log, 2x8 g8, hipGraph, us; fused / dequant + GEMM / dense fp16): 4096^2 at 16 / 128 / 256 rows
# 8.2 / 16.8 / 33.2 vs 36 / 41 / 41 vs 12.7 / 24.6 / 23.5; 4096 -> 11008 at 16 / 128 / 256 rows 18.0 / 41.8 / 79 vs 53 / 60 / 79.
FUSED_KX8_MFMA_MAX_ROWS = 128         # any layer
FUSED_KX8_MFMA_MAX_ROWS_SMALL = 256   # layers of <= 4096 x 4096
USE_FUSED_KX8_MFMA = True
USE_FUSED_KX8_KSPLIT = True   # False: never hand the fused op a workspace (no K split; A/B runs)


def _fused_kx8_mfma(input, codes, codebooks, scales, bias, dt):
    """The fused dequant -> MFMA kernel for 1x8 g8 / 2x8 g8 (W never materialised), or None when the call is outside it."""
    K, size, og, g = codebooks.shape
    if not USE_FUSED_KX8_MFMA or K not in (1, 2) or size != 256 or og != 1 or g != 8 or codes.dtype != torch.int8:
        return None
    in_features = codes.shape[1] * g
    if in_features % 128 != 0 or in_features < 384 or input.shape[-1] != in_features:
        return None
    if codebooks.dtype != input.dtype or scales.dtype != input.dtype or (bias is not None and bias.dtype != input.dtype):
        return None
    if not input.is_cuda or any(t is not None and t.device != input.device for t in (codes, codebooks, scales, bias)):
        return None  # (the dequantise + GEMM route raises torch's own device-mismatch error)
    x = _flat_rows(input)
    B = x.shape[0]
    out_features = codes.shape[0]
    if B < 1 or B > (FUSED_KX8_MFMA_MAX_ROWS_SMALL if out_features * in_features <= (1 << 24) else FUSED_KX8_MFMA_MAX_ROWS):
        return None
    codes, codebooks, scales = _c(codes), _c(codebooks), _c(scales)
    if bias is not None:
        bias = _c(bias)
    y = torch.empty((B, out_features), dtype=input.dtype, device=input.device)
    # 49+ rows: fp32 partials for the K-split form (two row tiles per block, the K range dealt to 2 / 4 blocks: every CU pulls half /
    # a quarter of X through its L1); below, and when the plan does not split, the workspace is not touched
    ws_bytes = _lib.aqlm_hip_workspace_bytes(_native.OP_GEMM_KX8_MFMA, B, out_features, in_features) if USE_FUSED_KX8_KSPLIT else 0
    stream = _stream_ptr(input.device)
    ws = _workspace(input.device, ws_bytes, stream) if ws_bytes else None
    with _device_guard(input.device):
        rc = _lib.aqlm_hip_gemm_kx8_mfma_ws(codes.data_ptr(), codebooks.data_ptr(), scales.data_ptr(), _ptr(bias), x.data_ptr(), y.data_ptr(),
                                            B, out_features, in_features, K, g, x.stride(0), out_features, dt,
                                            ws.data_ptr() if ws is not None else None, ws_bytes, stream)
    if rc == _native.E_UNSUPPORTED:
        return None
    if rc:
        _native.check(rc, "aqlm gemm_kx8_mfma")
    return y.reshape(input.shape[:-1] + (out_features,))


# 8x8 g32 beyond one row (aqlm_hip_gemm_8x8_mfma, round 5): the codebooks in LDS, one MFMA per codebook and k-step, cost independent
# of the number of rows up to 16 and +8 MFMAs per k-step for every further 16.  Below fused_8x8_min_rows(layer) rows the look-up-table
# matvec (one set of workgroups per row) is faster; above FUSED_8X8_MFMA_MAX_ROWS W is dequantised once and hipBLASLt runs the GEMM,
# as the reference does.  Numerics: exact products, fp32 sums (the table kernel: the same terms in another order).
USE_FUSED_8X8_MFMA = True
FUSED_8X8_MFMA_MIN_ROWS = 0   # 0 = by the measured cost model below (fused_8x8_min_rows); n > 0 = from n rows on, whatever the layer
FUSED_8X8_MFMA_MAX_ROWS = 64    # one slab; two slabs (128 rows) cost what dequantise + GEMM costs (4096^2: 44 vs 47 us; 4096 -> 11008: 104 vs 84)


def fused_8x8_min_rows(out_features: int, in_features: int) -> int:
    """Rows from which the fused MFMA kernel beats the look-up-table matvec on an 8x8 g32 layer.  Both times are affine in what
    they scale with (profiles/r05_gemm_8x8_mfma.log, r05_mb_lutrows.log; us, MI355X): the fused kernel costs 3.6 + 2.15 per round
    of 256 sixteen-row tiles and 1024 input features, whatever the rows (<= 16); the table kernel 1.3 + rows x (3.7 + 0.05 per
    million weights).  4096 x 4096: 3 rows; 4096 -> 11008 and 8192 x 8192: 5; 11008 -> 4096: 4.
    The comparison is with what the operator can run INSTEAD -- the table kernel -- not with not quantising: on the MLP shapes the fused
    kernel is faster than the table kernel from these row counts on and still slower than a dense fp16 GEMM (4096 -> 11008: 28.4 us for
    5..16 rows against 19.8-20.1 dense, 8192 x 8192 35 against 29-30; at 4096 x 4096 12.2 against 12.8; bench.py
    `detail.small_batch_rows_8x8g32` prints `dense_fp16_us` beside every count, profiles/r05_gemm_8x8_mfma_pmc.json has the reason: 54 %
    of the kernel's LDS cycles are bank conflicts of the codebook gathers).  A deployment that prefers speed to memory at those batch
    sizes has `prefer_dense_below_rows`."""
    if FUSED_8X8_MFMA_MIN_ROWS > 0:
        return FUSED_8X8_MFMA_MIN_ROWS
    tiles = (out_features + 15) // 16
    rounds = (tiles + 255) // 256
    fused = 3.6 + 2.15 * rounds * in_features / 1024.0
    per_row = 3.7 + 0.05 * out_features * in_features * 1e-6
    return max(2, int((fused - 1.3) / per_row) + 1)


def _fused_8x8_mfma(input, codes, codebooks, scales, bias, dt):
    """The fused dequant -> MFMA kernel for 8x8 g32 on checkpoint-layout codes (W never materialised), or None when the call is
    outside it."""
    K, size, og, g = codebooks.shape
    if not USE_FUSED_8X8_MFMA or K != 8 or size != 256 or og != 1 or g != 32 or codes.dtype != torch.int8 or codes.dim() != 3:
        return None
    in_features = codes.shape[1] * g
    if in_features % 256 != 0 or in_features < 2048 or input.shape[-1] != in_features:
        return None
    if codebooks.dtype != input.dtype or scales.dtype != input.dtype or (bias is not None and bias.dtype != input.dtype):
        return None
    if not input.is_cuda or any(t is not None and t.device != input.device for t in (codes, codebooks, scales, bias)):
        return None
    x = _flat_rows(input)
    B = x.shape[0]
    out_features = codes.shape[0]
    if B < 1 or B > FUSED_8X8_MFMA_MAX_ROWS:
        return None
    codes, codebooks, scales = _c(codes), _c(codebooks), _c(scales)
    if bias is not None:
        bias = _c(bias)
    y = torch.empty((B, out_features), dtype=input.dtype, device=input.device)
    with _device_guard(input.device):
        rc = _lib.aqlm_hip_gemm_8x8_mfma(codes.data_ptr(), codebooks.data_ptr(), scales.data_ptr(), _ptr(bias), x.data_ptr(), y.data_ptr(),
                                         B, out_features, in_features, g, x.stride(0), out_features, dt, _stream_ptr(input.device))
    if rc == _native.E_UNSUPPORTED:
        return None
    if rc:
        _native.check(rc, "aqlm gemm_8x8_mfma")
    return y.reshape(input.shape[:-1] + (out_features,))


def code2x8_matmat_dequant(input, codes, codebooks, scales, bias=None):
    return _matmat_dequant_kx8(input, codes, codebooks, scales, bias)


def code1x8_matmat_dequant(input, codes, codebooks, scales, bias=None):
    return _matmat_dequant_kx8(input, codes, codebooks, scales, bias)


def _matmat_dequant_transposed(input, codes, codebooks, scales, bias, kind):
    """grad_input = (grad_output * scales) @ W  (+ bias): backward of the linear layer
    (cuda_kernel.cpp:303-354; generic definition kernel_selector.py:145-161)."""
    _dtype_id(input)
    W = _dequant(codes, codebooks, scales, kind)  # scales folded into W rows == scaling grad_output columns
    out = torch.matmul(input, W)
    if bias is not None:
        out = out + bias
    return out


def generic_dequant(codes, codebooks, scales):
    """W[out, in] for any scheme (aqlm_hip_dequant_generic) -- the reference's `_dequantize_weight` (utils.py:43-70)."""
    return _dequant(codes, codebooks, scales.reshape(-1) if scales is not None else None, "generic")


def generic_matmat_dequant(input, codes, codebooks, scales, bias=None):
    """Large-batch forward of a scheme without a tuned kernel: generic dequant + library GEMM (dequantize_gemm,
    dequantization.py:9-21).  W is kept unscaled (exact); y is scaled afterwards."""
    _dtype_id(input)
    W = _dequant(codes, codebooks, None, "generic")
    return _scale_bias_fp32(F.linear(input, W), scales, bias)


def generic_matmat_dequant_transposed(input, codes, codebooks, scales, bias=None):
    """Backward of any scheme: grad_input = (grad_output * scales) @ W (kernel_selector.py:145-161)."""
    return _matmat_dequant_transposed(input, codes, codebooks, scales, bias, "generic")


def code1x16_matmat_dequant_transposed(input, codes, codebooks, scales, bias=None):
    return _matmat_dequant_transposed(input, codes, codebooks, scales, bias, "1x16")


def code2x8_matmat_dequant_transposed(input, codes, codebooks, scales, bias=None):
    return _matmat_dequant_transposed(input, codes, codebooks, scales, bias, "kx8")


def code1x8_matmat_dequant_transposed(input, codes, codebooks, scales, bias=None):
    return _matmat_dequant_transposed(input, codes, codebooks, scales, bias, "kx8")


# ------------------------------------------------------------------------------------------------------
# registration: same names + schemas as cuda_kernel.py:13-132 (bias declared optional, which is what the
# reference's C++ signature std::optional<torch::Tensor> actually accepts)
# ------------------------------------------------------------------------------------------------------
_SCHEMA = "(Tensor input, Tensor codes, Tensor codebooks, Tensor scales, Tensor? bias) -> Tensor"


def _fake_forward(input, codes, codebooks, scales, bias=None):
    return torch.empty(input.shape[:-1] + (codes.shape[0],), device=input.device, dtype=input.dtype)


def _fake_transposed(input, codes, codebooks, scales, bias=None):
    return torch.empty(input.shape[:-1] + (codes.shape[1] * codebooks.shape[3],), device=input.device, dtype=input.dtype)


_OPS = {
    "code1x16_matmat": (code1x16_matmat, _fake_forward),
    "code1x16_matmat_dequant": (code1x16_matmat_dequant, _fake_forward),
    "code1x16_matmat_dequant_transposed": (code1x16_matmat_dequant_transposed, _fake_transposed),
    "code2x8_matmat": (code2x8_matmat, _fake_forward),
    "code2x8_matmat_dequant": (code2x8_matmat_dequant, _fake_forward),
    "code2x8_matmat_dequant_transposed": (code2x8_matmat_dequant_transposed, _fake_transposed),
    "code1x8_matmat": (code1x8_matmat, _fake_forward),
    "code1x8_matmat_dequant": (code1x8_matmat_dequant, _fake_forward),
    "code1x8_matmat_dequant_transposed": (code1x8_matmat_dequant_transposed, _fake_transposed),
    # additions (no reference counterpart: the reference sends these schemes to Triton)
    "codekx8_matmat": (codekx8_matmat, _fake_forward),
    "generic_matmat": (generic_matmat, _fake_forward),
    "generic_matmat_dequant": (generic_matmat_dequant, _fake_forward),
    "generic_matmat_dequant_transposed": (generic_matmat_dequant_transposed, _fake_transposed),
}

# the three reference matvec ops get compiled kernels when the front end is built (front.cpp: decode calls are launched from
# C++, everything else comes back to the functions above); without it the functions above ARE the kernels
_RAW_FAST_NAMES = ("code1x16_matmat", "code2x8_matmat", "code1x8_matmat")
from .. import _front  # noqa: E402

_compiled_raw = _front.available() and hasattr(_front.ext, "raw_install") and os.environ.get("AQLM_AMD_NO_RAW_FRONT", "0") != "1"
for _name, (_impl, _fake) in _OPS.items():
    _LIB.define(f"{_name}{_SCHEMA}")
    if not (_compiled_raw and _name in _RAW_FAST_NAMES):
        _LIB.impl(_name, _impl, "CUDA")
    torch.library.register_fake(f"aqlm::{_name}")(_fake)
if _compiled_raw:
    _front.ext.raw_install(code1x16_matmat, code2x8_matmat, code1x8_matmat)
    _RAW_FAST = _front.ext
    _raw_sync_config()

# shared-input launch (no reference counterpart)
def _fake_multi(input, codes, codebooks, scales, bias):
    return [torch.empty(input.shape[:-1] + (c.shape[0],), device=input.device, dtype=input.dtype) for c in codes]


for _name, _impl in (("code1x16_matmat_multi", code1x16_matmat_multi), ("codekx8_matmat_multi", codekx8_matmat_multi)):
    register_op(_name, "(Tensor input, Tensor[] codes, Tensor[] codebooks, Tensor[] scales, Tensor?[] bias) -> Tensor[]", _impl,
                _fake_multi)


# the prepacked op as a dispatcher op, so that a QuantizedLinear on the packed path traces under torch.compile
# (the descriptor travels as a list of ints; eager calls skip the dispatcher and use code1x16_matmat_packed directly)
_N_DESC_INTS = 17


def _packed_op(input, packed, codebooks, scales, bias, desc):
    pk = PackedCodes(packed, _native.PackedDesc.from_ints(desc[:_N_DESC_INTS]))
    now = (codebooks.data_ptr(), tensor_version(codebooks))
    if len(desc) >= _N_DESC_INTS + 2:
        # the descriptor says which codebook its range (and a relabelled buffer's codebook image) came from: anything else is
        # refreshed by code1x16_matmat_packed -> refresh_range (outside a capture; inside one the stale range means the two-kernel
        # form, and a stale image is refused with a message)
        pk._range_of = now if (int(desc[_N_DESC_INTS]), int(desc[_N_DESC_INTS + 1])) == now else (0, -2)
    else:
        pk._range_of = now  # (descriptors without a fingerprint are taken at their word: 0 = unknown range)
    return code1x16_matmat_packed(input, pk, codebooks, scales, bias)


def _fake_packed(input, packed, codebooks, scales, bias, desc):
    return torch.empty(input.shape[:-1] + (int(desc[2]),), device=input.device, dtype=input.dtype)


register_op("code1x16_matmat_packed", "(Tensor input, Tensor packed, Tensor codebooks, Tensor scales, Tensor? bias, "
            "int[] desc) -> Tensor", _packed_op, _fake_packed)


# W from a packed buffer as a dispatcher op (the packed-dequant routes of QuantizedLinear under torch.compile)
def _packed_dequant_op(packed, codebooks, scales, desc):
    return dequant_1x16_packed(PackedCodes(packed, _native.PackedDesc.from_ints(desc[:_N_DESC_INTS])), codebooks, scales)


def _fake_packed_dequant(packed, codebooks, scales, desc):
    return torch.empty((int(desc[2]), int(desc[3])), device=codebooks.device, dtype=codebooks.dtype)


register_op("code1x16_dequant_packed", "(Tensor packed, Tensor codebooks, Tensor? scales, int[] desc) -> Tensor", _packed_dequant_op,
            _fake_packed_dequant)


# the planar 8x8 matvec as a dispatcher op (same reason; geometry = [out_features, in_features, in_group_size], the codebook bound
# travels as a float: 0 = unknown -> the two-kernel form)
def _planar_op(input, planar, codebooks, scales, bias, geometry, codebook_absmax):
    pl = PlanarCodes(planar, int(geometry[0]), int(geometry[1]), int(geometry[2]))
    pl.codebook_absmax = float(codebook_absmax)
    pl._range_of = (codebooks.data_ptr(), tensor_version(codebooks))  # the caller's bound is taken at its word
    return code8x8_matmat_planar(input, pl, codebooks, scales, bias)


def _fake_planar(input, planar, codebooks, scales, bias, geometry, codebook_absmax):
    return torch.empty(input.shape[:-1] + (int(geometry[0]),), device=input.device, dtype=input.dtype)


register_op("code8x8_matmat_planar", "(Tensor input, Tensor planar, Tensor codebooks, Tensor scales, Tensor? bias, int[] geometry, "
            "float codebook_absmax) -> Tensor", _planar_op, _fake_planar)


# what benchmark/matmul_benchmark.py:6,103 reaches for: CUDA_KERNEL.code1x16_matmat etc. (pybind module in the
# reference, cuda_kernel.cpp:686-699)
HIP_KERNEL = SimpleNamespace(
    code1x16_matmat=code1x16_matmat,
    code1x16_dequant=code1x16_dequant,
    code1x16_matmat_dequant=code1x16_matmat_dequant,
    code1x16_matmat_dequant_transposed=code1x16_matmat_dequant_transposed,
    code2x8_matmat=code2x8_matmat,
    code2x8_dequant=code2x8_dequant,
    code2x8_matmat_dequant=code2x8_matmat_dequant,
    code2x8_matmat_dequant_transposed=code2x8_matmat_dequant_transposed,
    code1x8_matmat=code1x8_matmat,
    code1x8_dequant=code1x8_dequant,
    code1x8_matmat_dequant=code1x8_matmat_dequant,
    code1x8_matmat_dequant_transposed=code1x8_matmat_dequant_transposed,
    codekx8_matmat=codekx8_matmat,
    generic_matmat=generic_matmat,
    generic_dequant=generic_dequant,
    generic_matmat_dequant=generic_matmat_dequant,
    generic_matmat_dequant_transposed=generic_matmat_dequant_transposed,
    code1x16_matmat_multi=code1x16_matmat_multi,
    codekx8_matmat_multi=codekx8_matmat_multi,
)
if _RAW_FAST is not None:  # the compiled functions, as in the reference's pybind module (the Python ones above remain their fallback)
    HIP_KERNEL.code1x16_matmat = _RAW_FAST.code1x16_matmat
    HIP_KERNEL.code2x8_matmat = _RAW_FAST.code2x8_matmat
    HIP_KERNEL.code1x8_matmat = _RAW_FAST.code1x8_matmat
CUDA_KERNEL = HIP_KERNEL


# ------------------------------------------------------------------------------------------------------
# the op families: each module registers its own aqlm:: ops on import; every name it defines is re-exported here as the same object
# (tests/test_hip_kernel_layout_host.py holds the lists to the modules)
# ------------------------------------------------------------------------------------------------------
from .ops_moe import (  # noqa: E402, F401
    _MOE_SCHEMA, _ROUTED_PACKED_CELLS, ROUTED_PACKED_GEOMETRY_INTS, _bucket_words, _check_grouped_args, _check_routed_args,
    _desc_array, _fake_bucket, _fake_grouped, _fake_grouped_transposed, _fake_moe, _routed_launches, code1x16_moe_matmat,
    code1x16_moe_matmat_grouped, code1x16_moe_matmat_grouped_transposed, code1x16_moe_matmat_packed, grouped_supported,
    grouped_tile_pairs, grouped_transposed_supported, moe_bucket, release_routed_packed_cells, routed_chunks, routed_packed_cells,
    routed_packed_supported, routed_packed_table, routed_table,
)
from .ops_lora import (  # noqa: E402, F401
    _LORA_GMV_SCHEMA, SGMV_ROUTED_TILE_PAIRS, _check_lora_routed, _fake_lora_bgmv, _lora_gmv_, lora_bgmv_, lora_bgmv_routed_,
    lora_bgmv_routed_supported, lora_bgmv_supported, lora_grad_routed, lora_grad_routed_supported, lora_routed_table,
    lora_routed_transposed_layout, lora_routed_transposed_table, lora_sgmv_, lora_sgmv_routed_, lora_sgmv_routed_supported,
    lora_sgmv_routed_workspace_floats, lora_sgmv_splits, lora_sgmv_supported, lora_table, lora_transpose_routed_,
    lora_transpose_routed_supported,
)
from .ops_grad import (  # noqa: E402, F401
    CODEBOOK_GRAD_CHUNK, CODEBOOK_GRAD_ENTRIES, CodebookGradIndex, _calib_layer, _calib_scales, _check_calib_matrix, _check_dw,
    _check_kx8_codes, _check_scales, _codebook_grad_kx8_op, _codebook_grad_op, _scales_grad_kx8_op, _scales_grad_op,
    build_codebook_grad_index, calib_codebook_grad_1x16, calib_codebook_grad_kx8, calib_delta, calib_rows, calib_supported,
    codebook_grad_1x16, codebook_grad_kx8, codebook_grad_kx8_supported, codebook_grad_max_chunks, codebook_grad_supported,
    scales_grad_1x16, scales_grad_kx8,
)
from .ops_search import (  # noqa: E402, F401
    CODE_SEARCH_1X16_XTX_MAX_BEAM, CODE_SEARCH_EPS, CODE_SEARCH_KX8_MAX_BEAM, KMEANS_EPS, XtxStep, _aligned16,
    _code_search_1x16_impl, _code_search_1x16_op, _code_search_kx8_impl, _code_search_kx8_op, _dim_order, _fake_code_search_kx8,
    _fake_kmeans_assign, _kmeans_assign_op, _kmeans_operands, code_search_1x16, code_search_1x16_supported,
    code_search_1x16_xtx_step, code_search_1x16_xtx_supported, code_search_kx8, code_search_kx8_supported,
    code_search_kx8_xtx_step, code_search_kx8_xtx_supported, kmeans_assign, kmeans_supported, kmeans_update, kmeans_update_,
)

# two private names of the former registration block, for anything that reached them in this namespace
_GRAD_FAKE_DT = _GRAD_TORCH_DT
_lora_grad_routed_op = lora_grad_routed
