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
"""
from __future__ import annotations

import contextlib
import ctypes
import os
from types import SimpleNamespace
from typing import NamedTuple, Optional

import torch
import torch.nn.functional as F

from .. import _native
from .._native import lib as _lib
from ..derived import tensor_checksum, tensor_version

_version = tensor_version  # the name the tests reach

HIP_FOLDER = os.path.dirname(os.path.abspath(_native.LIB_PATH))
CUDA_FOLDER = HIP_FOLDER  # reference name (cuda_kernel.py:6); ROCm reports device type "cuda"

_DT = {torch.float16: _native.F16, torch.bfloat16: _native.BF16}


def _dtype_id(t: torch.Tensor) -> int:
    try:
        return _DT[t.dtype]
    except KeyError:
        # message mirrors check_use_bfloat16 (cuda_kernel.cpp:9-25)
        raise NotImplementedError(
            f"AQLM HIP kernels only support float16 and bfloat16. Got {t.dtype}. "
            "Please specify the correct `torch_dtype` when loading the model."
        ) from None


def _stream_ptr(device=None) -> int:
    """The current stream of ``device`` (default: the current device).  Always pass the tensor's device when the call
    is not inside ``torch.cuda.device(...)``: with accelerate's device_map the current device is not the layer's."""
    return torch.cuda.current_stream(device).cuda_stream


_NO_GUARD = contextlib.nullcontext()


def _device_guard(device: torch.device):
    """``torch.cuda.device(device)`` only when the tensor is not on the current device: an eager decode loop is host-bound
    and entering / leaving the guard costs as much as a kernel launch."""
    return _NO_GUARD if torch.cuda.current_device() == device.index else torch.cuda.device(device)


def _c(t: torch.Tensor) -> torch.Tensor:
    return t if t.is_contiguous() else t.contiguous()


def _flat_rows(input: torch.Tensor) -> torch.Tensor:
    x = input.reshape(-1, input.shape[-1])
    if x.stride(-1) != 1 or (x.shape[0] > 1 and x.stride(0) % 8 != 0) or x.data_ptr() % 16 != 0:
        x = x.contiguous()
    return x


def _ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


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


# fp32 partial workspaces, one per (device, stream): a decode loop calls the packed op hundreds of times per token and
# the allocator round trip is a measurable part of an eager call.  Not used while a hipGraph is being captured (the
# capture's private pool must own what the graph touches).
_WORKSPACES = {}


def _workspace(device: torch.device, nbytes: int, stream: Optional[int] = None) -> torch.Tensor:
    if torch.cuda.is_current_stream_capturing():
        return torch.empty((nbytes // 4,), dtype=torch.float32, device=device)
    key = (device.index, torch.cuda.current_stream(device).cuda_stream if stream is None else stream)
    ws = _WORKSPACES.get(key)
    if ws is None or ws.numel() * 4 < nbytes:
        ws = torch.empty((max(nbytes, 1 << 20) // 4,), dtype=torch.float32, device=device)
        _WORKSPACES[key] = ws
    return ws


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


# ------------------------------------------------------------------------------------------------------
# gradients of the codebook and the scales of a 1x16 layer (aqlm_hip_codebook_grad_1x16, aqlm_hip_scales_grad_1x16)
# ------------------------------------------------------------------------------------------------------
CODEBOOK_GRAD_CHUNK = int(_lib.aqlm_hip_codebook_grad_chunk())  # positions per chunk of an entry's list (a constant of the library)
CODEBOOK_GRAD_ENTRIES = 65536
_GRAD_DT = {torch.float16: _native.F16, torch.bfloat16: _native.BF16, torch.float32: _native.F32}


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
        if scales.numel() != out_features or scales.device != dw.device:
            raise ValueError(f"codebook_grad_1x16: scales must hold {out_features} elements on {dw.device}")
        dt = _dtype_id(scales)
        scales = _c(scales)
    out_dtype = {v: k for k, v in _GRAD_DT.items()}[out_dt]
    out = torch.empty((CODEBOOK_GRAD_ENTRIES, g), dtype=out_dtype, device=dw.device)
    ws_bytes = int(_lib.aqlm_hip_codebook_grad_1x16_workspace_bytes(out_features, in_features, g))
    ws = _workspace(dw.device, max(ws_bytes, 16))
    with _device_guard(dw.device):
        rc = _lib.aqlm_hip_codebook_grad_1x16(dw.data_ptr(), dw.stride(0), _GRAD_DT[dw.dtype], _ptr(scales), dt, starts.data_ptr(),
                                              order.data_ptr(), chunks.data_ptr(), chunk_starts.data_ptr(), out_features, in_features,
                                              g, out.data_ptr(), out_dt, ws.data_ptr(), ws.numel() * 4, _stream_ptr(dw.device))
    if rc:
        _native.check(rc, "aqlm codebook grad")
    return out


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
    out_dtype = {v: k for k, v in _GRAD_DT.items()}[out_dt]
    out = torch.empty((out_features,), dtype=out_dtype, device=dw.device)
    with _device_guard(dw.device):
        rc = _lib.aqlm_hip_scales_grad_1x16(dw.data_ptr(), dw.stride(0), _GRAD_DT[dw.dtype], codes.data_ptr(), codebooks.data_ptr(), dt,
                                            out_features, in_features, g, out.data_ptr(), out_dt, _stream_ptr(dw.device))
    if rc:
        _native.check(rc, "aqlm scales grad")
    return out


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
        if scales.numel() != out_features or scales.device != dw.device:
            raise ValueError(f"codebook_grad_kx8: scales must hold {out_features} elements on {dw.device}")
        dt = _dtype_id(scales)
        scales = _c(scales)
    out_dtype = {v: k for k, v in _GRAD_DT.items()}[out_dt]
    out = torch.empty((K, 256, g), dtype=out_dtype, device=dw.device)
    ws_bytes = int(_lib.aqlm_hip_codebook_grad_kx8_workspace_bytes(out_features, in_features, K, g))
    ws = _workspace(dw.device, max(ws_bytes, 16))
    with _device_guard(dw.device):
        rc = _lib.aqlm_hip_codebook_grad_kx8(dw.data_ptr(), dw.stride(0), _GRAD_DT[dw.dtype], _ptr(scales), dt, codes.data_ptr(),
                                             out_features, in_features, K, g, out.data_ptr(), out_dt, ws.data_ptr(), ws.numel() * 4,
                                             _stream_ptr(dw.device))
    if rc:
        _native.check(rc, "aqlm codebook grad kx8")
    return out


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
    out_dtype = {v: k for k, v in _GRAD_DT.items()}[out_dt]
    out = torch.empty((out_features,), dtype=out_dtype, device=dw.device)
    with _device_guard(dw.device):
        rc = _lib.aqlm_hip_scales_grad_kx8(dw.data_ptr(), dw.stride(0), _GRAD_DT[dw.dtype], codes.data_ptr(), codebooks.data_ptr(), dt,
                                           out_features, in_features, K, g, out.data_ptr(), out_dt, _stream_ptr(dw.device))
    if rc:
        _native.check(rc, "aqlm scales grad kx8")
    return out


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
        if scales.numel() != out_features or scales.dtype != torch.float32 or scales.device != codebooks.device:
            raise ValueError(f"{who}: scales must hold {out_features} fp32 elements on {codebooks.device}")
        scales = _c(scales.detach()).reshape(-1)
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
    if scales.numel() != o or scales.dtype != torch.float32 or scales.device != g_matrix.device:
        raise ValueError(f"calib_codebook_grad_1x16: scales must hold {o} fp32 elements on {g_matrix.device}")
    scales = _c(scales.detach()).reshape(-1)
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
    if scales.numel() != o or scales.dtype != torch.float32 or scales.device != g_matrix.device:
        raise ValueError(f"calib_codebook_grad_kx8: scales must hold {o} fp32 elements on {g_matrix.device}")
    scales = _c(scales.detach()).reshape(-1)
    out = torch.empty((K, 256, g), dtype=torch.float32, device=g_matrix.device)
    ws_bytes = int(_lib.aqlm_hip_calib_codebook_grad_kx8_workspace_bytes(o, i, K, g))
    ws = _workspace(g_matrix.device, max(ws_bytes, 16))
    with _device_guard(g_matrix.device):
        rc = _lib.aqlm_hip_calib_codebook_grad_kx8(g_matrix.data_ptr(), g_matrix.stride(0), scales.data_ptr(), codes.data_ptr(), o, i, K, g,
                                                   out.data_ptr(), ws.data_ptr(), ws.numel() * 4, _stream_ptr(g_matrix.device))
    if rc:
        _native.check(rc, "aqlm calib codebook grad kx8")
    return out


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


# ------------------------------------------------------------------------------------------------------
# expert-routed matvec on PREPACKED experts (mixture-of-experts decode; aqlm_hip_gemv_1x16_routed_packed)
# ------------------------------------------------------------------------------------------------------
ROUTED_PACKED_GEOMETRY_INTS = 11  # [E, S, out, in, g, top_k] + rows_per_group, max_waves, slice_first, lds_bytes, table words


def _desc_array(packed_list):
    return (_native._descp * len(packed_list))(*[ctypes.pointer(p.desc) for p in packed_list])


def routed_packed_supported(packed_list) -> bool:
    """Will aqlm_hip_gemv_1x16_routed_packed serve a table of these ``PackedCodes`` (one shape; 4-byte entries, uniform geometry, a
    codebook range each)?  A host query on the descriptors."""
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
_LIB = torch.library.Library("aqlm", "DEF")


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
    _LIB.define(f"{_name}(Tensor input, Tensor[] codes, Tensor[] codebooks, Tensor[] scales, Tensor?[] bias) -> Tensor[]")
    _LIB.impl(_name, _impl, "CUDA")
    torch.library.register_fake(f"aqlm::{_name}")(_fake_multi)


# expert-routed matvec (mixture-of-experts decode; no reference counterpart)
def _fake_moe(input, expert_ids, table, geometry, x_per_pair):
    return input.new_empty((expert_ids.shape[0] * expert_ids.shape[1], int(geometry[1]), int(geometry[2])))


_LIB.define("code1x16_moe_matmat(Tensor input, Tensor expert_ids, Tensor table, int[] geometry, bool x_per_pair) -> Tensor")
_LIB.impl("code1x16_moe_matmat", code1x16_moe_matmat, "CUDA")
torch.library.register_fake("aqlm::code1x16_moe_matmat")(_fake_moe)


_LIB.define("code1x16_moe_matmat_packed(Tensor input, Tensor expert_ids, Tensor table, int[] geometry, bool x_per_pair) -> Tensor")
_LIB.impl("code1x16_moe_matmat_packed", code1x16_moe_matmat_packed, "CUDA")
torch.library.register_fake("aqlm::code1x16_moe_matmat_packed")(_fake_moe)


# per-row LoRA adapters on top of a layer's output (no reference counterpart); mutates y, returns nothing
def _fake_lora_bgmv(y, x, ids, table, geometry):
    return None


_LIB.define("lora_bgmv_(Tensor(a!) y, Tensor x, Tensor? ids, Tensor table, int[] geometry) -> ()")
_LIB.impl("lora_bgmv_", lora_bgmv_, "CUDA")
torch.library.register_fake("aqlm::lora_bgmv_")(_fake_lora_bgmv)

_LIB.define("lora_bgmv_routed_(Tensor(a!) y, Tensor x, Tensor? adapter_ids, Tensor expert_ids, Tensor table, int[] geometry, "
            "bool x_per_pair) -> ()")
_LIB.impl("lora_bgmv_routed_", lora_bgmv_routed_, "CUDA")
torch.library.register_fake("aqlm::lora_bgmv_routed_")(lambda y, x, adapter_ids, expert_ids, table, geometry, x_per_pair: None)

_LIB.define("lora_sgmv_(Tensor(a!) y, Tensor x, Tensor? ids, Tensor table, int[] geometry) -> ()")
_LIB.impl("lora_sgmv_", lora_sgmv_, "CUDA")
torch.library.register_fake("aqlm::lora_sgmv_")(_fake_lora_bgmv)

_LIB.define("lora_sgmv_routed_(Tensor(a!) y, Tensor x, Tensor? adapter_ids, Tensor expert_ids, Tensor bucket, Tensor table, "
            "int[] geometry, bool x_per_pair) -> ()")
_LIB.impl("lora_sgmv_routed_", lora_sgmv_routed_, "CUDA")
torch.library.register_fake("aqlm::lora_sgmv_routed_")(
    lambda y, x, adapter_ids, expert_ids, bucket, table, geometry, x_per_pair: None)


# the backward of the routed adapters: the transposed copies (mutates buffer) and the reduction both weight gradients are
_LIB.define("lora_transpose_routed_(Tensor(a!) buffer, Tensor table, Tensor transposed, int[] geometry) -> ()")
_LIB.impl("lora_transpose_routed_", lora_transpose_routed_, "CUDA")
torch.library.register_fake("aqlm::lora_transpose_routed_")(lambda buffer, table, transposed, geometry: None)


def _lora_grad_routed_op(v, w, adapter_ids, expert_ids, bucket, table, geometry, layout):
    return lora_grad_routed(v, w, adapter_ids, expert_ids, bucket, table, geometry, layout)


_LIB.define("lora_grad_routed(Tensor v, Tensor w, Tensor? adapter_ids, Tensor expert_ids, Tensor bucket, Tensor table, "
            "int[] geometry, int[] layout) -> Tensor")
_LIB.impl("lora_grad_routed", _lora_grad_routed_op, "CUDA")
torch.library.register_fake("aqlm::lora_grad_routed")(
    lambda v, w, adapter_ids, expert_ids, bucket, table, geometry, layout: v.new_empty(
        (int(geometry[1]), int(geometry[2]), int(geometry[3]), int(geometry[4])), dtype=torch.float32))


# gradients of the codebook and the scales of a 1x16 layer; geometry = [out_features, in_features, g, output dtype id]
_GRAD_FAKE_DT = {_native.F16: torch.float16, _native.BF16: torch.bfloat16, _native.F32: torch.float32}
_LIB.define("codebook_grad_1x16(Tensor dw, Tensor? scales, Tensor starts, Tensor order, Tensor chunks, Tensor chunk_starts, "
            "int[] geometry) -> Tensor")
_LIB.impl("codebook_grad_1x16", _codebook_grad_op, "CUDA")
torch.library.register_fake("aqlm::codebook_grad_1x16")(
    lambda dw, scales, starts, order, chunks, chunk_starts, geometry: dw.new_empty(
        (CODEBOOK_GRAD_ENTRIES, int(geometry[2])), dtype=_GRAD_FAKE_DT[int(geometry[3])]))
_LIB.define("scales_grad_1x16(Tensor dw, Tensor codes, Tensor codebooks, int[] geometry) -> Tensor")
_LIB.impl("scales_grad_1x16", _scales_grad_op, "CUDA")
torch.library.register_fake("aqlm::scales_grad_1x16")(
    lambda dw, codes, codebooks, geometry: dw.new_empty((int(geometry[0]),), dtype=_GRAD_FAKE_DT[int(geometry[3])]))
# ... of a K x 8 layer; geometry = [out_features, in_features, K, g, output dtype id]
_LIB.define("codebook_grad_kx8(Tensor dw, Tensor? scales, Tensor codes, int[] geometry) -> Tensor")
_LIB.impl("codebook_grad_kx8", _codebook_grad_kx8_op, "CUDA")
torch.library.register_fake("aqlm::codebook_grad_kx8")(
    lambda dw, scales, codes, geometry: dw.new_empty((int(geometry[2]), 256, int(geometry[3])), dtype=_GRAD_FAKE_DT[int(geometry[4])]))
_LIB.define("scales_grad_kx8(Tensor dw, Tensor codes, Tensor codebooks, int[] geometry) -> Tensor")
_LIB.impl("scales_grad_kx8", _scales_grad_kx8_op, "CUDA")
torch.library.register_fake("aqlm::scales_grad_kx8")(
    lambda dw, codes, codebooks, geometry: dw.new_empty((int(geometry[0]),), dtype=_GRAD_FAKE_DT[int(geometry[4])]))

# nearest-codeword search of a 1x16 layer; geometry = [out_features, in_features, g]
_LIB.define("code_search_1x16(Tensor reference, Tensor? scales, Tensor codebook, Tensor? group_ids, int[] geometry) -> Tensor")
_LIB.impl("code_search_1x16", _code_search_1x16_op, "CUDA")
torch.library.register_fake("aqlm::code_search_1x16")(
    lambda reference, scales, codebook, group_ids, geometry: reference.new_empty(
        (int(group_ids.numel()) if group_ids is not None else int(geometry[0]) * (int(geometry[1]) // int(geometry[2])),), dtype=torch.int16))
# one Lloyd iteration of k-means: the assignment with the clusters' fixed-point sums, and the update of the centroids in place
_LIB.define("kmeans_assign(Tensor data, Tensor centroids, float data_absmax, bool with_sums) -> (Tensor, Tensor, Tensor)")
_LIB.impl("kmeans_assign", _kmeans_assign_op, "CUDA")


def _fake_kmeans_assign(data, centroids, data_absmax, with_sums):
    k, d = (int(centroids.shape[0]), int(centroids.shape[1])) if with_sums else (0, int(centroids.shape[1]))
    return (data.new_empty((data.shape[0],), dtype=torch.int32), data.new_empty((k, d), dtype=torch.int64),
            data.new_empty((k,), dtype=torch.int32))


torch.library.register_fake("aqlm::kmeans_assign")(_fake_kmeans_assign)
_LIB.define("kmeans_update_(Tensor(a!) centroids, Tensor sums, Tensor counts, int n, float data_absmax) -> ()")
_LIB.impl("kmeans_update_", kmeans_update_, "CUDA")
torch.library.register_fake("aqlm::kmeans_update_")(lambda centroids, sums, counts, n, data_absmax: None)

# beam search over the codebooks of a K x 8 layer; geometry = [out_features, in_features, K, g, beam_size] + dim_order (or nothing);
# returns the codes [n, K] int8 and the fp32 score of every returned hypothesis [n]
_LIB.define("code_search_kx8(Tensor reference, Tensor? scales, Tensor codebooks, Tensor prev_codes, Tensor? group_ids, int[] geometry)"
            " -> (Tensor, Tensor)")
_LIB.impl("code_search_kx8", _code_search_kx8_op, "CUDA")


def _fake_code_search_kx8(reference, scales, codebooks, prev_codes, group_ids, geometry):
    n = int(group_ids.numel()) if group_ids is not None else int(geometry[0]) * (int(geometry[1]) // int(geometry[3]))
    return reference.new_empty((n, int(geometry[2])), dtype=torch.int8), reference.new_empty((n,), dtype=torch.float32)


torch.library.register_fake("aqlm::code_search_kx8")(_fake_code_search_kx8)


# expert-grouped GEMM (mixture-of-experts prefill / training; no reference counterpart)
def _fake_bucket(expert_ids, num_experts, tile_pairs):
    return expert_ids.new_empty((_bucket_words(expert_ids.shape[0] * expert_ids.shape[1], num_experts, tile_pairs),),
                                dtype=torch.int32)


def _fake_grouped(input, bucket, table, geometry, x_per_pair):
    return input.new_empty((int(geometry[7]), int(geometry[1]), int(geometry[2])))


_LIB.define("moe_bucket(Tensor expert_ids, int num_experts, int tile_pairs) -> Tensor")
_LIB.impl("moe_bucket", moe_bucket, "CUDA")
torch.library.register_fake("aqlm::moe_bucket")(_fake_bucket)
_LIB.define("code1x16_moe_matmat_grouped(Tensor input, Tensor bucket, Tensor table, int[] geometry, bool x_per_pair) -> Tensor")
_LIB.impl("code1x16_moe_matmat_grouped", code1x16_moe_matmat_grouped, "CUDA")
torch.library.register_fake("aqlm::code1x16_moe_matmat_grouped")(_fake_grouped)



def _fake_grouped_transposed(grad_output, bucket, table, geometry):
    return grad_output.new_empty((int(geometry[7]), int(geometry[3])), dtype=torch.float32)


_LIB.define("code1x16_moe_matmat_grouped_transposed(Tensor grad_output, Tensor bucket, Tensor table, int[] geometry) -> Tensor")
_LIB.impl("code1x16_moe_matmat_grouped_transposed", code1x16_moe_matmat_grouped_transposed, "CUDA")
torch.library.register_fake("aqlm::code1x16_moe_matmat_grouped_transposed")(_fake_grouped_transposed)


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


_LIB.define("code1x16_matmat_packed(Tensor input, Tensor packed, Tensor codebooks, Tensor scales, Tensor? bias, "
            "int[] desc) -> Tensor")
_LIB.impl("code1x16_matmat_packed", _packed_op, "CUDA")
torch.library.register_fake("aqlm::code1x16_matmat_packed")(_fake_packed)


# W from a packed buffer as a dispatcher op (the packed-dequant routes of QuantizedLinear under torch.compile)
def _packed_dequant_op(packed, codebooks, scales, desc):
    return dequant_1x16_packed(PackedCodes(packed, _native.PackedDesc.from_ints(desc[:_N_DESC_INTS])), codebooks, scales)


def _fake_packed_dequant(packed, codebooks, scales, desc):
    return torch.empty((int(desc[2]), int(desc[3])), device=codebooks.device, dtype=codebooks.dtype)


_LIB.define("code1x16_dequant_packed(Tensor packed, Tensor codebooks, Tensor? scales, int[] desc) -> Tensor")
_LIB.impl("code1x16_dequant_packed", _packed_dequant_op, "CUDA")
torch.library.register_fake("aqlm::code1x16_dequant_packed")(_fake_packed_dequant)


# the planar 8x8 matvec as a dispatcher op (same reason; geometry = [out_features, in_features, in_group_size], the codebook bound
# travels as a float: 0 = unknown -> the two-kernel form)
def _planar_op(input, planar, codebooks, scales, bias, geometry, codebook_absmax):
    pl = PlanarCodes(planar, int(geometry[0]), int(geometry[1]), int(geometry[2]))
    pl.codebook_absmax = float(codebook_absmax)
    pl._range_of = (codebooks.data_ptr(), tensor_version(codebooks))  # the caller's bound is taken at its word
    return code8x8_matmat_planar(input, pl, codebooks, scales, bias)


def _fake_planar(input, planar, codebooks, scales, bias, geometry, codebook_absmax):
    return torch.empty(input.shape[:-1] + (int(geometry[0]),), device=input.device, dtype=input.dtype)


_LIB.define("code8x8_matmat_planar(Tensor input, Tensor planar, Tensor codebooks, Tensor scales, Tensor? bias, int[] geometry, "
            "float codebook_absmax) -> Tensor")
_LIB.impl("code8x8_matmat_planar", _planar_op, "CUDA")
torch.library.register_fake("aqlm::code8x8_matmat_planar")(_fake_planar)


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
