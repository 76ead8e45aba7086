"""What every op module of this package launches with: dtype ids, the current stream, the device guard, operand helpers, the
cached fp32 workspace, and the one ``aqlm`` op library with ``register_op``.  A leaf: it imports ``_native`` only, and
``hip_kernel`` and the ``ops_*`` family modules import its names one by one (plain global look-ups on the decode path)."""
from __future__ import annotations

import contextlib
from typing import Optional

import torch

from .. import _native

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


# the element types of the training ops (dW, reference weights, gradients), and the way back from an id an op's geometry carries
_GRAD_DT = {torch.float16: _native.F16, torch.bfloat16: _native.BF16, torch.float32: _native.F32}
_GRAD_TORCH_DT = {v: k for k, v in _GRAD_DT.items()}


_LIB = torch.library.Library("aqlm", "DEF")


def register_op(name: str, schema: str, impl, fake) -> None:
    """Define ``aqlm::<name><schema>``, bind ``impl`` to the CUDA key (ROCm reports device type "cuda") and ``fake`` as the shape
    function that tracing runs in its place."""
    _LIB.define(f"{name}{schema}")
    _LIB.impl(name, impl, "CUDA")
    torch.library.register_fake(f"aqlm::{name}")(fake)
