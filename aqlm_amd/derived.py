"""What every copy derived from a parameter is validated against (prepacked / planar / permuted codes, the codebook range and
image, a dense W, the compiled fast lane, the raw op's cache).

A derived copy is current while the tensor it came from has the same identity, storage and version counter.  A write through
``.data`` changes none of them, so the owners of derived state also compare a checksum of the tensor's bytes now and then.  Host
code only: the HIP library is loaded at the first checksum of a GPU tensor, not at import.
"""
from __future__ import annotations

import torch


def tensor_version(t: torch.Tensor) -> int:
    """The tensor's version counter; inference tensors (created under ``torch.inference_mode()``) carry none and cannot be
    written in place outside inference mode, so a constant stands in."""
    try:
        return t._version
    except RuntimeError:
        return 0


def codes_fingerprint(t: torch.Tensor):
    """Identity, storage, shape and version of a ``codes`` tensor: what a repacked copy of it is keyed on."""
    return (id(t), t.data_ptr() if t.numel() else 0, tuple(t.shape), tensor_version(t))


def tensor_checksum(t: torch.Tensor):
    """Position-sensitive checksum of a tensor's bytes, for the writes the version counter does not see.  GPU tensors:
    aqlm_hip_checksum + a 16-byte read-back (synchronises: never while a hipGraph is being captured); host tensors: crc32."""
    t = t.detach()
    if not t.is_contiguous():
        t = t.contiguous()
    if not t.is_cuda:
        import zlib

        return (zlib.crc32(t.reshape(-1).view(torch.uint8).numpy().data), t.numel())
    from . import _native

    out = torch.empty((2,), dtype=torch.int64, device=t.device)
    with torch.cuda.device(t.device):
        rc = _native.lib.aqlm_hip_checksum(t.data_ptr() if t.numel() else None, t.numel() * t.element_size(), out.data_ptr(),
                                           torch.cuda.current_stream(t.device).cuda_stream)
    if rc:
        _native.check(rc, "aqlm checksum")
    return tuple(out.tolist())
