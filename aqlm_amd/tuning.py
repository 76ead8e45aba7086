"""Fine-tuning the continuous parameters of AQLM layers: codebooks, scales and biases train, the codes stay fixed -- what the
reference's ``finetune.py`` does after quantising.

    import aqlm
    params = aqlm.tuning.make_trainable(model)          # codebooks and scales of every QuantizedLinear
    aqlm.tuning.prepare(model)                          # optional: build the inverted indices now (needed before a hipGraph capture)
    opt = torch.optim.SGD(params, lr=1e-4)

A ``QuantizedLinear`` with a trainable parameter leaves every inference route that reads a derived copy of its weights (fast
lane, packed matvec, planar look-up tables, dense W, shared-input launches) and runs under autograd:
  * 1x16 layers (g 8 / 16) on the MI355X with fp16 / bf16 parameters: the forward kernel of the frozen layer, and a backward of
    ``grad_input`` (the frozen layer's kernel), ``dbias``, one library GEMM ``dW = grad_y^T @ x`` and two launches that reduce dW
    to the codebook and scale gradients through an inverted index of the codes (``aqlm_hip_codebook_grad_1x16``,
    ``aqlm_hip_scales_grad_1x16``): no atomics, bit-reproducible;
  * K x 8 layers (1 to 8 codebooks of 256 entries, g 8 / 16 / 32: 2x8 g8, 1x8 g8, 8x8 g32, 4x8 g16 ...) under the same
    conditions: the same forward and backward, with dW reduced by ``aqlm_hip_codebook_grad_kx8`` -- no index: the K * 256 * g sums
    live in LDS while dW streams past once per pass of 64 / g codebooks, taken as fixed-point integers, so that LDS atomics
    cannot change a bit and the sum of the quantised terms is exact -- and ``aqlm_hip_scales_grad_kx8`` (codebooks staged in
    LDS).  A non-finite element of dW or the scales makes the WHOLE codebook gradient NaN (a gradient scaler skips the step);
  * everything else (host tensors, other schemes such as codebooks of other sizes or g 4, ``out_group_size > 1``, fp32 master
    parameters, ``CODEBOOK_GRAD_KERNEL = False``): the reference's definition under autograd, ``F.linear(x,
    _dequantize_weight(codes % 2**nbits, codebooks, scales), bias)`` -- slow, correct, never silent.

Memory: the 1x16 index costs 4 bytes per code (plus ~0.5 MB of tables) next to the 2 bytes of the codes themselves; it is derived
state of the layer (rebuilt when the codes change, never saved, copied or pickled).  ``checkpoint.memory_report`` lists it.  The
K x 8 route keeps no derived state: its transient is the per-stream workspace (at most 33.6 MB).

Precision: fp16 / bf16 parameters stepped by a plain optimizer lose every update smaller than half a unit in the last place of
the parameter (Adam's small steps on a codebook entry of magnitude 1 vanish below 5e-4 in fp16).  This module does not ship an
fp32-master-weight optimizer wrapper; keep the parameters in fp32 (``model.float()``: the torch route above) when that matters.

Out of scope: the experts of a ``QuantizedMixtralExperts`` block (their routed launches carry gradients to the hidden states
only) and ``ShardedQuantizedLinear`` -- ``make_trainable`` leaves both frozen and names them in ``.skipped`` of its result.
"""
from __future__ import annotations

from typing import List

import torch
import torch.nn as nn

# The switch of the HIP route: False sends every trainable layer through the torch route (the reference's definition).
CODEBOOK_GRAD_KERNEL = True
# dW in fp32 (``torch.mm(grad_y^T, x, out_dtype=torch.float32)``, where the installed torch has that overload on the device)
# instead of the storage dtype the reference's autograd produces it in: one rounding less in front of the two reductions, twice
# the bytes of the transient.
CODEBOOK_GRAD_FP32_DW = False


def takes_codebook_grad_kernel(num_codebooks: int, nbits_per_codebook: int, out_group_size: int, in_group_size: int, on_gpu: bool,
                               dtypes_ok: bool, supported: bool, compiling: bool) -> bool:
    """Whether a trainable layer's call runs the HIP route -- a pure function of: the scheme (1x16, ``out_group_size`` 1, g 8 or
    16), ``on_gpu`` (parameters and input on the GPU), ``dtypes_ok`` (input, codebooks, scales and bias in ONE dtype, fp16 or
    bf16), ``supported`` (the library's ``_supported`` queries for the shape), not ``compiling`` and the switch."""
    return bool(CODEBOOK_GRAD_KERNEL and num_codebooks == 1 and nbits_per_codebook == 16 and out_group_size == 1
                and in_group_size in (8, 16) and on_gpu and dtypes_ok and supported and not compiling)


def takes_codebook_grad_kernel_kx8(num_codebooks: int, nbits_per_codebook: int, out_group_size: int, in_group_size: int, on_gpu: bool,
                                   dtypes_ok: bool, supported: bool, compiling: bool) -> bool:
    """The same for the K x 8 route: 1 to 8 codebooks of 8 bits, ``out_group_size`` 1, g 8, 16 or 32; the other arguments and the
    switch as in ``takes_codebook_grad_kernel``.  The two predicates are never true together."""
    return bool(CODEBOOK_GRAD_KERNEL and 1 <= num_codebooks <= 8 and nbits_per_codebook == 8 and out_group_size == 1
                and in_group_size in (8, 16, 32) and on_gpu and dtypes_ok and supported and not compiling)


def param_grad_needed(layer) -> bool:
    """A call of ``layer`` must produce gradients for its own parameters."""
    return torch.is_grad_enabled() and (layer.codebooks.requires_grad or layer.scales.requires_grad
                                        or (layer.bias is not None and layer.bias.requires_grad))


class TrainableParameters(list):
    """What ``make_trainable`` returns: the list of parameters, plus ``skipped`` -- the names of the modules it left frozen."""

    skipped: List[str]


def make_trainable(model: nn.Module, codebooks: bool = True, scales: bool = True, bias: bool = False) -> TrainableParameters:
    """Set ``requires_grad`` on the chosen parameters of every ``QuantizedLinear`` of ``model`` and return them (a list, for an
    optimizer).  The codes never train.  ``QuantizedMixtralExperts`` blocks (and the expert layers inside them) and
    ``ShardedQuantizedLinear`` modules are left frozen: their names are in ``.skipped`` of the result."""
    from .inference import QuantizedLinear
    from .moe import QuantizedMixtralExperts
    from .sharded import ShardedQuantizedLinear

    out = TrainableParameters()
    out.skipped = []
    seen = set()
    for name, m in model.named_modules():
        if isinstance(m, (QuantizedMixtralExperts, ShardedQuantizedLinear)):
            out.skipped.append(name)
        elif isinstance(m, QuantizedLinear) and not getattr(m, "_moe_expert", False):
            for want, p in ((codebooks, m.codebooks), (scales, m.scales), (bias, m.bias)):
                if want and p is not None and id(p) not in seen:
                    p.requires_grad_(True)
                    seen.add(id(p))
                    out.append(p)
    return out


def prepare(model: nn.Module) -> int:
    """Build the inverted index of every ``QuantizedLinear`` with a trainable parameter that would take the HIP route, now: a
    hipGraph capture needs it to exist, and the memory (4 bytes per code) is then allocated at a known time.  Call it after
    ``make_trainable``.  Returns the bytes the indices hold.  K x 8 layers need nothing built: their route has no index."""
    from .inference import QuantizedLinear

    total = 0
    for m in model.modules():
        if not isinstance(m, QuantizedLinear) or getattr(m, "_moe_expert", False):
            continue
        trains = m.codebooks.requires_grad or m.scales.requires_grad or (m.bias is not None and m.bias.requires_grad)
        if trains and m._takes_codebook_grad_kernel(None):
            total += m.codebook_grad_index().nbytes()
    return total
