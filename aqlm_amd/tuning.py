"""PV-tuning of AQLM layers: the continuous parameters train (codebooks, scales and biases -- what the reference's ``finetune.py``
does after quantising: the P step), and the codes of a layer are re-chosen against a dense target (the reference's
``beam_search_optimal_codes``: the V step).

    import aqlm
    params = aqlm.tuning.make_trainable(model)          # codebooks and scales of every QuantizedLinear
    aqlm.tuning.prepare(model)                          # optional: build the inverted indices now (needed before a hipGraph capture)
    opt = torch.optim.SGD(params, lr=1e-4)
    ...
    changed = aqlm.tuning.update_codes_(layer, reference_weight, max_update_fraction=0.01)   # every n steps

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

Updating the codes (``find_optimal_codes``, ``update_codes_``): for every group of weights the codes that minimise ``||reference -
dequantised||^2`` with the codebooks and scales held fixed, optionally only for the ``max_update_fraction`` of the groups that are
furthest from the target, and only while the change stays within ``trust_ratio``:
  * 1x16 layers (g 8 / 16, ``out_group_size`` 1) with every tensor on the MI355X, codebooks and scales in one of fp16 / bf16 and
    the target in fp32 / fp16 / bf16: ``aqlm_hip_code_search_1x16`` -- the 65536 scores of a group are
    accumulators of the matrix unit and never reach memory; equal scores give the smallest index, the result is a function of
    the inputs alone.  Selection and trust ratio are torch operations around the kernel (they synchronise: the V step is not
    meant to be captured into a hipGraph);
  * K x 8 layers (1 to 8 codebooks of 256 entries, g 8 / 16 / 32, ``out_group_size`` 1, ``beam_size`` up to 16) under the same
    conditions, codes int8: ``aqlm_hip_code_search_kx8`` -- the reference's beam search over the codebooks
    in ``dim_order``, one wave per group, the ``beams x 256`` scores of a step in registers.  It is held to its own arithmetic bit
    for bit (every product and sum one fp32 operation in a stated order, equal scores to the smaller ``position * 256 + code``):
    tests/kx8_search_model.py restates it;
  * everything else (``beam_size > 16``, codebooks of other sizes, ``out_group_size > 1``, host tensors, fp32 parameters,
    ``CODE_SEARCH_KERNEL = False``): a torch route written from the reference's definition -- chunked scores, the best
    ``beam_size`` hypotheses per step, ``dim_order`` -- slow, correct, never silent.
A group whose unscaled target has a non-finite element keeps its previous code (the reference's result there is whatever
``argmin`` makes of NaNs); so does, on a kernel route, a group with an element of magnitude 2^100 (K x 8: 2^60) or more (the
kernels' stated ranges).  The new codes are written in place, so the version counter of ``codes`` moves and every derived copy
(packed and planar codes, dense W, the fast lane, the inverted index) is rebuilt at the next call by the fingerprint rule that
already covers ``load_state_dict``.  Not offered: ``stochastic_rounding_tau`` and ``force_update`` (``NotImplementedError``).

The calibrated update (``find_optimal_codes_calibrated``, ``update_codes_calibrated_``, ``calibrated_error``): the codes that lower
``||X W_ref^T - X W_q^T||^2`` given ``XTX = X^T X`` of calibration activations -- the reference's src/beam_search_xtx.py, the search
that produces an AQLM layer.  K x 8 layers on the MI355X (fp16 / bf16 codebooks and scales, int8 codes, fp32 ``XTX``, ``beam_size`` up
to 16) run ``aqlm_hip_code_search_kx8_xtx`` once per input group (tests/kx8_xtx_model.py restates its
arithmetic); 1x16 layers (int16 codes, ``beam_size`` up to 8) run ``aqlm_hip_code_search_1x16_xtx`` the same way (section 4.8q;
tests/x16_xtx_model.py); everything else runs a torch route of the same incremental form.

The first codes and codebooks (``fit_kmeans``, ``find_nearest_cluster``, ``init_aq_kmeans``, ``init_layer_kmeans_``): the reference's
residual k-means (src/aq.py ``init_aq_kmeans``, src/kmeans.py).  fp32 data on the MI355X with 8 or 16 values per point and 128 to
65536 centroids (a multiple of 128) runs one Lloyd iteration as ``aqlm_hip_kmeans_assign`` -- the assignment on the matrix unit with
both operands as split fp16 pairs, the clusters' sums as fixed-point integers in the same launch -- and ``aqlm_hip_kmeans_update``
(tests/kmeans_model.py restates the integer side); everything else runs the reference's formula in torch.

Producing a layer (``accumulate_xtx_``, ``calibrated_loss_and_grads``, ``quantize_layer_``): the loop of the reference's
``AQEngine.quantize`` (aq_engine.py) -- the k-means initialisation, then per epoch Adam steps on fp32 masters of the codebooks and scales
against ``tr((W_q - W_ref) XTX (W_q - W_ref)^T) / out_features`` and one calibrated search.  A step on the MI355X runs
``aqlm_hip_calib_delta``, one library GEMM ``G = D XTX``, ``aqlm_hip_calib_rows`` and ``aqlm_hip_calib_codebook_grad_1x16`` / ``_kx8``
(tests/calib_grad_model.py restates their arithmetic); everything else runs autograd through
``_dequantize_weight``.

Memory: the 1x16 index costs 4 bytes per code (plus ~0.5 MB of tables) next to the 2 bytes of the codes themselves; it is derived
state of the layer (rebuilt when the codes change, never saved, copied or pickled).  ``checkpoint.memory_report`` lists it.  The
K x 8 route keeps no derived state: its transient is the per-stream workspace (at most 33.6 MB).

Precision: fp16 / bf16 parameters stepped by a plain optimizer lose every update smaller than half a unit in the last place of
the parameter (Adam's small steps on a codebook entry of magnitude 1 vanish below 5e-4 in fp16).  ``make_trainable`` does not ship an
fp32-master-weight optimizer wrapper; keep the parameters in fp32 (``model.float()``: the torch route above) when that matters.
``quantize_layer_`` keeps fp32 masters of its own.

Out of scope: the experts of a ``QuantizedMixtralExperts`` block (their routed launches carry gradients to the hidden states
only) and ``ShardedQuantizedLinear`` -- ``make_trainable`` leaves both frozen and names them in ``.skipped`` of its result, and
``update_codes_`` raises ``TypeError`` for them.
"""
from __future__ import annotations

import math
import warnings
from typing import List, Optional, Sequence

import torch
import torch.nn as nn

# The switch of the HIP route: False sends every trainable layer through the torch route (the reference's definition).
CODEBOOK_GRAD_KERNEL = True
# dW in fp32 (``torch.mm(grad_y^T, x, out_dtype=torch.float32)``, where the installed torch has that overload on the device)
# instead of the storage dtype the reference's autograd produces it in: one rounding less in front of the two reductions, twice
# the bytes of the transient.
CODEBOOK_GRAD_FP32_DW = False
# The switch of the code search kernel: False sends every ``find_optimal_codes`` call through the torch route.
CODE_SEARCH_KERNEL = True
# Scores the torch route materialises at a time (fp32 values: 512 MiB).
CODE_SEARCH_CHUNK_VALUES = 1 << 27


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
    optimizer).  The codes are not parameters of an optimizer (``update_codes_`` re-chooses them).  ``QuantizedMixtralExperts`` blocks (and the expert layers inside them) and
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


# ---------------------------------------------------------------------------------------------------------------------------
# the V step: new codes against a dense target
# ---------------------------------------------------------------------------------------------------------------------------
def takes_code_search_kernel(num_codebooks: int, nbits_per_codebook: int, out_group_size: int, in_group_size: int, on_gpu: bool,
                             dtypes_ok: bool, supported: bool) -> bool:
    """Whether a ``find_optimal_codes`` call runs ``aqlm_hip_code_search_1x16`` -- a pure function of: the scheme (1x16,
    ``out_group_size`` 1, g 8 or 16), ``on_gpu`` (every tensor on the GPU), ``dtypes_ok`` (codebooks and scales in ONE of fp16 / bf16,
    the target in fp32 / fp16 / bf16), ``supported`` (the library's ``_supported`` query for the shape) and the switch."""
    return bool(CODE_SEARCH_KERNEL and num_codebooks == 1 and nbits_per_codebook == 16 and out_group_size == 1
                and in_group_size in (8, 16) and on_gpu and dtypes_ok and supported)


def takes_code_search_kernel_kx8(num_codebooks: int, nbits_per_codebook: int, out_group_size: int, in_group_size: int, beam_size: int,
                                 on_gpu: bool, dtypes_ok: bool, supported: bool) -> bool:
    """The same for ``aqlm_hip_code_search_kx8``: 1 to 8 codebooks of 8 bits, ``out_group_size`` 1, g 8, 16 or 32, ``beam_size`` 1 to 16;
    ``dtypes_ok``: codebooks and scales in ONE of fp16 / bf16, the target in fp32 / fp16 / bf16, codes int8; the other arguments and the
    switch as in ``takes_code_search_kernel``.  The two predicates are never true together."""
    return bool(CODE_SEARCH_KERNEL and 1 <= num_codebooks <= 8 and nbits_per_codebook == 8 and out_group_size == 1
                and in_group_size in (8, 16, 32) and 1 <= beam_size <= 16 and on_gpu and dtypes_ok and supported)


def _greedy_codes_torch(reference: torch.Tensor, codebook: torch.Tensor, chunk_values: int) -> torch.Tensor:
    """[N] int64: per row of ``reference`` [N, d] the first index that minimises ``|C_c|^2 - 2 <r, C_c>`` over ``codebook`` [S, d]."""
    norms = codebook.square().sum(-1)[None]
    transposed = codebook.T.contiguous()
    rows = max(1, chunk_values // codebook.shape[0])
    out = torch.empty((reference.shape[0],), dtype=torch.int64, device=reference.device)
    for a in range(0, reference.shape[0], rows):
        out[a:a + rows] = torch.addmm(norms, reference[a:a + rows], transposed, alpha=-2).argmin(-1)
    return out


def _beam_codes_torch(reference: torch.Tensor, codebooks: torch.Tensor, codes: torch.Tensor, beam_size: int, dim_order: Sequence[int],
                      chunk_values: int) -> torch.Tensor:
    """[N, K] int64: ``codes`` [N, K] improved one codebook at a time in ``dim_order``.  A step frees its codebook's term of every
    hypothesis, scores all ``beams x S`` continuations by the squared error they leave and keeps the best ``beam_size`` (the last
    step: the best one).  Like the reference, a step subtracts the chosen entries from the residues POSITION BY POSITION: the
    residue at beam position b stays there when the hypothesis that now occupies b descends from another position."""
    num_codebooks, size, _ = codebooks.shape
    norms = codebooks.square().sum(-1)  # [K, S]
    beams = codes[:, None, :].clone()  # [N, beams, K]
    kept = codebooks[0][codes[:, 0]]
    for c in range(1, num_codebooks):
        kept = kept + codebooks[c][codes[:, c]]
    residue = (reference - kept)[:, None, :]  # [N, beams, d]
    for step, c in enumerate(dim_order):
        last = step == len(dim_order) - 1
        residue = residue + codebooks[c][beams[..., c]]
        width, keep = residue.shape[1], (1 if last else beam_size)
        picked = torch.empty((reference.shape[0], keep), dtype=torch.int64, device=reference.device)
        rows = max(1, chunk_values // (size * width))
        for a in range(0, reference.shape[0], rows):
            part = residue[a:a + rows]
            scores = torch.matmul(part, codebooks[c].T)  # [n, beams, S]
            if beam_size > 1:
                scores = part.square().sum(-1, keepdim=True) - 2 * scores + norms[c]
            else:
                scores = -2 * scores + norms[c]  # one hypothesis: its residue's norm is the same for every candidate
            picked[a:a + rows] = torch.topk(scores.flatten(1), keep, dim=-1, largest=False, sorted=True).indices
        source, chosen = picked // size, picked % size
        beams = torch.gather(beams, 1, source[:, :, None].expand(-1, -1, num_codebooks)).clone()
        beams[..., c] = chosen
        if not last:
            residue = residue - codebooks[c][chosen]
    return beams[:, 0, :]


def _group_sq_norms(delta: torch.Tensor, out_group_size: int, in_group_size: int) -> torch.Tensor:
    """[out_groups, in_groups]: the squared sum of every (out_group_size, in_group_size) tile of ``delta`` [out, in]."""
    return delta.reshape(delta.shape[0] // out_group_size, out_group_size, delta.shape[1] // in_group_size,
                         in_group_size).square().sum(dim=(1, 3))


@torch.no_grad()
def find_optimal_codes(reference_weight: torch.Tensor, codebooks: torch.Tensor, prev_codes: torch.Tensor,
                       scales: Optional[torch.Tensor], *, beam_size: int = 1, max_update_fraction: float = 1.0,
                       trust_ratio: Optional[float] = None, code_selection_temperature: float = 0.0,
                       dim_order: Optional[Sequence[int]] = None, generator: Optional[torch.Generator] = None, **unsupported) -> torch.Tensor:
    """New codes (shape and dtype of ``prev_codes``) that minimise ``||reference_weight - dequantised||^2`` with ``codebooks`` [K, S,
    out_group_size, in_group_size] and ``scales`` ([out_groups, 1, 1, 1] or None) held fixed -- the reference's
    ``beam_search_optimal_codes`` on this package's tensors: ``prev_codes`` [out_groups, in_groups, K] in the stored int8 / int16
    wrap-around form.

    ``beam_size``: hypotheses kept per step of the search over several codebooks (with one codebook it does not change the
    answer).  ``dim_order``: the order in which the codebooks are revisited (default 0 .. K - 1).  ``max_update_fraction`` < 1:
    only the ceil(fraction * groups) groups with the largest ``||reference - dequant(prev)||^2`` are searched (the others keep
    their codes) -- chosen by top-k, or with ``code_selection_temperature`` T > 0 sampled without replacement in proportion to
    norm^(1 / T) from ``generator``.  ``trust_ratio``: the changes are admitted in that order while the cumulative ``||dW||`` stays
    within ``trust_ratio * ||W_prev||``; one change is always admitted.  A group whose unscaled target has a non-finite element
    keeps its previous codes.  Routes: module docstring.  ``stochastic_rounding_tau`` and ``force_update`` raise
    ``NotImplementedError``."""
    for name in ("stochastic_rounding_tau", "force_update"):
        if name in unsupported:
            raise NotImplementedError(f"find_optimal_codes: {name} is not offered (the reference's defaults do not use it)")
    if unsupported:
        raise TypeError(f"find_optimal_codes: unexpected arguments {sorted(unsupported)}")
    if not 0 < max_update_fraction <= 1 or (trust_ratio is not None and not trust_ratio > 0) or beam_size < 1:
        raise ValueError("find_optimal_codes: 0 < max_update_fraction <= 1, trust_ratio > 0, beam_size >= 1")
    out_groups, in_groups, num_codebooks = prev_codes.shape
    K, size, out_group_size, in_group_size = codebooks.shape
    if K != num_codebooks or tuple(reference_weight.shape) != (out_groups * out_group_size, in_groups * in_group_size):
        raise ValueError(f"find_optimal_codes: codes {tuple(prev_codes.shape)}, codebooks {tuple(codebooks.shape)} and a target of "
                         f"{tuple(reference_weight.shape)} do not describe one layer")
    order = list(range(K)) if dim_order is None else [int(c) for c in dim_order]
    if sorted(order) != list(range(K)):
        raise ValueError(f"find_optimal_codes: dim_order must be a permutation of 0 .. {K - 1}, got {order}")
    nbits = int(math.log2(size))
    num_groups = out_groups * in_groups

    tensors = [reference_weight, codebooks, prev_codes] + ([] if scales is None else [scales])
    on_gpu = all(t.is_cuda for t in tensors)
    floats_ok = (codebooks.dtype in (torch.float16, torch.bfloat16) and (scales is None or scales.dtype == codebooks.dtype)
                 and reference_weight.dtype in (torch.float32, torch.float16, torch.bfloat16))
    dtypes_ok = floats_ok and prev_codes.dtype == torch.int16
    supported = False
    if CODE_SEARCH_KERNEL and on_gpu and K == 1 and nbits == 16 and out_group_size == 1 and in_group_size in (8, 16):
        from .inference_kernels import hip_kernel

        supported = hip_kernel.code_search_1x16_supported(reference_weight.shape[0], reference_weight.shape[1], in_group_size)
    kernel = takes_code_search_kernel(K, nbits, out_group_size, in_group_size, on_gpu, dtypes_ok, supported)
    supported_kx8 = False
    if (CODE_SEARCH_KERNEL and on_gpu and 1 <= K <= 8 and nbits == 8 and out_group_size == 1 and in_group_size in (8, 16, 32)
            and 1 <= beam_size <= 16):
        from .inference_kernels import hip_kernel

        supported_kx8 = hip_kernel.code_search_kx8_supported(reference_weight.shape[0], reference_weight.shape[1], K, in_group_size, beam_size)
    kernel_kx8 = takes_code_search_kernel_kx8(K, nbits, out_group_size, in_group_size, beam_size, on_gpu,
                                              floats_ok and prev_codes.dtype == torch.int8, supported_kx8)

    from .utils import _dequantize_weight

    device = reference_weight.device
    compute = torch.float64 if reference_weight.dtype == torch.float64 else torch.float32
    books = codebooks.detach().to(compute)
    factors = None if scales is None else scales.detach().to(compute)
    unsigned_prev = prev_codes.to(torch.int64) % size
    flat_prev = unsigned_prev.reshape(num_groups, K)

    # the groups that may change, most important first
    selected = prev_weight = None
    if max_update_fraction < 1 or trust_ratio is not None:
        prev_weight = _dequantize_weight(unsigned_prev, books, factors)
        count = int(math.ceil(max_update_fraction * num_groups))
        distance = _group_sq_norms(reference_weight.to(compute) - prev_weight, out_group_size, in_group_size).flatten()
        if code_selection_temperature > 0:
            selected = torch.pow(distance, 0.5 / code_selection_temperature).multinomial(count, replacement=False, generator=generator)
        else:
            selected = torch.topk(distance, k=count, largest=True, sorted=True).indices
    searched = selected if max_update_fraction < 1 else None

    def unscaled(ids):
        """[n, out_group_size * in_group_size]: the targets of the groups ``ids`` (None: all) divided by their scales."""
        tiles = reference_weight.reshape(out_groups, out_group_size, in_groups, in_group_size).permute(0, 2, 1, 3).reshape(
            num_groups, out_group_size, in_group_size)
        tiles = (tiles if ids is None else tiles[ids]).to(compute)
        if factors is not None:
            per_group = factors.reshape(out_groups, 1).expand(out_groups, in_groups).reshape(num_groups)
            tiles = tiles / (per_group if ids is None else per_group[ids])[:, None, None]
        return tiles.flatten(1)

    if kernel:
        from .inference_kernels import hip_kernel

        found = hip_kernel.code_search_1x16(reference_weight.detach(), None if scales is None else scales.detach().reshape(-1),
                                            codebooks.detach(), in_group_size, group_ids=searched)
        found = (found.to(torch.int64) % size)[:, None]
        targets = None
    elif kernel_kx8:
        from .inference_kernels import hip_kernel

        found = hip_kernel.code_search_kx8(reference_weight.detach(), None if scales is None else scales.detach().reshape(-1),
                                           codebooks.detach(), prev_codes.detach().reshape(num_groups, K), in_group_size, beam_size,
                                           dim_order=order, group_ids=searched)
        found = found.to(torch.int64) % size
        targets = None
    else:
        targets = unscaled(searched)
        before = flat_prev if searched is None else flat_prev[searched]
        flat_books = books.flatten(-2, -1)
        if K == 1:
            found = _greedy_codes_torch(targets, flat_books[0], CODE_SEARCH_CHUNK_VALUES)[:, None]
        else:
            found = _beam_codes_torch(targets, flat_books, before, beam_size, order, CODE_SEARCH_CHUNK_VALUES)
    # a group with a non-finite target keeps what it had
    before = flat_prev if searched is None else flat_prev[searched]
    if targets is None:  # (the kernel routes)
        # (... and one beyond the kernel's stated range, max|r| >= 2^100 for 1x16 and 2^60 for K x 8, where fp32 scores can overflow
        # and tie)
        finite = (unscaled(searched).abs() < 2.0 ** (60 if kernel_kx8 else 100)).all(-1)
    else:
        finite = torch.isfinite(targets).all(-1)
    found = torch.where(finite[:, None], found, before)
    flat_new = found if searched is None else flat_prev.index_put((searched[:, None], torch.arange(K, device=device)[None, :]), found)

    if trust_ratio is not None:
        new_weight = _dequantize_weight(flat_new.reshape(out_groups, in_groups, K), books, factors)
        change = _group_sq_norms(new_weight - prev_weight, out_group_size, in_group_size).flatten()[selected]
        cumulative = change.cumsum(0).sqrt()
        admitted = 1 + int(torch.searchsorted(cumulative, trust_ratio * prev_weight.norm(), side="left"))
        kept = selected[:admitted]
        flat_new = flat_prev.index_put((kept[:, None], torch.arange(K, device=device)[None, :]), flat_new[kept])

    wrapped = torch.where(flat_new >= size // 2, flat_new - size, flat_new) if prev_codes.dtype in (torch.int8, torch.int16) and nbits in (8, 16) \
        else flat_new
    return wrapped.to(prev_codes.dtype).reshape(prev_codes.shape)


@torch.no_grad()
def update_codes_(layer, reference_weight: torch.Tensor, **options) -> torch.Tensor:
    """Re-choose the codes of ``layer`` (a ``QuantizedLinear``) against the dense target ``reference_weight`` [out, in] with
    ``find_optimal_codes`` (same options) and write them IN PLACE: the parameter object stays, its version counter moves, and every
    derived copy of the codes (packed / planar codes, dense W, fast lane, inverted index) is rebuilt at the layer's next call.  A
    layer whose canonical codes were dropped gets them back first; codes that are an inference tensor raise ``RuntimeError``.  Returns the number of groups whose codes changed (a 0-dim
    tensor on the layer's device).  The experts of a ``QuantizedMixtralExperts`` block and ``ShardedQuantizedLinear`` raise
    ``TypeError``."""
    from .inference import QuantizedLinear
    from .moe import QuantizedMixtralExperts
    from .sharded import ShardedQuantizedLinear

    if isinstance(layer, (QuantizedMixtralExperts, ShardedQuantizedLinear)) or getattr(layer, "_moe_expert", False):
        raise TypeError(f"update_codes_: {type(layer).__name__}{' (an expert of a QuantizedMixtralExperts block)' if getattr(layer, '_moe_expert', False) else ''}"
                        " is outside the scope of the code update (as it is of make_trainable)")
    if not isinstance(layer, QuantizedLinear):
        raise TypeError(f"update_codes_: expected a QuantizedLinear, got {type(layer).__name__}")
    for name in ("stochastic_rounding_tau", "force_update"):
        if name in options:
            raise NotImplementedError(f"update_codes_: {name} is not offered (the reference's defaults do not use it)")
    layer.restore_canonical_codes()
    codes = layer.codes
    if codes.is_inference():
        # an inference tensor carries no version counter and cannot be written outside inference mode: the in-place write that the
        # derived state is keyed on does not exist for it
        raise RuntimeError("update_codes_: the codes of this layer are an inference tensor (the model was built or loaded under "
                           "torch.inference_mode()); they cannot be written in place -- build the model outside inference mode")
    new = find_optimal_codes(reference_weight, layer.codebooks.detach(), codes.detach(), layer.scales.detach(), **options)
    changed = (new != codes).any(-1).sum()
    codes.copy_(new)
    return changed


# ---------------------------------------------------------------------------------------------------------------------------
# the calibrated V step: new codes against the layer's OUTPUT on calibration data (XTX = X^T X)
# ---------------------------------------------------------------------------------------------------------------------------
def takes_code_search_kernel_kx8_xtx(num_codebooks: int, nbits_per_codebook: int, out_group_size: int, in_group_size: int, beam_size: int,
                                     on_gpu: bool, dtypes_ok: bool, supported: bool) -> bool:
    """Whether a ``find_optimal_codes_calibrated`` call runs ``aqlm_hip_code_search_kx8_xtx`` -- a pure function of: the scheme (1 to 8
    codebooks of 8 bits, ``out_group_size`` 1, g 8, 16 or 32), ``beam_size`` 1 to 16, ``on_gpu`` (every tensor on the GPU), ``dtypes_ok``
    (codebooks and scales in ONE of fp16 / bf16, codes int8, ``XTX`` fp32, the target fp32 / fp16 / bf16 -- a float64 target asks for
    float64 arithmetic and takes the torch route), ``supported`` (the library's ``_supported`` query) and the ``CODE_SEARCH_KERNEL``
    switch.  No region is declined on timing grounds: the kernel route took 0.06 to 0.27 of the torch route's time in every cell
    measured (profiles/code_update_xtx.json)."""
    return bool(CODE_SEARCH_KERNEL and 1 <= num_codebooks <= 8 and nbits_per_codebook == 8 and out_group_size == 1
                and in_group_size in (8, 16, 32) and 1 <= beam_size <= 16 and on_gpu and dtypes_ok and supported)


def takes_code_search_kernel_1x16_xtx(nbits_per_codebook: int, num_codebooks: int, out_group_size: int, in_group_size: int, beam_size: int,
                                      on_gpu: bool, dtypes_ok: bool, supported: bool) -> bool:
    """Whether a ``find_optimal_codes_calibrated`` call runs ``aqlm_hip_code_search_1x16_xtx`` -- a pure function of: the scheme (ONE
    codebook of 16 bits, ``out_group_size`` 1, g 8 or 16), ``beam_size`` 1 to 8, ``on_gpu`` (every tensor on the GPU), ``dtypes_ok``
    (codebooks and scales in ONE of fp16 / bf16, codes int16, ``XTX`` fp32, the target fp32 / fp16 / bf16 -- a float64 target asks for
    float64 arithmetic and takes the torch route), ``supported`` (the library's ``_supported`` query) and the ``CODE_SEARCH_KERNEL``
    switch.  No region is declined on timing grounds: the kernel route took 0.028 to 0.124 of the torch route's time in every cell
    measured (profiles/code_update_xtx_1x16.json)."""
    return bool(CODE_SEARCH_KERNEL and num_codebooks == 1 and nbits_per_codebook == 16 and out_group_size == 1
                and in_group_size in (8, 16) and 1 <= beam_size <= 8 and on_gpu and dtypes_ok and supported)


def _channel_errors(weight: torch.Tensor, reference: torch.Tensor, XTX: torch.Tensor) -> torch.Tensor:
    """[out]: ``(W - W_ref)[o] XTX (W - W_ref)[o]^T``"""
    error = weight - reference
    return ((error @ XTX) * error).sum(-1)


@torch.no_grad()
def calibrated_error(weight_or_layer, reference_weight: torch.Tensor, XTX: torch.Tensor) -> torch.Tensor:
    """``sum_o (W - W_ref)[o] XTX (W - W_ref)[o]^T`` -- ``||X W^T - X W_ref^T||^2`` for ``XTX = X^T X``, the objective of the calibrated code
    search (the reference's ``_channelwise_squared_error``, summed) -- for a dense ``W`` [out, in] or a ``QuantizedLinear`` (its
    dequantised weight).  Computed in the dtype of ``reference_weight`` (fp16 / bf16: in fp32); a 0-dim tensor."""
    compute = reference_weight.dtype if reference_weight.dtype in (torch.float32, torch.float64) else torch.float32
    if isinstance(weight_or_layer, torch.Tensor):
        weight = weight_or_layer
    else:
        from .utils import _dequantize_weight, unpack_int_data

        layer = weight_or_layer
        layer.restore_canonical_codes()
        nbits = int(math.log2(layer.codebooks.shape[1]))
        weight = _dequantize_weight(unpack_int_data(layer.codes.detach(), nbits), layer.codebooks.detach().to(compute),
                                    layer.scales.detach().to(compute))
    return _channel_errors(weight.to(compute), reference_weight.to(compute), XTX.to(compute)).sum()


def _calibrated_codes_torch(XTX: torch.Tensor, reference: torch.Tensor, books: torch.Tensor, codes: torch.Tensor,
                            factors: Optional[torch.Tensor], beam_size: int, group_order: Sequence[int],
                            dim_orders: Sequence[Sequence[int]], chunk_values: int) -> torch.Tensor:
    """[out_groups, in_groups, K] int64: the reference's ``beam_search_optimal_codes`` of src/beam_search_xtx.py in its incremental
    form.  With ``T_b = (W_ref - W_b) XTX`` per beam position, the K steps of an input group read and write only ``T_b[group]``, the
    block ``H = XTX[group, group]`` and ``q_c[s] = C_c[s] H C_c[s]^T``; the other columns of ``T`` take the group's weight change once,
    when the group is done.  ``books`` [K, S, out_group_size, g], ``codes`` unsigned, ``factors`` [out_groups] or None, all tensors in
    the compute dtype.  Transient memory: two copies of ``T`` [beam_size, out, in] and one chunk of scores."""
    K, size, ogs, g = books.shape
    og, ng, _ = codes.shape
    from .utils import _dequantize_weight

    s = torch.ones((og,), dtype=books.dtype, device=books.device) if factors is None else factors.reshape(og)
    error = reference - _dequantize_weight(codes, books, s.reshape(og, 1, 1, 1))
    T = (error @ XTX).reshape(1, og, ogs, ng * g)
    loss = (T[0] * error.reshape(og, ogs, ng * g)).sum(dim=(-1, -2))[None]  # [P, og]
    beams = codes[None]  # [P, og, ng, K]
    flat_books = books.flatten(2)  # [K, S, ogs * g]
    rows = torch.arange(og, device=books.device)[None, :]
    s4 = s[None, :, None, None]
    for j, order in zip(group_order, dim_orders):
        cols = slice(j * g, (j + 1) * g)
        H = XTX[cols, cols]
        q = torch.einsum("ksrf,fh,ksrh->ks", books, H, books)
        tl = T[..., cols].clone()  # [P, og, ogs, g]
        local = beams[:, :, j, :].clone()  # [P, og, K]
        ancestor = torch.arange(tl.shape[0], device=books.device)[:, None].expand(-1, og)
        delta = torch.zeros_like(tl)
        for c in order:
            P = tl.shape[0]
            code = local[..., c]
            prev_entry = books[c][code]  # [P, og, ogs, g]
            u = (tl + (s4 * prev_entry) @ H).flatten(2)
            base = loss + 2 * s * (prev_entry.flatten(2) * u).sum(-1) - s * s * q[c][code]
            keep = min(beam_size, P * size)
            values = torch.empty((og, keep), dtype=books.dtype, device=books.device)
            picked = torch.empty((og, keep), dtype=torch.int64, device=books.device)
            n = max(1, chunk_values // (P * size))
            for a in range(0, og, n):
                sa = s[a:a + n, None]
                scores = base[:, a:a + n, None] - (2 * sa) * (u[:, a:a + n] @ flat_books[c].T) + (sa * sa) * q[c][None, :]
                top = torch.topk(scores.permute(1, 0, 2).flatten(1), keep, dim=-1, largest=False, sorted=True)
                values[a:a + n], picked[a:a + n] = top.values, top.indices
            source, chosen = (picked // size).T, (picked % size).T  # [keep, og]
            dw = s4 * (books[c][chosen] - books[c][code[source, rows]])
            tl = tl[source, rows] - dw @ H
            delta = delta[source, rows] + dw
            local = local[source, rows].clone()
            local[..., c] = chosen
            ancestor = ancestor[source, rows]
            loss = values.T
        T = T[ancestor, rows] - delta @ XTX[cols, :]
        beams = beams[ancestor, rows].clone()
        beams[:, :, j, :] = local
    return beams[0]


# Input groups per block of the kernel route: within a block every group's weight change reaches the block's own columns of T at once
# (a gather and a small GEMM); the other columns take the whole block's change in one GEMM at the block's end.
CALIBRATED_BLOCK_GROUPS = 16


def _xtx_step_kx8(t, loss, codes_in, H, q, books, scales, beam_size, order):
    from .inference_kernels import hip_kernel

    return hip_kernel.code_search_kx8_xtx_step(t, loss, codes_in, H, q, books, scales, beam_size, dim_order=order)


def _xtx_step_1x16(t, loss, codes_in, H, q, books, scales, beam_size, order):
    from .inference_kernels import hip_kernel

    return hip_kernel.code_search_1x16_xtx_step(t, loss, codes_in, H, q[0], books, scales, beam_size)  # (one codebook: no order)


def _calibrated_codes_kernel(XTX: torch.Tensor, reference: torch.Tensor, codebooks: torch.Tensor, prev_codes: torch.Tensor,
                             scales: Optional[torch.Tensor], beam_size: int, group_order: Sequence[int],
                             dim_orders: Sequence[Sequence[int]], block_groups: int, step_fn=_xtx_step_kx8,
                             q_per_block: bool = False) -> torch.Tensor:
    """[out, in_groups, K] in the dtype of ``prev_codes``: the same search with one call of ``step_fn`` per input group
    (``_xtx_step_kx8``: ``aqlm_hip_code_search_kx8_xtx``, int8 codes, tables of 256; ``_xtx_step_1x16``: ``aqlm_hip_code_search_1x16_xtx``,
    int16 codes, one table of 65536).  A host loop, no ``.item()`` and no host synchronisation; hypotheses are carried by back-pointers
    (``source`` of every launch) resolved at the end.  The initial ``T`` and losses are formed in float64 and rounded once.
    ``q_per_block``: ``q = C H C^T`` is formed for the groups of a block when the block starts (a table of 65536 entries: 256 KB per
    group), not for the whole layer up front.  Transient memory: ``T`` [beam_size, out, in] fp32 and, at a block's end, its gathered
    copy; float64 copies of ``XTX`` and the target while ``T`` is formed."""
    from .utils import _dequantize_weight

    K, size, _, g = codebooks.shape
    out, ng, _ = prev_codes.shape
    fin, dev = ng * g, reference.device
    flat_books = codebooks.detach().reshape(K, size, g).contiguous()
    flat_scales = None if scales is None else scales.detach().reshape(-1).contiguous()
    wide = torch.float64
    error = reference.to(wide) - _dequantize_weight(prev_codes.to(torch.int64) % size, codebooks.detach().to(wide),
                                                    None if scales is None else scales.detach().to(wide))
    T = error @ XTX.to(wide)
    loss = (T * error).sum(-1).to(torch.float32)[None].contiguous()
    T = T.to(torch.float32)[None]  # [P, out, in]
    del error
    blocks = XTX.reshape(ng, g, ng, g).diagonal(dim1=0, dim2=2).permute(2, 0, 1).contiguous()  # [ng, g, g]
    books32 = flat_books.to(torch.float32)
    q_all = None if q_per_block else torch.einsum("ksf,jfh,ksh->jks", books32, blocks, books32).contiguous()  # [ng, K, size]
    columns = (torch.tensor(list(group_order), dtype=torch.int64)[:, None] * g + torch.arange(g)[None, :]).flatten().to(dev)
    history = []
    block_groups = max(1, int(block_groups))
    for start in range(0, ng, block_groups):
        members = list(group_order[start:start + block_groups])
        cols = columns[start * g:(start + len(members)) * g]
        width = cols.numel()
        x_rows = XTX.index_select(0, cols)  # [width, in]
        x_block = x_rows.index_select(1, cols)  # [width, width]
        t_block = T.index_select(2, cols)  # [P, out, width]
        d_block = ancestor = None
        if q_per_block:  # [members, K, size]: (C_c H_j) . C_c row by row
            h_block = blocks[torch.tensor(members, dtype=torch.int64, device=dev)]
            q_block = ((books32[None] @ h_block[:, None]) * books32[None]).sum(-1).contiguous()
        for i, j in enumerate(members):
            P = t_block.shape[0]
            step = step_fn(t_block[:, :, i * g:(i + 1) * g], loss, prev_codes[None, :, j, :].expand(P, out, K).contiguous(), blocks[j],
                           q_block[i] if q_per_block else q_all[j], flat_books, flat_scales, beam_size, dim_orders[start + i])
            loss = step.loss
            history.append((j, step.codes, step.source))
            source = step.source.to(torch.int64)
            wide_source = source[:, :, None].expand(-1, -1, width)
            t_block = torch.gather(t_block, 0, wide_source)
            t_block.view(-1, width).addmm_(step.delta.view(-1, g), x_block[i * g:(i + 1) * g], alpha=-1)
            d_block = torch.zeros_like(t_block) if d_block is None else torch.gather(d_block, 0, wide_source)
            d_block[:, :, i * g:(i + 1) * g] = step.delta
            ancestor = source if ancestor is None else torch.gather(ancestor, 0, source)
        if start + len(members) < ng:  # the columns outside the block: one gather and one GEMM for the whole block
            T = torch.gather(T, 0, ancestor[:, :, None].expand(-1, -1, fin))
            T.view(-1, fin).addmm_(d_block.view(-1, width), x_rows, alpha=-1)
    new = prev_codes.clone()
    position = torch.zeros((1, out), dtype=torch.int64, device=dev)
    for j, codes, source in reversed(history):
        new[:, j, :] = torch.gather(codes, 0, position[:, :, None].expand(-1, -1, K))[0]
        position = torch.gather(source.to(torch.int64), 0, position)
    return new


def _permutation(values, n: int, what: str) -> List[int]:
    got = [int(v) for v in values]
    if sorted(got) != list(range(n)):
        raise ValueError(f"find_optimal_codes_calibrated: {what} must be a permutation of 0 .. {n - 1}, got {got}")
    return got


@torch.no_grad()
def find_optimal_codes_calibrated(XTX: torch.Tensor, reference_weight: torch.Tensor, codebooks: torch.Tensor, prev_codes: torch.Tensor,
                                  scales: Optional[torch.Tensor], *, beam_size: int = 1, group_order: Optional[Sequence[int]] = None,
                                  dim_order=None, **unsupported) -> torch.Tensor:
    """New codes (shape, dtype and wrap-around form of ``prev_codes``) that lower ``||X W_ref^T - X W_q^T||^2`` for ``XTX = X^T X`` [in, in]
    with ``codebooks`` [K, S, out_group_size, in_group_size] and ``scales`` ([out_groups, 1, 1, 1] or None) held fixed -- the reference's
    ``beam_search_optimal_codes`` of src/beam_search_xtx.py, the search that PRODUCES an AQLM layer: the input groups are visited once
    each in ``group_order`` (default 0 .. in_groups - 1), the codebooks of a group in ``dim_order`` (one permutation of 0 .. K - 1, or
    one per visited group: the reference draws a fresh one per group), ``beam_size`` hypotheses per output group survive every step
    and the best one is returned.  "No change" is always a candidate, so the objective (``calibrated_error``) never rises.

    Routes: K x 8 layers (1 to 8 codebooks of 256 entries, g 8 / 16 / 32, ``out_group_size`` 1, ``beam_size`` up to 16) with every tensor
    on the MI355X, codebooks and scales in one of fp16 / bf16, codes int8, ``XTX`` fp32 and a target in fp32 / fp16 / bf16 run
    ``aqlm_hip_code_search_kx8_xtx`` once per input group (transient: ``T`` [beam_size, out, in] fp32, twice at the
    end of every ``CALIBRATED_BLOCK_GROUPS`` groups); 1x16 layers (one codebook of 65536 entries, g 8 / 16, ``out_group_size`` 1,
    ``beam_size`` up to 8, int16 codes, the same dtypes otherwise) run ``aqlm_hip_code_search_1x16_xtx`` through the same host loop
    (``q`` is formed per block of groups; a ``dim_order`` is accepted and has no effect); everything else -- host
    tensors, fp32 / fp64 parameters, a float64 target (on the GPU too), ``out_group_size > 1``, ``beam_size > 16`` (1x16: > 8),
    ``CODE_SEARCH_KERNEL = False`` -- runs a torch route written
    from the reference's definition (float64 when the target is float64;
    scores in chunks of ``CODE_SEARCH_CHUNK_VALUES``; the same transient in the compute dtype).  ``sparsity_regularizer`` raises
    ``NotImplementedError``."""
    if unsupported.pop("sparsity_regularizer", 0):
        raise NotImplementedError("find_optimal_codes_calibrated: sparsity_regularizer is not offered")
    if unsupported:
        raise TypeError(f"find_optimal_codes_calibrated: unexpected arguments {sorted(unsupported)}")
    if beam_size < 1:
        raise ValueError("find_optimal_codes_calibrated: beam_size >= 1")
    if prev_codes.dim() != 3 or codebooks.dim() != 4:
        raise ValueError("find_optimal_codes_calibrated: codes are [out_groups, in_groups, K], codebooks [K, S, out_group_size, in_group_size]")
    out_groups, in_groups, num_codebooks = prev_codes.shape
    K, size, out_group_size, in_group_size = codebooks.shape
    out_features, in_features = out_groups * out_group_size, in_groups * in_group_size
    if K != num_codebooks or tuple(reference_weight.shape) != (out_features, in_features):
        raise ValueError(f"find_optimal_codes_calibrated: codes {tuple(prev_codes.shape)}, codebooks {tuple(codebooks.shape)} and a target of "
                         f"{tuple(reference_weight.shape)} do not describe one layer")
    if tuple(XTX.shape) != (in_features, in_features):
        raise ValueError(f"find_optimal_codes_calibrated: XTX must be [{in_features}, {in_features}], got {tuple(XTX.shape)}")
    if scales is not None and scales.numel() != out_groups:
        raise ValueError(f"find_optimal_codes_calibrated: scales must hold one factor per output group ({out_groups}), got {tuple(scales.shape)}")
    groups = list(range(in_groups)) if group_order is None else _permutation(group_order, in_groups, "group_order")
    if dim_order is None:
        orders = [list(range(K))] * in_groups
    else:
        given = list(dim_order)
        if given and (isinstance(given[0], (list, tuple)) or getattr(given[0], "ndim", 0) >= 1):
            if len(given) != in_groups:
                raise ValueError(f"find_optimal_codes_calibrated: dim_order holds {len(given)} permutations for {in_groups} input groups")
            orders = [_permutation(one, K, "every dim_order") for one in given]
        else:
            orders = [_permutation(given, K, "dim_order")] * in_groups
    nbits = int(math.log2(size))

    tensors = [XTX, reference_weight, codebooks, prev_codes] + ([] if scales is None else [scales])
    on_gpu = all(t.is_cuda for t in tensors)
    dtypes_ok = (codebooks.dtype in (torch.float16, torch.bfloat16) and (scales is None or scales.dtype == codebooks.dtype)
                 and prev_codes.dtype == torch.int8 and XTX.dtype == torch.float32
                 and reference_weight.dtype in (torch.float32, torch.float16, torch.bfloat16))
    supported = False
    if (CODE_SEARCH_KERNEL and on_gpu and 1 <= K <= 8 and nbits == 8 and out_group_size == 1 and in_group_size in (8, 16, 32)
            and 1 <= beam_size <= 16):
        from .inference_kernels import hip_kernel

        supported = hip_kernel.code_search_kx8_xtx_supported(out_features, K, in_group_size, beam_size, beam_size)
    if takes_code_search_kernel_kx8_xtx(K, nbits, out_group_size, in_group_size, beam_size, on_gpu, dtypes_ok, supported):
        return _calibrated_codes_kernel(XTX, reference_weight, codebooks, prev_codes, scales, beam_size, groups, orders,
                                        CALIBRATED_BLOCK_GROUPS).reshape(prev_codes.shape)

    wide_ok = (codebooks.dtype in (torch.float16, torch.bfloat16) and (scales is None or scales.dtype == codebooks.dtype)
               and prev_codes.dtype == torch.int16 and XTX.dtype == torch.float32
               and reference_weight.dtype in (torch.float32, torch.float16, torch.bfloat16))
    wide_supported = False
    if CODE_SEARCH_KERNEL and on_gpu and K == 1 and nbits == 16 and out_group_size == 1 and in_group_size in (8, 16) and 1 <= beam_size <= 8:
        from .inference_kernels import hip_kernel

        wide_supported = hip_kernel.code_search_1x16_xtx_supported(out_features, in_group_size, beam_size, beam_size)
    if takes_code_search_kernel_1x16_xtx(nbits, K, out_group_size, in_group_size, beam_size, on_gpu, wide_ok, wide_supported):
        # (dim_order of a one-codebook layer was checked above and has no effect)
        return _calibrated_codes_kernel(XTX, reference_weight, codebooks, prev_codes, scales, beam_size, groups, orders,
                                        CALIBRATED_BLOCK_GROUPS, _xtx_step_1x16, True).reshape(prev_codes.shape)

    compute = torch.float64 if reference_weight.dtype == torch.float64 else torch.float32
    found = _calibrated_codes_torch(XTX.to(compute), reference_weight.to(compute), codebooks.detach().to(compute),
                                    prev_codes.to(torch.int64) % size, None if scales is None else scales.detach().to(compute),
                                    beam_size, groups, orders, CODE_SEARCH_CHUNK_VALUES)
    wrapped = torch.where(found >= size // 2, found - size, found) if prev_codes.dtype in (torch.int8, torch.int16) and nbits in (8, 16) \
        else found
    return wrapped.to(prev_codes.dtype).reshape(prev_codes.shape)


@torch.no_grad()
def update_codes_calibrated_(layer, reference_weight: torch.Tensor, XTX: torch.Tensor, **options) -> torch.Tensor:
    """Re-choose the codes of ``layer`` (a ``QuantizedLinear``) against the dense target ``reference_weight`` [out, in] under the
    calibration statistics ``XTX`` with ``find_optimal_codes_calibrated`` (same options) and write them IN PLACE, by the rules of
    ``update_codes_``: dropped canonical codes come back first, inference tensors raise ``RuntimeError``, the version counter of
    ``codes`` moves so that every derived copy is rebuilt at the layer's next call, and the experts of a ``QuantizedMixtralExperts``
    block and ``ShardedQuantizedLinear`` raise ``TypeError``.  Returns the number of groups whose codes changed (a 0-dim tensor)."""
    from .inference import QuantizedLinear
    from .moe import QuantizedMixtralExperts
    from .sharded import ShardedQuantizedLinear

    if isinstance(layer, (QuantizedMixtralExperts, ShardedQuantizedLinear)) or getattr(layer, "_moe_expert", False):
        raise TypeError(f"update_codes_calibrated_: {type(layer).__name__}{' (an expert of a QuantizedMixtralExperts block)' if getattr(layer, '_moe_expert', False) else ''}"
                        " is outside the scope of the code update (as it is of make_trainable)")
    if not isinstance(layer, QuantizedLinear):
        raise TypeError(f"update_codes_calibrated_: expected a QuantizedLinear, got {type(layer).__name__}")
    if options.get("sparsity_regularizer", 0):
        raise NotImplementedError("update_codes_calibrated_: sparsity_regularizer is not offered")
    layer.restore_canonical_codes()
    codes = layer.codes
    if codes.is_inference():
        raise RuntimeError("update_codes_calibrated_: the codes of this layer are an inference tensor (the model was built or loaded under "
                           "torch.inference_mode()); they cannot be written in place -- build the model outside inference mode")
    new = find_optimal_codes_calibrated(XTX, reference_weight, layer.codebooks.detach(), codes.detach(), layer.scales.detach(), **options)
    changed = (new != codes).any(-1).sum()
    codes.copy_(new)
    return changed


# ---------------------------------------------------------------------------------------------------------------------------
# residual k-means: the first codes and codebooks of a layer (the reference's init_aq_kmeans)
# ---------------------------------------------------------------------------------------------------------------------------
# The switch of the k-means kernels: False sends every k-means call through the torch route.
KMEANS_KERNEL = True
# Scores the torch route of k-means materialises at a time (the reference's ``block_size_vals`` is 2^30).
KMEANS_CHUNK_VALUES = 1 << 27
_KMEANS_NOT_OFFERED = ("greedy_init", "use_faiss", "devices")


def takes_kmeans_kernel(k: int, dim: int, on_gpu: bool, dtype: torch.dtype, out_group_size: int = 1) -> bool:
    """Whether a k-means call runs ``aqlm_hip_kmeans_assign`` / ``aqlm_hip_kmeans_update`` -- a pure function of: ``k`` (a multiple of
    128 from 128 to 65536: both the 256-entry and the 65536-entry codebooks), ``dim`` (8 or 16 values per point), ``on_gpu`` (data and
    centroids on the GPU), ``dtype`` (fp32), ``out_group_size`` 1 (the points of ``init_aq_kmeans`` are then groups of ``dim`` input
    features) and the ``KMEANS_KERNEL`` switch.  No region is declined on timing grounds: the kernel route took 0.028 to 0.068 of the
    torch route's time per iteration and 0.032 to 0.139 for a whole initialisation in every cell measured, k = 256 included
    (profiles/kmeans.json)."""
    return bool(KMEANS_KERNEL and on_gpu and dtype == torch.float32 and dim in (8, 16) and out_group_size == 1
                and 128 <= k <= 65536 and k % 128 == 0)


def _kmeans_refuse(who: str, options: dict) -> None:
    for name in _KMEANS_NOT_OFFERED:
        if options.pop(name, None):
            raise NotImplementedError(f"{who}: {name} is not offered")
    if options:
        raise TypeError(f"{who}: unexpected arguments {sorted(options)}")


def _kmeans_absmax(who: str, data: torch.Tensor) -> float:
    """max|data| -- the one synchronisation of a fit; a NaN or an Inf anywhere in ``data`` comes out of it and raises."""
    if data.dim() != 2 or not data.is_floating_point() or data.shape[0] < 1:
        raise ValueError(f"{who}: data must be a floating-point [n, d] tensor with n >= 1, got {data.dtype} {tuple(data.shape)}")
    absmax = float(data.abs().max())
    if not math.isfinite(absmax):
        raise ValueError(f"{who}: data holds a non-finite value")
    return absmax


def _nearest_torch(data: torch.Tensor, centroids: torch.Tensor) -> torch.Tensor:
    """[n] int64, the reference's formula: ``argmax_c <x, C_c> - |C_c|^2 / 2`` in chunks of ``KMEANS_CHUNK_VALUES`` scores."""
    norms = torch.bmm(centroids[:, None, :], centroids[:, :, None]).flatten()
    rows = max(1, KMEANS_CHUNK_VALUES // centroids.shape[0])
    out = torch.empty((data.shape[0],), dtype=torch.int64, device=data.device)
    for a in range(0, data.shape[0], rows):
        out[a:a + rows] = torch.addmm(norms, data[a:a + rows], centroids.T, beta=-0.5).argmax(1)
    return out


def _kmeans_nearest(data: torch.Tensor, centroids: torch.Tensor, kernel: bool) -> torch.Tensor:
    if kernel:
        from .inference_kernels import hip_kernel

        return hip_kernel.kmeans_assign(data, centroids, 0.0, with_sums=False)[0].to(torch.int64)
    return _nearest_torch(data, centroids)


def _kmeans_step(data: torch.Tensor, centroids: torch.Tensor, absmax: float, kernel: bool) -> torch.Tensor:
    """The centroids after one Lloyd iteration; a cluster without points keeps its centroid."""
    if kernel:
        from .inference_kernels import hip_kernel

        _, sums, counts = hip_kernel.kmeans_assign(data, centroids, absmax)
        return hip_kernel.kmeans_update(centroids, sums, counts, data.shape[0], absmax)
    with warnings.catch_warnings():
        warnings.filterwarnings("ignore", message="index_reduce.. is in beta")
        return centroids.clone().index_reduce_(0, _nearest_torch(data, centroids), data, "mean", include_self=False)


def _randperm(n: int, generator: Optional[torch.Generator], device) -> torch.Tensor:
    where = generator.device if generator is not None else "cpu"
    return torch.randperm(n, generator=generator, device=where).to(device)


@torch.no_grad()
def _fit_kmeans(data, k, max_iter, check_every, rtol, atol, initial_centroids, generator, out_group_size=1):
    absmax = _kmeans_absmax("fit_kmeans", data)
    if k < 1:
        raise ValueError(f"fit_kmeans: k = {k} centroids")
    if initial_centroids is None:
        rows = _randperm(data.shape[0], generator, data.device)[:k]
        if k > data.shape[0]:  # fewer points than centroids (a 65536-entry codebook on a small layer): the draw repeats
            rows = rows[torch.arange(k, device=data.device) % data.shape[0]]
        centroids = data[rows, :]
    else:
        if tuple(initial_centroids.shape) != (k, data.shape[1]):
            raise ValueError(f"fit_kmeans: initial_centroids must be [{k}, {data.shape[1]}], got {tuple(initial_centroids.shape)}")
        centroids = initial_centroids.to(device=data.device, dtype=data.dtype)
    data = data.contiguous()
    centroids = centroids.contiguous()
    kernel = takes_kmeans_kernel(k, data.shape[1], data.is_cuda, data.dtype, out_group_size)
    iterations = 0
    for i in range(max_iter):
        new_centroids = _kmeans_step(data, centroids, absmax, kernel)
        iterations = i + 1
        if i % check_every == 0 and torch.allclose(new_centroids, centroids, rtol=rtol, atol=atol):
            break
        centroids = new_centroids
    indices = _kmeans_nearest(data, centroids, kernel)
    return centroids, indices, centroids[indices], iterations


def fit_kmeans(data: torch.Tensor, k: int, max_iter: int = 1000, check_every: int = 10, rtol: float = 1e-6, atol: float = 1e-8,
               initial_centroids: Optional[torch.Tensor] = None, generator: Optional[torch.Generator] = None, *,
               return_iterations: bool = False, **unsupported):
    """Lloyd's k-means of ``data`` [n, d] into ``k`` centroids -- the reference's ``fit_kmeans`` (src/kmeans.py:24-117) -> ``(centroids
    [k, d], indices int64 [n], reconstructed [n, d])``, with the number of Lloyd iterations run as a fourth item under
    ``return_iterations``.  The start is ``initial_centroids`` or ``data[randperm(n, generator)[:k]]`` (with fewer than ``k`` points the
    draw repeats -- the reference fails there: the repeats tie with their originals, never win and stay where they are, so a
    65536-entry codebook can be fitted to a small layer).  Every iteration assigns each
    point to ``argmin_c |C_c|^2 - 2 <x, C_c>`` and moves every centroid that has points to their mean (one without keeps its place);
    at ``i % check_every == 0`` the loop stops when ``allclose(new, old, rtol, atol)`` and keeps the OLD centroids, as the reference
    does (this synchronises: k-means is not meant to be captured); a last assignment gives the indices.

    Routes: fp32 data on the MI355X with d 8 / 16 and k a multiple of 128 up to 65536 runs ``aqlm_hip_kmeans_assign`` /
    ``aqlm_hip_kmeans_update`` (the n x k scores are accumulators of the matrix unit; equal scores give the smallest
    index; the means are sums of fixed-point integers, so they are bit-reproducible); everything else (host tensors, other d or k,
    other dtypes, ``KMEANS_KERNEL = False``) runs the reference's formula in torch.  Once per fit ``data`` is checked to be finite
    (one synchronisation; ``ValueError`` on both routes).  Not offered: ``greedy_init``, ``use_faiss``, ``devices``
    (``NotImplementedError``)."""
    _kmeans_refuse("fit_kmeans", unsupported)
    out = _fit_kmeans(data, int(k), int(max_iter), int(check_every), rtol, atol, initial_centroids, generator)
    return out if return_iterations else out[:3]


@torch.no_grad()
def find_nearest_cluster(data: torch.Tensor, centroids: torch.Tensor, **unsupported):
    """``(indices int64 [n], reconstructed [n, d])``: per row of ``data`` the nearest row of ``centroids`` and that row -- the reference's
    ``find_nearest_cluster`` (src/kmeans.py:162-186); routes and the finite check as in ``fit_kmeans`` (the kernel route is the
    assignment entry without its sums)."""
    _kmeans_refuse("find_nearest_cluster", unsupported)
    _kmeans_absmax("find_nearest_cluster", data)
    if centroids.dim() != 2 or centroids.shape[1] != data.shape[1]:
        raise ValueError(f"find_nearest_cluster: centroids must be [k, {data.shape[1]}], got {tuple(centroids.shape)}")
    centroids = centroids.to(device=data.device, dtype=data.dtype).contiguous()
    kernel = takes_kmeans_kernel(centroids.shape[0], data.shape[1], data.is_cuda, data.dtype)
    indices = _kmeans_nearest(data.contiguous(), centroids, kernel)
    return indices, centroids[indices]


@torch.no_grad()
def init_aq_kmeans(reference_weight: torch.Tensor, *, num_codebooks: int, out_group_size: int, in_group_size: int, codebook_size: int,
                   max_iter: int = 100, max_points_per_centroid: Optional[int] = None, generator: Optional[torch.Generator] = None,
                   **options):
    """Initial ``(codes int64 [out_groups, in_groups, K], codebooks fp32 [K, codebook_size, out_group_size, in_group_size])`` of an AQLM
    layer by residual k-means -- the reference's ``init_aq_kmeans`` (src/aq.py:288-356): for each codebook in turn the residue of
    ``reference_weight`` [out, in], cut into groups of ``out_group_size x in_group_size`` weights, is clustered into ``codebook_size``
    centroids (``fit_kmeans`` with ``max_iter``, default the 100 of the reference's recipes, and the other ``options`` it takes:
    ``check_every``, ``rtol``, ``atol``) -- on a random subsample of ``max_points_per_centroid * codebook_size`` groups when that is
    set -- then every group takes its nearest centroid, which is subtracted from the residue.  Routes as in ``fit_kmeans``;
    ``out_group_size > 1`` runs the torch route.  A float64 weight is clustered in float64, any other in fp32."""
    _kmeans_refuse("init_aq_kmeans", {name: options.pop(name) for name in _KMEANS_NOT_OFFERED if name in options})
    fit_options = {name: options.pop(name) for name in ("check_every", "rtol", "atol") if name in options}
    if options:
        raise TypeError(f"init_aq_kmeans: unexpected arguments {sorted(options)}")
    if reference_weight.dim() != 2 or reference_weight.shape[0] % out_group_size or reference_weight.shape[1] % in_group_size:
        raise ValueError(f"init_aq_kmeans: a weight of {tuple(reference_weight.shape)} does not divide into groups of "
                         f"{out_group_size} x {in_group_size}")
    out_features, in_features = reference_weight.shape
    out_groups, in_groups = out_features // out_group_size, in_features // in_group_size
    compute = torch.float64 if reference_weight.dtype == torch.float64 else torch.float32
    residue = (reference_weight.detach().to(compute).reshape(out_groups, out_group_size, in_groups, in_group_size).swapaxes(-3, -2)
               .reshape(out_groups * in_groups, out_group_size * in_group_size).clone())
    kernel = takes_kmeans_kernel(codebook_size, residue.shape[1], residue.is_cuda, residue.dtype, out_group_size)
    codes, codebooks = [], []
    for _ in range(num_codebooks):
        sample = residue
        if max_points_per_centroid is not None:
            sample = residue[_randperm(residue.shape[0], generator, residue.device)[:max_points_per_centroid * codebook_size], :]
        book = _fit_kmeans(sample, int(codebook_size), int(max_iter), int(fit_options.get("check_every", 10)), fit_options.get("rtol", 1e-6),
                           fit_options.get("atol", 1e-8), None, generator, out_group_size)[0]
        chosen = _kmeans_nearest(residue, book, kernel)
        residue -= book[chosen]
        codes.append(chosen.reshape(out_groups, in_groups, 1))
        codebooks.append(book.reshape(1, codebook_size, out_group_size, in_group_size))
    return torch.cat(codes, dim=-1), torch.cat(codebooks, dim=0).to(torch.float32)


@torch.no_grad()
def init_layer_kmeans_(layer, reference_weight: torch.Tensor, **options) -> torch.Tensor:
    """Give ``layer`` (a ``QuantizedLinear``) its first codes, codebooks and scales from the dense ``reference_weight`` [out, in], as the
    reference's ``QuantizedWeight.__init__`` does with ``scale_nbits = 0`` (src/aq.py:76-115): ``scales`` = the norm of every output
    group + 1e-9, ``init_aq_kmeans`` (same ``options``) on ``W / scales``.  Everything is written IN PLACE -- the codes in the
    checkpoint's storage type, codebooks and scales in the layer's dtype -- so the version counters move and every derived copy
    (packed / planar codes, dense W, fast lane, inverted index) is rebuilt at the layer's next call, by the rule of ``update_codes_``;
    dropped canonical codes come back first, inference tensors raise ``RuntimeError``, the experts of a ``QuantizedMixtralExperts``
    block and ``ShardedQuantizedLinear`` raise ``TypeError``.  Returns ``||W - W_q||^2 / ||W||^2`` of the values written (a 0-dim
    tensor, before their rounding to the layer's dtype)."""
    from .inference import QuantizedLinear
    from .moe import QuantizedMixtralExperts
    from .sharded import ShardedQuantizedLinear
    from .utils import _dequantize_weight, pack_int_data

    if isinstance(layer, (QuantizedMixtralExperts, ShardedQuantizedLinear)) or getattr(layer, "_moe_expert", False):
        raise TypeError(f"init_layer_kmeans_: {type(layer).__name__}{' (an expert of a QuantizedMixtralExperts block)' if getattr(layer, '_moe_expert', False) else ''}"
                        " is outside the scope of the initialisation (as it is of make_trainable)")
    if not isinstance(layer, QuantizedLinear):
        raise TypeError(f"init_layer_kmeans_: expected a QuantizedLinear, got {type(layer).__name__}")
    _kmeans_refuse("init_layer_kmeans_", {name: options[name] for name in _KMEANS_NOT_OFFERED if name in options})
    if tuple(reference_weight.shape) != (layer.out_features, layer.in_features):
        raise ValueError(f"init_layer_kmeans_: the layer is {layer.in_features} -> {layer.out_features}, the weight {tuple(reference_weight.shape)}")
    layer.restore_canonical_codes()
    if layer.codes.is_inference() or layer.codebooks.is_inference() or layer.scales.is_inference():
        raise RuntimeError("init_layer_kmeans_: the parameters of this layer are inference tensors (the model was built or loaded under "
                           "torch.inference_mode()); they cannot be written in place -- build the model outside inference mode")
    weight = reference_weight.detach().to(device=layer.codes.device, dtype=torch.float32)
    out_groups = layer.out_features // layer.out_group_size
    scales = weight.reshape(out_groups, -1).norm(dim=-1) + 1e-9
    unscaled = (weight.reshape(out_groups, -1) / scales[:, None]).reshape_as(weight)
    codes, codebooks = init_aq_kmeans(unscaled, num_codebooks=layer.num_codebooks, out_group_size=layer.out_group_size,
                                      in_group_size=layer.in_group_size, codebook_size=layer.codebook_size, **options)
    layer.codes.copy_(pack_int_data(codes, layer.nbits_per_codebook))
    layer.codebooks.copy_(codebooks)
    layer.scales.copy_(scales.reshape(-1, 1, 1, 1))
    error = weight - _dequantize_weight(codes, codebooks, scales.reshape(-1, 1, 1, 1))
    return error.square().sum() / weight.square().sum()


# ---------------------------------------------------------------------------------------------------------------------------
# calibrated training of codebooks and scales, and the loop that produces a layer (the reference's AQEngine: aq_engine.py)
# ---------------------------------------------------------------------------------------------------------------------------
# The switch of the calibrated gradient kernels: False sends every ``calibrated_loss_and_grads`` call through the torch route.
CALIBRATED_GRAD_KERNEL = True


def takes_calibrated_grad_kernel(num_codebooks: int, nbits_per_codebook: int, out_group_size: int, in_group_size: int, on_gpu: bool,
                                 dtypes_ok: bool, supported: bool) -> bool:
    """Whether a ``calibrated_loss_and_grads`` call runs the ``aqlm_hip_calib_*`` entries -- a pure function of: the scheme (one codebook
    of 16 bits with g 8 / 16, or 1 to 8 codebooks of 8 bits with g 8 / 16 / 32; ``out_group_size`` 1), ``on_gpu`` (every tensor on the GPU),
    ``dtypes_ok`` (codebooks, scales and ``XTX`` fp32, the target fp32 / fp16 / bf16, codes int16 for 16 bits and int8 for 8), ``supported``
    (the library's ``_supported`` queries) and the ``CALIBRATED_GRAD_KERNEL`` switch.  No region is declined on timing grounds: the kernel
    route took 0.10 to 0.37 of the torch route's time per step in every cell measured (profiles/calibrated_train.json)."""
    wide = num_codebooks == 1 and nbits_per_codebook == 16 and in_group_size in (8, 16)
    narrow = 1 <= num_codebooks <= 8 and nbits_per_codebook == 8 and in_group_size in (8, 16, 32)
    return bool(CALIBRATED_GRAD_KERNEL and (wide or narrow) and out_group_size == 1 and on_gpu and dtypes_ok and supported)


def _calibrated_grad_route(codes, codebooks, scales, reference_weight, XTX) -> bool:
    K, size, out_group_size, in_group_size = codebooks.shape
    nbits = int(math.log2(size))
    on_gpu = all(t.is_cuda for t in (codes, codebooks, scales, reference_weight, XTX))
    dtypes_ok = (codebooks.dtype == torch.float32 and scales.dtype == torch.float32 and XTX.dtype == torch.float32
                 and reference_weight.dtype in (torch.float32, torch.float16, torch.bfloat16)
                 and codes.dtype == (torch.int16 if nbits == 16 else torch.int8))
    supported = False
    if CALIBRATED_GRAD_KERNEL and on_gpu and out_group_size == 1 and nbits in (8, 16):
        from .inference_kernels import hip_kernel

        supported = hip_kernel.calib_supported(reference_weight.shape[0], reference_weight.shape[1], K, nbits, in_group_size)
    return takes_calibrated_grad_kernel(K, nbits, out_group_size, in_group_size, on_gpu, dtypes_ok, supported)


def calibrated_loss_and_grads(codes: torch.Tensor, codebooks: torch.Tensor, scales: torch.Tensor, reference_weight: torch.Tensor,
                              XTX: torch.Tensor, *, index=None):
    """``(loss, d_codebooks, d_scales)`` of the calibrated objective ``loss = tr((W_q - W_ref) XTX (W_q - W_ref)^T) / out_features`` -- the
    reference's ``AQEngine._compute_mse`` (aq_engine.py:108-131) and its backward -- for ``codes`` [out_groups, in_groups, K] in the stored
    int8 / int16 wrap-around form, ``codebooks`` [K, S, out_group_size, in_group_size] and ``scales`` [out_groups, 1, 1, 1].  ``loss`` is a
    0-dim tensor (fp64 on the kernel route, which adds the fp32 shares of the rows in fp64; the compute dtype on the torch route), the
    gradients have the shapes of their parameters.

    ``XTX`` IS TAKEN TO BE SYMMETRIC (``X^T X`` is; ``quantize_layer_`` symmetrises what it is given): the kernel route forms the one
    product ``G = D XTX`` and uses it for the loss and, as ``(XTX + XTX^T) D^T / 2``, for both gradients.

    Routes: fp32 codebooks and scales (master parameters), fp32 ``XTX`` and an fp32 / fp16 / bf16 target on the MI355X, for 1x16 layers
    (g 8 / 16) and K x 8 layers (K 1 to 8, g 8 / 16 / 32) with ``out_group_size`` 1, run ``aqlm_hip_calib_delta`` (``D = W_q - W_ref``,
    the bits of torch's fp32 ``_dequantize_weight(...) - W_ref``), ``torch.mm(D, XTX)``, ``aqlm_hip_calib_rows`` (per row the scale
    gradient and the row's share of the loss, from the stored ``D``) and ``aqlm_hip_calib_codebook_grad_1x16`` (through ``index``, a
    ``hip_kernel.CodebookGradIndex`` of these codes: built here when None, which a hipGraph capture cannot do) or
    ``aqlm_hip_calib_codebook_grad_kx8`` (a non-finite element of ``G`` or the scales makes the whole K x 8 codebook
    gradient NaN).  No atomics, bit-reproducible, no host synchronisation.  Everything else -- host tensors, ``out_group_size > 1``,
    other schemes, g 32 with 16-bit codes, fp16 / bf16 or fp64 parameters, ``CALIBRATED_GRAD_KERNEL = False`` -- runs ``_compute_mse``
    restated on ``_dequantize_weight`` under autograd, in fp32 (fp64 when any input is fp64): slow, correct, never silent."""
    if codes.dim() != 3 or codebooks.dim() != 4 or codes.shape[2] != codebooks.shape[0]:
        raise ValueError("calibrated_loss_and_grads: codes are [out_groups, in_groups, K], codebooks [K, S, out_group_size, in_group_size]")
    K, size, out_group_size, in_group_size = codebooks.shape
    out_features, in_features = codes.shape[0] * out_group_size, codes.shape[1] * in_group_size
    if tuple(reference_weight.shape) != (out_features, in_features) or tuple(XTX.shape) != (in_features, in_features):
        raise ValueError(f"calibrated_loss_and_grads: a layer of {in_features} -> {out_features} needs a target of [{out_features}, "
                         f"{in_features}] and XTX [{in_features}, {in_features}], got {tuple(reference_weight.shape)} and {tuple(XTX.shape)}")
    if scales.numel() != codes.shape[0]:
        raise ValueError(f"calibrated_loss_and_grads: scales must hold one factor per output group ({codes.shape[0]})")
    if _calibrated_grad_route(codes, codebooks, scales, reference_weight, XTX):
        from .inference_kernels import hip_kernel

        with torch.no_grad():
            stored = codes.detach()
            stored = stored if stored.is_contiguous() else stored.contiguous()
            reference = reference_weight.detach()
            reference = reference if reference.stride(1) == 1 else reference.contiguous()
            delta = hip_kernel.calib_delta(stored, codebooks, scales, reference)
            product = torch.mm(delta, XTX.detach())
            ds_raw, rowloss = hip_kernel.calib_rows(product, delta, stored, codebooks)
            if size == 65536:
                if index is None:
                    index = hip_kernel.build_codebook_grad_index(stored, in_group_size)
                d_books = hip_kernel.calib_codebook_grad_1x16(product, scales, index)
            else:
                d_books = hip_kernel.calib_codebook_grad_kx8(product, scales, stored, in_group_size)
            factor = 2.0 / out_features
            # (the rows' shares are added in fp64: the last sum of the loss adds no rounding of its own to theirs)
            return rowloss.sum(dtype=torch.float64) / out_features, (d_books * factor).reshape(codebooks.shape), (ds_raw * factor).reshape(scales.shape)

    from .utils import _dequantize_weight

    wide = any(t.dtype == torch.float64 for t in (codebooks, scales, reference_weight, XTX))
    compute = torch.float64 if wide else torch.float32
    with torch.enable_grad():
        books = codebooks.detach().to(compute).requires_grad_(True)
        factors = scales.detach().to(compute).requires_grad_(True)
        weight = _dequantize_weight(codes.detach().to(torch.int64) % size, books, factors)
        delta = weight - reference_weight.detach().to(compute)
        loss = (delta @ XTX.detach().to(compute)).flatten() @ delta.flatten() / out_features
        d_books, d_factors = torch.autograd.grad(loss, (books, factors))
    return loss.detach(), d_books, d_factors


@torch.no_grad()
def accumulate_xtx_(XTX: torch.Tensor, nsamples: int, inp: torch.Tensor) -> int:
    """Add a batch of layer inputs ``inp`` ([n, in] or [batch, seq, in]) to the running mean ``XTX`` [in, in] of ``x x^T`` over the
    ``nsamples`` rows seen so far, IN PLACE and in the accumulator's dtype -- the reference's ``AQEngine.add_batch`` (aq_engine.py:30-42):
    ``XTX *= nsamples / (nsamples + n); XTX += (x / sqrt(nsamples + n))^T (x / sqrt(nsamples + n))``.  Returns the new ``nsamples``."""
    if inp.dim() == 3:
        inp = inp.reshape(-1, inp.shape[-1])
    if inp.dim() != 2 or XTX.dim() != 2 or tuple(XTX.shape) != (inp.shape[1], inp.shape[1]):
        raise ValueError(f"accumulate_xtx_: inputs of {tuple(inp.shape)} do not fit an accumulator of {tuple(XTX.shape)}")
    rows = int(inp.shape[0])
    XTX *= nsamples / (nsamples + rows)
    nsamples = int(nsamples) + rows
    scaled = math.sqrt(1 / nsamples) * inp.t().to(XTX.dtype)
    XTX += scaled.matmul(scaled.t())
    return nsamples


def _calibrated_search_route(layer, reference_weight, XTX, beam_size: int) -> str:
    """"kernel" or "torch": what ``find_optimal_codes_calibrated`` runs for this layer (its predicates on its conditions)."""
    K, nbits, g = layer.num_codebooks, layer.nbits_per_codebook, layer.in_group_size
    tensors = (XTX, reference_weight, layer.codebooks, layer.codes, layer.scales)
    on_gpu = all(t.is_cuda for t in tensors)
    floats_ok = (layer.codebooks.dtype in (torch.float16, torch.bfloat16) and layer.scales.dtype == layer.codebooks.dtype
                 and XTX.dtype == torch.float32 and reference_weight.dtype in (torch.float32, torch.float16, torch.bfloat16))
    if not (CODE_SEARCH_KERNEL and on_gpu and floats_ok and layer.out_group_size == 1):
        return "torch"
    from .inference_kernels import hip_kernel

    if nbits == 8 and 1 <= K <= 8 and g in (8, 16, 32) and 1 <= beam_size <= 16:
        supported = hip_kernel.code_search_kx8_xtx_supported(layer.out_features, K, g, beam_size, beam_size)
        taken = takes_code_search_kernel_kx8_xtx(K, nbits, 1, g, beam_size, on_gpu, layer.codes.dtype == torch.int8, supported)
    elif nbits == 16 and K == 1 and g in (8, 16) and 1 <= beam_size <= 8:
        supported = hip_kernel.code_search_1x16_xtx_supported(layer.out_features, g, beam_size, beam_size)
        taken = takes_code_search_kernel_1x16_xtx(nbits, K, 1, g, beam_size, on_gpu, layer.codes.dtype == torch.int16, supported)
    else:
        taken = False
    return "kernel" if taken else "torch"


def quantize_layer_(layer, reference_weight: torch.Tensor, XTX: torch.Tensor, *, lr: float = 1e-4, max_epochs: int = 1000,
                    steps_per_epoch: int = 100, relative_mse_tolerance: Optional[float] = None, beam_size: int = 1, init: bool = True,
                    init_max_iter: int = 100, init_max_points_per_centroid: Optional[int] = None,
                    generator: Optional[torch.Generator] = None, seed=None, callback=None) -> dict:
    """Turn the dense ``reference_weight`` [out, in] and the calibration statistics ``XTX`` [in, in] (``accumulate_xtx_``) into the codes,
    codebooks and scales of ``layer`` (a ``QuantizedLinear``), IN PLACE -- the loop of the reference's ``AQEngine.quantize``
    (aq_engine.py:44-106):
      * ``XTX`` is made symmetric once, ``(XTX + XTX^T) / 2``: the objective does not change and the one-GEMM gradient of
        ``calibrated_loss_and_grads`` is exact.  It is used in fp32 (fp64 when the target is fp64);
      * unless ``init=False`` the layer is initialised by ``init_layer_kmeans_`` (``init_max_iter``, ``init_max_points_per_centroid``,
        ``generator``);
      * fp32 masters of the codebooks and scales (fp64 for an fp64 layer) train under ``torch.optim.Adam(lr, betas=(0.0, 0.95),
        amsgrad=True)``: every epoch ``steps_per_epoch`` steps of ``calibrated_loss_and_grads``, with the reference's early stop on the
        loss of an epoch's step 0 (``relative_mse_tolerance``: stop when ``loss / best so far > 1 - tolerance``; a non-finite loss
        raises ``ValueError``);
      * at the end of an epoch the masters are written into the layer IN ITS DTYPE and the codes are re-chosen by
        ``update_codes_calibrated_(beam_size=..., dim_order=...)``, one order of the codebooks per input group drawn from
        ``random.Random(seed)``.  THE SEARCH THEREFORE SEES THE CODEBOOKS AND SCALES AS INFERENCE WILL -- rounded to the layer's dtype --
        while the masters keep training unrounded (the reference searches on its fp32 parameters and rounds once at the end).  An fp32
        layer's masters are exact copies of its own parameters; its search takes the torch route;
      * the inverted index of a 1x16 layer is the layer's cached one (``codebook_grad_index``): rebuilt only when a search changed codes.
    ``callback(event, epoch, info)`` is called with ``"trained"`` (masters written, before the search; ``info["loss"]``: the loss of the
    epoch's step 0 or None) and ``"searched"`` (``info["changed"]``).

    Returns a dict: ``losses`` (per epoch, the loss at its step 0), ``changed`` (groups whose codes each search changed),
    ``initial_error`` and ``error`` (``calibrated_error`` of the layer before the first epoch and at the end), ``epochs`` run,
    ``stopped_early`` and ``routes`` (``{"init", "grad", "search"}``: "kernel" or "torch" each; "init" None without one).  Refusals as in
    ``update_codes_calibrated_``: the experts of a ``QuantizedMixtralExperts`` block and ``ShardedQuantizedLinear`` raise ``TypeError``,
    inference tensors ``RuntimeError``."""
    import random

    from .inference import QuantizedLinear
    from .moe import QuantizedMixtralExperts
    from .sharded import ShardedQuantizedLinear

    if isinstance(layer, (QuantizedMixtralExperts, ShardedQuantizedLinear)) or getattr(layer, "_moe_expert", False):
        raise TypeError(f"quantize_layer_: {type(layer).__name__}{' (an expert of a QuantizedMixtralExperts block)' if getattr(layer, '_moe_expert', False) else ''}"
                        " is outside the scope of the quantization loop (as it is of make_trainable)")
    if not isinstance(layer, QuantizedLinear):
        raise TypeError(f"quantize_layer_: expected a QuantizedLinear, got {type(layer).__name__}")
    if tuple(reference_weight.shape) != (layer.out_features, layer.in_features) or tuple(XTX.shape) != (layer.in_features, layer.in_features):
        raise ValueError(f"quantize_layer_: the layer is {layer.in_features} -> {layer.out_features}, the weight {tuple(reference_weight.shape)}, "
                         f"XTX {tuple(XTX.shape)}")
    if max_epochs < 0 or steps_per_epoch < 0 or not lr > 0:
        raise ValueError("quantize_layer_: max_epochs >= 0, steps_per_epoch >= 0, lr > 0")
    with torch.no_grad():
        layer.restore_canonical_codes()
        if layer.codes.is_inference() or layer.codebooks.is_inference() or layer.scales.is_inference():
            raise RuntimeError("quantize_layer_: the parameters of this layer are inference tensors (the model was built or loaded under "
                               "torch.inference_mode()); they cannot be written in place -- build the model outside inference mode")
        device = layer.codes.device
        wide = reference_weight.dtype == torch.float64
        reference = reference_weight.detach().to(device)
        stats = XTX.detach().to(device)
        stats = (0.5 * (stats + stats.T)).to(torch.float64 if wide else torch.float32).contiguous()
        routes = {"init": None, "grad": None, "search": None}
        if init:
            routes["init"] = "kernel" if takes_kmeans_kernel(layer.codebook_size, layer.in_group_size, device.type == "cuda", torch.float32,
                                                             layer.out_group_size) else "torch"
            init_layer_kmeans_(layer, reference, max_iter=init_max_iter, max_points_per_centroid=init_max_points_per_centroid,
                               generator=generator)
        master_dtype = torch.float64 if layer.codebooks.dtype == torch.float64 else torch.float32
        books = layer.codebooks.detach().to(master_dtype).clone()
        factors = layer.scales.detach().to(master_dtype).clone()
        initial_error = float(calibrated_error(layer, reference, stats))
    optimizer = torch.optim.Adam([books, factors], lr=lr, betas=(0.0, 0.95), amsgrad=True)
    rng = random.Random(seed)
    takes_index = layer.num_codebooks == 1 and layer.nbits_per_codebook == 16
    losses, changed = [], []
    best, stopped, epochs = float("inf"), False, 0
    for epoch in range(max_epochs):
        first = None
        if steps_per_epoch:
            kernel = _calibrated_grad_route(layer.codes, books, factors, reference, stats)
            routes["grad"] = "kernel" if kernel else "torch"
            index = layer.codebook_grad_index() if kernel and takes_index else None
        for step in range(steps_per_epoch):
            loss, d_books, d_factors = calibrated_loss_and_grads(layer.codes.detach(), books, factors, reference, stats, index=index)
            value = float(loss)
            if not math.isfinite(value):
                raise ValueError(f"quantize_layer_: the calibrated loss is {value}")
            if step == 0:
                first = value
                if relative_mse_tolerance is not None:
                    if value / best > 1.0 - relative_mse_tolerance:
                        stopped = True  # (no update after the last epoch's search, as in the reference)
                        break
                    best = min(best, value)
            books.grad, factors.grad = d_books.to(master_dtype), d_factors.to(master_dtype)
            optimizer.step()
        if stopped:
            break
        epochs = epoch + 1
        if first is not None:
            losses.append(first)
        with torch.no_grad():
            layer.codebooks.copy_(books)
            layer.scales.copy_(factors)
        if callback is not None:
            callback("trained", epoch, {"loss": first})
        routes["search"] = _calibrated_search_route(layer, reference, stats, beam_size)
        K = layer.num_codebooks
        orders = [rng.sample(range(K), K) for _ in range(layer.in_features // layer.in_group_size)]
        moved = int(update_codes_calibrated_(layer, reference, stats, beam_size=beam_size, dim_order=orders))
        changed.append(moved)
        if callback is not None:
            callback("searched", epoch, {"changed": moved})
    return {"losses": losses, "changed": changed, "initial_error": initial_error, "error": float(calibrated_error(layer, reference, stats)),
            "epochs": epochs, "stopped_early": stopped, "routes": routes}
