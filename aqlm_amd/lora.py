"""LoRA adapters served on top of AQLM layers, a different adapter for every row of a decode batch if need be.

An adapter cannot be merged into an AQLM base -- the weights exist as codes + codebooks only -- so a fine-tuned AQLM model keeps
its adapters at inference, at every token.  ``attach_adapters(model, {...})`` wraps the targeted dense ``QuantizedLinear`` layers
(attention and MLP projections, the attention projections of Mixtral included) in ``LoraQuantizedLinear``, every
``QuantizedMixtralExperts`` block whose experts an adapter targets (``...experts.<e>.w1`` / ``w2`` / ``w3``) in
``LoraQuantizedMixtralExperts``, and returns the ``AdapterBank`` that says which adapter serves which row:

    bank = aqlm.lora.attach_adapters(model, {"math": "adapters/math", "code": "adapters/code"})
    bank.select("math")            # every row
    bank.select(ids)               # a device tensor of adapter ids per row (or per sequence); kept by reference
    bank.select(None)              # base model only: no adapter launch at all

Decode-sized calls run ``aqlm_hip_lora_bgmv`` (aqlm_amd/csrc/lora_bgmv.hip): two launches per layer whatever the mix of adapters,
ids read on the device only, capturable.  Larger calls -- prefill, big batches -- have ``aqlm_hip_lora_sgmv``
(aqlm_amd/csrc/lora_sgmv.hip), the same two launches on the matrix unit, one pass per distinct adapter of every 16-row tile, for
the row counts at which it was measured to win (``SGMV_MAX_ROWS``).  Everything else -- training, host tensors, shapes the kernels
decline -- runs the adapters as torch ops, differentiable in x, A and B, so the same module trains.

Adapters on the ROUTED EXPERTS of a Mixtral block ride on whichever launches the block takes: for up to
``ROUTED_BGMV_MAX_PAIRS`` (token, expert) pairs ``aqlm_hip_lora_bgmv_routed`` (aqlm_amd/csrc/lora_bgmv_routed.hip) adds them in place to
the output of the gate / up launch and of the down launch -- two launches each, adapter ids and expert ids read on the device only,
capturable --; calls of ``ROUTED_SGMV_MIN_PAIRS`` .. ``ROUTED_SGMV_MAX_PAIRS`` pairs (prefill) have ``aqlm_hip_lora_sgmv_routed``
(aqlm_amd/csrc/lora_sgmv_routed.hip), the segmented adapter GEMM on row tiles gathered through an expert bucket of 16-pair tiles that
the provider builds once per forward (one small launch, no sync, capturable), for the pair counts at which it was measured to
win; a call that needs a GRADIENT (``ROUTED_TRAIN_MIN_PAIRS`` .. ``ROUTED_TRAIN_MAX_PAIRS`` pairs) runs that same launch inside an autograd
function whose backward is device launches only -- the launch again on a transposed table for grad_x, ``aqlm_hip_lora_grad_routed``
(aqlm_amd/csrc/lora_routed_bwd.hip) for grad_A and grad_B; no host sync, no atomics, capturable, bit-reproducible --; every other call
(host tensors, ``torch.compile``, shapes the kernels decline) runs PEFT's formula per (adapter,
expert) as masked torch ops in fp32 without a host sync, differentiable in x, A and B, so expert adapters serve prefill and train.  Their
``state_dict()`` keys are ``<block>.base_layer.<e>.<w>.codes``, ``<block>.lora_A.<name>.<e>.<w>.weight`` and
``<block>.lora_B.<name>.<e>.<w>.weight`` (PEFT has no per-expert module convention for fused experts to follow); adapter FILES name
expert targets by the published layout, ``...block_sparse_moe.experts.<e>.w1.lora_A.weight``, or with ``.mlp.`` in its place.

The directory format is PEFT's (``adapter_config.json`` + ``adapter_model.safetensors``) and the parameter names are PEFT's
(``...q_proj.lora_A.<name>.weight``, ``...q_proj.base_layer.codes``); ``peft`` itself is not needed.
"""
from __future__ import annotations

import json
import math
import os
import re
from typing import Dict, List, Optional, Tuple, Union

import torch
import torch.nn as nn
import torch.nn.functional as F

from .derived import tensor_version
from .inference import QuantizedLinear

AQLM_HIP_MAX_LORA_ROWS = 256  # include/aqlm_hip.h: rows one aqlm_hip_lora_bgmv call takes

# Largest of the row counts 1 / 2 / 4 / 8 / 16 / 32 / 64 up to which the captured BGMV route beat the captured plain-torch-ops
# route (x @ A^T @ B^T * scaling + add on top of the unchanged base layer) on a Llama-3-8B-shaped prepacked 1x16 g8 stack with
# rank-16 adapters on all seven projections: profiles/lora_bgmv.json, written by `python tools/lora_benchmark.py`.  0 switches
# the route off.
BGMV_MAX_ROWS = 64

AQLM_HIP_MAX_LORA_SGMV_ROWS = 65536  # include/aqlm_hip.h: rows one aqlm_hip_lora_sgmv call takes

# Calls of SGMV_MIN_ROWS .. SGMV_MAX_ROWS rows run the segmented adapter GEMM (aqlm_hip_lora_sgmv); below, the BGMV route keeps
# every call it had.  SGMV_MAX_ROWS is the largest of the row counts 96 / 128 / 256 / 512 / 1024 / 2048 / 4096 up to which the
# captured SGMV route beat the captured torch path on the same block in all three adapter mixes (one adapter, 4 contiguous
# sequences, 4 adapters interleaved row by row): profiles/lora_sgmv.json, written by `python tools/lora_benchmark.py --prefill`;
# AQLM_HIP_MAX_LORA_SGMV_ROWS when it won at every measured count, which it did.  0 switches the route off.
SGMV_MIN_ROWS = 65
SGMV_MAX_ROWS = AQLM_HIP_MAX_LORA_SGMV_ROWS

# (token, expert) pairs up to which a call on the routed experts runs aqlm_hip_lora_bgmv_routed; beyond it, the torch path.  A
# measured route constant (profiles/lora_moe.json, written by `python tools/lora_moe_benchmark.py`): the largest
# of the pair counts 2 / 4 / 8 / 16 / 32 / 64 / 128 / 256 (T = 1 .. 128 at top_k 2) up to which the captured block with the HIP
# route replayed faster than the captured block with the torch path at every smaller count too, in both adapter mixes (one
# adapter; four adapters mixed per token), on a Mixtral-8x7B-shaped prepacked block with rank-16 adapters on w1 / w2 / w3 of all
# experts.  Measured: it won at every count in both mixes (one token: 119.3 against 843 us captured, bare block 90.4; four adapters
# over 128 tokens: 1707 against 6203 us), so the constant is the launch's own limit.  0 switches the route off.
ROUTED_BGMV_MAX_PAIRS = 256

AQLM_HIP_MAX_LORA_SGMV_ROUTED_PAIRS = 65536  # include/aqlm_hip.h: pairs one aqlm_hip_lora_sgmv_routed call takes

# Calls of ROUTED_SGMV_MIN_PAIRS .. ROUTED_SGMV_MAX_PAIRS pairs on the routed experts run aqlm_hip_lora_sgmv_routed; up to 256
# pairs every call keeps the route it had (the torch path included, when ROUTED_BGMV_MAX_PAIRS is lowered).  ROUTED_SGMV_MAX_PAIRS
# is a measured route constant (profiles/lora_moe_prefill.json, written by `python tools/lora_moe_benchmark.py
# --prefill`): the largest of the pair counts 512 / 1024 / 2048 / 4096 / 8192 (T = 256 .. 4096 at top_k 2) up to which the captured
# block with the HIP route replayed faster than the captured block with the torch path at that count and every smaller one in all
# three adapter mixes (one adapter; four adapters as four contiguous sequences; four adapters interleaved per token), on a
# Mixtral-8x7B-shaped prepacked block with rank-16 adapters on w1 / w2 / w3 of all experts; the launch's own limit when it won at
# every measured count.  Measured: it won at every count in all three mixes (four sequences over 1024 tokens: 4963 against 17090 us
# captured, bare block 4496; four adapters interleaved over 4096 tokens: 19055 against 59975 us, bare block 16351), so the constant
# is the launch's own limit.  0 switches the route off.
ROUTED_SGMV_MIN_PAIRS = 257
ROUTED_SGMV_MAX_PAIRS = AQLM_HIP_MAX_LORA_SGMV_ROUTED_PAIRS

# Calls on the routed experts that NEED A GRADIENT (of x, of the launch's output or of an adapter weight) and have
# ROUTED_TRAIN_MIN_PAIRS .. ROUTED_TRAIN_MAX_PAIRS pairs run aqlm_hip_lora_sgmv_routed inside an autograd function whose backward is
# device launches only (the same launch on a transposed table for grad_x, aqlm_hip_lora_grad_routed for grad_A / grad_B; DESIGN.md
# 4.8k); beyond it, the torch path.  The launch serves every pair count, so one kernel family trains at every size: the BGMV route
# stays out of training.  ROUTED_TRAIN_MAX_PAIRS is a measured route constant (profiles/lora_moe_train.json, written by `python
# tools/lora_moe_benchmark.py --train`): the largest of the pair counts 16 / 512 / 2048 / 8192 up to which forward + backward on
# this route beat the torch path of the same commit at that count and every smaller one in all three adapter mixes (one adapter;
# four contiguous sequences; four adapters interleaved per token), on a Mixtral-8x7B-shaped prepacked block with rank-16 adapters
# on w1 / w2 / w3 of all experts, one of them trained; the launch's own limit when it won at every measured count.  Measured: it
# won at every count in all three mixes and on the skewed routing, eager and captured (four sequences over 1024 tokens: 9442
# against 32444 us captured, bare block's step 8292; one adapter over 4096 tokens: 31007 against 51332 us, bare block 26914; 8
# tokens, four adapters: 2551 against 10213 us), so the constant is the launch's own limit.  0 switches the route off.
ROUTED_TRAIN_MIN_PAIRS = 1
ROUTED_TRAIN_MAX_PAIRS = AQLM_HIP_MAX_LORA_SGMV_ROUTED_PAIRS

_PREFIX = "base_model.model."
_DTYPES_OK = (torch.float16, torch.bfloat16)


def takes_bgmv_route(is_cuda: bool, dtype_ok: bool, grad_needed: bool, compiling: bool, rows: int, supported: bool) -> bool:
    """Whether a call runs the two BGMV launches (else the torch path): tensors on the device, one fp16 / bf16 dtype throughout,
    no gradient needed, not being traced by torch.compile, 1..BGMV_MAX_ROWS rows (never more than one launch takes), and a shape
    the entry accepts."""
    return bool(is_cuda and dtype_ok and not grad_needed and not compiling
                and 1 <= rows <= min(BGMV_MAX_ROWS, AQLM_HIP_MAX_LORA_ROWS) and supported)


def takes_sgmv_route(is_cuda: bool, dtype_ok: bool, grad_needed: bool, compiling: bool, rows: int, supported: bool) -> bool:
    """Whether a call that did not take the BGMV route runs the two SGMV launches (else the torch path): the same conditions as
    ``takes_bgmv_route`` with SGMV_MIN_ROWS..SGMV_MAX_ROWS rows (never more than one launch takes)."""
    return bool(is_cuda and dtype_ok and not grad_needed and not compiling
                and SGMV_MIN_ROWS <= rows <= min(SGMV_MAX_ROWS, AQLM_HIP_MAX_LORA_SGMV_ROWS) and supported)


def takes_routed_bgmv_route(is_cuda: bool, dtype_ok: bool, grad_needed: bool, compiling: bool, pairs: int, supported: bool) -> bool:
    """Whether a call on the routed experts runs the two launches of aqlm_hip_lora_bgmv_routed (else the torch path): the conditions
    of ``takes_bgmv_route`` with 1..ROUTED_BGMV_MAX_PAIRS (token, expert) pairs (never more than one launch takes)."""
    return bool(is_cuda and dtype_ok and not grad_needed and not compiling
                and 1 <= pairs <= min(ROUTED_BGMV_MAX_PAIRS, AQLM_HIP_MAX_LORA_ROWS) and supported)


def takes_routed_sgmv_route(is_cuda: bool, dtype_ok: bool, grad_needed: bool, compiling: bool, pairs: int, supported: bool) -> bool:
    """Whether a call on the routed experts that did not take the BGMV route runs the two launches of aqlm_hip_lora_sgmv_routed
    (else the torch path): the conditions of ``takes_routed_bgmv_route`` with ROUTED_SGMV_MIN_PAIRS..ROUTED_SGMV_MAX_PAIRS
    (token, expert) pairs (never more than one launch takes)."""
    return bool(is_cuda and dtype_ok and not grad_needed and not compiling
                and ROUTED_SGMV_MIN_PAIRS <= pairs <= min(ROUTED_SGMV_MAX_PAIRS, AQLM_HIP_MAX_LORA_SGMV_ROUTED_PAIRS) and supported)


def takes_routed_train_route(is_cuda: bool, dtype_ok: bool, grad_needed: bool, compiling: bool, pairs: int, supported: bool) -> bool:
    """Whether a call on the routed experts that needs a gradient runs the device route (aqlm_hip_lora_sgmv_routed under autograd,
    backward on launches only; else the torch path): tensors on the device, one fp16 / bf16 dtype throughout, a gradient needed,
    not being traced by torch.compile, ROUTED_TRAIN_MIN_PAIRS..ROUTED_TRAIN_MAX_PAIRS (token, expert) pairs (never more than one
    launch takes), and shapes the launches accept."""
    return bool(is_cuda and dtype_ok and grad_needed and not compiling
                and ROUTED_TRAIN_MIN_PAIRS <= pairs <= min(ROUTED_TRAIN_MAX_PAIRS, AQLM_HIP_MAX_LORA_SGMV_ROUTED_PAIRS) and supported)


class AdapterBank:
    """The adapters attached to one model and the current selection.  ``names[i]`` is the adapter that id ``i`` selects."""

    def __init__(self, names: List[str]):
        self.names: List[str] = list(names)
        self.layers: List[Union["LoraQuantizedLinear", "LoraQuantizedMixtralExperts"]] = []
        self.selection: Union[None, str, torch.Tensor] = None
        self._replaced: List[Tuple[nn.Module, str, nn.Module]] = []  # (parent, child name, the original module)

    def index(self, name: str) -> int:
        return self.names.index(name)

    def select(self, which: Union[None, str, torch.Tensor]) -> "AdapterBank":
        """``None``: base only.  A name: every row uses that adapter.  An int64 / int32 tensor of ids (indices into ``names``), one
        per row of the flattened input -- or one per sequence of a [B, S, K] input, broadcast over S on the device -- on the
        device of the inputs: kept BY REFERENCE, so a captured decode step follows ids written into it in place.  Rows whose id
        lies outside [0, len(names)) get the base model's output."""
        if which is None or isinstance(which, torch.Tensor):
            if which is not None and (which.dim() != 1 or which.dtype not in (torch.int64, torch.int32)):
                raise ValueError(f"adapter ids must be a 1-D int64 / int32 tensor, got {tuple(which.shape)} {which.dtype}")
        elif which not in self.names:
            raise KeyError(f"no adapter named {which!r}; attached: {self.names}")
        self.selection = which
        return self


class LoraQuantizedLinear(nn.Module):
    """An unchanged ``QuantizedLinear`` (``base_layer``) plus LoRA adapters, in PEFT's layout: ``lora_A[name]`` / ``lora_B[name]``
    are bias-free ``nn.Linear`` (in -> rank, rank -> out) and ``scaling[name]`` the factor, so ``state_dict()`` carries PEFT's
    key names.  Which adapter serves which row is the bank's selection."""

    def __init__(self, base_layer: QuantizedLinear, bank: Optional[AdapterBank] = None):
        super().__init__()
        if not isinstance(base_layer, QuantizedLinear):
            raise TypeError(f"LoraQuantizedLinear wraps a QuantizedLinear, got {type(base_layer).__name__}")
        self.base_layer = base_layer
        self.lora_A = nn.ModuleDict()
        self.lora_B = nn.ModuleDict()
        self.scaling: Dict[str, float] = {}
        self.bank = bank if bank is not None else AdapterBank([])
        self.bank.layers.append(self)
        self.in_features, self.out_features = base_layer.in_features, base_layer.out_features
        self._table = None       # (key, device table, ranks): rebuilt when an A / B moved or was written
        self._slot_map = None    # (key, device tensor bank id -> table slot): layers that lack some of the bank's adapters

    def add_adapter(self, name: str, a: torch.Tensor, b: torch.Tensor, scaling: float) -> None:
        """``a`` [rank, in_features], ``b`` [out_features, rank]; copied into new bias-free ``nn.Linear`` modules on the base
        layer's device.  The weights do not require gradients (serving); ``requires_grad_(True)`` makes the module train."""
        rank = a.shape[0]
        if a.dim() != 2 or b.dim() != 2 or tuple(a.shape) != (rank, self.in_features) or tuple(b.shape) != (self.out_features, rank):
            raise ValueError(f"adapter {name!r}: lora_A must be [r, {self.in_features}] and lora_B [{self.out_features}, r], got "
                             f"{tuple(a.shape)} / {tuple(b.shape)}")
        if name not in self.bank.names:
            self.bank.names.append(name)
        dev = self.base_layer.codebooks.device
        la = nn.Linear(self.in_features, rank, bias=False, device=dev, dtype=a.dtype)
        lb = nn.Linear(rank, self.out_features, bias=False, device=dev, dtype=b.dtype)
        with torch.no_grad():
            la.weight.copy_(a)
            lb.weight.copy_(b)
        la.weight.requires_grad_(False)
        lb.weight.requires_grad_(False)
        self.lora_A[name], self.lora_B[name], self.scaling[name] = la, lb, float(scaling)
        self._table = self._slot_map = None

    # -- what the layer holds, in bank order --------------------------------------------------------------------------------
    def _present(self) -> List[Tuple[int, str]]:
        return [(i, n) for i, n in enumerate(self.bank.names) if n in self.lora_A]

    def _weights(self, name: str) -> Tuple[torch.Tensor, torch.Tensor, float]:
        return self.lora_A[name].weight, self.lora_B[name].weight, self.scaling[name]

    def _device_table(self, device: torch.device):
        """The device table of this layer's adapters (one slot per adapter the layer HAS, in bank order), keyed on data_ptr and
        version of every A and B and rebuilt on an eager call when one of them moved or was written."""
        present = self._present()
        key = (device, tuple((n, a.data_ptr(), tensor_version(a), b.data_ptr(), tensor_version(b), s)
                             for n, (a, b, s) in ((n, self._weights(n)) for _, n in present)))
        if self._table is None or self._table[0] != key:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("LoraQuantizedLinear: the adapter table is built by a host-to-device copy; run one eager forward "
                                   "before capturing (and again after moving or rewriting an adapter)")
            from .inference_kernels import hip_kernel

            table = hip_kernel.lora_table([self._weights(n) for _, n in present], device)
            self._table = (key, table, [self.lora_A[n].weight.shape[0] for _, n in present])
        return self._table[1], self._table[2]

    def _local_ids(self, ids: torch.Tensor) -> torch.Tensor:
        """Bank ids -> this layer's table slots, on the device, without a sync.  A layer that holds every adapter of the bank
        uses the ids as they are; else absent adapters (and ids outside the bank) become -1 = no adapter."""
        present = self._present()
        n = len(self.bank.names)
        if len(present) == n:
            return ids
        key = (ids.device, tuple(i for i, _ in present), n)
        if self._slot_map is None or self._slot_map[0] != key:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("LoraQuantizedLinear: the adapter slot map is built by a host-to-device copy; run one eager "
                                   "forward before capturing")
            slots = [-1] * n
            for slot, (i, _) in enumerate(present):
                slots[i] = slot
            self._slot_map = (key, torch.tensor(slots, dtype=torch.int64).to(ids.device))
        inside = (ids >= 0) & (ids < n)
        return torch.where(inside, self._slot_map[1][ids.clamp(0, n - 1).long()], -1)

    def _row_ids(self, sel: torch.Tensor, x: torch.Tensor) -> torch.Tensor:
        """The selection as one id per row of the flattened input; per-sequence ids of a [B, S, K] input are broadcast over S."""
        rows = math.prod(x.shape[:-1])
        if sel.device != x.device:
            raise ValueError(f"adapter ids live on {sel.device}, the input on {x.device}")
        if sel.numel() == rows:
            return sel
        if x.dim() == 3 and sel.numel() == x.shape[0]:
            return sel[:, None].expand(x.shape[0], x.shape[1]).reshape(-1)
        raise ValueError(f"{sel.numel()} adapter ids for an input of shape {tuple(x.shape)}: one per row ({rows}) or one per "
                         f"sequence ({x.shape[0]}) expected")

    # -- forward ------------------------------------------------------------------------------------------------------------
    def forward(self, x: torch.Tensor) -> torch.Tensor:
        y = self.base_layer(x)  # the very tensor object: shared-input groups (fusion.py) recognise their input by identity
        sel = self.bank.selection
        if sel is None or len(self.lora_A) == 0:
            return y
        if isinstance(sel, str):
            if sel not in self.lora_A:
                return y
            names = [sel]
        else:
            names = [n for _, n in self._present()]
        weights = [self._weights(n) for n in names]
        rows = math.prod(x.shape[:-1])
        compiling = torch.compiler.is_compiling()
        dtype_ok = x.dtype in _DTYPES_OK and y.dtype == x.dtype and all(a.dtype == x.dtype and b.dtype == x.dtype for a, b, _ in weights)
        grad_needed = torch.is_grad_enabled() and (x.requires_grad or y.requires_grad
                                                   or any(a.requires_grad or b.requires_grad for a, b, _ in weights))
        supported = False
        if x.is_cuda and dtype_ok and not grad_needed and not compiling and 1 <= rows <= min(BGMV_MAX_ROWS, AQLM_HIP_MAX_LORA_ROWS):
            from .inference_kernels import hip_kernel

            ranks = [a.shape[0] for a, _, _ in weights]
            supported = (all(r % 8 == 0 for r in ranks) and y.stride(-1) == 1
                         and hip_kernel.lora_bgmv_supported(self.out_features, self.in_features, max(ranks), rows))
        if takes_bgmv_route(x.is_cuda, dtype_ok, grad_needed, compiling, rows, supported):
            try:
                y2 = y.view(-1, self.out_features)
            except RuntimeError:
                y2 = None  # an output whose rows are no regular view: the torch path
            if y2 is not None:
                self._bgmv(y2, x.reshape(-1, self.in_features), sel if isinstance(sel, str) else self._row_ids(sel, x))
                return y
        supported = False
        if (x.is_cuda and dtype_ok and not grad_needed and not compiling
                and SGMV_MIN_ROWS <= rows <= min(SGMV_MAX_ROWS, AQLM_HIP_MAX_LORA_SGMV_ROWS)):
            from .inference_kernels import hip_kernel

            ranks = [a.shape[0] for a, _, _ in weights]
            supported = (all(r % 8 == 0 for r in ranks) and y.stride(-1) == 1 and y.data_ptr() % 8 == 0
                         and hip_kernel.lora_sgmv_supported(self.out_features, self.in_features, max(ranks), rows))
        if takes_sgmv_route(x.is_cuda, dtype_ok, grad_needed, compiling, rows, supported):
            try:
                y2 = y.view(-1, self.out_features)
            except RuntimeError:
                y2 = None
            if y2 is not None and y2.stride(0) % 4 == 0:  # y is written in groups of 4 outputs
                self._bgmv(y2, x.reshape(-1, self.in_features), sel if isinstance(sel, str) else self._row_ids(sel, x),
                           hip_kernel.lora_sgmv_)
                return y
        return self._torch_path(y, x, sel, names)

    def _bgmv(self, y2: torch.Tensor, x2: torch.Tensor, sel, launch=None) -> None:
        """``sel``: an adapter name, or one bank id per row of ``x2``.  ``launch``: ``hip_kernel.lora_sgmv_`` for the SGMV route
        (the same table, ids and geometry); default the BGMV launch."""
        from .inference_kernels import hip_kernel

        launch = hip_kernel.lora_bgmv_ if launch is None else launch
        table, ranks = self._device_table(x2.device)
        if isinstance(sel, str):
            # one adapter for every row: its slot of the table alone, NULL ids, and a grid sized by its own rank
            slot = [n for _, n in self._present()].index(sel)
            words = table.shape[0] // len(ranks)
            launch(y2, x2, None, table[slot * words:(slot + 1) * words], [1, ranks[slot], self.out_features, self.in_features])
            return
        launch(y2, x2, self._local_ids(sel), table, [len(ranks), max(ranks), self.out_features, self.in_features])

    def _torch_path(self, y: torch.Tensor, x: torch.Tensor, sel, names: List[str]) -> torch.Tensor:
        """PEFT's formula per adapter of the bank, masked by ``ids == a``: a loop over the bank, not over the ids, so it never
        syncs; differentiable in x, A and B; serves host tensors too."""
        ids = None
        if not isinstance(sel, str):
            ids = self._row_ids(sel, x).reshape(x.shape[:-1])
        out = y
        for name in names:
            a, b, scaling = self._weights(name)
            delta = F.linear(F.linear(x.to(a.dtype), a), b) * scaling
            if ids is not None:
                delta = torch.where((ids == self.bank.index(name))[..., None], delta, torch.zeros((), dtype=delta.dtype, device=delta.device))
            out = out + delta.to(y.dtype)
        return out

    def extra_repr(self) -> str:
        return "adapters=" + ", ".join(f"{n} (r={self.lora_A[n].weight.shape[0]}, scaling={self.scaling[n]:g})" for n in self.lora_A)


_EXPERT_SEGMENTS = (("w1", "w3"), ("w2",))  # the projections of the gate / up launch and of the down launch


class LoraQuantizedMixtralExperts(nn.Module):
    """An unchanged ``QuantizedMixtralExperts`` (``base_layer``, the very object) plus LoRA adapters on its experts' projections:
    ``lora_A[name][e][w]`` / ``lora_B[name][e][w]`` (e = "0" .. "E-1", w = "w1" / "w2" / "w3") are bias-free ``nn.Linear`` and
    ``scaling[name]`` the factor; an adapter may cover some experts and some projections only.  Same call signature as the block
    it replaces.  Which adapter serves which TOKEN is the bank's selection: a name, or one id per row of the [T, H] input, or
    one id per sequence (T a multiple of their number: broadcast over T / n consecutive rows on the device)."""

    def __init__(self, base_layer, bank: Optional[AdapterBank] = None):
        super().__init__()
        from .moe import QuantizedMixtralExperts

        if not isinstance(base_layer, QuantizedMixtralExperts):
            raise TypeError(f"LoraQuantizedMixtralExperts wraps a QuantizedMixtralExperts, got {type(base_layer).__name__}")
        self.base_layer = base_layer
        self.lora_A = nn.ModuleDict()
        self.lora_B = nn.ModuleDict()
        self.scaling: Dict[str, float] = {}
        self.bank = bank if bank is not None else AdapterBank([])
        self.bank.layers.append(self)
        self.num_experts = base_layer.num_experts
        self._tables = None  # (key, {segments: (device table, max rank per bank adapter, every rank a multiple of 8)})

    def _shape(self, w: str) -> Tuple[int, int]:
        """(in_features, out_features) of projection ``w``."""
        H, I = self.base_layer.hidden_dim, self.base_layer.intermediate_dim
        return (I, H) if w == "w2" else (H, I)

    def add_adapter(self, name: str, expert: int, w: str, a: torch.Tensor, b: torch.Tensor, scaling: float) -> None:
        """Adapter ``name`` on projection ``w`` of expert ``expert``: ``a`` [rank, in], ``b`` [out, rank], copied into new bias-free
        ``nn.Linear`` modules on the block's device (no gradients required: serving; ``requires_grad_(True)`` trains them)."""
        if w not in ("w1", "w2", "w3") or not 0 <= int(expert) < self.num_experts:
            raise ValueError(f"adapter {name!r}: no projection {w!r} of expert {expert} in a block of {self.num_experts} experts")
        fin, fout = self._shape(w)
        rank = a.shape[0]
        if a.dim() != 2 or b.dim() != 2 or tuple(a.shape) != (rank, fin) or tuple(b.shape) != (fout, rank):
            raise ValueError(f"adapter {name!r}: expert {expert} {w}: lora_A must be [r, {fin}] and lora_B [{fout}, r], got "
                             f"{tuple(a.shape)} / {tuple(b.shape)}")
        if name in self.scaling and self.scaling[name] != float(scaling):
            raise ValueError(f"adapter {name!r}: one scaling per adapter and block ({self.scaling[name]} / {scaling})")
        if name not in self.bank.names:
            self.bank.names.append(name)
        dev = self.base_layer.expert(0).w1.codebooks.device
        la = nn.Linear(fin, rank, bias=False, device=dev, dtype=a.dtype)
        lb = nn.Linear(rank, fout, bias=False, device=dev, dtype=b.dtype)
        with torch.no_grad():
            la.weight.copy_(a)
            lb.weight.copy_(b)
        la.weight.requires_grad_(False)
        lb.weight.requires_grad_(False)
        for store, lin in ((self.lora_A, la), (self.lora_B, lb)):
            if name not in store:
                store[name] = nn.ModuleDict()
            if str(int(expert)) not in store[name]:
                store[name][str(int(expert))] = nn.ModuleDict()
            store[name][str(int(expert))][w] = lin
        self.scaling[name] = float(scaling)
        self._tables = None

    def _weights(self, name: str, e: int, w: str):
        """(A, B, scaling) of adapter ``name`` on projection ``w`` of expert ``e``, or None when it has none."""
        per = self.lora_A[name] if name in self.lora_A else None
        if per is None or str(e) not in per or w not in per[str(e)]:
            return None
        return per[str(e)][w].weight, self.lora_B[name][str(e)][w].weight, self.scaling[name]

    def _all_weights(self, names):
        return [wt for n in names for e in range(self.num_experts) for w in ("w1", "w3", "w2")
                for wt in (self._weights(n, e, w),) if wt is not None]

    def _device_tables(self, device: torch.device, transposed=None):
        """The device tables of the two launches over ALL adapters of the bank ([bank][E][S]; what this block lacks is a zero
        entry), keyed on data_ptr and version of every A and B and rebuilt on an eager call when one of them moved or was written.
        ``transposed``: the projection group whose TRANSPOSED side the caller needs as well (the training route): the buffer of
        the B^T / A^T copies and the table [S][bank][E] over it, built here under the same key the first time it is asked for
        (its copies are written by a launch at the start of every backward, not here)."""
        names = list(self.bank.names)
        key = (device, tuple(names), tuple((a.data_ptr(), tensor_version(a), b.data_ptr(), tensor_version(b), s)
                                           for a, b, s in self._all_weights(names)))
        if self._tables is None or self._tables[0] != key:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("LoraQuantizedMixtralExperts: the adapter table is built by a host-to-device copy; run one eager "
                                   "forward before capturing (and again after moving or rewriting an adapter)")
            from .inference_kernels import hip_kernel

            tables = {}
            for segments in _EXPERT_SEGMENTS:
                entries = [[[self._weights(n, e, w) for w in segments] for e in range(self.num_experts)] for n in names]
                ranks = [[wt[0].shape[0] for per in pa for wt in per if wt is not None] for pa in entries]
                tables[segments] = (hip_kernel.lora_routed_table(entries, device), [max(r, default=0) for r in ranks],
                                    all(v % 8 == 0 for r in ranks for v in r))
            self._tables = (key, tables, {})
        if transposed is not None and transposed not in self._tables[2]:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("LoraQuantizedMixtralExperts: the transposed adapter table is built by a host-to-device copy; run "
                                   "one eager training step before capturing (and again after moving or rewriting an adapter)")
            from .inference_kernels import hip_kernel

            entries = [[[self._weights(n, e, w) for w in transposed] for e in range(self.num_experts)] for n in names]
            self._tables[2][transposed] = hip_kernel.lora_routed_transposed_table(entries, device)[:2]
        return self._tables[1]

    def _transposed_tables(self, segments):
        """(buffer, transposed device table) of projection group ``segments``, as ``_device_tables(..., transposed=segments)`` built it."""
        return self._tables[2][segments]

    def _token_ids(self, sel: torch.Tensor, x: torch.Tensor) -> torch.Tensor:
        """The selection as one id per row of the [T, H] input; per-sequence ids are broadcast over T / n consecutive rows."""
        T = x.shape[0]
        if sel.device != x.device:
            raise ValueError(f"adapter ids live on {sel.device}, the input on {x.device}")
        n = sel.numel()
        if n == T:
            return sel
        if n and T % n == 0:
            return sel[:, None].expand(n, T // n).reshape(-1)
        raise ValueError(f"{n} adapter ids for an input of shape {tuple(x.shape)}: one per row ({T}) or one per sequence (a divisor "
                         f"of {T}) expected")

    def forward(self, hidden_states: torch.Tensor, top_k_index: torch.Tensor, top_k_weights: torch.Tensor) -> torch.Tensor:
        sel = self.bank.selection
        if sel is None or len(self.lora_A) == 0 or (isinstance(sel, str) and sel not in self.lora_A):
            return self.base_layer(hidden_states, top_k_index, top_k_weights)  # bits and launches of the bare block
        ids = None if isinstance(sel, str) else self._token_ids(sel, hidden_states)
        if torch.is_grad_enabled() and not hidden_states.requires_grad:
            # The base block chooses raw ops (no autograd) by ``hidden_states.requires_grad`` alone: with a frozen input -- the
            # first block over a frozen embedding -- its w2 launch would cut the adapters of w1 / w3 off the graph.  So an input that
            # requires grad whenever a selected adapter trains; nothing flows back into the caller's tensor.
            names = [sel] if isinstance(sel, str) else [n for n in self.bank.names if n in self.lora_A]
            trained = next((t for a, b, _ in self._all_weights(names) for t in (a, b) if t.requires_grad), None)
            if trained is not None:
                hidden_states = _AsTrainedInput.apply(hidden_states, trained)
        return self.base_layer(hidden_states, top_k_index, top_k_weights, adapters=_ExpertAdapters(self, sel, ids))

    def extra_repr(self) -> str:
        return "adapters=" + ", ".join(f"{n} ({len(self._all_weights([n]))} projections, scaling={self.scaling[n]:g})" for n in self.lora_A)


class _ExpertAdapters:
    """The adapter provider of one ``LoraQuantizedMixtralExperts.forward`` (``QuantizedMixtralExperts.forward(adapters=...)``):
    ``name`` selected for every token, or ``ids`` [T] bank ids per token."""

    def __init__(self, layer: LoraQuantizedMixtralExperts, sel, ids: Optional[torch.Tensor]):
        self.layer, self.ids = layer, ids
        self._tables = None  # the layer's device tables, looked up (and their key compared) once per forward
        self._bucket = None  # the 16-pair expert bucket of the SGMV route, built once per forward and read by both calls
        self.names = [sel] if isinstance(sel, str) else [n for n in layer.bank.names if n in layer.lora_A]

    def on_pairs(self, out: torch.Tensor, x: torch.Tensor, top_k_index: torch.Tensor, segments, x_per_pair: bool) -> torch.Tensor:
        """``out`` [P, S, M], the output of a pair-batched launch on projections ``segments``; ``x`` [T, K] token rows or [P, K] pair
        rows.  -> ``out`` with every pair's adapter term added: the very tensor (HIP routes, in place; with a gradient needed, as
        the output of ``_RoutedAdapterFunction``) or a new one (torch path)."""
        layer = self.layer
        segments = tuple(segments)
        P, S, M = out.shape
        weights = [wt for n in self.names for e in range(layer.num_experts) for w in segments
                   for wt in (layer._weights(n, e, w),) if wt is not None]
        if not weights:
            return out
        compiling = torch.compiler.is_compiling()
        dtype_ok = x.dtype in _DTYPES_OK and out.dtype == x.dtype and all(a.dtype == x.dtype and b.dtype == x.dtype for a, b, _ in weights)
        grad_needed = torch.is_grad_enabled() and (x.requires_grad or out.requires_grad
                                                   or any(a.requires_grad or b.requires_grad for a, b, _ in weights))
        bgmv = 1 <= P <= min(ROUTED_BGMV_MAX_PAIRS, AQLM_HIP_MAX_LORA_ROWS)
        sgmv = ROUTED_SGMV_MIN_PAIRS <= P <= min(ROUTED_SGMV_MAX_PAIRS, AQLM_HIP_MAX_LORA_SGMV_ROUTED_PAIRS)
        fast = (x.is_cuda and dtype_ok and not grad_needed and not compiling and top_k_index.dim() == 2 and out.is_contiguous()
                and (bgmv or sgmv))
        if fast:
            from .inference_kernels import hip_kernel

            if self._tables is None:
                self._tables = layer._device_tables(x.device)
            table, max_ranks, ranks_ok = self._tables[segments]
            if self.ids is None:  # one adapter for every token: its [1][E][S] slice of the table, NULL ids, its own rank
                a = layer.bank.index(self.names[0])
                words = table.shape[0] // len(max_ranks)
                table, n, max_rank = table[a * words:(a + 1) * words], 1, max_ranks[a]
            else:
                n, max_rank = len(max_ranks), max(max_ranks)
            geometry = [n, layer.num_experts, S, max_rank, M, x.shape[1], top_k_index.shape[1]]
            supported = bgmv and ranks_ok and hip_kernel.lora_bgmv_routed_supported(M, x.shape[1], max_rank, P, layer.num_experts, S)
            if takes_routed_bgmv_route(x.is_cuda, dtype_ok, grad_needed, compiling, P, supported):
                hip_kernel.lora_bgmv_routed_(out, x, self.ids, top_k_index, table, geometry, x_per_pair)
                return out
            supported = (sgmv and ranks_ok and out.data_ptr() % 8 == 0
                         and hip_kernel.lora_sgmv_routed_supported(M, x.shape[1], max_rank, P, layer.num_experts, S))
            if takes_routed_sgmv_route(x.is_cuda, dtype_ok, grad_needed, compiling, P, supported):
                if self._bucket is None:
                    self._bucket = torch.ops.aqlm.moe_bucket(top_k_index, layer.num_experts, hip_kernel.SGMV_ROUTED_TILE_PAIRS)
                hip_kernel.lora_sgmv_routed_(out, x, self.ids, top_k_index, self._bucket, table, geometry, x_per_pair)
                return out
        train = (x.is_cuda and dtype_ok and grad_needed and not compiling and top_k_index.dim() == 2 and out.is_contiguous()
                 and ROUTED_TRAIN_MIN_PAIRS <= P <= min(ROUTED_TRAIN_MAX_PAIRS, AQLM_HIP_MAX_LORA_SGMV_ROUTED_PAIRS))
        if train:
            from .inference_kernels import hip_kernel

            E, Kin = layer.num_experts, x.shape[1]
            if self._tables is None:
                self._tables = layer._device_tables(x.device)
            table, max_ranks, ranks_ok = self._tables[segments]
            a0 = None if self.ids is not None else layer.bank.index(self.names[0])
            n, max_rank = (len(max_ranks), max(max_ranks)) if a0 is None else (1, max_ranks[a0])
            supported = (ranks_ok and out.data_ptr() % 8 == 0 and M % 8 == 0
                         and hip_kernel.lora_sgmv_routed_supported(M, Kin, max_rank, P, E, S)
                         and hip_kernel.lora_sgmv_routed_supported(Kin, M, max_rank, P, E, 1)
                         and hip_kernel.lora_transpose_routed_supported(M, Kin, max(max_ranks), E, S)
                         and hip_kernel.lora_grad_routed_supported(M, max_rank, P, E, S)
                         and hip_kernel.lora_grad_routed_supported(Kin, max_rank, P, E, S))
            if takes_routed_train_route(x.is_cuda, dtype_ok, grad_needed, compiling, P, supported):
                if segments not in layer._tables[2]:
                    layer._device_tables(x.device, transposed=segments)
                if self._bucket is None:
                    self._bucket = torch.ops.aqlm.moe_bucket(top_k_index, E, hip_kernel.SGMV_ROUTED_TILE_PAIRS)
                # the weights autograd has to see: A and B of every live entry of the adapters in play, in table order
                who = [(layer.bank.index(name), e, s, t) for name in self.names for e in range(E) for s, w in enumerate(segments)
                       for wt in (layer._weights(name, e, w),) if wt is not None for t in (0, 1)]
                flat = [layer._weights(layer.bank.names[a], e, segments[s])[t] for a, e, s, t in who]
                call = _RoutedCall(layer, segments, self.ids, top_k_index, self._bucket, table, a0, n, max_rank, x_per_pair, who)
                return _RoutedAdapterFunction.apply(out, x, call, *flat)
        return self._torch_pairs(out, x, top_k_index, segments, x_per_pair)

    def _torch_pairs(self, out, x, top_k_index, segments, x_per_pair):
        """PEFT's formula per (adapter of the bank, expert, projection), masked by ``(adapter_id == a) & (expert_id == e)``: a loop
        over bank x experts, never over the ids, so it never syncs; out of place; differentiable in x, A and B.  The rank-sized
        intermediate is masked (a pair has at most one live term per projection), so the sum below adds zeros to it.  Evaluated
        in fp32 and added to ``out`` with ONE rounding, as the HIP route does (PEFT rounds the intermediate and the term to the
        storage type first): the term passes through the activation and the down projection, where two roundings more per
        element of ``gu`` would show as a difference between the two routes of the size of the block's own rounding error."""
        layer = self.layer
        P, S, M = out.shape
        eid = top_k_index.reshape(-1)
        k = P // x.shape[0] if not x_per_pair else 1
        aid = None
        if self.ids is not None:
            aid = self.ids if P == self.ids.numel() else self.ids[:, None].expand(self.ids.numel(), P // self.ids.numel()).reshape(-1)
        deltas = [None] * S
        xf = x.float()
        for name in self.names:
            amask = None if aid is None else aid == layer.bank.index(name)
            for e in range(layer.num_experts):
                mask = None
                for s, w in enumerate(segments):
                    wt = layer._weights(name, e, w)
                    if wt is None:
                        continue
                    if mask is None:
                        mask = (eid == e) if amask is None else (amask & (eid == e))
                    a, b, scaling = wt
                    t = F.linear(xf, a.float())  # [rows, r]
                    if k > 1:
                        t = t[:, None, :].expand(t.shape[0], k, t.shape[1]).reshape(P, t.shape[1])
                    t = torch.where(mask[:, None], t, torch.zeros((), dtype=t.dtype, device=t.device))
                    d = F.linear(t, b.float()) * scaling
                    deltas[s] = d if deltas[s] is None else deltas[s] + d
        if all(d is None for d in deltas):
            return out
        zero = None
        cols = []
        for d in deltas:
            if d is None:
                zero = torch.zeros((P, M), dtype=torch.float32, device=out.device) if zero is None else zero
                d = zero
            cols.append(d)
        return (out.float() + torch.stack(cols, dim=1)).to(out.dtype)

    def on_rows(self, out: torch.Tensor, x: torch.Tensor, e: int, w: str, tok: torch.Tensor) -> torch.Tensor:
        """``out`` [n, M] = projection ``w`` of expert ``e`` on the rows ``x`` [n, K] of the tokens ``tok`` (the per-expert loop):
        the torch path on those rows (fp32, one rounding, as ``_torch_pairs``), masked by the tokens' adapter ids."""
        layer = self.layer
        ids = None if self.ids is None else self.ids[tok]
        total = None
        for name in self.names:
            wt = layer._weights(name, e, w)
            if wt is None:
                continue
            a, b, scaling = wt
            delta = F.linear(F.linear(x.float(), a.float()), b.float()) * scaling
            if ids is not None:
                delta = torch.where((ids == layer.bank.index(name))[:, None], delta, torch.zeros((), dtype=delta.dtype, device=delta.device))
            total = delta if total is None else total + delta
        return out if total is None else (out.float() + total).to(out.dtype)


class _AsTrainedInput(torch.autograd.Function):
    """``x`` as a tensor that requires grad because ``trained`` does (``LoraQuantizedMixtralExperts.forward``); no gradient flows
    back into either."""

    @staticmethod
    def forward(ctx, x, trained):
        return x.view_as(x)

    @staticmethod
    def backward(ctx, grad):
        return None, None


class _RoutedCall:
    """What one training call of ``on_pairs`` hands to its autograd function besides the tensors autograd differentiates."""

    def __init__(self, layer, segments, ids, top_k_index, bucket, table, adapter0, n, max_rank, x_per_pair, who):
        self.layer, self.segments, self.ids, self.top_k_index, self.bucket, self.table = layer, segments, ids, top_k_index, bucket, table
        self.adapter0, self.n, self.max_rank, self.x_per_pair, self.who = adapter0, n, max_rank, x_per_pair, who


class _RoutedAdapterFunction(torch.autograd.Function):
    """``out += adapters(x)`` on the routed experts with a backward on device launches only.  Forward:
    ``aqlm_hip_lora_sgmv_routed`` in place -- the bits of the serving route -- into a workspace this call owns (the cached one
    would be overwritten by the next layer): it keeps t = A x of every pair.  Backward, with gy the gradient of ``out``:
    the transposed copies of the weights as they are now (one launch), per projection the same launch on the transposed table
    with x := gy[:, s] (its workspace then holds u = B^T gy, its output scaling * A^T u = grad_x per pair), and per trained
    adapter one ``aqlm_hip_lora_grad_routed`` for grad_A (V = x, w = u) and one for grad_B^T (V = gy, w = t).  No host
    synchronisation, no atomics, capturable, bit-reproducible."""

    @staticmethod
    def forward(ctx, out, x, call, *weights):
        from .inference_kernels import hip_kernel

        P, S, M = out.shape
        K = x.shape[1]
        E = call.layer.num_experts
        k = call.top_k_index.shape[1]
        geometry = [call.n, E, S, call.max_rank, M, K, k]
        table = call.table
        if call.adapter0 is not None:
            words = table.shape[0] // len(call.layer.bank.names)
            table = table[call.adapter0 * words:(call.adapter0 + 1) * words]
        t = torch.empty((hip_kernel.lora_sgmv_routed_workspace_floats(P, S, call.max_rank, K),), dtype=torch.float32, device=x.device)
        hip_kernel.lora_sgmv_routed_(out, x, call.ids, call.top_k_index, call.bucket, table, geometry, call.x_per_pair, workspace=t)
        ctx.mark_dirty(out)
        ctx.call, ctx.geometry = call, geometry
        ctx.save_for_backward(x, t, table, call.bucket, call.top_k_index, *(() if call.ids is None else (call.ids,)))
        return out

    @staticmethod
    def backward(ctx, gy):
        from .inference_kernels import hip_kernel

        call = ctx.call
        x, t, table, bucket, top_k_index = ctx.saved_tensors[:5]
        ids = ctx.saved_tensors[5] if len(ctx.saved_tensors) > 5 else None
        n, E, S, max_rank, M, K, k = ctx.geometry
        P = gy.shape[0]
        gy = gy.contiguous()
        x = hip_kernel._flat_rows(x)  # rows the launches can address, as the forward's launch saw them
        layer, segments = call.layer, call.segments
        need_x = ctx.needs_input_grad[1]
        need_w = [ctx.needs_input_grad[3 + i] for i in range(len(call.who))]
        need_a = any(nd for nd, (_, _, _, which) in zip(need_w, call.who) if which == 0)
        grads = [None] * len(call.who)
        gx = None
        if need_x or need_a:
            # u = B^T gy and grad_x per pair: the forward's launch on the transposed table, a segment at a time
            full = layer._device_tables(x.device, transposed=segments)[segments][0]
            buffer, ttable = layer._transposed_tables(segments)
            names = len(layer.bank.names)
            hip_kernel.lora_transpose_routed_(buffer, full, ttable, [names, E, S, max(layer._tables[1][segments][1]), M, K])
            splits_m = hip_kernel.lora_sgmv_splits(M)
            u = torch.empty((S, P, splits_m, max_rank), dtype=torch.float32, device=x.device)
            words = ttable.shape[0] // (S * names)  # one adapter of one segment: [E] entries
            total = None
            for s in range(S):
                a_first = 0 if call.adapter0 is None else call.adapter0
                tt = ttable[(s * names + a_first) * words:(s * names + a_first + n) * words]
                gxs = torch.zeros((P, 1, K), dtype=gy.dtype, device=x.device)
                hip_kernel.lora_sgmv_routed_(gxs, gy[:, s, :], ids, top_k_index, bucket, tt, [n, E, 1, max_rank, K, M, k], True,
                                             workspace=u[s].view(-1))
                if need_x:
                    total = gxs.view(P, K).float() if total is None else total + gxs.view(P, K).float()
            if need_x:
                if not call.x_per_pair:
                    total = total.view(P // k, k, K).sum(dim=1)  # the token's pairs in ascending order
                gx = total.to(x.dtype)
        for a in sorted({a for nd, (a, _, _, _) in zip(need_w, call.who) if nd}):
            a_local = a if call.adapter0 is None else 0
            mine = [(i, e, s, which) for i, (a_, e, s, which) in enumerate(call.who) if a_ == a and need_w[i]]
            # (every entry read below is live -- the route needs every rank a multiple of 8 -- and the kernel writes all of a live
            # entry, so the outputs need no memset)
            if any(which == 0 for _, _, _, which in mine):
                ga = hip_kernel.lora_grad_routed(x, u, ids, top_k_index, bucket, table, [n, E, S, max_rank, K, k, a_local],
                                                 [x.stride(0) if x.shape[0] > 1 else K, 0, int(call.x_per_pair),
                                                  u.stride(1), u.stride(0), u.shape[2], max_rank],
                                                 out=torch.empty((E, S, max_rank, K), dtype=torch.float32, device=x.device))
            if any(which == 1 for _, _, _, which in mine):
                splits_k = t.numel() // (P * S * max_rank)
                gb = hip_kernel.lora_grad_routed(gy, t, ids, top_k_index, bucket, table, [n, E, S, max_rank, M, k, a_local],
                                                 [S * M, M, 1, S * splits_k * max_rank, splits_k * max_rank, splits_k, max_rank],
                                                 out=torch.empty((E, S, max_rank, M), dtype=torch.float32, device=x.device))
            for i, e, s, which in mine:
                w = layer._weights(layer.bank.names[a], e, segments[s])[which]
                r = w.shape[1] if which else w.shape[0]
                grads[i] = ga[e, s, :r].to(w.dtype) if which == 0 else gb[e, s, :r].t().to(w.dtype)
        return (gy, gx, None, *grads)


# ---------------------------------------------------------------------------------------------------------------------------
# loading
# ---------------------------------------------------------------------------------------------------------------------------
def _load_adapter(source) -> Tuple[Dict[str, torch.Tensor], dict]:
    if isinstance(source, (str, os.PathLike)):
        path = os.fspath(source)
        with open(os.path.join(path, "adapter_config.json")) as f:
            config = json.load(f)
        from safetensors.torch import load_file

        return load_file(os.path.join(path, "adapter_model.safetensors")), config
    state, config = source
    return dict(state), dict(config)


def _check_config(name: str, config: dict) -> Tuple[int, float]:
    """Refuse by name what this loader does not implement; -> (r, scaling)."""
    if config.get("use_dora"):
        raise NotImplementedError(f"adapter {name!r}: use_dora is not supported (weight-decomposed adapters need the dense weight norm)")
    if config.get("bias", "none") not in ("none", None):
        raise NotImplementedError(f"adapter {name!r}: bias={config['bias']!r} is not supported (only bias=\"none\")")
    if config.get("modules_to_save"):
        raise NotImplementedError(f"adapter {name!r}: modules_to_save={config['modules_to_save']} is not supported")
    for key in ("rank_pattern", "alpha_pattern"):
        if config.get(key):
            raise NotImplementedError(f"adapter {name!r}: {key} is not supported (one r and one lora_alpha per adapter)")
    if config.get("peft_type", "LORA") != "LORA":
        raise NotImplementedError(f"adapter {name!r}: peft_type={config['peft_type']!r} is not supported (only LORA)")
    r, alpha = int(config["r"]), float(config.get("lora_alpha", config["r"]))
    return r, alpha / math.sqrt(r) if config.get("use_rslora") else alpha / r


def _is_target(path: str, target_modules) -> bool:
    if target_modules is None:
        return True
    if isinstance(target_modules, str):
        return re.fullmatch(target_modules, path) is not None
    return any(path == t or path.endswith("." + t) for t in target_modules)


def _adapter_modules(name: str, state: Dict[str, torch.Tensor]) -> Dict[str, Dict[str, torch.Tensor]]:
    """``base_model.model.<module path>.lora_{A,B}.weight`` -> {module path: {"A": ..., "B": ...}}."""
    modules: Dict[str, Dict[str, torch.Tensor]] = {}
    for key, value in state.items():
        m = re.fullmatch(r"(.+)\.lora_([AB])(?:\.default)?\.weight", key)
        if m is None:
            raise NotImplementedError(f"adapter {name!r}: key {key!r} is not a lora_A / lora_B weight of a linear layer")
        path = m.group(1)
        if path.startswith(_PREFIX):
            path = path[len(_PREFIX):]
        modules.setdefault(path, {})[m.group(2)] = value
    for path, ab in modules.items():
        if set(ab) != {"A", "B"}:
            raise ValueError(f"adapter {name!r}: {path} has lora_{next(iter(ab))} only")
    return modules


def _expert_block(model: nn.Module, path: str):
    """The ``QuantizedMixtralExperts`` two levels above the layer at ``path`` (``<block>.<e>.w{1,2,3}``), or None."""
    from .moe import QuantizedMixtralExperts

    parts = path.rsplit(".", 2)
    if len(parts) != 3 or not parts[1].isdigit() or parts[2] not in ("w1", "w2", "w3"):
        return None
    try:
        block = model.get_submodule(parts[0])
    except AttributeError:
        return None
    return block if isinstance(block, QuantizedMixtralExperts) else None


def attach_adapters(model: nn.Module, adapters: dict, target_modules=None) -> AdapterBank:
    """Wrap every ``QuantizedLinear`` the adapters target in ``LoraQuantizedLinear`` -- and every ``QuantizedMixtralExperts`` block
    with a targeted expert layer (``...experts.<e>.w1`` / ``w2`` / ``w3``; ``.block_sparse_moe.`` in a key is read as ``.mlp.`` when
    only that exists) in ``LoraQuantizedMixtralExperts`` -- and return the bank.  An adapter may cover some experts and some
    projections only, and mix expert targets with dense ones.  ``adapters`` maps a name
    to a PEFT adapter directory (``adapter_config.json`` + ``adapter_model.safetensors``) or to a ``(state_dict, config_dict)``
    pair with the same keys.  ``target_modules`` (names / path suffixes, or a regular expression) restricts the layers; default:
    every layer an adapter has weights for.  Apply ``fuse_shared_input_linears`` BEFORE attaching (it looks for
    ``QuantizedLinear`` children); the groups keep serving the wrapped layers."""
    if getattr(model, "_aqlm_adapter_bank", None) is not None:
        raise RuntimeError("adapters are already attached to this model; detach_adapters(model) first")
    loaded = []
    for name, source in adapters.items():
        if not isinstance(name, str) or not name or "." in name:
            raise ValueError(f"adapter names are non-empty strings without dots, got {name!r}")
        state, config = _load_adapter(source)
        r, scaling = _check_config(name, config)
        modules = {p: ab for p, ab in _adapter_modules(name, state).items() if _is_target(p, target_modules)}
        if not modules:
            raise ValueError(f"adapter {name!r} has no weights for the targeted modules")
        resolved = {}
        for path, ab in modules.items():
            try:
                target = model.get_submodule(path)
            except AttributeError:
                target = None
                if ".block_sparse_moe.experts." in path:  # the published Mixtral layout; transformers names the block .mlp.
                    renamed = path.replace(".block_sparse_moe.experts.", ".mlp.experts.")
                    try:
                        target, path = model.get_submodule(renamed), renamed
                    except AttributeError:
                        pass
                if target is None:
                    raise ValueError(f"adapter {name!r}: the model has no module {path!r}") from None
            resolved[path] = ab
            block = _expert_block(model, path) if getattr(target, "_moe_expert", False) else None
            if block is not None:
                fin, fout = target.in_features, target.out_features
                if ab["A"].shape[0] != r or ab["B"].shape[1] != r:
                    raise ValueError(f"adapter {name!r}: {path} has rank {ab['A'].shape[0]}, the config says r={r}")
                if tuple(ab["A"].shape) != (r, fin) or tuple(ab["B"].shape) != (fout, r):
                    raise ValueError(f"adapter {name!r}: {path}: lora_A must be [r, {fin}] and lora_B [{fout}, r], got "
                                     f"{tuple(ab['A'].shape)} / {tuple(ab['B'].shape)}")
                continue
            if getattr(target, "_moe_expert", False):
                raise NotImplementedError(f"adapter {name!r}: {path} is a routed mixture-of-experts expert layer; adapters on the "
                                          "routed experts are not supported (only dense QuantizedLinear layers: attention and MLP "
                                          "projections)")
            if not isinstance(target, QuantizedLinear):
                raise TypeError(f"adapter {name!r}: target {path} is a {type(target).__name__}, not a QuantizedLinear")
            if ab["A"].shape[0] != r or ab["B"].shape[1] != r:
                raise ValueError(f"adapter {name!r}: {path} has rank {ab['A'].shape[0]}, the config says r={r}")
        loaded.append((name, scaling, resolved))

    # expert targets "<block path>.<e>.<w>", found before any block is wrapped (a wrapped block moves its experts under base_layer)
    expert_targets = {path: (path.rsplit(".", 2)[0], int(path.rsplit(".", 2)[1]), path.rsplit(".", 1)[1])
                      for _, _, modules in loaded for path in modules if _expert_block(model, path) is not None}
    bank = AdapterBank([name for name, _, _ in loaded])
    wrappers: Dict[str, Union[LoraQuantizedLinear, LoraQuantizedMixtralExperts]] = {}
    for name, scaling, modules in loaded:
        for path, ab in modules.items():
            if path in expert_targets:
                block_path, e, w = expert_targets[path]
                wrapper = wrappers.get(block_path)
                if wrapper is None:
                    base = model.get_submodule(block_path)
                    parent_path, _, child = block_path.rpartition(".")
                    parent = model.get_submodule(parent_path) if parent_path else model
                    wrapper = wrappers[block_path] = LoraQuantizedMixtralExperts(base, bank)
                    setattr(parent, child, wrapper)
                    bank._replaced.append((parent, child, base))
                dtype = wrapper.base_layer.expert(e).w1.codebooks.dtype
                wrapper.add_adapter(name, e, w, ab["A"].to(dtype), ab["B"].to(dtype), scaling)
                continue
            wrapper = wrappers.get(path)
            if wrapper is None:
                base = model.get_submodule(path)
                parent_path, _, child = path.rpartition(".")
                parent = model.get_submodule(parent_path) if parent_path else model
                wrapper = wrappers[path] = LoraQuantizedLinear(base, bank)
                setattr(parent, child, wrapper)
                bank._replaced.append((parent, child, base))
            dtype = wrapper.base_layer.codebooks.dtype
            wrapper.add_adapter(name, ab["A"].to(dtype), ab["B"].to(dtype), scaling)
    model._aqlm_adapter_bank = bank
    return bank


def detach_adapters(model: nn.Module) -> None:
    """Put the original ``QuantizedLinear`` modules and expert blocks back (the very objects ``attach_adapters`` found) and drop the bank."""
    bank = getattr(model, "_aqlm_adapter_bank", None)
    if bank is None:
        return
    for parent, child, base in reversed(bank._replaced):
        setattr(parent, child, base)
    bank._replaced, bank.layers, bank.selection = [], [], None
    model._aqlm_adapter_bank = None
