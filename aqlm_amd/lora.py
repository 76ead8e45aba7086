"""LoRA adapters served on top of AQLM layers, a different adapter for every row of a decode batch if need be.

An adapter cannot be merged into an AQLM base -- the weights exist as codes + codebooks only -- so a fine-tuned AQLM model keeps
its adapters at inference, at every token.  ``attach_adapters(model, {...})`` wraps the targeted dense ``QuantizedLinear`` layers
(attention and MLP projections, the attention projections of Mixtral included; adapters on the routed experts are not covered) in
``LoraQuantizedLinear`` and returns the ``AdapterBank`` that says which adapter serves which row:

    bank = aqlm.lora.attach_adapters(model, {"math": "adapters/math", "code": "adapters/code"})
    bank.select("math")            # every row
    bank.select(ids)               # a device tensor of adapter ids per row (or per sequence); kept by reference
    bank.select(None)              # base model only: no adapter launch at all

Decode-sized calls run ``aqlm_hip_lora_bgmv`` (aqlm_amd/csrc/lora_bgmv.hip): two launches per layer whatever the mix of adapters,
ids read on the device only, capturable.  Larger calls -- prefill, big batches -- have ``aqlm_hip_lora_sgmv``
(aqlm_amd/csrc/lora_sgmv.hip), the same two launches on the matrix unit, one pass per distinct adapter of every 16-row tile, for
the row counts at which it was measured to win (``SGMV_MAX_ROWS``).  Everything else -- training, host tensors, shapes the kernels
decline -- runs the adapters as torch ops, differentiable in x, A and B, so the same module trains.

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


class AdapterBank:
    """The adapters attached to one model and the current selection.  ``names[i]`` is the adapter that id ``i`` selects."""

    def __init__(self, names: List[str]):
        self.names: List[str] = list(names)
        self.layers: List["LoraQuantizedLinear"] = []
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


def attach_adapters(model: nn.Module, adapters: dict, target_modules=None) -> AdapterBank:
    """Wrap every ``QuantizedLinear`` the adapters target in ``LoraQuantizedLinear`` and return the bank.  ``adapters`` maps a name
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
        for path, ab in modules.items():
            try:
                target = model.get_submodule(path)
            except AttributeError:
                raise ValueError(f"adapter {name!r}: the model has no module {path!r}") from None
            if getattr(target, "_moe_expert", False):
                raise NotImplementedError(f"adapter {name!r}: {path} is a routed mixture-of-experts expert layer; adapters on the "
                                          "routed experts are not supported (only dense QuantizedLinear layers: attention and MLP "
                                          "projections)")
            if not isinstance(target, QuantizedLinear):
                raise TypeError(f"adapter {name!r}: target {path} is a {type(target).__name__}, not a QuantizedLinear")
            if ab["A"].shape[0] != r or ab["B"].shape[1] != r:
                raise ValueError(f"adapter {name!r}: {path} has rank {ab['A'].shape[0]}, the config says r={r}")
        loaded.append((name, scaling, modules))

    bank = AdapterBank([name for name, _, _ in loaded])
    wrappers: Dict[str, LoraQuantizedLinear] = {}
    for name, scaling, modules in loaded:
        for path, ab in modules.items():
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
    """Put the original ``QuantizedLinear`` modules back (the very objects ``attach_adapters`` found) and drop the bank."""
    bank = getattr(model, "_aqlm_adapter_bank", None)
    if bank is None:
        return
    for parent, child, base in reversed(bank._replaced):
        setattr(parent, child, base)
    bank._replaced, bank.layers, bank.selection = [], [], None
    model._aqlm_adapter_bank = None
