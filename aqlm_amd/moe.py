"""Mixtral AQLM checkpoints: quantized experts and the hook that puts them in place while ``from_pretrained`` loads.

Transformers 5.x keeps all experts of a ``MixtralSparseMoeBlock`` as two 3-D parameters of ``MixtralExperts``
(``gate_up_proj [E, 2I, H]``, ``down_proj [E, H, I]``) and no ``nn.Linear``, so the AQLM integration's
``replace_with_aqlm_linear`` never reaches them: a published Mixtral AQLM checkpoint
(``...block_sparse_moe.experts.{e}.w{1,2,3}.{codes,codebooks,scales}``) would load with randomly initialised dense experts.
``QuantizedMixtralExperts`` is the drop-in replacement: children ``"0" .. "E-1"``, each with ``QuantizedLinear``s ``w1``, ``w3``
(hidden -> intermediate) and ``w2`` (intermediate -> hidden), so the checkpoint keys land by name once transformers renames
``.block_sparse_moe.`` to ``.mlp.``.

Forward, same signature and semantics as ``MixtralExperts.forward``:
  * MI355X, 1x16 g8 / g16, T * top_k <= 64 (decode): two launches of the expert-routed matvec (``aqlm::code1x16_moe_matmat``:
    w1 and w3 together, then w2 on the pair rows), the activation in between and an fp32 weighted sum on the device.  The expert
    ids never reach the host: no synchronisation, and the step can be captured in a hipGraph;
  * MI355X, 1x16 g8 / g16, more pairs (prefill, batched decode) or a gradient needed (any T): the expert-grouped GEMM
    (``aqlm::moe_bucket`` groups the pairs by expert on the device, then ``aqlm::code1x16_moe_matmat_grouped`` runs the w1|w3 and the
    w2 launch on grids fixed by the shapes).  No synchronisation either: prefill steps can be captured in a hipGraph too.  Under
    autograd each launch is a ``torch.autograd.Function`` whose backward runs per expert on ``code1x16_matmat_dequant_transposed``;
  * anything else (other schemes, host tensors, shapes the grouped kernel declines): a per-expert loop on the existing ops (host
    syncs allowed), differentiable through the layers' autograd op when a gradient is needed.
Either way each expert's output is multiplied by its fp32 router weight and the sum over top_k is rounded once to the activation
dtype; activation, product and weighted sum are plain torch ops, so ``top_k_weights`` gets its gradient from autograd.  No gradient
flows to codes, codebooks or scales (as in ``QuantizedLinear``).

Usage::

    from aqlm_amd.moe import from_pretrained, quantized_experts
    model = from_pretrained(path, torch_dtype=torch.float16, device_map="cuda")
    # or
    with quantized_experts():
        model = AutoModelForCausalLM.from_pretrained(path, ...)
"""
from __future__ import annotations

import contextlib

import torch
import torch.nn as nn

from .derived import tensor_version
from .inference import GEMV_MAX_ROWS, QuantizedLinear, _get_autograd_matmul_op
from .inference_kernels.kernel_selector import get_backward_pass_kernel, get_forward_pass_kernel

_SEGMENTS_13 = ("w1", "w3")
# (token, expert) pairs up to which a forward takes the routed launches (== AQLM_HIP_MAX_ROUTED_PAIRS: one launch per projection)
MAX_ROUTED_PAIRS = 64
# (token, expert) pairs up to which a forward may take the grouped launches (== AQLM_HIP_MAX_GROUPED_PAIRS)
MAX_GROUPED_PAIRS = 1 << 18
# pairs above which an eager call that needs no gradient keeps the per-expert loop: at 1024 pairs (Mixtral-8x7B block, T = 512) the
# grouped launches took 1.14x the loop's time, at 512 pairs 1.04x (profiles/moe_grouped.json).  Captures (the loop syncs with the
# host) and calls that need a gradient take the grouped launches at any size.
GROUPED_EAGER_MAX_PAIRS = 768


class _Expert(nn.Module):
    """One expert: ``w1`` (gate) and ``w3`` (up), hidden -> intermediate; ``w2`` (down), intermediate -> hidden."""

    def __init__(self, hidden: int, intermediate: int, scheme: dict, device=None, dtype=None):
        super().__init__()
        self.w1 = QuantizedLinear(hidden, intermediate, bias=False, device=device, dtype=dtype, **scheme)
        self.w3 = QuantizedLinear(hidden, intermediate, bias=False, device=device, dtype=dtype, **scheme)
        self.w2 = QuantizedLinear(intermediate, hidden, bias=False, device=device, dtype=dtype, **scheme)
        for lin in (self.w1, self.w3, self.w2):
            lin._moe_expert = True  # checkpoint.prepack_model leaves these alone: the routed kernel reads the canonical codes


def _scheme(quantization_config) -> dict:
    get = (lambda k: quantization_config[k]) if isinstance(quantization_config, dict) else (lambda k: getattr(quantization_config, k))
    return {k: int(get(k)) for k in ("in_group_size", "out_group_size", "num_codebooks", "nbits_per_codebook")}


class QuantizedMixtralExperts(nn.Module):
    """Drop-in for transformers' ``MixtralExperts`` with AQLM-quantized experts (module docstring)."""

    def __init__(self, config, quantization_config, device=None, dtype=None):
        super().__init__()
        from transformers.activations import ACT2FN

        self.num_experts = int(config.num_local_experts)
        self.hidden_dim = int(config.hidden_size)
        self.intermediate_dim = int(config.intermediate_size)
        self.act_fn = ACT2FN[config.hidden_act]
        scheme = _scheme(quantization_config)
        for e in range(self.num_experts):
            self.add_module(str(e), _Expert(self.hidden_dim, self.intermediate_dim, scheme, device=device, dtype=dtype))
        self._tables = None  # (key, table w1|w3, table w2): device pointer tables of the routed launches (derived, never saved)
        self._grouped_shapes = None  # whether the grouped kernel takes both projections' shapes (a host query, asked once)

    def expert(self, e: int) -> _Expert:
        return self._modules[str(e)]

    def extra_repr(self) -> str:
        w = self.expert(0).w1
        return (f"num_experts={self.num_experts}, hidden={self.hidden_dim}, intermediate={self.intermediate_dim}, "
                f"scheme={w.num_codebooks}x{w.nbits_per_codebook}g{w.in_group_size}")

    def __getstate__(self):
        state = dict(self.__dict__)
        state["_tables"] = None
        return state

    # ------------------------------------------------------------------------------------------------------------------
    def forward(self, hidden_states: torch.Tensor, top_k_index: torch.Tensor, top_k_weights: torch.Tensor) -> torch.Tensor:
        if self.takes_routed_path(hidden_states, top_k_index):
            return self._forward_routed(hidden_states, top_k_index, top_k_weights)
        if self.takes_grouped_path(hidden_states, top_k_index):
            return self._forward_grouped(hidden_states, top_k_index, top_k_weights)
        return self._forward_loop(hidden_states, top_k_index, top_k_weights)

    def takes_routed_path(self, hidden_states: torch.Tensor, top_k_index: torch.Tensor) -> bool:
        w = self.expert(0).w1
        return (hidden_states.is_cuda and hidden_states.dim() == 2 and w.codebooks.is_cuda
                and (w.num_codebooks, w.nbits_per_codebook, w.out_group_size) == (1, 16, 1) and w.in_group_size in (8, 16)
                and hidden_states.dtype in (torch.float16, torch.bfloat16) and hidden_states.dtype == w.codebooks.dtype
                and 0 < top_k_index.numel() <= MAX_ROUTED_PAIRS and not torch.compiler.is_compiling()
                and not (torch.is_grad_enabled() and hidden_states.requires_grad))

    def takes_grouped_path(self, hidden_states: torch.Tensor, top_k_index: torch.Tensor) -> bool:
        """The device-side grouped launches: same devices, scheme and dtypes as the routed path, and either more pairs than the
        routed launch takes or a gradient needed (a rule on shapes, dtypes and devices only: the routing never enters)."""
        w = self.expert(0).w1
        if not (hidden_states.is_cuda and hidden_states.dim() == 2 and top_k_index.dim() == 2 and w.codebooks.is_cuda
                and (w.num_codebooks, w.nbits_per_codebook, w.out_group_size) == (1, 16, 1) and w.in_group_size in (8, 16)
                and hidden_states.dtype in (torch.float16, torch.bfloat16) and hidden_states.dtype == w.codebooks.dtype
                and 0 < top_k_index.numel() <= MAX_GROUPED_PAIRS and not torch.compiler.is_compiling()):
            return False
        grad = _needs_grad(hidden_states)
        if not (top_k_index.numel() > MAX_ROUTED_PAIRS or grad):
            return False
        if not grad and top_k_index.numel() > GROUPED_EAGER_MAX_PAIRS and not torch.cuda.is_current_stream_capturing():
            return False
        if self._grouped_shapes is None:
            from .inference_kernels import hip_kernel

            H, I, g = self.hidden_dim, self.intermediate_dim, w.in_group_size
            self._grouped_shapes = (self.num_experts <= hip_kernel._native.MAX_ROUTED_EXPERTS
                                    and hip_kernel.grouped_supported(I, H, g) and hip_kernel.grouped_supported(H, I, g))
        return self._grouped_shapes

    def _table_tensors(self, segments):
        return [[(getattr(self.expert(e), s).codes, getattr(self.expert(e), s).codebooks, getattr(self.expert(e), s).scales,
                  getattr(self.expert(e), s).bias) for s in segments] for e in range(self.num_experts)]

    def routed_tables(self, device: torch.device):
        """The device tables of the two routed launches, rebuilt when any expert tensor moved or was written (data_ptr / version)."""
        from .inference_kernels import hip_kernel

        layers13, layers2 = self._table_tensors(_SEGMENTS_13), self._table_tensors(("w2",))
        key = (device, tuple((t.data_ptr(), tensor_version(t)) for per in layers13 + layers2 for seg in per
                             for t in seg if t is not None))
        if self._tables is None or self._tables[0] != key:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("QuantizedMixtralExperts: the expert tables are built by a host-to-device copy; run one eager "
                                   "forward before capturing (and again after moving or rewriting the experts)")
            self._tables = (key, hip_kernel.routed_table(layers13, device), hip_kernel.routed_table(layers2, device))
        return self._tables[1], self._tables[2]

    def _forward_routed(self, hidden_states, top_k_index, top_k_weights):
        T, H = hidden_states.shape
        k = top_k_index.shape[1]
        w = self.expert(0).w1
        tab13, tab2 = self.routed_tables(hidden_states.device)
        ops = torch.ops.aqlm
        gu = ops.code1x16_moe_matmat(hidden_states, top_k_index, tab13,
                                     [self.num_experts, 2, self.intermediate_dim, H, w.in_group_size, k], False)
        h = self.act_fn(gu[:, 0]) * gu[:, 1]  # [T * k, I]
        y = ops.code1x16_moe_matmat(h, top_k_index, tab2,
                                    [self.num_experts, 1, H, self.intermediate_dim, w.in_group_size, k], True)
        return (y.view(T, k, H).float() * top_k_weights.float().unsqueeze(-1)).sum(dim=1).to(hidden_states.dtype)

    def _forward_grouped(self, hidden_states, top_k_index, top_k_weights):
        """Pairs bucketed by expert once on the device, then two grouped launches (w1|w3 on the token rows, w2 on the pair rows)."""
        from .inference_kernels import hip_kernel

        T, H = hidden_states.shape
        k = top_k_index.shape[1]
        E, I, P = self.num_experts, self.intermediate_dim, T * k
        g = self.expert(0).w1.in_group_size
        tab13, tab2 = self.routed_tables(hidden_states.device)
        tp = hip_kernel.grouped_tile_pairs(P, E)
        bucket = torch.ops.aqlm.moe_bucket(top_k_index, E, tp)
        grad = _needs_grad(hidden_states)
        gu = _grouped(self, _SEGMENTS_13, hidden_states, bucket, tab13, [E, 2, I, H, g, k, tp, P], False, top_k_index, grad)
        h = self.act_fn(gu[:, 0]) * gu[:, 1]  # [T * k, I]
        y = _grouped(self, ("w2",), h, bucket, tab2, [E, 1, H, I, g, k, tp, P], True, top_k_index, grad)
        return (y.view(T, k, H).float() * top_k_weights.float().unsqueeze(-1)).sum(dim=1).to(hidden_states.dtype)

    def _forward_loop(self, hidden_states, top_k_index, top_k_weights):
        """Tokens grouped per expert, each group through the layer's ordinary ops (host syncs: the groups are sized on the host)."""
        out = torch.zeros(hidden_states.shape, dtype=torch.float32, device=hidden_states.device)
        hit = torch.unique(top_k_index).tolist()
        for e in hit:
            if not 0 <= e < self.num_experts:
                continue  # (MixtralExperts skips an id == num_experts the same way)
            tok, pos = torch.where(top_k_index == e)
            ex = self.expert(e)
            x = hidden_states[tok]
            h = self.act_fn(_apply(ex.w1, x)) * _apply(ex.w3, x)
            y = _apply(ex.w2, h)
            out.index_add_(0, tok, y.float() * top_k_weights[tok, pos, None].float())
        return out.to(hidden_states.dtype)


def _needs_grad(x: torch.Tensor) -> bool:
    return torch.is_grad_enabled() and x.requires_grad


class _GroupedProjection(torch.autograd.Function):
    """One grouped launch (one or two projections of every pair) with a gradient for its input rows:
    grad_x[row(p)] += sum_s (grad_y[p, s] * scales_{e_p, s}) @ W_{e_p, s}, per expert on ``code1x16_matmat_dequant_transposed``, summed
    over pairs and segments in fp32 and rounded once.  Codes, codebooks and scales get none (as in ``QuantizedLinear``)."""

    @staticmethod
    def forward(ctx, x, bucket, table, geometry, x_per_pair, experts, segments, top_k_index):
        ctx.experts, ctx.segments, ctx.geometry, ctx.x_per_pair, ctx.rows = experts, segments, geometry, x_per_pair, x.shape[0]
        ctx.save_for_backward(top_k_index)
        return torch.ops.aqlm.code1x16_moe_matmat_grouped(x, bucket, table, geometry, x_per_pair)

    @staticmethod
    def backward(ctx, grad_y):
        (top_k_index,) = ctx.saved_tensors
        E, S, _, K, _, k = (int(v) for v in ctx.geometry[:6])
        flat = top_k_index.reshape(-1)
        grad_x = torch.zeros((ctx.rows, K), dtype=torch.float32, device=grad_y.device)
        for e in torch.unique(flat).tolist():  # host syncs are fine in backward
            if not 0 <= e < E:
                continue  # zero rows in the forward: no gradient
            pairs = torch.nonzero(flat == e).squeeze(1)
            gy = grad_y[pairs]
            acc = None
            for s, name in enumerate(ctx.segments):
                lin = getattr(ctx.experts.expert(e), name)
                part = torch.ops.aqlm.code1x16_matmat_dequant_transposed(gy[:, s].contiguous(), lin.codes, lin.codebooks, lin.scales,
                                                                         None).float()
                acc = part if acc is None else acc + part
            grad_x.index_add_(0, pairs if ctx.x_per_pair else pairs // k, acc)
        return grad_x.to(grad_y.dtype), None, None, None, None, None, None, None


def _grouped(experts, segments, x, bucket, table, geometry, x_per_pair, top_k_index, grad):
    if grad:
        return _GroupedProjection.apply(x, bucket, table, geometry, x_per_pair, experts, tuple(segments), top_k_index)
    return torch.ops.aqlm.code1x16_moe_matmat_grouped(x, bucket, table, geometry, x_per_pair)


_AUTOGRAD_OPS = {}


def _apply(lin: QuantizedLinear, x: torch.Tensor) -> torch.Tensor:
    """``lin`` on ``x`` through the existing ops on its canonical codes, bypassing ``QuantizedLinear.forward`` (no prepack, no
    fast lane): the gemv op for up to GEMV_MAX_ROWS rows, the fused dequant / MFMA op beyond; on the host the direct 1x16 kernel or
    the torch dequantise + matmul (the host 8-bit kernel wants a permuted copy of the codes the experts do not keep).  When a
    gradient is needed the op runs inside the layers' autograd function (``_get_autograd_matmul_op``): the raw ops have no
    autograd kernel, and the host 1x16 kernel returns a tensor without history."""
    rows = x.shape[0]
    cb = lin.codebooks
    training = rows > GEMV_MAX_ROWS
    if cb.device.type == "cpu" and cb.shape[1] == 256:
        from .inference_kernels.kernel_selector import _torch_forward as op
    else:
        op = get_forward_pass_kernel(cb, training)
    x = x.to(cb.dtype)
    if not _needs_grad(x):
        return op(x, lin.codes, cb, lin.scales, lin.bias)
    key = (op, cb.device.type, tuple(cb.shape), training)
    fn = _AUTOGRAD_OPS.get(key)
    if fn is None:
        fn = _AUTOGRAD_OPS[key] = _get_autograd_matmul_op(op, get_backward_pass_kernel(cb, training))
    return fn.apply(x, lin.codes, cb, lin.scales, lin.bias)


# ----------------------------------------------------------------------------------------------------------------------
# loading
# ----------------------------------------------------------------------------------------------------------------------
def replace_moe_experts(model: nn.Module, quantization_config, modules_to_not_convert=None) -> int:
    """Swap every transformers ``MixtralExperts`` of ``model`` for a ``QuantizedMixtralExperts`` built on the device of the module
    it replaces (``meta`` while ``from_pretrained`` loads).  Returns how many were replaced."""
    try:
        from transformers.models.mixtral.modeling_mixtral import MixtralExperts
    except ImportError:  # pragma: no cover - transformers without Mixtral
        return 0
    from transformers.quantizers.quantizers_utils import should_convert_module

    config = getattr(model, "config", None)
    targets = [(name, m) for name, m in model.named_modules() if isinstance(m, MixtralExperts)
               and should_convert_module(name, modules_to_not_convert)]
    if targets and config is None:
        raise ValueError("replace_moe_experts needs the model's config (hidden_act, sizes)")
    for name, m in targets:
        new = QuantizedMixtralExperts(config, quantization_config, device=m.gate_up_proj.device)
        new.requires_grad_(False)
        model.set_submodule(name, new)
    return len(targets)


@contextlib.contextmanager
def quantized_experts():
    """While active, the AQLM quantizer of transformers also swaps the Mixtral experts for quantized ones (wraps the name
    ``transformers.quantizers.quantizer_aqlm.replace_with_aqlm_linear``, which the quantizer calls; restored on exit, exceptions
    included)."""
    import transformers.quantizers.quantizer_aqlm as qa

    original = qa.replace_with_aqlm_linear

    def replace_with_aqlm_linear(model, *args, **kwargs):
        out = original(model, *args, **kwargs)
        skip = kwargs.get("modules_to_not_convert", args[0] if len(args) > 0 else None)
        qc = kwargs.get("quantization_config", args[1] if len(args) > 1 else None)
        replace_moe_experts(model, qc, modules_to_not_convert=skip)
        return out

    replace_with_aqlm_linear.__wrapped__ = original
    qa.replace_with_aqlm_linear = replace_with_aqlm_linear
    try:
        yield
    finally:
        qa.replace_with_aqlm_linear = original


def from_pretrained(path, **kwargs):
    """``AutoModelForCausalLM.from_pretrained(path, **kwargs)`` with ``quantized_experts()`` active."""
    from transformers import AutoModelForCausalLM

    with quantized_experts():
        return AutoModelForCausalLM.from_pretrained(path, **kwargs)
