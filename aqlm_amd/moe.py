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
  * the same on PREPACKED experts (``prepack_experts``, opt-in: 4.8 more resident bits per expert weight), for up to
    ``ROUTED_PACKED_MAX_PAIRS`` pairs: the two launches run the packed matvec (``aqlm::code1x16_moe_matmat_packed``, codebook slices
    in LDS) instead of the direct one; same glue, no synchronisation, capturable;
  * MI355X, 1x16 g8 / g16, more pairs (prefill, batched decode) or a gradient needed (any T): the expert-grouped GEMM
    (``aqlm::moe_bucket`` groups the pairs by expert on the device, then ``aqlm::code1x16_moe_matmat_grouped`` runs the w1|w3 and the
    w2 launch on grids fixed by the shapes).  No synchronisation either: prefill steps can be captured in a hipGraph too.  Under
    autograd each launch is a ``torch.autograd.Function`` whose backward is ONE launch of the transposed grouped GEMM
    (``aqlm::code1x16_moe_matmat_grouped_transposed``) on the same bucket: no synchronisation, so a whole training step can be captured
    (``GROUPED_BACKWARD = False`` or a shape that launch declines: per expert on ``code1x16_matmat_dequant_transposed``, with host syncs);
  * anything else (other schemes, host tensors, shapes the grouped kernel declines): a per-expert loop on the existing ops (host
    syncs allowed), differentiable through the layers' autograd op when a gradient is needed.
LoRA adapters on the experts (``lora.LoraQuantizedMixtralExperts``) enter through one seam: ``forward`` takes an optional adapter
provider.  The three pair-batched routes call ``adapters.on_pairs`` twice -- on ``gu`` [P, 2, I] with the token rows, before the
activation, and on ``y`` [P, 1, H] with the pair rows ``h``, before the weighted sum --, the per-expert loop calls
``adapters.on_rows`` per expert and projection on that expert's rows; each returns the tensor to go on with (the same one, added to
in place, or a new one).  Without a provider every route runs exactly the ops above in the same order.
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

from .derived import codes_fingerprint, tensor_version
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
# (token, expert) pairs up to which a prepacked block (``prepack_experts``) takes the routed PACKED launches; beyond it the routes above
# apply unchanged.  A measured constant: the largest pair count, among T in {1, 2, 4, 8, 16, 32} at top_k 2, up to which the captured
# prepacked block replayed faster than both the captured direct-routed block and the eager per-expert loop in the same call of
# tools/moe_benchmark.py on the Mixtral-8x7B block shape (table, spread and command: profiles/moe_block_packed.json).
# Measured: the prepacked block won at every T (85.8 against 223.5 us captured at T = 1, 1328 against 1942 us at T = 32), so the
# constant is the launch's own limit of 64 pairs.
ROUTED_PACKED_MAX_PAIRS = 64
# The backward of the grouped launches runs on the device (one transposed grouped launch per projection group, no host
# synchronisation); False: the per-expert loop on code1x16_matmat_dequant_transposed, as before that launch existed (A/B runs;
# also the fallback for shapes the launch declines).
GROUPED_BACKWARD = True


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
        self._grouped_bwd_shapes = {}  # (out, in, g) -> whether the transposed grouped launch (the backward) takes the shape
        self._prepack = None  # options of prepack_experts() once it ran on this block (None: the experts are not prepacked)
        self._packed_tables = None  # (key, (table, geometry tail) w1|w3, the same for w2) or (key, None): the launch declined
        self._packed_calls = 0  # eager routed-packed forwards, for the periodic checksum of the parameters behind the packed copies

    def expert(self, e: int) -> _Expert:
        return self._modules[str(e)]

    def extra_repr(self) -> str:
        w = self.expert(0).w1
        return (f"num_experts={self.num_experts}, hidden={self.hidden_dim}, intermediate={self.intermediate_dim}, "
                f"scheme={w.num_codebooks}x{w.nbits_per_codebook}g{w.in_group_size}")

    def __getstate__(self):
        state = dict(self.__dict__)
        state["_tables"] = None
        state["_packed_tables"] = None
        return state

    # ------------------------------------------------------------------------------------------------------------------
    def forward(self, hidden_states: torch.Tensor, top_k_index: torch.Tensor, top_k_weights: torch.Tensor,
                adapters=None) -> torch.Tensor:
        """``adapters``: the optional adapter provider of ``lora.LoraQuantizedMixtralExperts`` (module docstring); None runs
        exactly the ops of the bare block."""
        if self._prepack is not None and self.takes_routed_path(hidden_states, top_k_index):
            tables = self._routed_packed_tables_for(hidden_states, top_k_index)
            if tables is not None:
                return self._forward_routed_packed(hidden_states, top_k_index, top_k_weights, tables, adapters)
        if self.takes_routed_path(hidden_states, top_k_index):
            return self._forward_routed(hidden_states, top_k_index, top_k_weights, adapters)
        if self.takes_grouped_path(hidden_states, top_k_index):
            return self._forward_grouped(hidden_states, top_k_index, top_k_weights, adapters)
        return self._forward_loop(hidden_states, top_k_index, top_k_weights, adapters)

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

    def _grouped_backward_shapes(self, out_features: int, in_features: int, in_group_size: int) -> bool:
        """Whether the transposed grouped launch takes a projection of this shape (a host query, asked once per shape)."""
        key = (out_features, in_features, in_group_size)
        if key not in self._grouped_bwd_shapes:
            from .inference_kernels import hip_kernel

            self._grouped_bwd_shapes[key] = hip_kernel.grouped_transposed_supported(*key)
        return self._grouped_bwd_shapes[key]

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

    # -------------------------------------------------------------------------------------------- prepacked experts
    def _expert_layers(self):
        return [getattr(self.expert(e), name) for e in range(self.num_experts) for name in _SEGMENTS_13 + ("w2",)]

    def _packed_layers(self, segments):
        return [[(getattr(self.expert(e), s)._packed_codes, getattr(self.expert(e), s).codebooks, getattr(self.expert(e), s).scales,
                  getattr(self.expert(e), s).bias) for s in segments] for e in range(self.num_experts)]

    def _repack_stale_experts(self) -> None:
        """Bring the packed copy of every expert layer in step with its ``codes`` (written in place, rebound, or forgotten by
        ``invalidate_derived_state()``).  Repacks synchronise: never while a hipGraph is being captured."""
        for lin in self._expert_layers():
            if lin._packed_codes is None or codes_fingerprint(lin.codes) != lin._packed_fingerprint:
                _prepack_layer(lin, **self._prepack)

    def _packed_key(self, device):
        return (device, tuple((codes_fingerprint(lin.codes), id(lin._packed_codes), lin._packed_fingerprint,
                               lin.codebooks.data_ptr(), tensor_version(lin.codebooks), lin.scales.data_ptr(), tensor_version(lin.scales),
                               0 if lin.bias is None else lin.bias.data_ptr(), 0 if lin.bias is None else tensor_version(lin.bias))
                              for lin in self._expert_layers()))

    def routed_packed_tables(self, device: torch.device):
        """The device tables (+ launch geometry) of the two routed packed launches, or None when this call keeps today's route.
        The packed buffers are derived from ``codes``, the tables bake in every buffer's address, the codebook range and -- for a
        relabelled buffer -- its codebook image, so they are keyed on identity and version of codes, codebooks, scales and biases
        and on the packed buffers themselves.  Anything out of step is rebuilt (repack, range, image, table) on an eager call;
        inside a hipGraph capture nothing can be rebuilt, and the call takes the routed launch on the canonical codes."""
        from .inference_kernels import hip_kernel

        cached = self._packed_tables
        if cached is not None and cached[0] == self._packed_key(device):
            if cached[1] is None or all(lin._packed_codes.range_is_current(lin.codebooks) for lin in self._expert_layers()):
                return cached[1]
        if torch.cuda.is_current_stream_capturing():
            return None  # stale and not rebuildable here: today's route reads the live tensors
        self._repack_stale_experts()
        if any(lin._packed_codes is None for lin in self._expert_layers()):
            tables = None  # a layer below min_codes, or one the packed format does not take
        else:
            try:
                tables = (hip_kernel.routed_packed_table(self._packed_layers(_SEGMENTS_13), device),
                          hip_kernel.routed_packed_table(self._packed_layers(("w2",)), device))
            except NotImplementedError:
                tables = None  # the launch declines the block (compact entries, no codebook range, a shape it refuses)
        for lin in self._expert_layers():  # the checksums the periodic check compares belong to the state that now exists
            if lin._packed_codes is not None:
                lin._record_derived_checks()
        self._packed_tables = (self._packed_key(device), tables)
        return tables

    def served_by_routed_packed(self) -> bool:
        """Whether the routed packed launch takes this block as it is now (prepacked, every layer packed, launch not declined)."""
        if self._prepack is None or not self.expert(0).w1.codebooks.is_cuda:
            return False
        return self.routed_packed_tables(self.expert(0).w1.codebooks.device) is not None

    def _routed_packed_tables_for(self, hidden_states, top_k_index):
        """The tables when this call takes the routed packed launches (``takes_routed_packed_route``), else None."""
        if top_k_index.numel() > ROUTED_PACKED_MAX_PAIRS:
            return None
        capturing = torch.cuda.is_current_stream_capturing()
        if not capturing:
            self._verify_some_expert()
        tables = self.routed_packed_tables(hidden_states.device)
        if not takes_routed_packed_route(True, _needs_grad(hidden_states), top_k_index.numel(), tables is not None):
            return None
        return tables

    def _verify_some_expert(self) -> None:
        """Writes through ``.data`` change neither identity nor version: like every owner of derived state, the block re-takes the
        checksums of its layers now and then (inference.DERIVED_CHECK_EVERY eager forwards for a full round, one layer at a time so
        that no step pays for all of them).  Synchronises; never during capture."""
        from . import inference

        every = inference.DERIVED_CHECK_EVERY
        if not every:
            return
        self._packed_calls += 1
        layers = self._expert_layers()
        step = max(1, every // len(layers))
        if self._packed_calls % step == 0:
            layers[(self._packed_calls // step) % len(layers)].verify_derived_state()

    def _forward_routed_packed(self, hidden_states, top_k_index, top_k_weights, tables, adapters=None):
        T, H = hidden_states.shape
        k = top_k_index.shape[1]
        w = self.expert(0).w1
        (tab13, tail13), (tab2, tail2) = tables
        ops = torch.ops.aqlm
        gu = ops.code1x16_moe_matmat_packed(hidden_states, top_k_index, tab13,
                                            [self.num_experts, 2, self.intermediate_dim, H, w.in_group_size, k] + tail13, False)
        if adapters is not None:
            gu = adapters.on_pairs(gu, hidden_states, top_k_index, _SEGMENTS_13, False)
        h = self.act_fn(gu[:, 0]) * gu[:, 1]  # [T * k, I]
        y = ops.code1x16_moe_matmat_packed(h, top_k_index, tab2,
                                           [self.num_experts, 1, H, self.intermediate_dim, w.in_group_size, k] + tail2, True)
        if adapters is not None:
            y = adapters.on_pairs(y, h, top_k_index, ("w2",), True)
        return (y.view(T, k, H).float() * top_k_weights.float().unsqueeze(-1)).sum(dim=1).to(hidden_states.dtype)

    def _forward_routed(self, hidden_states, top_k_index, top_k_weights, adapters=None):
        T, H = hidden_states.shape
        k = top_k_index.shape[1]
        w = self.expert(0).w1
        tab13, tab2 = self.routed_tables(hidden_states.device)
        ops = torch.ops.aqlm
        gu = ops.code1x16_moe_matmat(hidden_states, top_k_index, tab13,
                                     [self.num_experts, 2, self.intermediate_dim, H, w.in_group_size, k], False)
        if adapters is not None:
            gu = adapters.on_pairs(gu, hidden_states, top_k_index, _SEGMENTS_13, False)
        h = self.act_fn(gu[:, 0]) * gu[:, 1]  # [T * k, I]
        y = ops.code1x16_moe_matmat(h, top_k_index, tab2,
                                    [self.num_experts, 1, H, self.intermediate_dim, w.in_group_size, k], True)
        if adapters is not None:
            y = adapters.on_pairs(y, h, top_k_index, ("w2",), True)
        return (y.view(T, k, H).float() * top_k_weights.float().unsqueeze(-1)).sum(dim=1).to(hidden_states.dtype)

    def _forward_grouped(self, hidden_states, top_k_index, top_k_weights, adapters=None):
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
        if adapters is not None:
            gu = adapters.on_pairs(gu, hidden_states, top_k_index, _SEGMENTS_13, False)
        h = self.act_fn(gu[:, 0]) * gu[:, 1]  # [T * k, I]
        y = _grouped(self, ("w2",), h, bucket, tab2, [E, 1, H, I, g, k, tp, P], True, top_k_index, grad)
        if adapters is not None:
            y = adapters.on_pairs(y, h, top_k_index, ("w2",), True)
        return (y.view(T, k, H).float() * top_k_weights.float().unsqueeze(-1)).sum(dim=1).to(hidden_states.dtype)

    def _forward_loop(self, hidden_states, top_k_index, top_k_weights, adapters=None):
        """Tokens grouped per expert, each group through the layer's ordinary ops (host syncs: the groups are sized on the host)."""
        out = torch.zeros(hidden_states.shape, dtype=torch.float32, device=hidden_states.device)
        hit = torch.unique(top_k_index).tolist()
        for e in hit:
            if not 0 <= e < self.num_experts:
                continue  # (MixtralExperts skips an id == num_experts the same way)
            tok, pos = torch.where(top_k_index == e)
            ex = self.expert(e)
            x = hidden_states[tok]
            if adapters is None:
                h = self.act_fn(_apply(ex.w1, x)) * _apply(ex.w3, x)
                y = _apply(ex.w2, h)
            else:
                h = (self.act_fn(adapters.on_rows(_apply(ex.w1, x), x, e, "w1", tok))
                     * adapters.on_rows(_apply(ex.w3, x), x, e, "w3", tok))
                y = adapters.on_rows(_apply(ex.w2, h), h, e, "w2", tok)
            out.index_add_(0, tok, y.float() * top_k_weights[tok, pos, None].float())
        return out.to(hidden_states.dtype)


def takes_routed_packed_route(prepacked: bool, grad_needed: bool, pairs: int, supported: bool) -> bool:
    """The route predicate of the routed packed launches, a pure function: the block is prepacked, no gradient is needed, there
    are 1..ROUTED_PACKED_MAX_PAIRS (token, expert) pairs, and the launch takes the block's packed buffers.  (Device, scheme and
    dtype are the routed path's own conditions, ``takes_routed_path``.)"""
    return bool(prepacked and not grad_needed and 0 < pairs <= min(ROUTED_PACKED_MAX_PAIRS, MAX_ROUTED_PAIRS) and supported)


def takes_grouped_backward(enabled: bool, supported: bool) -> bool:
    """The route predicate of the device-side grouped backward (``aqlm::code1x16_moe_matmat_grouped_transposed``), a pure function:
    the route is switched on (``GROUPED_BACKWARD``) and the launch takes the projection's shape.  Pair count and capture state do
    not enter: the device route serves every size (the per-expert loop cannot be captured at all).  (Device, scheme and dtype are
    the grouped forward's own conditions, ``takes_grouped_path``: only its calls reach a backward.)"""
    return bool(enabled and supported)


def _needs_grad(x: torch.Tensor) -> bool:
    return torch.is_grad_enabled() and x.requires_grad


class _GroupedProjection(torch.autograd.Function):
    """One grouped launch (one or two projections of every pair) with a gradient for its input rows:
    grad_x[row(p)] += sum_s (grad_y[p, s] * scales_{e_p, s}) @ W_{e_p, s}, summed over pairs and segments in fp32 and rounded once.
    ONE launch of ``aqlm::code1x16_moe_matmat_grouped_transposed`` on the forward's bucket (no host synchronisation, capturable; it
    rounds grad_y * scales once to the storage type, W stays exact), or -- for shapes that launch declines, or with
    ``GROUPED_BACKWARD`` off -- per expert on ``code1x16_matmat_dequant_transposed`` (host syncs, W * scales rounded instead).
    Codes, codebooks and scales get none (as in ``QuantizedLinear``)."""

    @staticmethod
    def forward(ctx, x, bucket, table, geometry, x_per_pair, experts, segments, top_k_index):
        ctx.experts, ctx.segments, ctx.geometry, ctx.x_per_pair, ctx.rows = experts, segments, geometry, x_per_pair, x.shape[0]
        ctx.save_for_backward(top_k_index, bucket, table)
        return torch.ops.aqlm.code1x16_moe_matmat_grouped(x, bucket, table, geometry, x_per_pair)

    @staticmethod
    def backward(ctx, grad_y):
        top_k_index, bucket, table = ctx.saved_tensors
        E, S, M, K, g, k = (int(v) for v in ctx.geometry[:6])
        if takes_grouped_backward(GROUPED_BACKWARD, ctx.experts._grouped_backward_shapes(M, K, g)):
            gx = torch.ops.aqlm.code1x16_moe_matmat_grouped_transposed(grad_y, bucket, table, ctx.geometry)
            if not ctx.x_per_pair:
                gx = gx.view(ctx.rows, k, K).sum(dim=1)  # fp32, the token's pairs in ascending order
            return gx.to(grad_y.dtype), None, None, None, None, None, None, None
        flat = top_k_index.reshape(-1)
        grad_x = torch.zeros((ctx.rows, K), dtype=torch.float32, device=grad_y.device)
        for e in torch.unique(flat).tolist():  # host syncs: the fallback only
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
# prepacked experts
# ----------------------------------------------------------------------------------------------------------------------
def _prepack_layer(lin: QuantizedLinear, min_codes: int, relabel: bool) -> bool:
    """The packed copy of one expert layer, next to its canonical codes (the grouped GEMM and backward read those).  Uniform
    geometry always: the routed packed launch does not instantiate the variable-geometry kernel."""
    from .inference_kernels import hip_kernel

    lin._packed_codes = None
    lin._fast = None
    codes = lin.out_features * (lin.in_features // lin.in_group_size)
    if (min_codes and codes >= min_codes and (lin.num_codebooks, lin.nbits_per_codebook, lin.out_group_size) == (1, 16, 1)
            and lin.in_group_size in (8, 16) and lin.codes.is_cuda and lin.codebooks.dtype in (torch.float16, torch.bfloat16)):
        lin._packed_codes = hip_kernel.prepack_1x16(lin.codes, lin.in_group_size, codebooks=lin.codebooks, relabel=relabel,
                                                    uniform_only=True)
        lin._packed_fingerprint = codes_fingerprint(lin.codes)
    if lin._packed_codes is not None:
        lin._derived_checks = None
        lin._record_derived_checks()
    return lin._packed_codes is not None


def prepack_experts(model_or_block: nn.Module, min_codes=None, thorough: bool = False, relabel: bool = False) -> dict:
    """Prepack w1, w3 and w2 of every ``QuantizedMixtralExperts`` under ``model_or_block`` (GPU-resident, 1x16 g8 / g16 layers of at
    least ``min_codes`` codes; default ``inference.PREPACK_MIN_CODES``) so that decode steps of up to ``ROUTED_PACKED_MAX_PAIRS``
    pairs run the routed PACKED launches.  Strictly opt-in: ``checkpoint.prepack_model`` keeps leaving experts alone.

    The canonical codes are KEPT (the expert-grouped GEMM of prefill and the backward read them), so the price is the packed
    copy on top: 4.8 resident bits per expert weight in addition to the 2.0 of the codes.  Mixtral-8x7B has
    32 x 8 x 3 x 14336 x 4096 = 45.1 G expert weights: about 27 GB more.

    ``thorough`` as in ``prepack_model`` (local search of the entry order on every layer).  ``relabel=False`` (default) keeps the
    checkpoint's codebook labels, so the kernels read the live codebook tensor and a codebook rewritten through ``.data`` is picked
    up by the very next forward; ``relabel=True`` deals the codebook entries to the slices by use (faster on checkpoints whose
    label use is skewed) at the price of a derived codebook image, which follows a ``.data`` write only at the next periodic
    checksum or after ``invalidate_derived_state()``.  Variable-geometry buffers are never built here (the routed packed launch
    declines them).

    Returns ``{"blocks", "layers_packed", "layers_skipped", "packed_bytes", "blocks_served", "blocks_fallback",
    "prepack_seconds"}``: ``blocks_fallback`` blocks keep today's routes (a layer below ``min_codes`` or refused by the packed
    format, or a table the launch declines)."""
    import time

    from . import _native, inference

    blocks = [m for m in model_or_block.modules() if isinstance(m, QuantizedMixtralExperts)]
    min_codes = inference.PREPACK_MIN_CODES if min_codes is None else int(min_codes)
    old_arr = _native.get_tuning("packed_arrange")
    if thorough:
        _native.set_tuning("packed_arrange", 3)
    if torch.cuda.is_available():
        torch.cuda.synchronize()
    t0 = time.perf_counter()
    rep = {"blocks": len(blocks), "layers_packed": 0, "layers_skipped": 0, "packed_bytes": 0, "blocks_served": 0, "blocks_fallback": 0}
    try:
        for block in blocks:
            if not block.expert(0).w1.codes.is_cuda:
                raise NotImplementedError("prepack_experts needs the experts on an MI355X (`model.to('cuda')` first)")
            block._prepack = {"min_codes": min_codes, "relabel": bool(relabel)}
            block._packed_tables = None
            for lin in block._expert_layers():
                if _prepack_layer(lin, **block._prepack):
                    rep["layers_packed"] += 1
                    rep["packed_bytes"] += lin._packed_codes.numel()
                else:
                    rep["layers_skipped"] += 1
            served = block.served_by_routed_packed()
            rep["blocks_served" if served else "blocks_fallback"] += 1
    finally:
        _native.set_tuning("packed_arrange", old_arr)
    if torch.cuda.is_available():
        torch.cuda.synchronize()
    rep["prepack_seconds"] = time.perf_counter() - t0
    return rep


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
