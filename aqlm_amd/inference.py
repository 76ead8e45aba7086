"""``QuantizedLinear``: the module Hugging Face instantiates for every AQLM-quantized ``nn.Linear``.

Host-side mirror of the reference module (inference_lib/src/aqlm/inference.py:11-142): identical constructor
signature, parameter names / shapes / dtypes (so checkpoints written by convert_to_hf.py load unchanged,
including construction on the ``meta`` device by transformers/integrations/aqlm.py:47-57), identical
gemv-vs-gemm rule, autograd support -- with the kernels behind it replaced by the MI355X ops.
"""
from __future__ import annotations

import math
from typing import Optional

import torch
import torch.nn as nn

from .derived import codes_fingerprint, tensor_checksum, tensor_version
from .inference_kernels import get_backward_pass_kernel, get_forward_pass_kernel
from .utils import get_int_dtype

# rows (batch * seq) at or below which the gemv op is used; the reference's value (inference.py:95-96)
GEMV_MAX_ROWS = 6

# 1x16 (g8 / g16) matvecs (<= GEMV_MAX_ROWS rows) of layers with at least this many codes (out_features * in_features / g) run on
# slice-bucketed ("prepacked") codes (aqlm_hip_gemv_1x16_packed): 1.2-5x faster than the direct L2-gather kernel on
# MI355X, at the price of a one-off repack at first use and ~2.3x the code bytes (kept next to the original codes unless
# `drop_canonical_codes()` is called).  0 disables.  Measured cross-over (cold, single launch each): 4096->1024 (0.5 M
# codes) 4.6 us packed vs 5.3 us direct; below that the fixed cost of the 64 KiB LDS fill per CU dominates.
PREPACK_MIN_CODES = 500_000

# Everything a module derives from its parameters (prepacked / planar / permuted codes, the codebook image and range, a dense W)
# is keyed on the parameters' identity and version counter -- and a write through `.data` (`m.codes.data.copy_(...)`, some
# loaders, hand-written surgery) changes neither.  The reference has no such state (its launcher reads the live tensors on every
# call, cuda_kernel.cpp:148-182).  So every DERIVED_CHECK_EVERY-th forward of a module (never while a hipGraph is being captured
# or traced) re-takes a 128-bit checksum of the parameters the derived state came from (aqlm_hip_checksum: one small kernel + a
# 16-byte read-back per parameter, ~40 us) and rebuilds what no longer matches; `invalidate_derived_state()` does it on demand.
# 0 = never check.  The check is EAGER-ONLY by construction: it never runs under hipGraph replay (a captured forward does not pass
# through this Python at all) nor in a torch.compile'd graph -- there, call `invalidate_derived_state()` after such a write and
# re-capture.  The modules of a model start their counters at different offsets, so the checks do not land on the same step.
DERIVED_CHECK_EVERY = 256

# Rows above which the large-batch 1x16 op dequantises W and calls the library GEMM (hip_kernel.FUSED_MFMA_MAX_ROWS; restated here so
# that the route predicate below needs no GPU library -- tests hold the two together).
PACKED_DEQUANT_ABOVE_ROWS = 256

ROUTE_CANONICAL = "canonical"                # the layer has its codes: nothing below applies
ROUTE_PACKED_MATVEC = "packed_matvec"        # <= GEMV_MAX_ROWS rows, no gradient: the packed matvec
ROUTE_PACKED_DEQUANT = "packed_dequant"      # W straight from the packed buffer (aqlm_hip_dequant_1x16_packed) + library GEMM
ROUTE_RESTORE = "restore"                    # the canonical codes come back for good (one unpack), then the ordinary op
ROUTE_TRANSIENT_UNPACK = "transient_unpack"  # one unpack for this call, then the ordinary op


def dropped_layer_route(dropped: bool, strict: bool, rows_from_packed: int, rows: int, in_features_mod_64: int,
                        grad_needed: bool) -> str:
    """How a 1x16 layer whose canonical codes were dropped (its ``_packed_codes`` is a ``PackedCodes``) serves a forward of
    ``rows`` input rows -- a pure function, so the table can be tested without a GPU:
      * <= GEMV_MAX_ROWS rows without a gradient: the packed matvec;
      * more than PACKED_DEQUANT_ABOVE_ROWS rows, or ``in_features % 64 != 0`` at 7+ rows -- where the large-batch op is dequant +
        library GEMM + fp32 scale / bias anyway: W comes straight from the packed buffer, same arithmetic, same bits, and the
        layer stays dropped (with or without a gradient);
      * ``rows_from_packed`` > 0 (the opt-in, ``prepack_model(single_copy=True)``): every no-grad forward of at least that many
        rows (never fewer than 7) takes that route as well -- 7 .. 256-row results then differ from the fused MFMA op's in the
        last bits (another accumulation order);
      * anything else needs the canonical codes (the fused MFMA op of 7 .. 256 rows, a forward of <= 6 rows with a gradient): a
        strict drop unpacks for the call, a non-strict one restores the codes for good.
    The BACKWARD of a layer that is still dropped when it runs always dequantises from the packed buffer, whatever the forward
    took."""
    if not dropped:
        return ROUTE_CANONICAL
    if rows <= GEMV_MAX_ROWS and not grad_needed:
        return ROUTE_PACKED_MATVEC
    if rows > GEMV_MAX_ROWS:
        if rows > PACKED_DEQUANT_ABOVE_ROWS or in_features_mod_64 != 0:
            return ROUTE_PACKED_DEQUANT
        if rows_from_packed > 0 and rows >= rows_from_packed and not grad_needed:
            return ROUTE_PACKED_DEQUANT
    return ROUTE_TRANSIENT_UNPACK if strict else ROUTE_RESTORE


class QuantizedLinear(nn.Module):
    def __init__(
        self,
        in_features: int,
        out_features: int,
        in_group_size: int,
        out_group_size: int,
        num_codebooks: int,
        nbits_per_codebook: int,
        bias=True,
        device=None,
        dtype=None,
    ):
        super().__init__()
        if in_features % in_group_size or out_features % out_group_size:
            raise AssertionError("feature counts must be divisible by the group sizes")
        self.in_features, self.out_features = in_features, out_features
        self.in_group_size, self.out_group_size = in_group_size, out_group_size
        self.num_codebooks = num_codebooks
        self.nbits_per_codebook = nbits_per_codebook
        self.codebook_size = 2**nbits_per_codebook
        n_out, n_in = out_features // out_group_size, in_features // in_group_size
        fkw = {"device": device, "dtype": dtype}

        def frozen(t):
            return nn.Parameter(t, requires_grad=False)

        # same registration order as the reference (inference.py:39-61): codebooks, codes, scales, bias
        self.codebooks = frozen(torch.empty((num_codebooks, self.codebook_size, out_group_size, in_group_size), **fkw))
        self.codes = frozen(torch.empty((n_out, n_in, num_codebooks), device=device, dtype=get_int_dtype(nbits_per_codebook)))
        self.scales = frozen(torch.empty((n_out, 1, 1, 1), **fkw))
        if bias:
            self.bias = frozen(torch.empty(out_features, **fkw))
        else:
            self.register_parameter("bias", None)

        self._codes_dropped = False
        self._codes_drop_strict = True  # False: the first call that needs the canonical codes restores them for good (prepack_model's default)
        self._codes_shape = None
        self._shared_input_group = None  # set by aqlm_amd.fusion.fuse_shared_input_linears
        # Escape hatch for mid-size batches (7 .. N - 1 rows: prefill chunks, speculative verification): run them as a dense GEMM
        # on a cached fp16 / bf16 copy of W instead of the fused dequant -> MFMA op.  Measured on MI355X at 4096 x 4096
        # (BENCH detail `bs128_1x16g8_4096x4096`): dense 12.1 / 12.6 / 14.5 us at 16 / 32 / 64 rows against 15.6 / 16.7 / 18.1 us
        # fused -- the fused op's 2.1 M codebook gathers cannot stream like a dense weight does.  The price is the memory the
        # format exists to save (2 bytes per weight for every layer that uses it), so it is off (0) unless asked for:
        # `module.prefer_dense_below_rows = 129`, or `aqlm.checkpoint.enable_dense_below_rows(model, 129)`.
        self.prefer_dense_below_rows = 0
        # Opt-in (`prepack_model(single_copy=True)` sets 7): a layer whose canonical codes were dropped serves every no-grad forward
        # of at least this many rows as W-from-the-packed-buffer + library GEMM + fp32 scale / bias -- the large-batch op's > 256-row
        # arithmetic at any row count -- so that no call of an inference deployment ever unpacks.  0 = off (`dropped_layer_route`).
        self.rows_from_packed = 0
        self._reset_derived()

    # Everything the module derives from its parameters, in the state "not built yet": the kernel choice and autograd ops, the
    # prepacked / planar codes of the GPU decode kernels (`_packed_codes`, keyed on `_packed_fingerprint`) with their codebook
    # range, the permuted codes of the host LUT kernel, the dense W (`_dense`: (fingerprint, W)), the compiled fast lane of the
    # decode call (`_fast`, aqlm_amd/_front.py: a pybind11 object that cannot be pickled) and the checksums of the parameters it
    # was all built from (`_derived_checks`, see DERIVED_CHECK_EVERY), and the inverted index of the codes that the codebook
    # gradient of a trainable 1x16 layer is summed through (`_grad_index`: (fingerprint of the codes, CodebookGradIndex)).  `_prepack_deferred`: a transition inside a hipGraph
    # capture or a trace left its last step (`_settle`, and the repack if that waited too) to the first eager forward.  None of it is saved, copied or pickled:
    # `copy.deepcopy(model)`, `torch.save(model)` and `pickle` work at any time (EMA copies, PEFT `modules_to_save`, draft-model
    # clones), and the copy rebuilds its derived state at its first forward.  A module whose canonical codes were dropped hands
    # them back to the copy.
    _DERIVED_DEFAULTS = {"gemv_op": None, "gemm_op": None, "use_gemv_rule": None, "_fast": None, "_packed_codes": None,
                         "_packed_fingerprint": None, "_cpu_codes_alt": None, "_prepack_deferred": False, "_dense": None,
                         "_derived_checks": None, "_calls_since_check": 0, "_grad_index": None}

    def _reset_derived(self) -> None:
        """Forget everything derived from the parameters.  With the canonical codes dropped the packed buffer IS the weights: it
        stays and forgets only its codebook range."""
        packed = self._packed_codes if self._codes_dropped else None
        self.__dict__.update(self._DERIVED_DEFAULTS)
        if packed is not None:
            packed.forget_range()
            self._packed_codes = packed

    def __getstate__(self):
        state = dict(self.__dict__)
        if self._codes_dropped:
            params = state["_parameters"].copy()
            params["codes"] = nn.Parameter(self._canonical_codes(), requires_grad=False)
            state["_parameters"] = params
            state["_codes_dropped"] = False
        state.update(self._DERIVED_DEFAULTS)
        return state

    def extra_repr(self) -> str:
        return (f"in_features={self.in_features}, out_features={self.out_features}, scheme="
                f"{self.num_codebooks}x{self.nbits_per_codebook}g{self.in_group_size}, bias={self.bias is not None}")

    def invalidate_derived_state(self) -> None:
        """Forget everything derived from the parameters (kernel choice, prepacked / planar / permuted codes, the codebook image
        and range, the dense W, the compiled fast lane); the next forward rebuilds it.  Call it after writing a parameter through
        a path PyTorch does not version (``m.codes.data.copy_(...)``) when the periodic check (DERIVED_CHECK_EVERY) is too late
        or switched off.  A module whose canonical codes were dropped keeps its packed buffer (it IS the weights) and forgets only
        what came from the codebooks."""
        self._reset_derived()
        group = self._shared_input_group
        if group is not None and hasattr(group, "invalidate"):
            group.invalidate()

    def _settle(self) -> None:
        """The last step of every transition that creates, drops or restores derived state: bring the packed buffer's codebook
        range up to date, build the fast lane the state allows, and record the checks of exactly the state that now exists.  The
        range and the checksums are read back, which a hipGraph capture or a trace does not allow: there the step waits for the
        first eager forward (`_prepack_deferred`)."""
        self._derived_checks = None
        if torch.compiler.is_compiling() or (self.codebooks.is_cuda and torch.cuda.is_current_stream_capturing()):
            self._prepack_deferred = True
            return
        self._prepack_deferred = False
        if self._packed_codes is not None:
            from .inference_kernels.hip_kernel import refresh_range

            refresh_range(self._packed_codes, self.codebooks)
        if self._fast is None:
            self._build_fast_lane()
        self._record_derived_checks()

    def _record_derived_checks(self) -> None:
        """Checksums of the parameters the derived state was just built from (see DERIVED_CHECK_EVERY)."""
        # staggered start: the modules of a model were all built at the same forward; without an offset every 256th decode step would
        # verify all of them at once (one multi-millisecond spike per 256 tokens instead of one module's ~40 us now and then)
        self._calls_since_check = (id(self) >> 4) % DERIVED_CHECK_EVERY if DERIVED_CHECK_EVERY else 0
        if not DERIVED_CHECK_EVERY or (self._packed_codes is None and self._cpu_codes_alt is None and self._dense is None
                                       and self._grad_index is None):
            return
        checks = {}
        if not self._codes_dropped:
            checks["codes"] = tensor_checksum(self.codes)
        if self._packed_codes is not None or self._dense is not None:
            checks["codebooks"] = tensor_checksum(self.codebooks)
        if self._dense is not None:
            checks["scales"] = tensor_checksum(self.scales)
        self._derived_checks = checks

    def verify_derived_state(self) -> bool:
        """Re-take the checksums of `_record_derived_checks` and compare; a mismatch (a parameter was overwritten behind the
        version counter's back) invalidates the derived state.  Returns whether everything still matched.  Synchronises."""
        checks = self._derived_checks
        if not checks:
            return True
        ok = all(tensor_checksum(getattr(self, name)) == value for name, value in checks.items())
        if not ok:
            self.invalidate_derived_state()
        return ok

    def forward(self, input: torch.Tensor) -> torch.Tensor:
        # (is_compiling() FIRST: Dynamo specialises int attributes of a module, so a counter touched while tracing installs a guard
        # `_calls_since_check == k` that fails on the next call and recompiles until the limit -- ADVICE r05)
        if not torch.compiler.is_compiling():
            if self._derived_checks is not None:
                n = self._calls_since_check + 1
                if n >= DERIVED_CHECK_EVERY > 0 and not (input.is_cuda and torch.cuda.is_current_stream_capturing()):
                    n = 0
                    self.verify_derived_state()
                self._calls_since_check = n
            elif self._prepack_deferred and not (input.is_cuda and torch.cuda.is_current_stream_capturing()):
                # the first eager forward after a transition inside a capture / trace: finish it (and the repack, if that waited too)
                if self._packed_codes is None:
                    self.prepare_matmul_op(input)
                else:
                    self._settle()
        if torch.is_grad_enabled() and (self.codebooks.requires_grad or self.scales.requires_grad
                                        or (self.bias is not None and self.bias.requires_grad)):
            # a parameter of this layer trains: none of the routes below (they read derived copies or skip autograd)
            return self._forward_trainable(input)
        group = self._shared_input_group
        if group is not None and group.applicable(input):
            return group.forward(self, input)  # one launch for all projections of this input (fusion.py)
        fast = self._fast
        if fast is not None and not torch.compiler.is_compiling():
            out = fast(input)  # None: not a call for the fast lane (rows, dtype, grad, a parameter changed) -> below
            if out is not None:
                return out
            if not fast.is_current():
                self.gemv_op = None  # a parameter was rebound / written in place: resolve everything again
        if self.gemv_op is None or (not torch.compiler.is_compiling() and self._derived_state_is_stale()):
            self.prepare_matmul_op(input)
        packed = self._packed_codes
        if (packed is not None and input.dtype == self.codebooks.dtype and input.is_cuda
                and math.prod(input.shape[:-1]) <= GEMV_MAX_ROWS and not (torch.is_grad_enabled() and input.requires_grad)):
            from .inference_kernels import hip_kernel

            if isinstance(packed, hip_kernel.PlanarCodes):
                # 8x8 on planar codes: the look-up-table matvec takes the gemv rule's 1..6 rows (2+: one launch of rows x the
                # single-row workgroups); anything else goes through the ordinary ops below.  8x8 g32 calls of
                # fused_8x8_min_rows(layer)+ rows (3 at 4096 x 4096) go to the ops too while the checkpoint-layout codes are there:
                # the fused MFMA kernel (aqlm_hip_gemm_8x8_mfma, round 5) costs the same for 3 rows as for 16.
                if input.numel() >= input.shape[-1] > 0 and not self._rows_take_the_fused_8x8_op(input):
                    if torch.compiler.is_compiling():  # traced: the dispatcher op (it has a fake implementation)
                        return torch.ops.aqlm.code8x8_matmat_planar(input, packed.buf, self.codebooks, self.scales, self.bias,
                                                                    [packed.out_features, packed.in_features, packed.in_group_size],
                                                                    packed.codebook_absmax)
                    return hip_kernel.code8x8_matmat_planar(input, packed, self.codebooks, self.scales, self.bias)
            elif (not torch.compiler.is_compiling() and torch.cuda.is_current_stream_capturing() and packed.desc.relabelled
                  and not self._codes_dropped and not packed.range_is_current(self.codebooks)):
                # a relabelled buffer's kernels read a derived codebook IMAGE; the codebook changed and the image cannot be rewritten
                # inside a capture (it reads a bound back): this call runs the direct kernel on the canonical codes and the live
                # codebook instead of raising; the first eager forward rewrites the image
                return self.gemv_op.apply(input, self.codes, self.codebooks, self.scales, self.bias)
            elif torch.compiler.is_compiling():  # traced: go through the dispatcher op (it has a fake implementation)
                return torch.ops.aqlm.code1x16_matmat_packed(input, packed.buf, self.codebooks, self.scales, self.bias,
                                                             packed.op_ints())
            else:
                return hip_kernel.code1x16_matmat_packed(input, packed, self.codebooks, self.scales, self.bias)
        if (self.prefer_dense_below_rows and input.is_cuda and GEMV_MAX_ROWS < math.prod(input.shape[:-1]) < self.prefer_dense_below_rows
                and input.dtype == self.codebooks.dtype and not (torch.is_grad_enabled() and input.requires_grad)
                and not torch.compiler.is_compiling()):
            return torch.nn.functional.linear(input, self._dense_weight(), self.bias)
        op = self.gemv_op if self.use_gemv_rule(input) else self.gemm_op
        if self._codes_dropped and self._serves_from_packed(input):
            grad_needed = torch.is_grad_enabled() and input.requires_grad
            route = dropped_layer_route(True, self._codes_drop_strict, self.rows_from_packed, math.prod(input.shape[:-1]),
                                        self.in_features % 64, grad_needed)
            if route == ROUTE_PACKED_DEQUANT:
                if not grad_needed:
                    return self._forward_from_packed(input)
                return _MatmulFromPacked.apply(input, self, self._forward_from_packed)
            if route == ROUTE_TRANSIENT_UNPACK and grad_needed:
                # the ordinary forward on codes unpacked for this call; nothing unpacked is kept for the backward
                kernel = op.forward_pass_kernel
                return _MatmulFromPacked.apply(input, self, lambda x: kernel(x, self._canonical_codes(), self.codebooks, self.scales, self.bias))
        return op.apply(input, self._codes_for_ops(), self.codebooks, self.scales, self.bias)

    def _takes_codebook_grad_kernel(self, input: Optional[torch.Tensor]) -> bool:
        """`tuning.takes_codebook_grad_kernel` for this layer and this input (None: any input in the parameters' dtype)."""
        from . import tuning

        cb, dt = self.codebooks, self.codebooks.dtype
        scheme = (self.num_codebooks == 1 and self.nbits_per_codebook == 16 and self.out_group_size == 1
                  and self.in_group_size in (8, 16))
        on_gpu = cb.is_cuda and self.scales.is_cuda and (input is None or input.is_cuda)
        dtypes_ok = (dt in (torch.float16, torch.bfloat16) and self.scales.dtype == dt
                     and (self.bias is None or self.bias.dtype == dt) and (input is None or input.dtype == dt))
        supported = False
        if scheme and on_gpu and tuning.CODEBOOK_GRAD_KERNEL:
            from .inference_kernels import hip_kernel

            supported = hip_kernel.codebook_grad_supported(self.out_features, self.in_features, self.in_group_size)
        return tuning.takes_codebook_grad_kernel(self.num_codebooks, self.nbits_per_codebook, self.out_group_size, self.in_group_size,
                                                 on_gpu, dtypes_ok, supported, torch.compiler.is_compiling())

    def _takes_codebook_grad_kernel_kx8(self, input: Optional[torch.Tensor]) -> bool:
        """`tuning.takes_codebook_grad_kernel_kx8` for this layer and this input (None: any input in the parameters' dtype)."""
        from . import tuning

        cb, dt = self.codebooks, self.codebooks.dtype
        scheme = (1 <= self.num_codebooks <= 8 and self.nbits_per_codebook == 8 and self.out_group_size == 1
                  and self.in_group_size in (8, 16, 32))
        on_gpu = cb.is_cuda and self.scales.is_cuda and (input is None or input.is_cuda)
        dtypes_ok = (dt in (torch.float16, torch.bfloat16) and self.scales.dtype == dt
                     and (self.bias is None or self.bias.dtype == dt) and (input is None or input.dtype == dt))
        supported = False
        if scheme and on_gpu and tuning.CODEBOOK_GRAD_KERNEL:
            from .inference_kernels import hip_kernel

            supported = hip_kernel.codebook_grad_kx8_supported(self.out_features, self.in_features, self.num_codebooks, self.in_group_size)
        return tuning.takes_codebook_grad_kernel_kx8(self.num_codebooks, self.nbits_per_codebook, self.out_group_size,
                                                     self.in_group_size, on_gpu, dtypes_ok, supported, torch.compiler.is_compiling())

    def codebook_grad_index(self):
        """The inverted index of this layer's codes (hip_kernel.CodebookGradIndex) that the codebook gradient is summed through:
        derived state like the packed codes -- keyed on ``codes_fingerprint(self.codes)``, forgotten by ``_reset_derived()`` /
        ``invalidate_derived_state()``, covered by the periodic checksum of the codes, never saved, copied or pickled.  It costs 4
        bytes per code (plus ~0.5 MB of tables) next to the 2 bytes of the codes themselves.  Built at the first training step, or
        by ``aqlm.tuning.prepare(model)``; never inside a hipGraph capture (the build sorts and allocates): there it must exist.
        A layer whose canonical codes were dropped (``prepack_model``) builds it from ``_canonical_codes()`` -- one transient
        unpack, which does not undo the drop.  The training calls themselves read the canonical codes (forward kernel, scale
        gradient): after a non-strict drop (``prepack_model``'s default) the first of them restores the codes for good, after a
        strict one every call unpacks them for its forward and keeps that copy until its backward has run."""
        fp = codes_fingerprint(self.codes)
        cached = self._grad_index
        if cached is not None and cached[0] == fp:
            return cached[1]
        if self.codebooks.is_cuda and torch.cuda.is_current_stream_capturing():
            raise RuntimeError("QuantizedLinear: a trainable layer needs the inverted index of its codes, and it cannot be built "
                               "inside a hipGraph capture; call aqlm.tuning.prepare(model) before capturing")
        from .inference_kernels import hip_kernel

        index = hip_kernel.build_codebook_grad_index(self._canonical_codes(), self.in_group_size)
        self._grad_index = (fp, index)
        if not torch.compiler.is_compiling():
            self._record_derived_checks()
        return index

    def _forward_trainable(self, input: torch.Tensor) -> torch.Tensor:
        """A call that must produce gradients for codebooks / scales / bias (module docstring of aqlm_amd/tuning.py)."""
        if self._takes_codebook_grad_kernel(input):
            index = self.codebook_grad_index()  # (first: inside a capture a missing index raises before any launch)
            return _TrainableMatmul1x16.apply(input, self.codebooks, self.scales, self.bias, self._codes_for_ops(), index)
        if self._takes_codebook_grad_kernel_kx8(input):
            # no index: the canonical codes are all the route reads (dropped planar 8x8 codes follow the rules of
            # `codebook_grad_index`'s docstring: restored for good after a non-strict drop, unpacked per call after a strict one)
            return _TrainableMatmulKx8.apply(input, self.codebooks, self.scales, self.bias, self._codes_for_ops())
        from .utils import _dequantize_weight

        # the reference's definition under autograd; the arithmetic on the codes outside inference mode (`unpack_int_data` runs
        # inside it, and its result could not be saved for the backward)
        with torch.inference_mode(False):
            unsigned = self._codes_for_ops().detach().to(torch.int64) % self.codebook_size
        return torch.nn.functional.linear(input, _dequantize_weight(unsigned, self.codebooks, self.scales), self.bias)

    def _serves_from_packed(self, input: torch.Tensor) -> bool:
        """A call the packed-dequant routes can take: a 1x16 layer on slice-bucketed codes, input on the GPU in the codebook dtype."""
        from .inference_kernels import hip_kernel

        return (isinstance(self._packed_codes, hip_kernel.PackedCodes) and input.is_cuda and input.dtype == self.codebooks.dtype
                and self.scales.dtype == self.codebooks.dtype)

    def _weight_from_packed(self, scaled: bool) -> torch.Tensor:
        """W [out, in] straight from the packed buffer and the live codebook (aqlm_hip_dequant_1x16_packed): the bits of the dequant
        kernel on the unpacked codes, without unpacking."""
        from .inference_kernels import hip_kernel

        packed, scales = self._packed_codes, (self.scales if scaled else None)
        if torch.compiler.is_compiling():  # traced: the dispatcher op (it has a fake implementation)
            return torch.ops.aqlm.code1x16_dequant_packed(packed.buf, self.codebooks, scales, packed.op_ints())
        return hip_kernel.dequant_1x16_packed(packed, self.codebooks, scales)

    def _forward_from_packed(self, input: torch.Tensor) -> torch.Tensor:
        """The large-batch op's dequant route (hip_kernel.code1x16_matmat_dequant above FUSED_MFMA_MAX_ROWS) with W taken from the
        packed buffer: unscaled W (exact in the storage dtype), one library GEMM, scale + bias in fp32 with one rounding."""
        from .inference_kernels import hip_kernel

        if input.shape[-1] != self.in_features:
            raise ValueError(f"input has {input.shape[-1]} features, layer expects {self.in_features}")
        x = hip_kernel._flat_rows(input)
        y = torch.nn.functional.linear(x, self._weight_from_packed(scaled=False))
        return hip_kernel._scale_bias_fp32(y, self.scales, self.bias).reshape(input.shape[:-1] + (self.out_features,))

    def _rows_take_the_fused_8x8_op(self, input: torch.Tensor) -> bool:
        from .inference_kernels import hip_kernel

        return (hip_kernel.USE_FUSED_8X8_MFMA and not self._codes_dropped and self.in_group_size == 32 and self.in_features % 256 == 0
                and self.in_features >= 2048
                and math.prod(input.shape[:-1]) >= hip_kernel.fused_8x8_min_rows(self.out_features, self.in_features)
                and not torch.compiler.is_compiling())

    def _dense_weight(self) -> torch.Tensor:
        """W in the storage dtype, dequantised once and kept while codes / codebooks / scales are what they were (identity +
        version, and the periodic checksum of DERIVED_CHECK_EVERY for writes through ``.data``).  The scales are folded into W
        BEFORE it is rounded to fp16 / bf16 -- one more rounding per weight than the reference's large-batch path, which
        dequantises unscaled and scales y after the GEMM (cuda_kernel.cpp:249-301, 294-300), and than the fused ops here
        (fp32 accumulate, scale, one rounding); the price of running the opt-in dense route as ONE library GEMM with the bias
        fused."""
        fp = (codes_fingerprint(self.codes), self.codebooks.data_ptr(), tensor_version(self.codebooks), self.scales.data_ptr(),
              tensor_version(self.scales))
        if self._dense is None or self._dense[0] != fp:
            from .utils import _dequantize_weight, unpack_int_data

            with torch.no_grad():
                if self._codes_dropped and self._serves_from_packed(self.codebooks):
                    w = self._weight_from_packed(scaled=True)  # the same bits (codebook entry x scale, one rounding) without an unpack
                else:
                    w = _dequantize_weight(unpack_int_data(self._canonical_codes(), self.nbits_per_codebook), self.codebooks, self.scales)
            self._dense = (fp, w.to(self.codebooks.dtype).contiguous())
            self._settle()
        return self._dense[1]

    def _derived_state_is_stale(self) -> bool:
        """The prepacked buffer is derived from ``codes``: rebuild it when ``codes`` was written in place
        (``load_state_dict`` / ``copy_`` after the first forward), rebound (``module.codes = ...``, accelerate's
        ``set_module_tensor_to_device``) or when a repack was postponed during graph capture."""
        if self._codes_dropped:
            return False
        if self._packed_codes is None and self._cpu_codes_alt is None:
            return self._prepack_deferred and not torch.cuda.is_current_stream_capturing()
        return codes_fingerprint(self.codes) != self._packed_fingerprint

    def _canonical_codes(self) -> torch.Tensor:
        """``codes`` in the checkpoint layout; rebuilt from the prepacked buffer (lossless) when they were dropped."""
        if not self._codes_dropped:
            return self.codes
        return self._packed_codes.unpack()  # lossless inverse of the load-time re-layout (1x16 slices / 8x8 planes)

    def _codes_for_ops(self) -> torch.Tensor:
        """The canonical codes for an op that reads them (> 6 rows, backward, a call the packed kernel does not take).  Dropped and not
        `strict`: this module turns out to be used that way -- the codes come back for good (one unpack, 32 us for a 4096 x 4096
        layer, instead of one per call: `detail.unpack_1x16_us` puts a transient unpack at 2.4-2.9 x the 16-row op it would precede).
        Never inside a hipGraph capture or a trace (the restored parameter would belong to the capture): those calls unpack
        transiently."""
        if (self._codes_dropped and not self._codes_drop_strict and not torch.compiler.is_compiling()
                and not (self.codebooks.is_cuda and torch.cuda.is_current_stream_capturing())):
            self.restore_canonical_codes()
        return self._canonical_codes()

    def drop_canonical_codes(self, strict: bool = True) -> bool:
        """Inference-only memory saver: free ``codes`` of a prepacked layer (the packed buffer holds the same
        information; ``state_dict()`` and the large-batch / backward ops rebuild them on demand).  ``strict=False``: the first
        forward that needs them restores them for good (decode-only deployments keep one copy, a model that is also called with 7+
        rows pays one unpack per layer and ends up with both).  Returns whether anything was freed."""
        if self._packed_codes is None or self._codes_dropped:
            return False
        self._codes_drop_strict = bool(strict)
        self._codes_shape = tuple(self.codes.shape)
        self.codes = nn.Parameter(torch.empty((0,), dtype=self.codes.dtype, device=self.codes.device), requires_grad=False)
        self._codes_dropped = True
        self._fast = None  # the lane watched the codes it no longer reads
        self._settle()
        return True

    def restore_canonical_codes(self) -> None:
        if self._codes_dropped:
            codes = self._canonical_codes()
            self._codes_dropped = False
            self.codes = nn.Parameter(codes, requires_grad=False)
            self._packed_fingerprint = codes_fingerprint(self.codes)
            self._fast = None
            self._settle()

    def _save_to_state_dict(self, destination, prefix, keep_vars):
        super()._save_to_state_dict(destination, prefix, keep_vars)
        if self._codes_dropped:  # checkpoints always carry the reference layout
            destination[prefix + "codes"] = self._canonical_codes()

    def _load_from_state_dict(self, state_dict, prefix, *args, **kwargs):
        if self._codes_dropped and prefix + "codes" in state_dict:  # new codes arrive: give them a parameter to land in
            self._codes_dropped = False
            self._reset_derived()
            self.codes = nn.Parameter(torch.empty(self._codes_shape, dtype=self.codes.dtype, device=self.codes.device),
                                      requires_grad=False)
        super()._load_from_state_dict(state_dict, prefix, *args, **kwargs)

    def _apply(self, fn, *args, **kwargs):
        """``.to()`` / ``.half()`` / ``.cuda()`` replace the parameters: drop everything derived from them (kernel
        choice, prepacked codes); it is rebuilt at the next forward."""
        self.restore_canonical_codes()  # the derived buffer does not survive a conversion; the codes must
        out = super()._apply(fn, *args, **kwargs)
        self._reset_derived()
        return out

    def prepare_matmul_op(self, input: torch.Tensor):
        """Resolve the decode (gemv) and batch (gemm) operators once (reference inference.py:77-96).  For host modules
        with 8-bit codebooks the reference permutes ``codes`` IN PLACE to the LUT kernel's layout (inference.py:78-83,
        "TODO: fix this thing"); here the permuted copy is a derived buffer and ``codes`` keeps the checkpoint layout.  Then the
        packed copy of the codes (``_repack``) and the settle step."""
        from .inference_kernels.kernel_selector import cpu_kernel_takes_permuted_codes

        self._fast = None
        self._cpu_codes_alt = None
        if cpu_kernel_takes_permuted_codes(self.codebooks):
            from .inference_kernels.cpu_kernel import permute_codes_for_lut

            self._cpu_codes_alt = permute_codes_for_lut(self.codes)
            self._packed_fingerprint = codes_fingerprint(self.codes)
        fwd_gemv, fwd_gemm = get_forward_pass_kernel(self.codebooks, False), get_forward_pass_kernel(self.codebooks, True)
        if self._cpu_codes_alt is not None:
            # the LUT kernel reads the permuted copy; the op still receives (and saves for backward) the canonical codes
            alt, lut_gemv, lut_gemm = self._cpu_codes_alt, fwd_gemv, fwd_gemm
            fwd_gemv = lambda input, codes, codebooks, scales, bias: lut_gemv(input, alt, codebooks, scales, bias)  # noqa: E731
            fwd_gemm = lambda input, codes, codebooks, scales, bias: lut_gemm(input, alt, codebooks, scales, bias)  # noqa: E731
        self.gemv_op = _get_autograd_matmul_op(fwd_gemv, get_backward_pass_kernel(self.codebooks, False))
        self.gemm_op = _get_autograd_matmul_op(fwd_gemm, get_backward_pass_kernel(self.codebooks, True))
        self.use_gemv_rule = lambda x: math.prod(x.shape[:-1]) <= GEMV_MAX_ROWS
        # load-time re-layout of the codes for the decode kernel (the reference does the analogous thing for its CPU
        # kernel here, inference.py:78-83 -- but in place; we keep `codes` untouched and add a derived buffer)
        if not self._codes_dropped:  # (dropped: the packed buffer IS the weights now)
            self._repack()
        self._settle()

    def _repack(self) -> None:
        """The prepacked / planar copy of ``codes`` for the decode kernels, when the layer takes one."""
        self._packed_codes = None
        if (PREPACK_MIN_CODES and self.out_features * (self.in_features // self.in_group_size) >= PREPACK_MIN_CODES
                and self.num_codebooks == 1 and self.nbits_per_codebook == 16 and self.in_group_size in (8, 16) and self.out_group_size == 1
                and self.codes.is_cuda and self.codebooks.dtype in (torch.float16, torch.bfloat16)):
            if torch.cuda.is_current_stream_capturing():
                # the repack synchronises its stream: not allowed inside a hipGraph capture.  This call runs on the
                # direct kernel; the repack happens at the first forward outside a capture (with the deferred settle step).
                return
            from .inference_kernels import hip_kernel

            self._packed_codes = hip_kernel.prepack_1x16(self.codes, self.in_group_size, codebooks=self.codebooks)
            self._packed_fingerprint = codes_fingerprint(self.codes)
        elif (PREPACK_MIN_CODES and self.out_features * (self.in_features // self.in_group_size) * 8 >= PREPACK_MIN_CODES
                and self.num_codebooks == 8 and self.nbits_per_codebook == 8 and self.in_group_size in (8, 16, 32) and self.out_group_size == 1
                and self.codes.is_cuda and self.codebooks.dtype in (torch.float16, torch.bfloat16)):
            # 8 x 8-bit schemes: planar copy of the codes for the look-up-table matvec (same size as `codes`, lossless)
            if torch.cuda.is_current_stream_capturing():
                return  # the codebook bound is a host read-back: first forward outside a capture
            from .inference_kernels import hip_kernel

            self._packed_codes = hip_kernel.planar_8x8_pack(self.codes, self.in_group_size, codebooks=self.codebooks)
            self._packed_fingerprint = codes_fingerprint(self.codes)

    def _build_fast_lane(self) -> None:
        """The compiled fast lane of decode calls (<= GEMV_MAX_ROWS rows, no grad): flatten / allocate / launch without the
        interpreter.  Same kernels and same results as the ops the selector returned; it watches the parameters and hands
        any call it does not recognise back to the Python path (aqlm_amd/csrc_front/front.cpp)."""
        self._fast = None
        from . import _front

        if (not _front.available() or not self.codebooks.is_cuda or self.out_group_size != 1
                or self.codebooks.dtype not in (torch.float16, torch.bfloat16) or self.scales.dtype != self.codebooks.dtype
                or (self.bias is not None and self.bias.dtype != self.codebooks.dtype)
                or not (self.codebooks.is_contiguous() and self.scales.is_contiguous())):
            return
        from .inference_kernels import hip_kernel

        packed = self._packed_codes
        scheme = (self.num_codebooks, self.nbits_per_codebook, self.in_group_size)
        if isinstance(packed, hip_kernel.PlanarCodes):
            if not (hip_kernel.USE_8X8_LUT and hip_kernel.USE_8X8_LUT_FUSED and packed.codebook_absmax > 0.0 and packed.range_is_current(self.codebooks)):
                return  # two-kernel form (needs a workspace): Python path
            import struct

            kind, buf, desc = _front.KIND_LUT_PLANAR_8X8, packed.buf, struct.pack("<f", packed.codebook_absmax)
        elif packed is not None:
            if not (hip_kernel.FUSED_FINALIZE and packed.desc.codebook_absmax > 0.0 and packed.range_is_current(self.codebooks)):
                return  # two-kernel finalize (needs a workspace): Python path
            kind, buf, desc = _front.KIND_PACKED_1X16, packed.buf, bytes(packed.desc)
        elif self._codes_dropped or not (self.codes.is_cuda and self.codes.is_contiguous()):
            return
        elif scheme in ((1, 16, 8), (1, 16, 16)):
            if hip_kernel.RAW_OP_PREPACK and self.out_features * (self.in_features // self.in_group_size) >= hip_kernel.RAW_OP_PREPACK_MIN_CODES:
                return  # the raw op would pack this layer on its own (PREPACK_MIN_CODES was raised): leave it to the op
            kind, buf, desc = _front.KIND_GEMV_1X16, None, ""
        elif scheme in ((2, 8, 8), (1, 8, 8)):
            kind, buf, desc = _front.KIND_GEMV_KX8, None, ""
        else:
            return
        fused_from = 0
        if (kind == _front.KIND_LUT_PLANAR_8X8 and hip_kernel.USE_FUSED_8X8_MFMA and not self._codes_dropped and self.in_group_size == 32
                and self.in_features % 256 == 0 and self.in_features >= 2048 and self.codes.is_cuda and self.codes.is_contiguous()):
            # more rows: the lane launches the fused MFMA op on the checkpoint-layout codes (what forward would do through the ops)
            fused_from = hip_kernel.fused_8x8_min_rows(self.out_features, self.in_features)
        try:
            self._fast = _front.ext.FastLinear(self._parameters, kind, buf, desc, self.in_features, self.out_features,
                                               self.num_codebooks, self.in_group_size, not self._codes_dropped, GEMV_MAX_ROWS, fused_from)
        except RuntimeError:
            self._fast = None


def _get_autograd_matmul_op(forward_pass_kernel, backward_pass_kernel):
    """autograd.Function around a (forward, backward) kernel pair (reference inference.py:99-142): gradient flows
    to ``input`` only; codes / codebooks / scales / bias are frozen."""

    class _QuantizedMatmul(torch.autograd.Function):
        @staticmethod
        def forward(ctx, input, codes, codebooks, scales, bias: Optional[torch.Tensor]):
            ctx.save_for_backward(codes, codebooks, scales)
            return forward_pass_kernel(input, codes, codebooks, scales, bias)

        @staticmethod
        def backward(ctx, grad_output):
            codes, codebooks, scales = ctx.saved_tensors
            grad_input = backward_pass_kernel(grad_output.contiguous(), codes, codebooks, scales, None)
            return grad_input, None, None, None, None

    _QuantizedMatmul.forward_pass_kernel = staticmethod(forward_pass_kernel)
    return _QuantizedMatmul


class _TrainableMatmul1x16(torch.autograd.Function):
    """A 1x16 layer on the GPU with trainable codebooks / scales / bias.  Forward: the kernel the frozen layer runs for that row
    count on the canonical codes and the live parameters (the direct matvec up to GEMV_MAX_ROWS rows, the large-batch op above).
    Backward, in this order: grad_input by the frozen layer's backward kernel (only if needed; its W is released before the next
    step, so the two [out, in] transients never coexist), dbias, ``dW = grad_y^T @ x`` by the library GEMM (storage dtype, as the
    reference's autograd produces it; fp32 with ``tuning.CODEBOOK_GRAD_FP32_DW``), then the two reductions of dW
    (aqlm_hip_codebook_grad_1x16 through the inverted index, aqlm_hip_scales_grad_1x16).  Gradients in each parameter's dtype."""

    @staticmethod
    def forward(ctx, input, codebooks, scales, bias, codes, index):
        from .inference_kernels import hip_kernel

        ctx.save_for_backward(input, codes, codebooks, scales)
        ctx.index = index
        ctx.bias_dtype = None if bias is None else bias.dtype
        if math.prod(input.shape[:-1]) <= GEMV_MAX_ROWS:
            return hip_kernel._gemv(input, codes, codebooks, scales, bias, "1x16")
        return hip_kernel.code1x16_matmat_dequant(input, codes, codebooks, scales, bias)

    @staticmethod
    def backward(ctx, grad_output):
        from . import tuning
        from .inference_kernels import hip_kernel

        input, codes, codebooks, scales = ctx.saved_tensors
        grad_output = grad_output.contiguous()
        need_input, need_codebooks, need_scales, need_bias = ctx.needs_input_grad[:4]
        grad_input = grad_codebooks = grad_scales = grad_bias = None
        if need_input:
            grad_input = torch.ops.aqlm.code1x16_matmat_dequant_transposed(grad_output, codes, codebooks, scales, None)
        gy = grad_output.reshape(-1, grad_output.shape[-1])
        if need_bias and ctx.bias_dtype is not None:
            grad_bias = gy.sum(0, dtype=torch.float32).to(ctx.bias_dtype)
        if need_codebooks or need_scales:
            x = input.reshape(-1, input.shape[-1])
            if tuning.CODEBOOK_GRAD_FP32_DW:
                dw = torch.mm(gy.t(), x, out_dtype=torch.float32)
            else:
                dw = torch.mm(gy.t(), x)
            if need_codebooks:
                grad_codebooks = hip_kernel.codebook_grad_1x16(dw, scales, ctx.index, out_dtype=codebooks.dtype).reshape(codebooks.shape)
            if need_scales:
                grad_scales = hip_kernel.scales_grad_1x16(dw, codes, codebooks, out_dtype=scales.dtype).reshape(scales.shape)
        return grad_input, grad_codebooks, grad_scales, grad_bias, None, None


class _TrainableMatmulKx8(torch.autograd.Function):
    """A K x 8 layer (1 to 8 codebooks of 256 entries, g 8 / 16 / 32) on the GPU with trainable codebooks / scales / bias.  Forward:
    the kernel the frozen layer runs for that row count on the canonical codes and the live parameters.  Backward, in the order of
    `_TrainableMatmul1x16`: grad_input by the frozen layer's backward kernel (only if needed), dbias, ``dW = grad_y^T @ x`` by the
    library GEMM (fp32 with ``tuning.CODEBOOK_GRAD_FP32_DW``), then aqlm_hip_codebook_grad_kx8 (fixed-point sums in LDS, no index)
    and aqlm_hip_scales_grad_kx8.  Gradients in each parameter's dtype."""

    @staticmethod
    def forward(ctx, input, codebooks, scales, bias, codes):
        from .inference_kernels import get_forward_pass_kernel

        ctx.save_for_backward(input, codes, codebooks, scales)
        ctx.bias_dtype = None if bias is None else bias.dtype
        return get_forward_pass_kernel(codebooks, math.prod(input.shape[:-1]) > GEMV_MAX_ROWS)(input, codes, codebooks, scales, bias)

    @staticmethod
    def backward(ctx, grad_output):
        from . import tuning
        from .inference_kernels import get_backward_pass_kernel, hip_kernel

        input, codes, codebooks, scales = ctx.saved_tensors
        grad_output = grad_output.contiguous()
        need_input, need_codebooks, need_scales, need_bias = ctx.needs_input_grad[:4]
        grad_input = grad_codebooks = grad_scales = grad_bias = None
        if need_input:
            rows = math.prod(grad_output.shape[:-1])
            grad_input = get_backward_pass_kernel(codebooks, rows > GEMV_MAX_ROWS)(grad_output, codes, codebooks, scales, None)
        gy = grad_output.reshape(-1, grad_output.shape[-1])
        if need_bias and ctx.bias_dtype is not None:
            grad_bias = gy.sum(0, dtype=torch.float32).to(ctx.bias_dtype)
        if need_codebooks or need_scales:
            x = input.reshape(-1, input.shape[-1])
            if tuning.CODEBOOK_GRAD_FP32_DW:
                dw = torch.mm(gy.t(), x, out_dtype=torch.float32)
            else:
                dw = torch.mm(gy.t(), x)
            if need_codebooks:
                grad_codebooks = hip_kernel.codebook_grad_kx8(dw, scales, codes, int(codebooks.shape[3]),
                                                              out_dtype=codebooks.dtype).reshape(codebooks.shape)
            if need_scales:
                grad_scales = hip_kernel.scales_grad_kx8(dw, codes, codebooks, out_dtype=scales.dtype).reshape(scales.shape)
        return grad_input, grad_codebooks, grad_scales, grad_bias, None


class _MatmulFromPacked(torch.autograd.Function):
    """A forward of a layer whose canonical codes were dropped, with a gradient for its input: ``forward_fn(input)`` is the
    forward, and the backward is the ordinary one -- grad_input = grad_output @ W with the scales folded into W
    (hip_kernel._matmat_dequant_transposed) -- on a W dequantised straight from the packed buffer.  Nothing unpacked lives between
    the two; the packed buffer (which IS the weights) and the codebooks / scales the forward used are what the backward reads."""

    @staticmethod
    def forward(ctx, input, layer, forward_fn):
        ctx.packed = layer._packed_codes
        ctx.save_for_backward(layer.codebooks, layer.scales)
        return forward_fn(input)

    @staticmethod
    def backward(ctx, grad_output):
        from .inference_kernels import hip_kernel

        codebooks, scales = ctx.saved_tensors
        W = hip_kernel.dequant_1x16_packed(ctx.packed, codebooks, scales)
        return torch.matmul(grad_output.contiguous(), W), None, None
