"""Calibrated training of codebooks and scales, the parts that need no GPU: the C ABI of the aqlm_hip_calib_* entries (symbols, the
support and workspace queries, the argument checks on host buffers in their documented order -- nothing is launched), the route
predicate as a truth table, the torch route of ``aqlm.tuning.calibrated_loss_and_grads`` against autograd of the restated
``_compute_mse`` (fp32: bit for bit; fp64: within fp32 rounding), ``accumulate_xtx_`` against the reference's formula, and
``quantize_layer_`` end to end on a 64 -> 64 1x8 g8 host layer (512 groups for 256 centroids)."""
import copy
import ctypes
import itertools
import math
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("aqlm_hip_calib_delta_supported", "aqlm_hip_calib_delta", "aqlm_hip_calib_rows_supported", "aqlm_hip_calib_rows",
       "aqlm_hip_calib_codebook_grad_1x16_supported", "aqlm_hip_calib_codebook_grad_1x16_workspace_bytes", "aqlm_hip_calib_codebook_grad_1x16",
       "aqlm_hip_calib_codebook_grad_kx8_supported", "aqlm_hip_calib_codebook_grad_kx8_workspace_bytes", "aqlm_hip_calib_codebook_grad_kx8")


# ---------------------------------------------------------------------------------------------------------------------------
# 1. symbols and queries
# ---------------------------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_bound_and_exported_and_the_abi_version_stays():
    from aqlm_amd import _native as nat

    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "aqlm_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(aqlm_hip_[a-z0-9_]+)\s*\(", text))
    raw = ctypes.CDLL(nat.LIB_PATH)
    for name in NEW:
        assert name in declared and name in nat.SIGNATURES and hasattr(raw, name), name
    assert nat.lib.aqlm_hip_abi_version() == nat.ABI_VERSION == 9
    from aqlm_amd import tuning
    from aqlm_amd.inference_kernels import hip_kernel

    for fn in ("calib_supported", "calib_delta", "calib_rows", "calib_codebook_grad_1x16", "calib_codebook_grad_kx8"):
        assert callable(getattr(hip_kernel, fn))
    for fn in ("calibrated_loss_and_grads", "takes_calibrated_grad_kernel", "accumulate_xtx_", "quantize_layer_"):
        assert callable(getattr(tuning, fn))
    assert tuning.CALIBRATED_GRAD_KERNEL is True
    assert "calib_grad.hip" in open(os.path.join(ROOT, "aqlm_amd", "csrc", "Makefile")).read()


def test_supported_and_workspace_queries():
    from aqlm_amd import _native as nat
    from aqlm_amd.inference_kernels import hip_kernel as hk

    lib = nat.lib
    for fn in (lib.aqlm_hip_calib_delta_supported, lib.aqlm_hip_calib_rows_supported):
        for good in ((4096, 4096, 1, 16, 8), (48, 1120, 1, 16, 16), (80, 560, 1, 8, 8), (4096, 4096, 8, 8, 32), (1, 8, 2, 8, 8), (7, 64, 5, 8, 16)):
            assert fn(*good) == 1, good
        for bad in ((48, 560, 1, 16, 32), (48, 560, 2, 16, 8), (80, 560, 9, 8, 8), (80, 560, 0, 8, 8), (80, 561, 2, 8, 8), (80, 560, 2, 8, 4),
                    (0, 560, 2, 8, 8), (80, 560, 2, 4, 8), (80, 560, 1, 12, 8), (1 << 20, 1 << 16, 2, 8, 8)):
            assert fn(*bad) == 0, bad
    # the codebook gradients answer, and need, what their training siblings do
    for o, i, g in ((48, 560, 8), (4096, 4096, 16), (48, 560, 32), (0, 8, 8)):
        assert lib.aqlm_hip_calib_codebook_grad_1x16_supported(o, i, g) == lib.aqlm_hip_codebook_grad_1x16_supported(o, i, g)
        assert lib.aqlm_hip_calib_codebook_grad_1x16_workspace_bytes(o, i, g) == lib.aqlm_hip_codebook_grad_1x16_workspace_bytes(o, i, g)
    for o, i, K, g in ((80, 560, 2, 8), (4096, 4096, 8, 32), (80, 560, 9, 8), (80, 560, 2, 4)):
        assert lib.aqlm_hip_calib_codebook_grad_kx8_supported(o, i, K, g) == lib.aqlm_hip_codebook_grad_kx8_supported(o, i, K, g)
        assert lib.aqlm_hip_calib_codebook_grad_kx8_workspace_bytes(o, i, K, g) == lib.aqlm_hip_codebook_grad_kx8_workspace_bytes(o, i, K, g)
    assert lib.aqlm_hip_calib_codebook_grad_kx8_workspace_bytes(4096, 4096, 2, 8) > 0
    assert hk.calib_supported(4096, 4096, 1, 16, 8) and hk.calib_supported(4096, 4096, 8, 8, 32)
    assert not hk.calib_supported(4096, 4096, 1, 16, 32) and not hk.calib_supported(4096, 4096, 2, 16, 8)


# ---------------------------------------------------------------------------------------------------------------------------
# 2. the predicate, and the argument checks on dummy host pointers: every call returns before the device is touched
# ---------------------------------------------------------------------------------------------------------------------------
def test_predicate_truth_table():
    from aqlm_amd import tuning

    for K, nbits, ogs, g, on_gpu, dtypes_ok, supported in itertools.product((0, 1, 2, 8, 9), (8, 16, 12), (1, 2), (4, 8, 16, 32), (False, True),
                                                                            (False, True), (False, True)):
        scheme = (nbits == 16 and K == 1 and g in (8, 16)) or (nbits == 8 and 1 <= K <= 8 and g in (8, 16, 32))
        want = scheme and ogs == 1 and on_gpu and dtypes_ok and supported
        assert tuning.takes_calibrated_grad_kernel(K, nbits, ogs, g, on_gpu, dtypes_ok, supported) is want, (K, nbits, ogs, g)
    tuning.CALIBRATED_GRAD_KERNEL = False
    try:
        assert tuning.takes_calibrated_grad_kernel(1, 16, 1, 8, True, True, True) is False
        assert tuning.takes_calibrated_grad_kernel(2, 8, 1, 8, True, True, True) is False
    finally:
        tuning.CALIBRATED_GRAD_KERNEL = True
    # host tensors never reach the library
    codes = torch.zeros((8, 4, 2), dtype=torch.int8)
    assert not tuning._calibrated_grad_route(codes, torch.zeros((2, 256, 1, 8)), torch.ones((8, 1, 1, 1)), torch.zeros((8, 32)), torch.eye(32))


def _buffer():
    buf = ctypes.create_string_buffer(1 << 16)
    return buf, (ctypes.addressof(buf) + 15) // 16 * 16


def test_delta_and_rows_checks_report_the_documented_codes_in_the_documented_order():
    from aqlm_amd import _native as nat

    buf, p = _buffer()
    delta = lambda **kw: nat.lib.aqlm_hip_calib_delta(*[kw.get(n, d) for n, d in (  # noqa: E731
        ("codes", p + 2), ("books", p + 4096), ("scales", p + 8192 + 4), ("ref", p + 12288 + 2), ("ref_dt", nat.F16), ("ref_stride", 563),
        ("out", 48), ("fin", 560), ("K", 1), ("nbits", 16), ("g", 8), ("d", p + 16384), ("d_stride", 564), ("stream", None))])
    rows = lambda **kw: nat.lib.aqlm_hip_calib_rows(*[kw.get(n, d) for n, d in (  # noqa: E731
        ("gm", p), ("g_stride", 564), ("d", p + 16384), ("d_stride", 560), ("codes", p + 2), ("books", p + 4096), ("out", 48), ("fin", 560),
        ("K", 1), ("nbits", 16), ("g", 8), ("ds", p + 20480 + 4), ("rl", p + 24576 + 4), ("stream", None))])
    for call, pointers in ((delta, ("codes", "books", "scales", "ref", "d")), (rows, ("gm", "d", "codes", "books", "ds", "rl"))):
        for null in pointers:
            assert call(**{null: None}) == nat.E_INVALID and "null pointer" in nat.last_error(), null
        assert call(**{pointers[0]: None, "fin": 0, "g": 5}) == nat.E_INVALID and "null pointer" in nat.last_error(), "null pointers come first"
    for name, addr in (("codes", p + 1), ("books", p + 4096 + 8), ("scales", p + 8192 + 2), ("ref", p + 12288 + 1), ("d", p + 16384 + 4)):
        assert delta(**{name: addr}) == nat.E_INVALID and "misaligned" in nat.last_error(), name
    assert delta(ref=p + 12288 + 2, ref_dt=nat.F32) == nat.E_INVALID and "misaligned" in nat.last_error(), "an fp32 target is aligned to 4 bytes"
    for name, addr in (("gm", p + 8), ("d", p + 16384 + 4), ("codes", p + 1), ("books", p + 4096 + 4), ("ds", p + 20480 + 2), ("rl", p + 24576 + 2)):
        assert rows(**{name: addr}) == nat.E_INVALID and "misaligned" in nat.last_error(), name
    for call in (delta, rows):
        assert call(d=p + 16384 + 4, fin=0) == nat.E_INVALID and "misaligned" in nat.last_error(), "alignment comes before the sizes"
        for bad in ({"out": 0}, {"fin": 0}, {"g": 0}, {"fin": 562}, {"out": -3}):
            assert call(**bad) == nat.E_INVALID and "bad sizes" in nat.last_error(), bad
        assert call(d_stride=559) == nat.E_INVALID and "row stride" in nat.last_error()
        assert call(d_stride=559, nbits=12) == nat.E_INVALID, "the strides come before the scheme"
        for bad in ({"nbits": 12}, {"nbits": 4}, {"K": 2}, {"K": 0}, {"nbits": 8, "K": 9}, {"nbits": 8, "K": 0}, {"g": 4},
                    {"g": 32, "fin": 576, "d_stride": 576, "g_stride": 576, "ref_stride": 576}, {"g": 40, "nbits": 8, "K": 2}):
            assert call(**bad) == nat.E_UNSUPPORTED, bad
        assert call(d_stride=562) == nat.E_UNSUPPORTED and "16-byte aligned" in nat.last_error(), "odd fp32 row strides"
    assert delta(ref_stride=559) == nat.E_INVALID and "row stride" in nat.last_error()
    assert rows(g_stride=559) == nat.E_INVALID and "row stride" in nat.last_error()
    assert rows(g_stride=561) == nat.E_UNSUPPORTED and "16-byte aligned" in nat.last_error()
    assert delta(ref_dt=7) == nat.E_UNSUPPORTED and "W_ref is float16, bfloat16 or float32" in nat.last_error()
    assert delta(ref_dt=7, nbits=12) == nat.E_UNSUPPORTED and "W_ref" in nat.last_error(), "the dtype comes before the scheme"
    del buf


def test_codebook_gradient_checks_report_the_documented_codes_in_the_documented_order():
    from aqlm_amd import _native as nat

    buf, p = _buffer()
    need16 = nat.lib.aqlm_hip_calib_codebook_grad_1x16_workspace_bytes(48, 560, 8)
    need8 = nat.lib.aqlm_hip_calib_codebook_grad_kx8_workspace_bytes(80, 560, 2, 8)
    wide = lambda **kw: nat.lib.aqlm_hip_calib_codebook_grad_1x16(*[kw.get(n, d) for n, d in (  # noqa: E731
        ("gm", p), ("g_stride", 564), ("scales", p + 4096 + 4), ("starts", p + 8192 + 4), ("order", p + 12288 + 4), ("chunks", p + 16384 + 4),
        ("chunk_starts", p + 20480 + 4), ("out", 48), ("fin", 560), ("g", 8), ("dc", p + 24576), ("ws", p + 28672), ("ws_bytes", need16),
        ("stream", None))])
    narrow = lambda **kw: nat.lib.aqlm_hip_calib_codebook_grad_kx8(*[kw.get(n, d) for n, d in (  # noqa: E731
        ("gm", p), ("g_stride", 564), ("scales", p + 4096 + 4), ("codes", p + 8192 + 1), ("out", 80), ("fin", 560), ("K", 2), ("g", 8),
        ("dc", p + 24576), ("ws", p + 28672), ("ws_bytes", need8), ("stream", None))])
    for call, pointers in ((wide, ("gm", "scales", "starts", "order", "chunks", "chunk_starts", "dc", "ws")),
                           (narrow, ("gm", "scales", "codes", "dc", "ws"))):
        for null in pointers:
            assert call(**{null: None}) == nat.E_INVALID and "null pointer" in nat.last_error(), null
        assert call(gm=None, fin=0) == nat.E_INVALID and "null pointer" in nat.last_error(), "null pointers come first"
        for name, addr in (("gm", p + 8), ("scales", p + 4096 + 2), ("dc", p + 24576 + 8), ("ws", p + 28672 + 4)):
            assert call(**{name: addr}) == nat.E_INVALID and "misaligned" in nat.last_error(), name
        assert call(gm=p + 8, fin=0) == nat.E_INVALID and "misaligned" in nat.last_error(), "alignment comes before the sizes"
        for bad in ({"out": 0}, {"fin": 0}, {"g": 0}, {"fin": 562}):
            assert call(**bad) == nat.E_INVALID and "bad sizes" in nat.last_error(), bad
        assert call(g_stride=559) == nat.E_INVALID and "row stride" in nat.last_error()
        assert call(ws_bytes=(need16 if call is wide else need8) - 4) == nat.E_INVALID and "bytes are needed" in nat.last_error()
        assert call(ws_bytes=0, g=4) == nat.E_UNSUPPORTED, "an unsupported shape needs no workspace: its own refusal comes"
        assert call(g=4) == nat.E_UNSUPPORTED and call(g=40) == nat.E_UNSUPPORTED
        assert call(g_stride=562) == nat.E_UNSUPPORTED and "16-byte aligned" in nat.last_error()
    for name, addr in (("starts", p + 8192 + 2), ("order", p + 12288 + 2), ("chunks", p + 16384 + 2), ("chunk_starts", p + 20480 + 2)):
        assert wide(**{name: addr}) == nat.E_INVALID and "misaligned" in nat.last_error(), name
    assert wide(g=32, fin=576, g_stride=576) == nat.E_UNSUPPORTED
    assert narrow(K=0) == nat.E_UNSUPPORTED and narrow(K=9) == nat.E_UNSUPPORTED and "codebooks of 256 entries" in nat.last_error()
    # the existing training entries still refuse fp32 parameters
    assert nat.lib.aqlm_hip_codebook_grad_kx8(p, 564, nat.F32, p + 4096, nat.F32, p + 8192, 80, 560, 2, 8, p + 24576, nat.F32, p + 28672, need8,
                                              None) == nat.E_UNSUPPORTED
    del buf


# ---------------------------------------------------------------------------------------------------------------------------
# 3. the torch route, accumulate_xtx_
# ---------------------------------------------------------------------------------------------------------------------------
def restated_mse(codes_unsigned, codebooks, scales, reference, xtx):
    """(loss, d_codebooks, d_scales): the reference's ``_compute_mse`` on ``_dequantize_weight`` under autograd, in the inputs' dtype."""
    from aqlm_amd.utils import _dequantize_weight

    books = codebooks.detach().clone().requires_grad_(True)
    factors = scales.detach().clone().requires_grad_(True)
    delta = _dequantize_weight(codes_unsigned, books, factors) - reference
    loss = (delta @ xtx).flatten() @ delta.flatten() / reference.shape[0]
    d_books, d_factors = torch.autograd.grad(loss, (books, factors))
    return loss.detach(), d_books, d_factors


def host_case(K, nbits, ogs, g, out_groups=12, in_groups=9, seed=0):
    gen = torch.Generator().manual_seed(seed)
    size = 2 ** nbits
    unsigned = torch.randint(0, size, (out_groups, in_groups, K), generator=gen)
    codes = torch.where(unsigned >= size // 2, unsigned - size, unsigned).to(torch.int16 if nbits > 8 else torch.int8)
    codebooks = torch.randn((K, size, ogs, g), generator=gen)
    scales = torch.rand((out_groups, 1, 1, 1), generator=gen) + 0.5
    reference = torch.randn((out_groups * ogs, in_groups * g), generator=gen)
    x = torch.randn((3 * in_groups * g, in_groups * g), generator=gen)
    xtx = x.T @ x / x.shape[0]
    return unsigned, codes, codebooks, scales, reference, 0.5 * (xtx + xtx.T)


@pytest.mark.parametrize("scheme", [(1, 8, 1, 8), (2, 8, 1, 8), (1, 16, 1, 8), (2, 8, 2, 4), (3, 6, 1, 16), (1, 16, 1, 32)], ids=str)
def test_torch_route_is_autograd_of_the_restated_definition(scheme):
    from aqlm_amd import tuning

    unsigned, codes, codebooks, scales, reference, xtx = host_case(*scheme)
    if scheme[1] == 6:  # 64-entry codebooks live in int8 containers without wrap-around
        codes = unsigned.to(torch.int8)
    got = tuning.calibrated_loss_and_grads(codes, codebooks, scales, reference, xtx)
    want = restated_mse(unsigned, codebooks, scales, reference, xtx)
    assert got[0].dim() == 0 and got[1].shape == codebooks.shape and got[2].shape == scales.shape
    for a, b in zip(got, want):
        assert a.dtype == torch.float32 and torch.equal(a, b)
    # fp64 inputs run in fp64; the fp32 result agrees with it to fp32 rounding of sums of in_features * out_features terms
    wide = tuning.calibrated_loss_and_grads(codes, codebooks.double(), scales.double(), reference.double(), xtx.double())
    want64 = restated_mse(unsigned, codebooks.double(), scales.double(), reference.double(), xtx.double())
    for a, b, c in zip(wide, want64, got):
        assert a.dtype == torch.float64 and torch.equal(a, b)
        # every output is a sum of at most n = in * in * out products of magnitude <= the largest term: n * 2^-24 relative to the
        # sum of magnitudes is the textbook bound; the sums here are well conditioned, so it is taken relative to the largest output
        n = reference.numel() * reference.shape[1]
        assert float((c.double() - a).abs().max()) <= math.sqrt(n) * 2.0 ** -22 * float(a.abs().max())
    with pytest.raises(ValueError):
        tuning.calibrated_loss_and_grads(codes, codebooks, scales, reference[:, :-1], xtx)
    with pytest.raises(ValueError):
        tuning.calibrated_loss_and_grads(codes, codebooks, scales, reference, xtx[:-1])


def test_accumulate_xtx_is_the_running_mean_of_the_reference():
    from aqlm_amd import tuning

    gen = torch.Generator().manual_seed(2)
    batches = [torch.randn((5, 24), generator=gen), torch.randn((2, 7, 24), generator=gen).half(), torch.randn((1, 24), generator=gen)]
    for dtype in (torch.float64, torch.float32):
        acc = torch.zeros((24, 24), dtype=dtype)
        want = torch.zeros((24, 24), dtype=dtype)
        n = seen = 0
        for batch in batches:
            n = tuning.accumulate_xtx_(acc, n, batch)
            flat = batch.reshape(-1, batch.shape[-1])  # the reference's add_batch, restated
            want *= seen / (seen + flat.shape[0])
            seen += flat.shape[0]
            scaled = math.sqrt(1 / seen) * flat.t().to(dtype)
            want += scaled.matmul(scaled.t())
            assert n == seen
        assert n == 20 and torch.equal(acc, want)
        rows = torch.cat([b.reshape(-1, 24).double() for b in batches])
        assert torch.allclose(acc.double(), rows.T @ rows / 20, rtol=0, atol=(1e-12 if dtype == torch.float64 else 1e-5))
    with pytest.raises(ValueError):
        tuning.accumulate_xtx_(torch.zeros((24, 24)), 0, torch.zeros((3, 23)))
    with pytest.raises(ValueError):
        tuning.accumulate_xtx_(torch.zeros((24, 24)), 0, torch.zeros((24,)))


# ---------------------------------------------------------------------------------------------------------------------------
# 4. the loop, on a 64 -> 64 1x8 g8 host layer
# ---------------------------------------------------------------------------------------------------------------------------
# The step size of the descent run: halved from 1e-2 until the training phase of epoch 0 lowers the loss on this input (loss at step 0
# of epoch 0 against the objective of the parameters written at its end).  1e-2 itself does: checked on the CPU, and asserted below.
DESCENT_LR = 1e-2


def host_layer():
    from aqlm import QuantizedLinear

    gen = torch.Generator().manual_seed(3)
    layer = QuantizedLinear(64, 64, 8, 1, 1, 8, bias=False, dtype=torch.float32)
    with torch.no_grad():
        layer.codes.copy_(torch.randint(-128, 128, layer.codes.shape, generator=gen).to(torch.int8))
        layer.codebooks.copy_(torch.randn(layer.codebooks.shape, generator=gen))
        layer.scales.copy_(torch.rand(layer.scales.shape, generator=gen) + 0.5)
    weight = torch.randn((64, 64), generator=gen)
    x = torch.randn((200, 64), generator=gen)
    return layer, weight, x.T @ x / 200


def test_quantize_layer_descends_and_stops_early():
    from aqlm_amd import tuning

    layer_ref, weight, xtx = host_layer()
    start = float(tuning.calibrated_error(layer_ref, weight, xtx))
    work = copy.deepcopy(layer_ref)
    trace = []

    def watch(event, epoch, info):
        trace.append((event, epoch, float(tuning.calibrated_error(work, weight, xtx)), info))

    report = tuning.quantize_layer_(work, weight, xtx, lr=DESCENT_LR, max_epochs=2, steps_per_epoch=5, init=False, seed=5, callback=watch)
    assert report["routes"] == {"init": None, "grad": "torch", "search": "torch"} and report["epochs"] == 2 and not report["stopped_early"]
    assert len(report["losses"]) == 2 and len(report["changed"]) == 2
    assert [t[0] for t in trace] == ["trained", "searched", "trained", "searched"]
    # the loss is the objective over out_features; the training phase of epoch 0 lowers it at this step size
    assert math.isclose(report["losses"][0] * 64, start, rel_tol=1e-5) and report["initial_error"] == start
    assert trace[0][2] < start, "DESCENT_LR does not lower the loss in epoch 0: halve it"
    # every search leaves the objective of the stored parameters no higher than before it
    for trained, searched in ((trace[0], trace[1]), (trace[2], trace[3])):
        assert searched[2] <= trained[2] * (1 + 1e-6)
        assert searched[3]["changed"] == report["changed"][searched[1]]
    assert report["error"] < start and math.isclose(report["error"], trace[3][2], rel_tol=1e-6)
    # the early stop of the reference: the loss of epoch 1's step 0 is not below half the best so far -> no further update
    again = copy.deepcopy(layer_ref)
    stopped = tuning.quantize_layer_(again, weight, xtx, lr=DESCENT_LR, max_epochs=6, steps_per_epoch=5, init=False, seed=5,
                                     relative_mse_tolerance=0.5)
    assert stopped["stopped_early"] and stopped["epochs"] < 6 and len(stopped["changed"]) == stopped["epochs"]
    for epoch in range(1, stopped["epochs"]):
        assert stopped["losses"][epoch] / min(stopped["losses"][:epoch]) <= 0.5


def test_quantize_layer_is_reproducible_from_its_generator_and_seed():
    from aqlm_amd import tuning

    layer, weight, xtx = host_layer()
    results = []
    for _ in range(2):
        work = copy.deepcopy(layer)
        report = tuning.quantize_layer_(work, weight, xtx, max_epochs=2, steps_per_epoch=0, init=True,
                                        generator=torch.Generator().manual_seed(7), seed=9)
        assert report["routes"]["init"] == "torch" and report["routes"]["grad"] is None and report["losses"] == []
        results.append((work.codes.detach().clone(), work.codebooks.detach().clone(), work.scales.detach().clone(), report["changed"]))
    for a, b in zip(results[0][:3], results[1][:3]):
        assert torch.equal(a, b)
    assert results[0][3] == results[1][3]
    assert not torch.equal(results[0][0], layer.codes), "the initialisation wrote new codes"


def test_quantize_layer_refuses_what_the_code_update_refuses():
    from aqlm_amd import tuning

    layer, weight, xtx = host_layer()
    with pytest.raises(TypeError):
        tuning.quantize_layer_(torch.nn.Linear(64, 64), weight, xtx)
    layer._moe_expert = True
    with pytest.raises(TypeError):
        tuning.quantize_layer_(layer, weight, xtx)
    layer._moe_expert = False
    with pytest.raises(ValueError):
        tuning.quantize_layer_(layer, weight[:, :-8], xtx)
    with torch.inference_mode():
        frozen = copy.deepcopy(layer)
    with pytest.raises(RuntimeError):
        tuning.quantize_layer_(frozen, weight, xtx, max_epochs=1, steps_per_epoch=1)
