"""W straight from packed 1x16 codes on the MI355X: ``hk.dequant_1x16_packed`` (aqlm_hip_dequant_1x16_packed) against the route it
replaces, ``hk.code1x16_dequant(hk.unpack_1x16(packed), ...)`` -- bit for bit, scaled and unscaled, on every kind of packed buffer
the unpack entry serves (g8 / g16, ragged shapes, relabelled, variable geometry, 3-byte entries); its write discipline (every
element of W once, nothing outside W); that it reads the live codebook and never the buffer's codebook image; hipGraph capture; and
the routes of ``QuantizedLinear`` built on it: a dropped layer serves > 256-row forwards, ``in_features % 64 != 0``
forwards and every backward without restoring or unpacking, and ``prepack_model(single_copy=True)`` extends that to every row count.

Equalities are ``torch.equal``; the one tolerance is ``check_close`` of tests/test_hip_parity.py against the fp64 oracle (the
opt-in's 7 .. 256-row results, which are the large-batch op's > 256-row arithmetic)."""
import ctypes

import numpy as np
import pytest

from oracle import aqlm_oracle as orc
from tests.packed_model import zipf_codes
from tests.test_hip_parity import DEV, _module_from, check_close, tdtype, to_dev

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hk():
    assert torch.cuda.is_available(), "run with -m gpu on the MI355X box"
    from aqlm_amd.inference_kernels import hip_kernel

    return hip_kernel


def _layer(seed, fin, fout, g, dt, codes_unsigned=None):
    """Codes (uniform unless given), codebook and scales of one 1x16 layer on the device."""
    dtype = tdtype(dt)
    L = orc.make_layer(seed, fin, fout, 1, 16, g, batch=1, bias=False, float_dtype=np.float16 if dtype == torch.float16 else "bfloat16")
    if codes_unsigned is not None:
        L = dict(L, codes=orc.pack_int_data(codes_unsigned[:, :, None], 16))
    T = to_dev(L, dtype)
    return T["codes"], T["codebooks"], T["scales"]


def _reference(hk, packed, cb, scales):
    return hk.code1x16_dequant(hk.unpack_1x16(packed), cb, scales)


def _assert_same_bits(hk, packed, codes, cb, scales):
    assert torch.equal(hk.unpack_1x16(packed), codes)
    for s in (None, scales):
        W = hk.dequant_1x16_packed(packed, cb, s)
        assert W.shape == (packed.out_features, packed.in_features) and W.dtype == cb.dtype
        ref = _reference(hk, packed, cb, s)
        assert torch.equal(W.view(torch.int16), ref.view(torch.int16)), f"scaled={s is not None}"
        assert torch.equal(W, hk.code1x16_dequant(codes, cb, s))


UNIFORM = [
    (8, 2048, 1536, "float16"),
    (8, 4096, 1000, "float16"),    # ragged row groups
    (8, 4096, 37, "bfloat16"),     # fewer rows than 16 x waves
    (8, 520, 64, "float16"),       # 65 input groups
    (8, 64, 256, "float16"),       # almost all lane-steps null
    (16, 1040, 70, "bfloat16"),
    (16, 128, 256, "float16"),
    (16, 4096, 1000, "bfloat16"),
]


@pytest.mark.parametrize("g,fin,fout,dt", UNIFORM)
def test_uniform_codes_ragged_shapes(hk, g, fin, fout, dt):
    codes, cb, scales = _layer(900 + fin + fout + g, fin, fout, g, dt)
    packed = hk.prepack_1x16(codes, g, codebooks=cb)
    assert packed is not None, "the shape fell off the packed path"
    assert packed.in_group_size == g and packed.desc.entry_bytes == 4
    _assert_same_bits(hk, packed, codes, cb, scales)


def _zipf_packed(hk, alpha, sorted_labels, dt="float16"):
    fin, fout = 2048, 1536
    cu = zipf_codes(fout, fin // 8, alpha, sorted_labels, 7)
    codes, cb, scales = _layer(77, fin, fout, 8, dt, codes_unsigned=cu)
    packed = hk.prepack_1x16(codes, 8, codebooks=cb)
    assert packed is not None
    return packed, codes, cb, scales


def test_relabelled_buffer(hk):
    packed, codes, cb, scales = _zipf_packed(hk, 0.8, False)
    assert packed.desc.relabelled and not packed.desc.variable_geometry
    _assert_same_bits(hk, packed, codes, cb, scales)


@pytest.mark.parametrize("sorted_labels", [False, True])
def test_variable_geometry(hk, sorted_labels):
    packed, codes, cb, scales = _zipf_packed(hk, 1.2, sorted_labels, "bfloat16" if sorted_labels else "float16")
    assert packed.desc.variable_geometry
    _assert_same_bits(hk, packed, codes, cb, scales)


def test_three_byte_entries(hk):
    from aqlm_amd import _native

    codes, cb, scales = _layer(31, 2048, 1536, 8, "float16")
    old = _native.get_tuning("packed_entry_bytes")
    _native.set_tuning("packed_entry_bytes", 3)
    try:
        packed = hk.prepack_1x16(codes, 8, codebooks=cb)
    finally:
        _native.set_tuning("packed_entry_bytes", old)
    assert packed is not None and packed.desc.entry_bytes == 3
    _assert_same_bits(hk, packed, codes, cb, scales)


@pytest.mark.parametrize("by_xcd", [0, 2])
def test_both_grid_orders_give_the_same_bits(hk, by_xcd):
    """The knob `packed_dequant_by_xcd` (0 / 2: either order forced; 1, the default, picks by vector size) only renumbers the blocks:
    W does not depend on it (g8 and g16)."""
    from aqlm_amd import _native

    old = _native.get_tuning("packed_dequant_by_xcd")
    _native.set_tuning("packed_dequant_by_xcd", by_xcd)
    try:
        for g, fin, fout, dt in [(8, 4096, 1000, "float16"), (16, 1040, 70, "bfloat16")]:
            codes, cb, scales = _layer(5 + g, fin, fout, g, dt)
            packed = hk.prepack_1x16(codes, g, codebooks=cb)
            assert packed is not None
            _assert_same_bits(hk, packed, codes, cb, scales)
    finally:
        _native.set_tuning("packed_dequant_by_xcd", old)


@pytest.mark.parametrize("case", ["520x64", "zipf1.2"])
def test_write_discipline(hk, case):
    """W inside a larger buffer of sentinels (a NaN pattern no codebook entry or product has), guard rows before and after: the call
    leaves no sentinel inside W and touches no guard byte."""
    from aqlm_amd import _native

    if case == "520x64":
        codes, cb, scales = _layer(11, 520, 64, 8, "float16")
        packed = hk.prepack_1x16(codes, 8, codebooks=cb)
    else:
        packed, codes, cb, scales = _zipf_packed(hk, 1.2, False)
        assert packed.desc.variable_geometry
    assert packed is not None
    fout, fin = packed.out_features, packed.in_features
    guard = 4 * fin
    sentinel = 0x7E37   # an fp16 NaN
    for s in (None, scales):
        big = torch.full((guard + fout * fin + guard,), sentinel, dtype=torch.int16, device=DEV)
        W = big[guard:guard + fout * fin]
        assert W.data_ptr() % 16 == 0
        with torch.cuda.device(big.device):
            rc = _native.lib.aqlm_hip_dequant_1x16_packed(ctypes.byref(packed.desc), packed.data_ptr(), cb.data_ptr(),
                                                          None if s is None else s.data_ptr(), W.data_ptr(), _native.F16,
                                                          torch.cuda.current_stream().cuda_stream)
        assert rc == 0, _native.last_error()
        torch.cuda.synchronize()
        assert int((W == sentinel).sum()) == 0, "an element of W was not written"
        assert bool((big[:guard] == sentinel).all()) and bool((big[guard + fout * fin:] == sentinel).all()), "a guard row was written"
        assert torch.equal(W.view(torch.float16).reshape(fout, fin), _reference(hk, packed, cb, s))


def test_reads_the_live_codebook_not_the_image(hk):
    packed, codes, cb, scales = _zipf_packed(hk, 0.8, False)
    assert packed.desc.relabelled and packed.range_is_current(cb)   # the image holds the OLD codebook from here on
    new = (torch.randn_like(cb.float()) * 3.0).to(cb.dtype)
    cb.data.copy_(new)                                              # behind the version counter's back: nothing refreshes the image
    assert packed.range_is_current(cb)
    for s in (None, scales):
        W = hk.dequant_1x16_packed(packed, cb, s)
        assert torch.equal(W, hk.code1x16_dequant(codes, new, s))
    # ... nor the flag that says an image exists, nor the codebook range
    packed.forget_range()
    assert not (packed.desc.flags & 4) and packed.desc.codebook_absmax == 0.0
    assert torch.equal(hk.dequant_1x16_packed(packed, cb, scales), hk.code1x16_dequant(codes, new, scales))


def test_hipgraph_capture_and_replay(hk):
    packed, codes, cb, scales = _zipf_packed(hk, 0.8, False)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        hk.dequant_1x16_packed(packed, cb, scales)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        W = hk.dequant_1x16_packed(packed, cb, scales)
    for k in range(2):
        with torch.no_grad():
            cb.copy_((torch.randn_like(cb.float()) * (k + 1.5)).to(cb.dtype))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(W, hk.dequant_1x16_packed(packed, cb, scales))
        assert torch.equal(W, hk.code1x16_dequant(codes, cb, scales))


# ---------------------------------------------------------------------------------------------------------------- the module
def _no_unpack(monkeypatch, hk):
    def refuse(packed):
        raise AssertionError("this call was not to unpack the codes")

    monkeypatch.setattr(hk, "unpack_1x16", refuse)


def _module(seed, fin, fout, rows):
    L = orc.make_layer(seed, fin, fout, 1, 16, 8, batch=rows, bias=True)
    m, T = _module_from(L, 1, 16, 8, fin, fout, torch.float16)
    return m, T, L


def test_strict_drop_long_forward_and_backward_from_packed(hk, monkeypatch):
    from aqlm.checkpoint import prepack_model

    fin, fout = 2048, 1536
    m, T, _ = _module(51, fin, fout, 300)
    holder = torch.nn.ModuleDict({"l": m})
    gw = torch.randn(300, fout, device=DEV, dtype=torch.float16)
    prepack_model(holder, min_codes=100_000, drop_canonical=False)
    assert m._packed_codes is not None and not m._codes_dropped
    with torch.no_grad():
        ref = m(T["x"])
    xg = T["x"].clone().requires_grad_(True)
    (m(xg) * gw).sum().backward()
    grad_ref = xg.grad.clone()
    prepack_model(holder, min_codes=100_000, drop_canonical=True)
    assert m._codes_dropped and m._codes_drop_strict and isinstance(m._packed_codes, hk.PackedCodes)
    _no_unpack(monkeypatch, hk)
    with torch.no_grad():
        assert torch.equal(m(T["x"]), ref)                                   # 1. the 300-row forward, no unpack
    xg = T["x"].clone().requires_grad_(True)
    y = m(xg)
    assert torch.equal(y.detach(), ref)
    (y * gw).sum().backward()
    assert torch.equal(xg.grad, grad_ref) and m._codes_dropped               # 2. the same gradient, still dropped
    x2 = T["x"][:2].clone().requires_grad_(True)                             # a short forward with a gradient: its BACKWARD is packed too
    monkeypatch.undo()
    y2 = m(x2)                                                               # (the matvec op reads codes unpacked for this call)
    _no_unpack(monkeypatch, hk)
    (y2 * gw[:2]).sum().backward()
    assert m._codes_dropped and torch.isfinite(x2.grad).all()
    assert torch.equal(x2.grad, torch.matmul(gw[:2], hk.code1x16_dequant(T["codes"], m.codebooks, m.scales)))


def test_default_prepack_keeps_one_copy_through_prompt_and_training_step(hk, monkeypatch):
    from aqlm.checkpoint import prepack_model

    fin, fout = 2048, 1536
    m, T, _ = _module(52, fin, fout, 300)
    holder = torch.nn.ModuleDict({"l": m})
    prepack_model(holder, min_codes=100_000, drop_canonical=False)
    with torch.no_grad():
        ref300, ref9 = m(T["x"]), m(T["x"][:9])
    prepack_model(holder, min_codes=100_000)
    assert m._codes_dropped and not m._codes_drop_strict and m.rows_from_packed == 0
    _no_unpack(monkeypatch, hk)
    with torch.no_grad():
        assert torch.equal(m(T["x"]), ref300)
    xg = T["x"].clone().requires_grad_(True)
    m(xg).sum().backward()
    assert m._codes_dropped and m.codes.numel() == 0 and xg.grad is not None   # 3. neither restored the codes
    monkeypatch.undo()
    with torch.no_grad():
        assert torch.equal(m(T["x"][:9]), ref9)                                # 4. a 9-row call still does, as before
    assert not m._codes_dropped and torch.equal(m.codes, T["codes"])


def test_in_features_not_a_multiple_of_64_takes_the_packed_route(hk, monkeypatch):
    from aqlm.checkpoint import prepack_model

    fin, fout = 520, 64
    m, T, _ = _module(53, fin, fout, 9)
    holder = torch.nn.ModuleDict({"l": m})
    prepack_model(holder, min_codes=1000, drop_canonical=False)
    assert isinstance(m._packed_codes, hk.PackedCodes)
    with torch.no_grad():
        ref = m(T["x"])
    prepack_model(holder, min_codes=1000, drop_canonical=True)
    assert m._codes_dropped and m._codes_drop_strict
    _no_unpack(monkeypatch, hk)
    with torch.no_grad():
        assert torch.equal(m(T["x"]), ref) and m._codes_dropped                # 5.


def test_single_copy_serves_every_row_count_from_packed(hk, monkeypatch):
    import torch.nn.functional as F

    from aqlm.checkpoint import memory_report, prepack_model

    fin, fout = 2048, 1536
    m, T, L = _module(54, fin, fout, 64)
    holder = torch.nn.ModuleDict({"l": m})
    rep = prepack_model(holder, min_codes=100_000, single_copy=True)
    assert m._codes_dropped and m._codes_drop_strict and m.rows_from_packed == 7 and rep["codes_dropped_layers"] == 1
    assert rep["codes"] == 0 and memory_report(holder)["code_bits_per_weight"] == rep["code_bits_per_weight"]
    _no_unpack(monkeypatch, hk)
    y64 = orc.dequantize_gemm(L["x"], L["codes"], L["codebooks"], L["scales"], L["bias"])
    W = hk.code1x16_dequant(T["codes"], m.codebooks, None)
    with torch.no_grad():
        for rows in (9, 64):
            x = T["x"][:rows]
            y = m(x)
            assert m._codes_dropped
            assert torch.equal(y, hk._scale_bias_fp32(F.linear(x, W), m.scales, m.bias))   # 6. the op's > 256-row arithmetic
            check_close(y.float().cpu().numpy(), y64[:rows], torch.float16, f"single copy, {rows} rows")
        y3 = m(T["x"][:3])                                                                  # decode calls: the packed matvec, as ever
        assert torch.equal(y3, hk.code1x16_matmat_packed(T["x"][:3], m._packed_codes, m.codebooks, m.scales, m.bias))
    with pytest.raises(ValueError):
        prepack_model(holder, min_codes=100_000, single_copy=True, drop_canonical=False)


def test_dense_weight_of_a_dropped_layer_is_the_same_bits(hk, monkeypatch):
    from aqlm.checkpoint import prepack_model
    from aqlm_amd.utils import _dequantize_weight, unpack_int_data

    fin, fout = 2048, 1536
    m, T, _ = _module(55, fin, fout, 16)
    holder = torch.nn.ModuleDict({"l": m})
    prepack_model(holder, min_codes=100_000, drop_canonical=False)
    m.prefer_dense_below_rows = 129
    with torch.no_grad():
        w_before = m._dense_weight().clone()
        y_before = m(T["x"])
        # what `_dense_weight()` of a dropped layer computed before the packed dequant existed: torch indexing on the unpacked codes
        w_torch = _dequantize_weight(unpack_int_data(T["codes"], 16), m.codebooks, m.scales).to(torch.float16).contiguous()
    assert torch.equal(w_before, w_torch)
    prepack_model(holder, min_codes=100_000, drop_canonical=True)
    m._dense = None
    _no_unpack(monkeypatch, hk)
    with torch.no_grad():
        w_after = m._dense_weight()
        assert torch.equal(w_after, w_torch) and m._codes_dropped               # 7.
        assert torch.equal(m(T["x"]), y_before)
