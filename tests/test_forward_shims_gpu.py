"""GPU: what the shared host glue of the forward shims must hold whichever shim it serves (aqlm_amd/inference_kernels/hip_kernel.py).

Three properties, each over every shim that uses the helper: parameters that are strided views reach the kernels as their
contiguous copies (``_c``, the ``keep`` list of ``_segment_table``); a call of more rows than one launch takes is the same bits as
its slabs launched alone (``_row_slabs``); and both scratch forms -- the stream's fixed-point cells, the fp32 workspace of the
two-kernel form -- meet the fp64 oracle and leave the cells zero (``_packed_scratch``, ``_lut_scratch``).  Shapes are the
smallest the neighbouring tests of tests/test_hip_parity.py run per op.
"""
import functools
from types import SimpleNamespace

import numpy as np
import pytest

from oracle import aqlm_oracle as orc

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from tests.test_hip_parity import DEV, check_close, to_dev  # noqa: E402

ROWS = 9  # one full slab of MAX_GEMV_BATCH rows and one more
SCHEMES = {  # K, nbits, g, in_features, out_features of the two layers sharing x
    "1x16": (1, 16, 8, 1024, (37, 512)),
    "2x8": (2, 8, 8, 1024, (256, 512)),
    "8x8": (8, 8, 8, 512, (256, 40)),
    "planar": (8, 8, 8, 1024, (256, 40)),   # planar codes need at least 64 input groups
    "packed": (1, 16, 8, 4096, (300, 77)),
}
F16, BF16 = torch.float16, torch.bfloat16


@pytest.fixture(scope="module")
def hk():
    assert torch.cuda.is_available(), "run with -m gpu on the MI355X box"
    from aqlm_amd.inference_kernels import hip_kernel

    return hip_kernel


@functools.lru_cache(maxsize=None)
def case(name, dtype):
    """Two seeded layers of a scheme on the device, ROWS shared input rows and the fp64 oracle of both; made once, never written."""
    from aqlm_amd.inference_kernels import hip_kernel as hk

    K, nbits, g, fin, fouts = SCHEMES[name]
    fd = np.float16 if dtype == F16 else "bfloat16"
    Ls = [orc.make_layer(7300 + 31 * k + fin + K, fin, fo, K, nbits, g, batch=ROWS, bias=(k == 0), float_dtype=fd)
          for k, fo in enumerate(fouts)]
    Ts = [to_dev(L, dtype) for L in Ls]
    y64 = [orc.dequantize_gemm(Ls[0]["x"], L["codes"], L["codebooks"], L["scales"], L["bias"]) for L in Ls]
    derived = [None, None]
    if name == "packed":
        derived = [hk.prepack_1x16(T["codes"], g, T["codebooks"]) for T in Ts]
    elif name == "planar":
        derived = [hk.planar_8x8_pack(T["codes"], g, codebooks=T["codebooks"]) for T in Ts]
    assert name not in ("packed", "planar") or all(d is not None for d in derived)
    return SimpleNamespace(Ts=Ts, x=Ts[0]["x"], y64=y64, derived=derived)


def single(hk, name, x, T, derived):
    """The single-layer shim of a scheme."""
    params = (T["codebooks"], T["scales"], T["bias"])
    if name == "packed":
        return hk.code1x16_matmat_packed(x, derived, *params)
    if name == "planar":
        return hk.code8x8_matmat_planar(x, derived, *params)
    if name == "8x8":
        return hk._gemv_8x8_lut(x, T["codes"], *params)
    return hk._gemv(x, T["codes"], *params, "1x16" if name == "1x16" else "kx8")


def shared(hk, name, x, Ts, derived):
    """The shared-input launch of a scheme over both layers."""
    lists = [T["codebooks"] for T in Ts], [T["scales"] for T in Ts], [T["bias"] for T in Ts]
    if name == "packed":
        return hk.code1x16_matmat_packed_multi(x, derived, *lists)
    if name == "planar":
        return hk.code8x8_matmat_planar_multi(x, derived, *lists)
    if name == "8x8":
        return hk._gemv_8x8_lut_multi(x, [T["codes"] for T in Ts], *lists)
    return hk._gemv_multi(x, [T["codes"] for T in Ts], *lists, "1x16" if name == "1x16" else "kx8")


def strided(t):
    """A view with the values and shape of ``t`` that is not contiguous (every other element of a larger tensor)."""
    if t is None:
        return None
    view = torch.stack([t, torch.zeros_like(t)], dim=-1)[..., 0]
    assert not view.is_contiguous() and torch.equal(view, t)
    return view


def padded_rows(x):
    """The rows of ``x`` inside a wider buffer: a row stride larger than the row (a multiple of 8 elements: not copied)."""
    wide = torch.zeros(x.shape[0], x.shape[1] + 8, dtype=x.dtype, device=x.device)
    wide[:, :x.shape[1]] = x
    return wide[:, :x.shape[1]]


# ------------------------------------------------------------------ strided parameters
@pytest.mark.parametrize("name,dtype", [(n, F16) for n in SCHEMES] + [("1x16", BF16)])
def test_strided_parameters_give_the_bits_of_contiguous_ones(hk, name, dtype):
    c = case(name, dtype)
    views = [dict(T, codebooks=strided(T["codebooks"]), scales=strided(T["scales"]), bias=strided(T["bias"])) for T in c.Ts]
    x2 = padded_rows(c.x[:2])
    assert x2.stride(0) > x2.shape[1]
    for T, V, d in zip(c.Ts, views, c.derived):
        want = single(hk, name, c.x[:2].contiguous(), T, d)
        assert torch.equal(single(hk, name, x2, V, d), want)
    rows = 1 if name in ("8x8", "planar") else 2   # the shared-input look-up-table kernels take one row
    want = shared(hk, name, c.x[:rows].contiguous(), c.Ts, c.derived)
    got = shared(hk, name, x2[:rows], views, c.derived)
    assert len(got) == len(want) == 2 and all(torch.equal(a, b) for a, b in zip(got, want))
    for y, y64 in zip(got, c.y64):
        check_close(y.float().cpu().numpy(), y64[:rows], dtype, f"{name}, strided parameters")


# ------------------------------------------------------------------ the slab boundary
@pytest.mark.parametrize("name,multi", [("1x16", False), ("2x8", False), ("packed", False), ("1x16", True), ("2x8", True)])
def test_nine_rows_are_a_slab_of_eight_and_a_slab_of_one(hk, name, multi, monkeypatch):
    monkeypatch.setattr(hk, "_fused_kx8_mfma", lambda *a, **k: None)   # _gemv above 8 rows: the slab loop, not the MFMA detour
    c = case(name, F16)
    if multi:
        run = lambda x: shared(hk, name, x, c.Ts, c.derived)
    else:
        run = lambda x: [single(hk, name, x, c.Ts[0], c.derived[0])]
    by_rows = {n: run(c.x[:n]) for n in (1, 2, 8, 9)}
    last = run(c.x[8:9])
    for k, y9 in enumerate(by_rows[9]):
        for n, ys in by_rows.items():
            assert ys[k].shape == (n, y9.shape[1])
            check_close(ys[k].float().cpu().numpy(), c.y64[k][:n], F16, f"{name}, {n} rows")
        assert torch.equal(y9[:8], by_rows[8][k]), "rows 0..7 of the 9-row call differ from the 8-row call"
        assert torch.equal(y9[8:9], last[k]), "row 8 of the 9-row call differs from the row launched alone"


# ------------------------------------------------------------------ the scratch choice
@pytest.mark.parametrize("name", ["packed", "8x8", "planar"])
@pytest.mark.parametrize("multi", [False, True], ids=["single", "multi"])
def test_both_scratch_forms_meet_the_oracle_and_leave_the_cells_zero(hk, name, multi, monkeypatch):
    c = case(name, F16)
    choice = "_packed_scratch" if name == "packed" else "_lut_scratch"
    real, forms = getattr(hk, choice), []
    monkeypatch.setattr(hk, choice, lambda *a: (forms.append(real(*a)), forms[-1])[1])
    x = c.x[:1]
    run = (lambda: shared(hk, name, x, c.Ts, c.derived)) if multi else (lambda: [single(hk, name, x, c.Ts[0], c.derived[0])])
    with_cells = run()
    assert [f[0] for f in forms] == [True], "the default is the single-kernel form on the stream's cells"
    with monkeypatch.context() as m:
        if name == "packed":
            hk.set_fused_finalize(False)   # FUSED_FINALIZE and the library knob it mirrors
        elif name == "8x8":
            m.setattr(hk, "USE_8X8_LUT_FUSED", False)
        else:   # an unknown codebook bound, current for this codebook tensor
            for d, T in zip(c.derived, c.Ts):
                m.setattr(d, "codebook_absmax", 0.0)
                m.setattr(d, "_range_of", (T["codebooks"].data_ptr(), hk._version(T["codebooks"])))
        try:
            assert name != "packed" or hk.FUSED_FINALIZE is False
            two_kernels = run()
        finally:
            hk.set_fused_finalize(True)
    assert [f[0] for f in forms] == [True, False] and forms[1][1].dtype == torch.float32
    for k, (a, b) in enumerate(zip(with_cells, two_kernels)):
        check_close(a.float().cpu().numpy(), c.y64[k][:1], F16, f"{name}, cells")
        check_close(b.float().cpu().numpy(), c.y64[k][:1], F16, f"{name}, two kernels")
    torch.cuda.synchronize()
    cells = hk.accumulator_cells()
    assert cells and all(int(t.abs().max()) == 0 for t in cells), "cells must be zero when the kernels have finished"
