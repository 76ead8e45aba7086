"""Every hand-written forward route at checkpoint-scale, outlier and subnormal magnitudes (tests/magnitude.py), one launch each at
the route's smallest shape.  For every route and regime:

  (P) ``check_close`` of tests/test_hip_parity.py -- its own bounds -- against the fp64 oracle on the stored values;
  (T) ``torch.equal(route(layer), route(twin))``: the twin is the same real-valued layer with its operands moved by exact powers
      of two to unit magnitude, and a route that forms exact products, sums in fp32 and rounds once gives the same bits for both
      as long as nothing under- or overflows.  A flushed subnormal operand, a half-precision intermediate or an absolute constant
      breaks the equality.  ``outlier`` has no twin beyond ``checkpoint``'s: (P) only.

Routes with a fused and a two-kernel form run both, and the accumulator cells must read zero afterwards.  Each route asserts that
it was taken (a fall-through cannot satisfy the test).  The dequantise + library-GEMM routes are left out: W is held bit-exact by
tests/test_dequant_exact_gpu.py and the GEMM is not this project's.  No tolerance of this file's own: the only numbers are the
shifts and conditions of tests/magnitude.py and the bounds of ``check_close``."""
import contextlib
import functools

import numpy as np
import pytest

from tests import magnitude as mg
from tests.test_hip_parity import DEV, check_close, tdtype, to_dev

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


def regimes(misses=None):
    """Every (regime, dtype, check) as pytest params.  ``check`` says which of (P) and (T) the case asserts: "PT" for both in one
    case; a case in ``misses`` {(regime, dtype): measured figure} is split into "P", a hard assertion like everywhere else, and
    "T", the strict expected failure -- so a kernel that starts to flush the operand fails (P) there and is not taken for the
    expected miss of (T)."""
    out = []
    for r in mg.REGIMES:
        for d in mg.regime_dtypes(r):
            if misses and (r, d) in misses:
                out.append(pytest.param(r, d, "P", id=f"{r}-{d}-P"))
                out.append(pytest.param(r, d, "T", id=f"{r}-{d}-T", marks=pytest.mark.xfail(strict=True, reason=misses[(r, d)])))
            else:
                out.append(pytest.param(r, d, "PT", id=f"{r}-{d}"))
    return out


def regimes_f16(misses=None):
    """``regimes`` for the fp16-only routes: (regime, check)."""
    return [pytest.param(p.values[0], p.values[2], id=p.id.replace("-float16", ""), marks=p.marks)
            for p in regimes({(r, "float16"): v for r, v in (misses or {}).items()}) if p.values[1] == "float16"]


REG = [pytest.param(*p.values[:2], id=p.id) for p in regimes()]
REG_F16 = [pytest.param(r, id=r) for r in mg.REGIMES]

# What the suite measured on the MI355X ("Magnitudes"): v_dot2_f32_f16 and v_mfma_f32_16x16x32_f16 both KEEP
# fp16 subnormal operands -- (P) holds in every regime on every route, at the same figure for the layer and its twin, where a flush
# would cost 0.39 and more (tests/magnitude.py).  (T) holds on every route in every regime except the five cases marked below, all
# on the matrix unit with one operand mostly subnormal: one or two outputs in thousands differ from the twin's by one unit in the
# last place of fp16 (the transposed launch writes fp32, where every such difference shows: 7 % of the outputs).  Nothing is
# flushed and no tolerance is touched.  The instructions' fp32 result is correct to fp32 round-off on both sides (4e-8 of the
# fp64 sum) but is not bit for bit the same function of subnormal and of normalised operands: on one MFMA of random operands, one
# of them at 2**-14, 5 - 6 % of the fp32 results differ from the twin's whichever operand is the small one, none with operands
# at 2**-10 or above; v_dot2 shows the same in 1 - 2 % (tools/microbench/subnormal_probe.hip prints these figures).  One output
# rounding in a few thousand turns that into a visible bit.  Nothing is declined or rerouted for it: nothing is flushed and
# both results are correct to fp32 round-off, so a predicate (an abs-min over the codebook at load, over x per call) would cost
# speed and gain no accuracy.  The five cases stay as strict expected failures of (T) alone -- (P) is asserted in a case of its
# own -- with their figures.
# By the same measurement the (T) passes of the OTHER ``sub_*`` cases -- every dot2 route, the X-resident K x 8 kernel, 8x8 g32 at
# 3 rows, the 1x16 large-batch kernels -- are a matter of the seed and of the number of outputs, not a property of the route: a
# legitimate change of summation order, of a seed (tests/magnitude.py: SEEDS) or of a shape may flip one of them.  Such a flip
# with (P) unchanged and a handful of outputs one ulp apart is this effect, not a kernel bug; a flush moves (P) to 1e-2 .. 0.5.
# In ``checkpoint`` and ``small_normal`` (no, or next to no, subnormal operand) a (T) miss is a kernel bug.
MFMA_SUB = "MFMA route, %s mostly fp16-subnormal: nothing flushed ((P) holds in its own case), (T) %s outputs differ from the twin's"
MFMA_SUB_X = MFMA_SUB % ("x", "%s")


@pytest.fixture(scope="module")
def hk():
    assert torch.cuda.is_available(), "run with -m gpu on the MI355X box"
    from aqlm_amd.inference_kernels import hip_kernel

    return hip_kernel


@contextlib.contextmanager
def tuning(key, value):
    """A tuning key of the library set for the duration, read back (the route guard of the keyed kernels) and put back."""
    from aqlm_amd import _native

    keep = _native.get_tuning(key)
    _native.set_tuning(key, value)
    try:
        assert _native.get_tuning(key) == value
        yield
    finally:
        _native.set_tuning(key, keep)


@contextlib.contextmanager
def attr(obj, name, value):
    keep = getattr(obj, name)
    setattr(obj, name, value)
    try:
        yield
    finally:
        setattr(obj, name, keep)


@functools.lru_cache(maxsize=None)
def _dev(name, regime, dt):
    L, twin = mg.layer(name, regime, dt)
    return L, to_dev(L, tdtype(dt)), None if twin is None else to_dev(twin, tdtype(dt))


def _args(D):
    return D["codes"], D["codebooks"], D["scales"], D["bias"]


def _cells_at_rest(hk):
    """Every accumulator-cell set of the stream reads zero once the launch has finished.  (That the single-kernel form ran is
    what the callers' switches say -- ``FUSED_FINALIZE``, ``USE_8X8_LUT_FUSED``, a codebook bound > 0 --, not the existence of the
    cells: the registries outlive earlier tests.)"""
    torch.cuda.synchronize()
    cells = hk.accumulator_cells()
    assert cells, "the single-kernel forms take their cells from these registries: there must be a set for this stream"
    assert all(int(torch.count_nonzero(c)) == 0 for c in cells), "the accumulator cells must be zero when the kernel has finished"


def _hold(y, yt, y64, dtype, what, check="PT"):
    """(P) and / or (T) on one route's outputs (``check``: "PT", "P" or "T"); both figures are printed before either is asserted."""
    assert check in ("PT", "P", "T")
    y64 = np.asarray(y64, dtype=np.float64)
    yn = y.double().cpu().numpy()
    m = float(np.mean(np.abs(yn - y64)) / np.mean(np.abs(y64)))
    diff = None if yt is None else int((y != yt).sum() + (torch.isnan(y) | torch.isnan(yt)).sum())
    msg = f"[magnitude] {what}: (P) mean-rel {m:.3e}"
    if yt is not None:
        mt = float(np.mean(np.abs(yt.double().cpu().numpy() - y64)) / np.mean(np.abs(y64)))
        msg += f", twin {mt:.3e}; (T) {diff} of {y.numel()} outputs differ from the twin's"
    print(msg)
    if "P" in check:
        check_close(yn, y64, dtype, what)
        if yt is not None:
            check_close(yt.double().cpu().numpy(), y64, dtype, what + " (twin)")
    if "T" in check:
        assert yt is not None or check == "PT", f"{what}: a (T) case without a twin"
        if yt is not None:
            assert y.dtype == yt.dtype and torch.equal(y, yt), f"{what}: {diff} of {y.numel()} outputs differ between the layer and its twin"


def hold(route, name, regime, dt, rows, what, check="PT"):
    """``route(D)`` on the layer and on its twin, D the device tensors with the first ``rows`` rows of x."""
    L, T, Tt = _dev(name, regime, dt)
    cut = lambda D: dict(D, x=D["x"][:rows])  # noqa: E731
    y = route(cut(T))
    yt = None if Tt is None else route(cut(Tt))
    assert tuple(y.shape) == (rows, L["codes"].shape[0])
    _hold(y, yt, L["y64"][:rows], tdtype(dt), f"{what} {name} rows {rows} {regime} {dt}", check)


# ------------------------------------------------------------------ 1. direct 1x16 matvec
@pytest.mark.parametrize("regime,dt", REG)
@pytest.mark.parametrize("rows", [1, 8])
@pytest.mark.parametrize("name", ["1x16g8_512x64", "1x16g16_1024x64"])
def test_direct_1x16(hk, name, rows, regime, dt):
    hold(lambda D: hk._gemv(D["x"], *_args(D), "1x16"), name, regime, dt, rows, "direct 1x16")


# ------------------------------------------------------------------ 2. packed 1x16 matvec, single-kernel and two-kernel finalize
_PACKED = {}


def _packed_for(hk, D, name, g, entry_bytes):
    """The packed buffer of the layer's codes (layer, twin and every regime share the codes) with the range of THIS codebook."""
    key = (name, entry_bytes)
    if key not in _PACKED:
        with tuning("packed_entry_bytes", entry_bytes if g == 8 else 0):
            _PACKED[key] = hk.prepack_1x16(D["codes"], g)
        assert _PACKED[key] is not None and torch.equal(hk.unpack_1x16(_PACKED[key]), D["codes"])
    packed = _PACKED[key]
    assert packed.desc.entry_bytes == entry_bytes and packed.in_group_size == g
    packed.set_codebook_range(D["codebooks"])   # layer and twin have different ranges
    assert packed.desc.codebook_absmax == float(D["codebooks"].abs().max()) > 0.0 and packed.range_is_current(D["codebooks"])
    return packed


@pytest.mark.parametrize("regime,dt", REG)
@pytest.mark.parametrize("rows", [1, 8])
@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("name,g,entry_bytes", [("1x16g8_1024x256", 8, 3), ("1x16g8_1024x256", 8, 4), ("1x16g16_2048x256", 16, 4)])
def test_packed_1x16(hk, name, g, entry_bytes, fused, rows, regime, dt):
    def route(D):
        packed = _packed_for(hk, D, name, g, entry_bytes)
        y = hk.code1x16_matmat_packed(D["x"], packed, D["codebooks"], D["scales"], D["bias"])
        if fused:
            _cells_at_rest(hk)
        return y

    hk.set_fused_finalize(fused)
    try:
        assert hk.FUSED_FINALIZE == fused
        hold(route, name, regime, dt, rows, f"packed 1x16 entry_bytes {entry_bytes} fused {fused}")
    finally:
        hk.set_fused_finalize(True)


# ------------------------------------------------------------------ 3. K x 8 g8 matvec, plain and replicated-LDS kernels
@pytest.mark.parametrize("regime,dt", REG)
@pytest.mark.parametrize("replicas", [0, 2])
@pytest.mark.parametrize("name", ["1x8g8_1024x128", "2x8g8_1024x128"])
def test_kx8_matvec(hk, name, replicas, regime, dt):
    with tuning("kx8_replicas", replicas):   # 0 = never the replicated kernel, 2 = whenever the shape fits (it takes any row count)
        hold(lambda D: hk.codekx8_matmat(D["x"], *_args(D)), name, regime, dt, 1, f"K x 8 matvec replicas {replicas}")


# ------------------------------------------------------------------ 4. 8 x 8 look-up-table matvec
LUT_LAYERS = [("8x8g32_2048x72", 32), ("8x8g8_1024x64", 8)]


@pytest.mark.parametrize("regime,dt", REG)
@pytest.mark.parametrize("rows", [1, 8])
@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("name,g", LUT_LAYERS)
def test_8x8_lut(hk, name, g, fused, rows, regime, dt):
    """Canonical codes: one row and the 2..8-row form, single-kernel (fixed-point cells) and two-kernel finalize."""
    def route(D):
        if fused:
            assert hk._lut_cells(D["x"].device, hk._stream_ptr(D["x"].device), rows * D["codes"].shape[0]) is not None
        y = hk._gemv_8x8_lut(D["x"], *_args(D))
        if fused:
            _cells_at_rest(hk)
        return y

    with attr(hk, "USE_8X8_LUT_FUSED", fused):
        hold(route, name, regime, dt, rows, f"8x8 lut fused {fused}")


@pytest.mark.parametrize("regime,dt", REG)
@pytest.mark.parametrize("rows", [1, 8])
@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("waves", [8, 16])
@pytest.mark.parametrize("name,g", LUT_LAYERS)
def test_8x8_lut_planar(hk, name, g, waves, fused, rows, regime, dt):
    """Planar codes at both workgroup sizes; the two-kernel form is what a planar buffer without a codebook bound gets."""
    def route(D):
        planar = hk.planar_8x8_pack(D["codes"], g, codebooks=D["codebooks"])
        assert planar is not None and torch.equal(hk.planar_8x8_unpack(planar), D["codes"])
        assert planar.codebook_absmax == float(D["codebooks"].abs().max()) > 0.0
        if not fused:
            planar.codebook_absmax = 0.0
            assert planar.range_is_current(D["codebooks"])   # so the op does not take the bound again
        y = hk.code8x8_matmat_planar(D["x"], planar, D["codebooks"], D["scales"], D["bias"])
        assert (planar.codebook_absmax > 0.0) == fused
        if fused:
            _cells_at_rest(hk)
        return y

    assert hk.USE_8X8_LUT_FUSED
    with tuning("lut_waves", waves):
        hold(route, name, regime, dt, rows, f"8x8 lut planar waves {waves} fused {fused}")


# ------------------------------------------------------------------ 5. 1x16 large-batch op, every kernel behind it
@pytest.mark.parametrize("regime,dt", REG)
@pytest.mark.parametrize("name,rows,variant", [("1x16g8_512x48", 32, 1), ("1x16g8_512x48", 32, 2), ("1x16g8_512x48", 32, 3),
                                               ("1x16g16_1024x64_b20", 20, 1), ("1x16g16_1024x64_b20", 20, 2),
                                               ("1x16g16_1024x64_b20", 20, 3), ("1x16g8_1024x64_b5", 5, 4)])
def test_1x16_large_batch_op(hk, name, rows, variant, regime, dt):
    def route(D):
        assert hk._fused_mfma_ok(D["x"], D["x"].shape[1])
        y = hk.code1x16_matmat_dequant(D["x"], *_args(D))
        if variant == 4:   # the slice-scan kernel took it: its own entry gives the same bits
            ys = hk.code1x16_matmat_scan(D["x"], *_args(D))
            assert ys is not None and torch.equal(ys, y)
        return y

    with tuning("gemm_variant", variant):
        hold(route, name, regime, dt, rows, f"1x16 large-batch variant {variant}")


# ------------------------------------------------------------------ 6. fused K x 8 MFMA: streaming, K-split, X-resident
def _fused_kx8(hk, D):
    y = hk._fused_kx8_mfma(D["x"], *_args(D), hk._dtype_id(D["x"]))
    assert y is not None
    return y


@pytest.mark.parametrize("regime,dt,check", regimes({("sub_x", "float16"): MFMA_SUB_X % "1 of 1024"}))
def test_fused_kx8_streaming(hk, regime, dt, check):
    with tuning("kx8_xres", 0):
        hold(lambda D: _fused_kx8(hk, D), "2x8g8_384x64", regime, dt, 16, "fused K x 8 streaming", check)


@pytest.mark.parametrize("regime,dt,check", regimes({("sub_x", "float16"): MFMA_SUB_X % "2 of 4800"}))
def test_fused_kx8_ksplit(hk, regime, dt, check):
    from aqlm_amd import _native

    assert hk.USE_FUSED_KX8_KSPLIT and hk._lib.aqlm_hip_workspace_bytes(_native.OP_GEMM_KX8_MFMA, 100, 48, 640) > 0
    hold(lambda D: _fused_kx8(hk, D), "2x8g8_640x48", regime, dt, 100, "fused K x 8 K-split", check)


@pytest.mark.parametrize("regime,dt", REG)
@pytest.mark.parametrize("rows", [2, 16])
@pytest.mark.parametrize("op", ["code2x8_matmat_dequant", "code2x8_matmat"])
def test_fused_kx8_x_resident(hk, op, rows, regime, dt):
    from aqlm_amd import _native

    def route(D):
        y = getattr(hk, op)(D["x"], *_args(D))
        assert torch.equal(_fused_kx8(hk, D), y)   # the op arrived at the fused kernel
        return y

    assert _native.get_tuning("kx8_xres") == 1 and _native.get_tuning("kx8_mfma_min_rows") == 2
    hold(route, "2x8g8_384x40", regime, dt, rows, f"fused K x 8 X-resident {op}")


# ------------------------------------------------------------------ 7. fused 8x8 g32 MFMA
@pytest.mark.parametrize("name,rows,regime,dt,check", [
    pytest.param(n, r, *p.values, id=f"{n}-{r}-{p.id}", marks=p.marks)
    for n, r, miss in (("8x8g32_2304x72", 3, {}), ("8x8g32_2048x200", 64, {("sub_x", "float16"): MFMA_SUB_X % "1 of 12800"}))
    for p in regimes(miss)])
def test_fused_8x8g32_mfma(hk, name, rows, regime, dt, check):
    def route(D):
        y = hk._fused_8x8_mfma(D["x"], *_args(D), hk._dtype_id(D["x"]))
        assert y is not None
        return y

    hold(route, name, regime, dt, rows, "fused 8x8 g32 mfma", check)


# ------------------------------------------------------------------ 8. generic kernel
@pytest.mark.parametrize("regime,dt", REG)
def test_generic_matmat(hk, regime, dt):
    hold(lambda D: hk.generic_matmat(D["x"], *_args(D)), "3x5g8_512x40", regime, dt, 2, "generic")


# ------------------------------------------------------------------ 9. mixture of experts (fp16): routed, routed packed, grouped, transposed
MOE_E, MOE_S, MOE_FIN, MOE_FOUT, MOE_G, MOE_TOP_K, MOE_TOKENS = 4, 1, 512, 64, 8, 2, 8
MOE_FIN_GROUPED = 960   # the shortest K the expert-grouped 16-row kernel takes (15 chunks of 64)


def _pow2_pair(t, s_layer, s_twin, clean):
    """A device tensor at the layer's shift and at the twin's, the low side rounded first (tests/magnitude.py); multiplying by a
    power of two is exact on the device as it is on the host."""
    lo = min(s_layer, s_layer if s_twin is None else s_twin)
    hi = max(s_layer, s_layer if s_twin is None else s_twin)
    low = (t.float() * 2.0 ** lo).to(torch.float16)
    if clean:
        low = torch.where(low.abs() < mg.MIN_NORMAL_F16, torch.zeros_like(low), low)
    high = (low.float() * 2.0 ** (hi - lo)).to(torch.float16)
    assert torch.isfinite(high).all() and torch.equal(high.float(), low.float() * 2.0 ** (hi - lo))
    if s_twin is None:
        return low.contiguous(), None
    return (low.contiguous(), high.contiguous()) if s_layer <= s_twin else (high.contiguous(), low.contiguous())


@functools.lru_cache(maxsize=None)
def _moe(regime, fin=MOE_FIN):
    """-> per side (layer, twin or None): (layers[e][s] = (codes, codebooks, scales, bias), x [tokens, in], gy [pairs, S, out]),
    and the router's ids.  ``plain_experts`` at the regime's shifts; x and gy share the activation's shift."""
    from tests import moe_experts as mx

    dev = torch.device(DEV)
    s = mg.regime_shifts(regime, 1, "float16")
    twin = s["b"] is not None
    clean = regime == "small_normal"
    base = mx.plain_experts(MOE_E, 4100, MOE_S, fin, MOE_FOUT, MOE_G, torch.float16, dev, bias=True)
    gen = torch.Generator(device=dev).manual_seed(4101)
    ids = mx.router_ids(MOE_TOKENS, MOE_TOP_K, MOE_E, gen, dev)
    acts = []
    for shape in ((MOE_TOKENS, fin), (MOE_TOKENS * MOE_TOP_K * MOE_S, MOE_FOUT)):
        a = torch.randn(shape, generator=gen, device=dev)
        if regime == "outlier":
            a[:, 3], a[:, shape[1] - 5] = mg.OUTLIER, -mg.OUTLIER
        acts.append(_pow2_pair(a, s["x"], s["x"] - s["a"] if twin else None, clean))
    sides = []
    for side in (0, 1):
        if side == 1 and not twin:
            sides.append(None)
            continue
        layers = []
        for per in base:
            row = []
            for codes, cb, sc, bias in per:
                cbp = _pow2_pair(cb, s["cb"][0], s["cb"][0] + s["b"] if twin else None, clean)
                scp = _pow2_pair(sc, s["sc"], s["sc"] + s["a"] - s["b"] if twin else None, clean)
                row.append((codes, cbp[side], scp[side], bias))
            layers.append(row)
        sides.append((layers, acts[0][side], acts[1][side].reshape(MOE_TOKENS * MOE_TOP_K, MOE_S, MOE_FOUT)))
    # The transposed launch rounds gy * scales ONCE into the storage type (its documented contract, tests/test_moe_grouped_bwd_gpu.py):
    # that intermediate is part of "nothing under- or overflows".  An entry of gy whose product with its expert's scale would
    # leave the normal range on either side is set to zero on both.
    for p, e in enumerate(ids.reshape(-1).tolist()):
        prods = [side[2][p, 0].float() * side[0][e][0][2].reshape(-1).float() for side in sides if side is not None]
        assert all(float(q.abs().max()) < 6e4 for q in prods)
        under = functools.reduce(torch.logical_or, [q.abs() < mg.MIN_NORMAL_F16 for q in prods])
        for side in sides:
            if side is not None:
                side[2][p, 0][under] = 0
    if regime in ("sub_codebook", "sub_x"):   # the builder's condition on the shifted operand
        ops = [l[0][1] for l in sides[0][0]] if regime == "sub_codebook" else [sides[0][1], sides[0][2]]
        for op in ops:
            sub = ((op.abs() > 0) & (op.abs() < mg.MIN_NORMAL_F16)).sum().item() / (op != 0).sum().item()
            assert sub >= mg.subnormal_share_floor(regime, 1), (regime, sub)
    return sides, ids


def _w64(layer):
    codes, cb, sc, _ = layer
    idx = codes.reshape(codes.shape[0], -1).long() & 0xFFFF
    return cb.double().reshape(65536, -1)[idx].reshape(codes.shape[0], -1) * sc.double().reshape(-1, 1)


def _moe_forward_oracle(side, ids):
    layers, x, _ = side
    flat = ids.reshape(-1).tolist()
    rows = [x[p // MOE_TOP_K].double() @ _w64(layers[e][0]).T + layers[e][0][3].double() for p, e in enumerate(flat)]
    y64 = torch.stack(rows).cpu().numpy()
    assert np.isfinite(y64).all() and np.abs(y64).max() < 6e4
    return y64


def _moe_hold(run, regime, what, transposed=False, fin=MOE_FIN, check="PT"):
    sides, ids = _moe(regime, fin)
    ys = [None if side is None else run(side, ids) for side in sides]
    if transposed:
        flat = ids.reshape(-1).tolist()
        layers, _, gy = sides[0]
        y64 = torch.stack([gy[p, 0].double() @ _w64(layers[e][0]) for p, e in enumerate(flat)]).cpu().numpy()
        assert np.isfinite(y64).all()
    else:
        y64 = _moe_forward_oracle(sides[0], ids)
    _hold(ys[0], ys[1], y64, torch.float16, f"{what} {regime} float16", check)


def _geometry(fin=MOE_FIN):
    return [MOE_E, MOE_S, MOE_FOUT, fin, MOE_G, MOE_TOP_K]


@pytest.mark.parametrize("regime", REG_F16)
def test_moe_routed_matvec(hk, regime):
    def run(side, ids):
        layers, x, _ = side
        table = hk.routed_table(layers, x.device)
        return hk.code1x16_moe_matmat(x, ids, table, _geometry(), False)[:, 0]

    _moe_hold(run, regime, "moe routed matvec")


@pytest.mark.parametrize("regime", REG_F16)
def test_moe_routed_packed_matvec(hk, regime):
    def run(side, ids):
        layers, x, _ = side
        packed = []
        for (codes, cb, sc, bias), in layers:
            pk = hk.prepack_1x16(codes, MOE_G, codebooks=cb, uniform_only=True)
            assert pk is not None and pk.desc.codebook_absmax == float(cb.abs().max()) > 0.0
            packed.append([(pk, cb, sc, bias)])
        assert hk.routed_packed_supported([row[0][0] for row in packed])
        table, tail = hk.routed_packed_table(packed, x.device)
        y = hk.code1x16_moe_matmat_packed(x, ids, table, _geometry() + tail, False)[:, 0]
        torch.cuda.synchronize()
        assert hk._ROUTED_PACKED_CELLS and all(int(torch.count_nonzero(c)) == 0 for c in hk._ROUTED_PACKED_CELLS.values())
        return y

    _moe_hold(run, regime, "moe routed packed matvec")


def _bucket(hk, ids, fin=MOE_FIN):
    P = ids.numel()
    tp = hk.grouped_tile_pairs(P, MOE_E)
    return hk.moe_bucket(ids, MOE_E, tp), _geometry(fin) + [tp, P]


@pytest.mark.parametrize("regime,check", regimes_f16({"sub_codebook": MFMA_SUB % ("the codebook", "1 of 1024")}))
def test_moe_grouped_gemm(hk, regime, check):
    def run(side, ids):
        layers, x, _ = side
        assert hk.grouped_supported(MOE_FOUT, MOE_FIN_GROUPED, MOE_G) and not hk.grouped_supported(MOE_FOUT, MOE_FIN, MOE_G)
        bucket, geometry = _bucket(hk, ids, MOE_FIN_GROUPED)
        return hk.code1x16_moe_matmat_grouped(x, bucket, hk.routed_table(layers, x.device), geometry, False)[:, 0]

    _moe_hold(run, regime, "moe grouped gemm", fin=MOE_FIN_GROUPED, check=check)


@pytest.mark.parametrize("regime,check", regimes_f16({"sub_codebook": MFMA_SUB % ("the codebook", "593 of 8192 fp32")}))
def test_moe_grouped_gemm_transposed(hk, regime, check):
    """grad_y plays the part of x; the output is fp32 and carries the storage type's bounds like the op's own tests.

    This launch is not "round once": by contract it rounds gy * scales into the storage type before the MFMA, so that product is
    part of "nothing under- or overflows".  ``_moe`` therefore edits the input, in every regime: an entry of gy whose product with
    its expert's scale would leave the fp16 normal range on either side is set to zero on both.  In ``sub_x`` that takes the
    smallest activations (|N(0, 1)| below about 2**-6, some 1 %) out of the only case with subnormal gy; the share condition on what
    remains is asserted."""
    def run(side, ids):
        layers, _, gy = side
        assert hk.grouped_transposed_supported(MOE_FOUT, MOE_FIN, MOE_G)
        bucket, geometry = _bucket(hk, ids)
        gx = hk.code1x16_moe_matmat_grouped_transposed(gy, bucket, hk.routed_table(layers, gy.device), geometry)
        assert gx.dtype == torch.float32
        return gx

    _moe_hold(run, regime, "moe grouped gemm transposed", transposed=True, check=check)
