"""The dense forward entries of include/aqlm_hip.h held to any y row stride and alignment, through the raw C ABI on the MI355X.

Every Python wrapper passes ``y_row_stride == out_features`` and a fresh allocation, so the branches the store sites keep for
hard layouts -- ``(M & 3, ys & 3, pointer & 7)`` choose between one 8-byte store and four guarded 2-byte stores -- and every
``Y + b0 * ys`` of the slab loops never see anything else in the rest of the suite.  Here each route runs in the six layouts of
tests/y_layout.py (gaps, odd strides, 2- / 4- / 6-byte offsets) at out_features 48, 45, 46, 47 (M & 3 = 0 .. 3: three 16-row
tiles, the last one ragged), both storage types, bias on for fp16 and off for bf16, and ``y_layout.check`` asserts, bit for bit:

  (a) nothing outside the batch x out_features windows was written (front pad, gaps, back pad keep the sentinel);
  (b) the windows equal the entry's own result in the ``flat`` layout (same inputs, same tuning).

No dense entry routes on y or y_row_stride (read off api / gemm_mfma / gemm_8x8 / gemm_1x16_scan / gemv / gemv_kx8_lut /
packed_gemv_entries: the kernel is chosen from the sizes, x, the codes' alignment and the tuning keys; y only reaches the stores),
so (b) holds for every entry.  The ``flat`` result itself is held to the fp64 oracle with the suite's ``check_close``.
Workspaces have exactly the advertised size with sentinels around them; accumulator cells must be zero at rest afterwards.

The library does not say which kernel ran: a test names its route by the tuning keys it sets (asserted to be in force) and the
shapes, batches and keys are those the routing code maps to that kernel (quoted at each test)."""
import contextlib
import ctypes
import functools
import types

import numpy as np
import pytest

from oracle import aqlm_oracle as orc
from tests import y_layout as yl
from tests.test_hip_parity import DEV, check_close, tdtype, to_dev

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

DTYPES = ["float16", "bfloat16"]
MS = [48, 45, 46, 47]
ALL = list(yl.LAYOUTS)
OFFSETS = ["flat", "off1", "off2", "off3"]     # single-row entries: no stride to vary
# the defaults aqlm_common.h names for the keys these tests touch
DEFAULTS = {"gemm_variant": 0, "kx8_xres": 1, "kx8_phase_tpb": 0, "kx8_phase_quads": 0, "kx8_ksplit": 0, "kx8_rt": 0,
            "kx8_mfma_min_rows": 2, "kx8_replicas": 1, "force_generic": 0, "packed_fused_finalize": 1, "packed_entry_bytes": 0}


@pytest.fixture(scope="module")
def nat():
    assert torch.cuda.is_available(), "run with -m gpu on the MI355X box"
    from aqlm_amd import _native

    for key, value in DEFAULTS.items():
        assert _native.get_tuning(key) == value, (key, _native.get_tuning(key))
    return _native


@pytest.fixture(scope="module")
def hk(nat):
    from aqlm_amd.inference_kernels import hip_kernel

    return hip_kernel


@contextlib.contextmanager
def tuning(nat, **keys):
    try:
        for key, value in keys.items():
            nat.set_tuning(key, value)
            assert nat.get_tuning(key) == value
        yield
    finally:
        for key in keys:
            nat.set_tuning(key, DEFAULTS[key])


@functools.lru_cache(maxsize=6)
def layer(K, nbits, g, fin, M, dt, batch):
    """One synthetic layer per (scheme, shape, dtype) with `batch` rows of x and their fp64 oracle; bias on for fp16, off for bf16."""
    fd = np.float16 if dt == "float16" else "bfloat16"
    L = orc.make_layer(9100 + 13 * K + nbits + g + fin + 7 * M, fin, M, K, nbits, g, batch=batch, bias=dt == "float16", float_dtype=fd)
    T = to_dev(L, tdtype(dt))
    y64 = orc.dequantize_gemm(L["x"], L["codes"], L["codebooks"], L["scales"], L["bias"])
    ptr = lambda t: None if t is None else t.data_ptr()
    return types.SimpleNamespace(L=L, T=T, y64=y64, K=K, nbits=nbits, g=g, fin=fin, M=M, dt=dt, dtype=tdtype(dt), batch=batch,
                                 dtid=0 if dt == "float16" else 1, codes=ptr(T["codes"]), cb=ptr(T["codebooks"]), scales=ptr(T["scales"]),
                                 bias=ptr(T["bias"]), x=ptr(T["x"]))


def stream():
    return torch.cuda.current_stream().cuda_stream


def values(bits, dtype):
    return torch.from_numpy(np.ascontiguousarray(bits).view(np.int16)).view(dtype).double().numpy()


def run(nat, call, win, ws_bytes=0, cells=False):
    """One call of an entry into a fresh sentinel buffer: call(y_ptr, ys, ws_ptr, ws_bytes) -> rc.  Returns the y buffer."""
    buf = torch.full((win.size,), yl.SENTINEL, dtype=torch.int16, device=DEV)
    ws = yl.Workspace(ws_bytes)
    wbuf = torch.empty((ws.size,), dtype=torch.uint8, device=DEV)
    ws.fill(wbuf, zero_inside=cells)
    rc = call(win.ptr(buf.data_ptr()), win.ys, ws.ptr(wbuf.data_ptr()), ws.nbytes)
    assert rc == 0, (rc, nat.last_error())
    torch.cuda.synchronize()
    yl.check_workspace(wbuf, ws_bytes, f"{win.layout} workspace of {ws_bytes} bytes", zero_at_rest=cells)
    return buf


def hold(nat, call, lay, B, what, ws_bytes=0, cells=False, layouts=ALL, y64=None):
    """The entry behind `call` in every layout: `flat` against the oracle, the others against `flat` and the sentinels.  Returns the
    flat result's bit patterns."""
    M = lay.M
    buf = run(nat, call, yl.Window("flat", B, M), ws_bytes, cells)
    base = yl.check(buf, "flat", B, M, yl.windows(buf, "flat", B, M), what)          # (a) for the flat layout: the two pads
    check_close(values(base, lay.dtype), lay.y64[:B] if y64 is None else y64, lay.dtype, f"{what}, {B} rows, flat")
    for layout in layouts:
        if layout != "flat":
            yl.check(run(nat, call, yl.Window(layout, B, M), ws_bytes, cells), layout, B, M, base, f"{what}, {B} rows")
    return base


# ================================================================================================ aqlm_hip_gemm_1x16_mfma
def gemm_1x16(nat, lay, B):
    return lambda y, ys, ws, n: nat.lib.aqlm_hip_gemm_1x16_mfma(lay.codes, lay.cb, lay.scales, lay.bias, lay.x, y, B, lay.M, lay.fin, lay.g,
                                                                lay.fin, ys, lay.dtid, ws, n, stream())


def ws_1x16(nat, lay, B):
    n = nat.lib.aqlm_hip_workspace_bytes(nat.OP_GEMM_1X16_MFMA, B, lay.M, lay.fin)
    assert n > 0
    return n


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("g", [8, 16])
def test_gemm_1x16_rows16(nat, g, M, dt):
    """gemm_variant 2: the 16-row blocks (gemm_rows16_body.h).  plan_rows16: 1792 features = 28 chunks, 4 per step up to 32 rows and
    2 above; 1024 features = 16 chunks, one per step up to 32 rows.  130 rows = a slab of 128 and one of 2 (Y + 128 * ys)."""
    with tuning(nat, gemm_variant=2):
        for fin in (1792, 1024):
            lay = layer(1, 16, g, fin, M, dt, 130)
            for B in (1, 16, 17, 33, 65, 130):
                hold(nat, gemm_1x16(nat, lay, B), lay, B, f"rows16 g{g} {fin}->{M} {dt}", ws_1x16(nat, lay, B))


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("g", [8, 16])
def test_gemm_1x16_pipeline(nat, g, M, dt):
    """gemm_variant 3: the LDS-DMA pipeline.  plan_glds: 192 features = 3 chunks, no K split, the block writes y itself
    (gemm_mfma.hip, epilogue of gemm_1x16_glds_kernel); 1024 features = two K slices, fp32 partials, gemm_glds_finalize_kernel."""
    with tuning(nat, gemm_variant=3):
        for fin in (192, 1024):
            lay = layer(1, 16, g, fin, M, dt, 130)
            for B in (1, 17, 33, 81, 130):
                hold(nat, gemm_1x16(nat, lay, B), lay, B, f"pipeline g{g} {fin}->{M} {dt}", ws_1x16(nat, lay, B))


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("g", [8, 16])
def test_gemm_1x16_register_staged(nat, g, M, dt):
    """gemm_variant 1: the register-staged kernel, partials [K slice][M][Bpad] with Bpad = rows rounded up to 32, and gemm_finalize_kernel."""
    with tuning(nat, gemm_variant=1):
        lay = layer(1, 16, g, 256, M, dt, 130)
        for B in (1, 33, 65, 97, 130):
            hold(nat, gemm_1x16(nat, lay, B), lay, B, f"register-staged g{g} 256->{M} {dt}", ws_1x16(nat, lay, B))


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("M", MS)
def test_gemm_1x16_scan(nat, M, dt):
    """The slice-scan kernel + its finalize (gemm_1x16_scan.hip): through aqlm_hip_gemm_1x16_mfma with gemm_variant 4 and through its own
    entry, each with exactly its advertised workspace; 256 features is the smallest input the plan takes."""
    lay = layer(1, 16, 8, 256, M, dt, 17)
    for B in (1, 8, 17):
        n = nat.lib.aqlm_hip_gemm_1x16_scan_workspace_bytes(B, M, 256)
        assert n == 8 * B * M * 4, n          # 8 codebook slices x one K chunk
        direct = lambda y, ys, ws, nb: nat.lib.aqlm_hip_gemm_1x16_scan(lay.codes, lay.cb, lay.scales, lay.bias, lay.x, y, B, M, 256, 256, ys,
                                                                       lay.dtid, ws, nb, stream())
        base = hold(nat, direct, lay, B, f"scan entry 256->{M} {dt}", n)
        with tuning(nat, gemm_variant=4):
            via = hold(nat, gemm_1x16(nat, lay, B), lay, B, f"scan through gemm_1x16_mfma 256->{M} {dt}", ws_1x16(nat, lay, B))
        assert np.array_equal(via, base), "gemm_variant 4 did not run the slice-scan kernel"


# ================================================================================================ aqlm_hip_gemm_kx8_mfma_ws
def gemm_kx8(nat, lay, B, workspace=True):
    if workspace:
        return lambda y, ys, ws, n: nat.lib.aqlm_hip_gemm_kx8_mfma_ws(lay.codes, lay.cb, lay.scales, lay.bias, lay.x, y, B, lay.M, lay.fin, lay.K, 8,
                                                                      lay.fin, ys, lay.dtid, ws, n, stream())
    return lambda y, ys, ws, n: nat.lib.aqlm_hip_gemm_kx8_mfma(lay.codes, lay.cb, lay.scales, lay.bias, lay.x, y, B, lay.M, lay.fin, lay.K, 8,
                                                               lay.fin, ys, lay.dtid, stream())


def ws_kx8(nat, lay, B):
    return nat.lib.aqlm_hip_workspace_bytes(nat.OP_GEMM_KX8_MFMA, B, lay.M, lay.fin)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("K", [1, 2])
def test_gemm_kx8_x_resident(nat, K, M, dt):
    """Default routing at <= 16 rows of 384 features: gemm_kx8_xres_kernel (xres_fits; three tiles, so never phased first)."""
    lay = layer(K, 8, 8, 384, M, dt, 16)
    for B in (1, 2, 7, 16):
        assert ws_kx8(nat, lay, B) == 0
        hold(nat, gemm_kx8(nat, lay, B), lay, B, f"x-resident {K}x8 384->{M} {dt}")


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("K", [1, 2])
def test_gemm_kx8_phased(nat, K, M, dt):
    """kx8_phase_tpb 1 .. 3 sends every <= 32-row call to gemm_kx8_xres_phased_kernel first; kx8_phase_quads 8 cuts the 17 quads of
    2176 features into three phases, the last one short.  <= 16 rows: one batch tile, 17+ rows: two.  The phased kernel's bits are
    the single-phase kernel's (same summation order), whatever the tiles per workgroup."""
    lay = layer(K, 8, 8, 2176, M, dt, 32)
    for B in (7, 16, 17, 32):
        bases = []
        for tpb in (1, 2, 3):
            with tuning(nat, kx8_phase_quads=8, kx8_phase_tpb=tpb):
                bases.append(hold(nat, gemm_kx8(nat, lay, B), lay, B, f"phased {K}x8 2176->{M} {dt}, {tpb} tiles per workgroup"))
        assert np.array_equal(bases[0], bases[1]) and np.array_equal(bases[0], bases[2])
        if B <= 16:   # default routing: the image of <= 16 rows fits the LDS at once, three tiles are never phased first
            assert np.array_equal(bases[0], hold(nat, gemm_kx8(nat, lay, B), lay, B, f"x-resident {K}x8 2176->{M} {dt}", layouts=["flat"]))


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("K", [1, 2])
def test_gemm_kx8_streaming(nat, K, M, dt):
    """kx8_xres 0: gemm_kx8_rows16_kernel at every row count.  plan_kx8: 384 features = steps of 2 chunks, 1024 features = steps of
    4 chunks up to 32 rows."""
    with tuning(nat, kx8_xres=0):
        for fin in (384, 1024):
            lay = layer(K, 8, 8, fin, M, dt, 65)
            for B in (3, 17, 40, 65):
                hold(nat, gemm_kx8(nat, lay, B), lay, B, f"streaming {K}x8 {fin}->{M} {dt}", ws_kx8(nat, lay, B))


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("K", [1, 2])
def test_gemm_kx8_k_split(nat, K, M, dt):
    """49+ rows with a workspace of exactly the advertised size and kx8_ksplit 2: two K slices of 3 steps (768 features), one or two row
    tiles per block, fp32 partials + gemm_glds_finalize_kernel; 130 rows = a split slab of 128 and an unsplit one of 2.  The
    no-workspace entry sums in another order: held to its own flat result, the sentinels and the oracle, not to the split form's bits."""
    lay = layer(K, 8, 8, 768, M, dt, 130)
    for B in (49, 130):
        n = ws_kx8(nat, lay, B)
        assert n == 4 * min(B, 128) * M * 4
        for rt in (1, 2):
            with tuning(nat, kx8_ksplit=2, kx8_rt=rt):
                hold(nat, gemm_kx8(nat, lay, B), lay, B, f"K split {K}x8 768->{M} {dt}, {rt} row tiles", n)
        hold(nat, gemm_kx8(nat, lay, B, workspace=False), lay, B, f"no workspace {K}x8 768->{M} {dt}")


# ================================================================================================ aqlm_hip_gemm_8x8_mfma
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("M", MS)
def test_gemm_8x8(nat, M, dt):
    """gemm_8x8g32_rows16_kernel: 1, 2 and 4 batch tiles; 65 rows = a slab of 64 and one of 1."""
    lay = layer(8, 8, 32, 2048, M, dt, 65)
    for B in (1, 3, 17, 33, 65):
        call = lambda y, ys, ws, n: nat.lib.aqlm_hip_gemm_8x8_mfma(lay.codes, lay.cb, lay.scales, lay.bias, lay.x, y, B, M, 2048, 32, 2048, ys,
                                                                   lay.dtid, stream())
        hold(nat, call, lay, B, f"8x8 g32 2048->{M} {dt}")


# ================================================================================================ matvec entries
GEMV_BATCHES = (1, 3, 7, 8)      # 7 rows = launches of 4 + 2 + 1 rows, each at y + done * ys


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("g", [8, 16])
def test_gemv_1x16(nat, g, M, dt):
    """aqlm_hip_gemv_1x16: 8 input groups = the fast kernel (gemv_body.h), 9 = the generic kernel, and force_generic on the fast shape."""
    for groups in (8, 9):
        lay = layer(1, 16, g, g * groups, M, dt, 8)
        call = lambda B: (lambda y, ys, ws, n: nat.lib.aqlm_hip_gemv_1x16(lay.codes, lay.cb, lay.scales, lay.bias, lay.x, y, M, lay.fin, g, B, lay.fin,
                                                                          ys, lay.dtid, stream()))
        for B in GEMV_BATCHES:
            hold(nat, call(B), lay, B, f"gemv 1x16 g{g} {lay.fin}->{M} {dt}")
            if groups == 8:
                with tuning(nat, force_generic=1):
                    hold(nat, call(B), lay, B, f"gemv 1x16 g{g} {lay.fin}->{M} {dt} force_generic")


def gemv_kx8(nat, lay, B):
    return lambda y, ys, ws, n: nat.lib.aqlm_hip_gemv_kx8(lay.codes, lay.cb, lay.scales, lay.bias, lay.x, y, lay.M, lay.fin, lay.K, lay.g, B, lay.fin,
                                                          ys, lay.dtid, stream())


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("M", MS)
def test_gemv_kx8(nat, M, dt):
    """aqlm_hip_gemv_kx8: 1x8 / 2x8 g8 on the plain LDS kernel (kx8_mfma_min_rows 0, kx8_replicas 0), the replicated-LDS kernel at one
    row (kx8_replicas 2), 8x8 g32, and 4x8 g16 (no tuned instance: the generic kernel)."""
    for K in (1, 2):
        lay = layer(K, 8, 8, 64, M, dt, 8)
        with tuning(nat, kx8_mfma_min_rows=0, kx8_replicas=0):
            for B in GEMV_BATCHES:
                hold(nat, gemv_kx8(nat, lay, B), lay, B, f"gemv {K}x8 g8 64->{M} {dt}")
        with tuning(nat, kx8_replicas=2):
            hold(nat, gemv_kx8(nat, lay, 1), lay, 1, f"gemv {K}x8 g8 64->{M} {dt} replicated", layouts=OFFSETS)
    for K, g, fin in ((8, 32, 256), (4, 16, 64)):
        lay = layer(K, 8, g, fin, M, dt, 8)
        for B in GEMV_BATCHES:
            hold(nat, gemv_kx8(nat, lay, B), lay, B, f"gemv {K}x8 g{g} {fin}->{M} {dt}")


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("M", MS)
def test_gemv_generic(nat, M, dt):
    lay = layer(3, 5, 8, 64, M, dt, 8)
    for B in GEMV_BATCHES:
        call = lambda y, ys, ws, n: nat.lib.aqlm_hip_gemv_generic(lay.codes, lay.cb, lay.scales, lay.bias, lay.x, y, M, 64, 3, 5, 8, B, 64, ys,
                                                                  lay.dtid, stream())
        hold(nat, call, lay, B, f"gemv generic 3x5 g8 64->{M} {dt}")


# ------------------------------------------------------------------------------------------------ 8x8 look-up-table matvec
LUT_G, LUT_IN = 8, 1024       # 128 input groups: one slab of the canonical layout, the planar layout's 128-group slab


def lut_layer(hk, M, dt):
    lay = layer(8, 8, LUT_G, LUT_IN, M, dt, 8)
    planar = hk.planar_8x8_pack(lay.T["codes"], LUT_G, codebooks=lay.T["codebooks"])
    assert planar is not None and planar.codebook_absmax > 0
    return lay, planar


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("M", MS)
def test_gemv_8x8_lut_batch(nat, hk, M, dt):
    """aqlm_hip_gemv_8x8_lut_batch, canonical and planar codes: row b writes y + b * ys and uses the cells [b * M, (b + 1) * M) of exactly
    batch * M * 8 bytes, zero at rest."""
    lay, planar = lut_layer(hk, M, dt)
    for is_planar, codes, absmax in ((0, lay.codes, 0.0), (1, planar.data_ptr(), planar.codebook_absmax)):
        for B in (2, 8):
            call = lambda y, ys, ws, n: nat.lib.aqlm_hip_gemv_8x8_lut_batch(codes, lay.cb, lay.scales, lay.bias, lay.x, y, M, LUT_IN, LUT_G, B, LUT_IN, ys,
                                                                            lay.dtid, is_planar, absmax, ws, n, stream())
            hold(nat, call, lay, B, f"lut batch planar={is_planar} {LUT_IN}->{M} {dt}", B * M * 8, cells=True)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("M", MS)
def test_gemv_8x8_lut_single_row(nat, hk, M, dt):
    """The single-row entries have no stride: offsets and the M tail.  Two-kernel form with exactly the advertised workspace (the
    query's batch argument carries the group size), single-kernel form with exactly M cells; canonical and planar codes."""
    lay, planar = lut_layer(hk, M, dt)
    n = nat.lib.aqlm_hip_workspace_bytes(nat.OP_GEMV_8X8_LUT, LUT_G, M, LUT_IN)
    assert n > 0 and n % (M * 4) == 0
    L = nat.lib
    two = lambda y, ys, ws, nb: L.aqlm_hip_gemv_8x8_lut(lay.codes, lay.cb, lay.scales, lay.bias, lay.x, y, M, LUT_IN, LUT_G, lay.dtid, ws, nb, stream())
    one = lambda y, ys, ws, nb: L.aqlm_hip_gemv_8x8_lut_fused(lay.codes, lay.cb, lay.scales, lay.bias, lay.x, y, M, LUT_IN, LUT_G, lay.dtid, ws, nb,
                                                               stream())
    ptwo = lambda y, ys, ws, nb: L.aqlm_hip_gemv_8x8_lut_planar(planar.data_ptr(), lay.cb, lay.scales, lay.bias, lay.x, y, M, LUT_IN, LUT_G, lay.dtid, 0.0,
                                                                ws, nb, 0, stream())
    pone = lambda y, ys, ws, nb: L.aqlm_hip_gemv_8x8_lut_planar(planar.data_ptr(), lay.cb, lay.scales, lay.bias, lay.x, y, M, LUT_IN, LUT_G, lay.dtid,
                                                                planar.codebook_absmax, ws, nb, 1, stream())
    hold(nat, two, lay, 1, f"lut {LUT_IN}->{M} {dt}", n, layouts=OFFSETS)
    hold(nat, one, lay, 1, f"lut fused {LUT_IN}->{M} {dt}", M * 8, cells=True, layouts=OFFSETS)
    hold(nat, ptwo, lay, 1, f"lut planar {LUT_IN}->{M} {dt}", n, layouts=OFFSETS)
    hold(nat, pone, lay, 1, f"lut planar fused {LUT_IN}->{M} {dt}", M * 8, cells=True, layouts=OFFSETS)


# ------------------------------------------------------------------------------------------------ packed 1x16
def packed_layer(nat, hk, M, dt, entry_bytes, fin=64):
    lay = layer(1, 16, 8, fin, M, dt, 8)
    with tuning(nat, packed_entry_bytes=entry_bytes):
        packed = hk.prepack_1x16(lay.T["codes"], 8, codebooks=lay.T["codebooks"])
    assert packed is not None and packed.desc.codebook_absmax > 0
    assert int(packed.desc.entry_bytes) == entry_bytes and not packed.desc.variable_geometry     # the route the test names
    return lay, packed


def packed_call(nat, lay, packed, B, cells=False):
    fn = nat.lib.aqlm_hip_gemv_1x16_packed_cells if cells else nat.lib.aqlm_hip_gemv_1x16_packed
    return lambda y, ys, ws, n: fn(ctypes.byref(packed.desc), packed.data_ptr(), lay.cb, lay.scales, lay.bias, lay.x, y, B, lay.fin, ys, lay.dtid, ws, n,
                                   stream())


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("entry_bytes", [3, 4])
def test_gemv_1x16_packed(nat, hk, entry_bytes, M, dt):
    """aqlm_hip_gemv_1x16_packed with the fused finalize (cells inside the packed buffer, no workspace: the epilogue of
    packed_gemv_kernels.h), with packed_fused_finalize 0 (exactly the advertised fp32 partials + gemv_1x16_packed_finalize), and
    aqlm_hip_gemv_1x16_packed_cells with exactly batch * M * 8 bytes of cells.  The three forms agree bit for bit."""
    lay, packed = packed_layer(nat, hk, M, dt, entry_bytes)
    for B in (1, 3, 8):
        what = f"packed 1x16 64->{M} {dt}, {int(packed.desc.entry_bytes)}-byte entries"
        fused = hold(nat, packed_call(nat, lay, packed, B), lay, B, what + ", fused finalize")
        n = nat.lib.aqlm_hip_workspace_bytes(nat.OP_GEMV_1X16_PACKED, B, M, 64)
        assert n == 16 * B * M * 4
        with tuning(nat, packed_fused_finalize=0):
            hold(nat, packed_call(nat, lay, packed, B), lay, B, what + ", finalize kernel", n)
        own = hold(nat, packed_call(nat, lay, packed, B, cells=True), lay, B, what + ", caller's cells", B * M * 8, cells=True)
        assert np.array_equal(own, fused)


# ================================================================================================ _multi entries into one buffer
SEGS = (45, 16, 47)             # q / k / v: the segments start at columns 0, 45 and 61 -- 2-byte aligned only
TOTAL = sum(SEGS)


def segment_array(nat, lays, y, ys, codes=None):
    segs = (nat.Segment * len(lays))()
    col = 0
    for k, (s, lay) in enumerate(zip(segs, lays)):
        s.codes, s.codebook, s.scales, s.bias = (lay.codes if codes is None else codes[k]), lay.cb, lay.scales, lay.bias
        s.y, s.y_row_stride, s.out_features = y + 2 * col, ys, lay.M
        col += lay.M
    return segs


def hold_multi(nat, multi, singles, lays, B, what, ws_bytes=0, cells=False, single_ws=None, layouts=ALL):
    """`multi(segs_for(y, ys), ws, n)` writes the segments side by side into ONE window of TOTAL columns; every segment's columns
    must equal that segment's single-entry flat result, everything else stays sentinel."""
    bases = []
    for k, (lay, single) in enumerate(zip(lays, singles)):
        n1, c1 = single_ws[k] if single_ws else (0, False)
        bases.append(hold(nat, single, lay, B, f"{what}, segment {k} alone", n1, cells=c1, layouts=["flat"], y64=lay.y64_shared[:B]))
    base = np.concatenate(bases, axis=1)
    assert base.shape == (B, TOTAL)
    for layout in layouts:
        win = yl.Window(layout, B, TOTAL)
        buf = run(nat, lambda y, ys, ws, n: multi(y, ys, ws, n), win, ws_bytes, cells)
        yl.check(buf, layout, B, TOTAL, base, f"{what}, {B} rows")


def shared_x_layers(K, nbits, g, fin, dt, batch):
    """Layers of SEGS rows that multiply the rows of x of the first one."""
    lays = [layer(K, nbits, g, fin, M + 0, dt, batch) for M in SEGS]
    lays = [types.SimpleNamespace(**vars(lay)) for lay in lays]
    for lay in lays:
        lay.x = lays[0].x
        lay.y64_shared = orc.dequantize_gemm(lays[0].L["x"], lay.L["codes"], lay.L["codebooks"], lay.L["scales"], lay.L["bias"])
    return lays


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("g", [8, 16])
def test_gemv_1x16_multi_into_one_buffer(nat, g, dt):
    fin = 8 * g
    lays = shared_x_layers(1, 16, g, fin, dt, 8)
    for B in GEMV_BATCHES:
        singles = [(lambda lay: lambda y, ys, ws, n: nat.lib.aqlm_hip_gemv_1x16(lay.codes, lay.cb, lay.scales, lay.bias, lay.x, y, lay.M, fin, g, B, fin,
                                                                               ys, lay.dtid, stream()))(lay) for lay in lays]
        multi = lambda y, ys, ws, n: nat.lib.aqlm_hip_gemv_1x16_multi(segment_array(nat, lays, y, ys), 3, lays[0].x, fin, g, B, fin, lays[0].dtid, stream())
        hold_multi(nat, multi, singles, lays, B, f"gemv_1x16_multi g{g} {dt}")


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("K", [1, 2])
def test_gemv_kx8_multi_into_one_buffer(nat, K, dt):
    """One row: the shared-input LDS kernel; 4 rows: ONE launch of the X-resident MFMA kernel over the three layers (KrSeg carries each
    layer's y and ys), bit-identical to the layers' own calls."""
    lays = shared_x_layers(K, 8, 8, 384, dt, 4)
    for B in (1, 4):
        singles = [gemv_kx8(nat, lay, B) for lay in lays]
        multi = lambda y, ys, ws, n: nat.lib.aqlm_hip_gemv_kx8_multi(segment_array(nat, lays, y, ys), 3, lays[0].x, 384, K, 8, B, 384, lays[0].dtid, stream())
        hold_multi(nat, multi, singles, lays, B, f"gemv_kx8_multi {K}x8 {dt}")


@pytest.mark.parametrize("dt", DTYPES)
def test_gemv_8x8_lut_multi_into_one_buffer(nat, hk, dt):
    """aqlm_hip_gemv_8x8_lut_multi (fp32 partials: exactly the sum of the segments' advertised bytes) and _planar_multi (single-kernel
    form: exactly sum(M) * 8 bytes of cells, zero at rest), one row of x."""
    lays = shared_x_layers(8, 8, LUT_G, LUT_IN, dt, 1)
    planars = [hk.planar_8x8_pack(lay.T["codes"], LUT_G, codebooks=lay.T["codebooks"]) for lay in lays]
    assert all(p is not None and p.codebook_absmax > 0 for p in planars)
    L, dtid, x = nat.lib, lays[0].dtid, lays[0].x
    ns = [L.aqlm_hip_workspace_bytes(nat.OP_GEMV_8X8_LUT, LUT_G, lay.M, LUT_IN) for lay in lays]
    singles = [(lambda lay: lambda y, ys, ws, n: L.aqlm_hip_gemv_8x8_lut(lay.codes, lay.cb, lay.scales, lay.bias, x, y, lay.M, LUT_IN, LUT_G, dtid, ws, n,
                                                                        stream()))(lay) for lay in lays]
    multi = lambda y, ys, ws, n: L.aqlm_hip_gemv_8x8_lut_multi(segment_array(nat, lays, y, ys), 3, x, LUT_IN, LUT_G, dtid, ws, n, stream())
    hold_multi(nat, multi, singles, lays, 1, f"gemv_8x8_lut_multi {dt}", sum(ns), single_ws=[(n, False) for n in ns], layouts=OFFSETS)
    absmax = (ctypes.c_float * 3)(*[p.codebook_absmax for p in planars])
    psingles = [(lambda lay, p: lambda y, ys, ws, n: L.aqlm_hip_gemv_8x8_lut_planar(p.data_ptr(), lay.cb, lay.scales, lay.bias, x, y, lay.M, LUT_IN, LUT_G,
                                                                                  dtid, p.codebook_absmax, ws, n, 1, stream()))(lay, p)
                for lay, p in zip(lays, planars)]
    pmulti = lambda y, ys, ws, n: L.aqlm_hip_gemv_8x8_lut_planar_multi(segment_array(nat, lays, y, ys, codes=[p.data_ptr() for p in planars]), absmax, 3, x,
                                                                      LUT_IN, LUT_G, dtid, ws, n, 1, stream())
    hold_multi(nat, pmulti, psingles, lays, 1, f"gemv_8x8_lut_planar_multi {dt}", TOTAL * 8, cells=True,
               single_ws=[(lay.M * 8, True) for lay in lays], layouts=OFFSETS)


@pytest.mark.parametrize("dt", DTYPES)
def test_gemv_1x16_packed_multi_into_one_buffer(nat, hk, dt):
    """aqlm_hip_gemv_1x16_packed_multi with the fused finalize (every descriptor carries its codebook range): one row = the pipe kernel
    over all segments, 3 rows = the shared-input kernel; bit-identical to aqlm_hip_gemv_1x16_packed per layer."""
    lays = shared_x_layers(1, 16, 8, 64, dt, 3)
    packs = []
    for lay in lays:
        with tuning(nat, packed_entry_bytes=4):
            packs.append(hk.prepack_1x16(lay.T["codes"], 8, codebooks=lay.T["codebooks"], uniform_only=True))
        assert packs[-1] is not None and packs[-1].desc.codebook_absmax > 0 and not packs[-1].desc.variable_geometry
    descs = (nat._descp * 3)(*[ctypes.pointer(p.desc) for p in packs])
    for B in (1, 3):
        singles = [packed_call(nat, lay, p, B) for lay, p in zip(lays, packs)]
        multi = lambda y, ys, ws, n: nat.lib.aqlm_hip_gemv_1x16_packed_multi(segment_array(nat, lays, y, ys, codes=[p.data_ptr() for p in packs]), descs, 3,
                                                                            lays[0].x, 64, B, 64, lays[0].dtid, None, 0, stream())
        hold_multi(nat, multi, singles, lays, B, f"gemv_1x16_packed_multi {dt}")
