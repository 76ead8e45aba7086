"""The dense forward entries of include/aqlm_hip.h held to any x row stride and alignment, through the raw C ABI on the MI355X: the
read side of tests/test_y_layout_gpu.py, whose route recipes -- the tuning keys asserted in force, the shapes, the row counts that the
routing code maps to each kernel -- are reused unchanged (imported, with their one-line justifications quoted at each test).

Python does not hide strides from the kernels: `hip_kernel._flat_rows` hands x through untouched when its last stride is 1, the
pointer is 16-byte aligned and stride(0) % 8 == 0, so a column slice of a fused projection, the last-token view hidden[:, -1, :],
x.expand(B, -1) and t.unfold(0, fin, 8) reach the C ABI with their own stride.  Here x lies in the layouts of tests/x_layout.py --
every element outside the union of the rows' windows is 0x7FFF, a NaN in fp16 and bf16 -- and y stays flat.  One out_features per
route, 45 (a ragged last tile); both storage types, bias on for fp16 and off for bf16.  Per route:

  (a)  gap8 / slice / overlap (16-byte aligned, stride % 8 == 0, below every routing limit): y is bit-identical to the same entry's
       result on the same values in the flat layout, no output is NaN, and the flat result is held to the fp64 oracle (check_close);
  (a') bcast (stride 0): the same, except on the K x 8 routes whose X-resident / phased kernels decline a stride of 0 -- there the
       call is held to the oracle and to the bits of a flat run pinned to the kernel that takes it (kx8_xres 0);
  (b)  odd / off1 / off2 / off4 (misaligned): the plain gemv entries and their _multi forms return 0 with the bits of their flat run
       under force_generic 1; every other entry returns its documented error code, leaves y untouched and names x in the message
       (aqlm_hip_gemv_1x16_packed_multi's codes and messages are pinned in tests/test_abi.py and not repeated);
  (c)  one row: x_row_stride is not read and selects no kernel -- in_features, 0, 7, in_features + 1, -8 and 2^40 give the flat bits;
  (d)  the last stride the X-resident and the phased K x 8 kernels accept and the first they decline, in 128 MiB buffers of NaNs;
  (e)  a slab of the register-staged 1x16 kernel whose last row lies past 4 GiB from x;
  (f)  arguments refused before any launch: a stride of 2^31 on the look-up-table batch entry, negative strides at 2 rows everywhere."""
import ctypes
import re
import types

import numpy as np
import pytest

from oracle import aqlm_oracle as orc
from tests import x_layout as xl
from tests import y_layout as yl
from tests.test_hip_parity import DEV, check_close
from tests.test_y_layout_gpu import (DTYPES, GEMV_BATCHES, LUT_G, LUT_IN, SEGS, TOTAL, hk, layer, lut_layer, nat, packed_layer,  # noqa: F401
                                     segment_array, shared_x_layers, stream, tuning, values)

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

M = 45                       # three 16-row tiles, the last one ragged
ONE_ROW_STRIDES = (None, 0, 7, "fin + 1", -8, 1 << 40)      # None: in_features
INVALID, UNSUPPORTED = -1, -2


# ------------------------------------------------------------------------------------------------ entries
def entry(name, lays, call, ws=lambda B: 0, cells=False, plain=False, err=(UNSUPPORTED, UNSUPPORTED), names_x=True, strided=True):
    """`call(B)(x, xs, y, ys, ws, n) -> rc`; `lays`: the layers side by side in y (one, or the segments of a _multi entry); `err`: the
    codes for a misaligned pointer and for a stride that is no multiple of 8; `plain`: accepts any 2-byte aligned x."""
    lays = lays if isinstance(lays, list) else [lays]
    return types.SimpleNamespace(name=name, lays=lays, lay=lays[0], call=call, ws=ws, cells=cells, plain=plain, err=err, names_x=names_x,
                                 strided=strided, M=sum(lay.M for lay in lays), fin=lays[0].fin, dt=lays[0].dt, dtype=lays[0].dtype)


def e_gemm_1x16(nat, lay):
    f = nat.lib.aqlm_hip_gemm_1x16_mfma
    return entry("aqlm_hip_gemm_1x16_mfma", lay,
                 lambda B: lambda x, xs, y, ys, ws, n: f(lay.codes, lay.cb, lay.scales, lay.bias, x, y, B, lay.M, lay.fin, lay.g, xs, ys, lay.dtid, ws, n, stream()),
                 ws=lambda B: nat.lib.aqlm_hip_workspace_bytes(nat.OP_GEMM_1X16_MFMA, B, lay.M, lay.fin))


def e_scan(nat, lay):
    f = nat.lib.aqlm_hip_gemm_1x16_scan
    return entry("aqlm_hip_gemm_1x16_scan", lay,
                 lambda B: lambda x, xs, y, ys, ws, n: f(lay.codes, lay.cb, lay.scales, lay.bias, x, y, B, lay.M, lay.fin, xs, ys, lay.dtid, ws, n, stream()),
                 ws=lambda B: nat.lib.aqlm_hip_gemm_1x16_scan_workspace_bytes(B, lay.M, lay.fin))


def e_gemm_kx8(nat, lay, workspace=True):
    if workspace:
        f = nat.lib.aqlm_hip_gemm_kx8_mfma_ws
        return entry("aqlm_hip_gemm_kx8_mfma_ws", lay,
                     lambda B: lambda x, xs, y, ys, ws, n: f(lay.codes, lay.cb, lay.scales, lay.bias, x, y, B, lay.M, lay.fin, lay.K, 8, xs, ys, lay.dtid, ws, n,
                                                             stream()),
                     ws=lambda B: nat.lib.aqlm_hip_workspace_bytes(nat.OP_GEMM_KX8_MFMA, B, lay.M, lay.fin))
    f = nat.lib.aqlm_hip_gemm_kx8_mfma
    return entry("aqlm_hip_gemm_kx8_mfma", lay,
                 lambda B: lambda x, xs, y, ys, ws, n: f(lay.codes, lay.cb, lay.scales, lay.bias, x, y, B, lay.M, lay.fin, lay.K, 8, xs, ys, lay.dtid, stream()))


def e_gemm_8x8(nat, lay):
    f = nat.lib.aqlm_hip_gemm_8x8_mfma
    return entry("aqlm_hip_gemm_8x8_mfma", lay,
                 lambda B: lambda x, xs, y, ys, ws, n: f(lay.codes, lay.cb, lay.scales, lay.bias, x, y, B, lay.M, lay.fin, 32, xs, ys, lay.dtid, stream()))


def e_gemv_1x16(nat, lay):
    f = nat.lib.aqlm_hip_gemv_1x16
    return entry("aqlm_hip_gemv_1x16", lay, plain=True,
                 call=lambda B: lambda x, xs, y, ys, ws, n: f(lay.codes, lay.cb, lay.scales, lay.bias, x, y, lay.M, lay.fin, lay.g, B, xs, ys, lay.dtid, stream()))


def e_gemv_kx8(nat, lay):
    f = nat.lib.aqlm_hip_gemv_kx8
    return entry("aqlm_hip_gemv_kx8", lay, plain=True,
                 call=lambda B: lambda x, xs, y, ys, ws, n: f(lay.codes, lay.cb, lay.scales, lay.bias, x, y, lay.M, lay.fin, lay.K, lay.g, B, xs, ys, lay.dtid,
                                                              stream()))


def e_gemv_generic(nat, lay):
    f = nat.lib.aqlm_hip_gemv_generic
    return entry("aqlm_hip_gemv_generic", lay, plain=True,
                 call=lambda B: lambda x, xs, y, ys, ws, n: f(lay.codes, lay.cb, lay.scales, lay.bias, x, y, lay.M, lay.fin, lay.K, lay.nbits, lay.g, B, xs, ys,
                                                              lay.dtid, stream()))


def e_lut_batch(nat, lay, planar=None):
    f = nat.lib.aqlm_hip_gemv_8x8_lut_batch
    codes, absmax = (lay.codes, 0.0) if planar is None else (planar.data_ptr(), planar.codebook_absmax)
    return entry(f"aqlm_hip_gemv_8x8_lut_batch planar={int(planar is not None)}", lay, cells=True, ws=lambda B: B * lay.M * 8, err=(UNSUPPORTED, INVALID),
                 call=lambda B: lambda x, xs, y, ys, ws, n: f(codes, lay.cb, lay.scales, lay.bias, x, y, lay.M, LUT_IN, LUT_G, B, xs, ys, lay.dtid,
                                                              int(planar is not None), absmax, ws, n, stream()))


def e_packed(nat, lay, packed, form="packed"):
    f = getattr(nat.lib, "aqlm_hip_gemv_1x16_" + form)
    head = lambda x, xs, y, ys, B, ws, n: (ctypes.byref(packed.desc), packed.data_ptr(), lay.cb, lay.scales, lay.bias, x, y, B, xs, ys, lay.dtid, ws, n)
    if form == "packed_chain":      # the hint names the layer itself as the next one
        call = lambda B: lambda x, xs, y, ys, ws, n: f(*head(x, xs, y, ys, B, ws, n), ctypes.byref(packed.desc), packed.data_ptr(), lay.cb, stream())
    else:
        call = lambda B: lambda x, xs, y, ys, ws, n: f(*head(x, xs, y, ys, B, ws, n), stream())
    cells = form == "packed_cells"
    return entry("aqlm_hip_gemv_1x16_" + form, lay, call, cells=cells, ws=(lambda B: B * lay.M * 8) if cells else (lambda B: 0), err=(INVALID, INVALID))


def e_gemv_1x16_multi(nat, lays):
    f, g, fin = nat.lib.aqlm_hip_gemv_1x16_multi, lays[0].g, lays[0].fin
    return entry("aqlm_hip_gemv_1x16_multi", lays, plain=True,
                 call=lambda B: lambda x, xs, y, ys, ws, n: f(segment_array(nat, lays, y, ys), 3, x, fin, g, B, xs, lays[0].dtid, stream()))


def e_gemv_kx8_multi(nat, lays):
    f, K, fin = nat.lib.aqlm_hip_gemv_kx8_multi, lays[0].K, lays[0].fin
    return entry("aqlm_hip_gemv_kx8_multi", lays, plain=True,
                 call=lambda B: lambda x, xs, y, ys, ws, n: f(segment_array(nat, lays, y, ys), 3, x, fin, K, 8, B, xs, lays[0].dtid, stream()))


def e_packed_multi(nat, lays, packs):
    f = nat.lib.aqlm_hip_gemv_1x16_packed_multi
    descs = (nat._descp * 3)(*[ctypes.pointer(p.desc) for p in packs])
    e = entry("aqlm_hip_gemv_1x16_packed_multi", lays, err=(INVALID, INVALID), names_x=False,
              call=lambda B: lambda x, xs, y, ys, ws, n: f(segment_array(nat, lays, y, ys, codes=[p.data_ptr() for p in packs]), descs, 3, x, lays[0].fin, B, xs,
                                                           lays[0].dtid, None, 0, stream()))
    e.keep = (descs, packs)
    return e


# ------------------------------------------------------------------------------------------------ running one call
def x_bits(lay, B):
    return lay.T["x"][:B].contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def oracle(e, rows):
    """fp64 result of the entry's layers on the rows `rows` (bit patterns), side by side as in y."""
    x = values(rows, e.dtype)
    return np.concatenate([orc.dequantize_gemm(x, lay.L["codes"], lay.L["codebooks"], lay.L["scales"], lay.L["bias"]) for lay in e.lays], axis=1)


def upload(buf):
    """The host buffer on the device, element 0 at an address == 16 mod 32 (x_layout.BASE_MOD32)."""
    t = torch.empty((8 + buf.size,), dtype=torch.int16, device=DEV)
    assert t.data_ptr() % 32 == 0
    t[8:].copy_(torch.from_numpy(buf.view(np.int16)))
    return t[8:]


def launch(nat, e, B, x_ptr, xs, rc_want=0):
    """One call with y flat in a sentinel buffer and exactly the advertised workspace.  -> the [B, M] bit patterns of y (rc 0); for
    an expected error: the code is `rc_want`, y is untouched, -> the message."""
    y = torch.full((B * e.M,), yl.SENTINEL, dtype=torch.int16, device=DEV)
    n = e.ws(B)
    ws = torch.zeros((max(n, 16),), dtype=torch.uint8, device=DEV)
    rc = e.call(B)(x_ptr, xs, y.data_ptr(), e.M, ws.data_ptr(), n)
    torch.cuda.synchronize()
    msg = nat.last_error() if rc else ""
    assert rc == rc_want, (e.name, B, xs, rc, msg)
    got = y.cpu().numpy().view(np.uint16).reshape(B, e.M)
    if rc_want == 0:
        if e.cells:
            assert not ws.any(), f"{e.name}: the cells are not zero at rest"
        return got
    assert (got == yl.SENTINEL).all(), f"{e.name}: refused with {rc}, yet y was written"
    return msg


def run(nat, e, rows, layout, stride=None, rc_want=0):
    placed = xl.place(rows, layout, stride)
    dev = upload(placed.buf)
    return launch(nat, e, rows.shape[0], placed.win.ptr(dev.data_ptr()), placed.win.xs, rc_want), placed


def flat(nat, e, rows, what, y64=None):
    """The entry on `rows` in the flat layout, held to the oracle."""
    base, placed = run(nat, e, rows, "flat")
    xl.check(base, base, placed.win, what, e.dt)          # no NaN
    check_close(values(base, e.dtype), oracle(e, rows) if y64 is None else y64, e.dtype, f"{what}, flat")
    return base


def misaligned(layout, B):
    offset, xs = xl.LAYOUTS[layout]
    return offset % 8 != 0 or (B > 1 and xs(64) % 8 != 0)


def hold(nat, e, B, what, bcast_declined=False):
    """(a), (a'), (b) for one entry under the tuning in force at `B` rows; (c) where B == 1."""
    what = f"{e.name}: {what}, {B} rows"
    rows = x_bits(e.lay, B)
    base = flat(nat, e, rows, what)
    generic = None
    for layout in xl.LAYOUTS:
        if layout == "flat" or (not e.strided and xl.LAYOUTS[layout][0] == 0):
            continue
        if misaligned(layout, B) and not e.plain:                                                      # (b), refused
            msg = run(nat, e, rows, layout, rc_want=e.err[0 if xl.LAYOUTS[layout][0] % 8 else 1])[0]
            assert not e.names_x or re.search(r"\bx\b", msg, re.I), (what, layout, msg)
            continue
        placed = xl.place(rows, layout)
        dev = upload(placed.buf)                                                                       # (alive until the call has run)
        got = launch(nat, e, B, placed.win.ptr(dev.data_ptr()), placed.win.xs)
        if misaligned(layout, B):                                                                      # (b), the generic kernel
            if generic is None:
                with tuning(nat, force_generic=1):
                    generic = flat(nat, e, rows, f"{what}, force_generic")
            xl.check(got, generic, placed.win, what, e.dt)
        elif layout == "bcast" and bcast_declined and B > 1:                                           # (a')
            check_close(values(got, e.dtype), oracle(e, placed.rows), e.dtype, f"{what}, bcast")
            with tuning(nat, kx8_xres=0):
                xl.check(got, flat(nat, e, placed.rows, f"{what}, rows of bcast, kx8_xres 0"), placed.win, what, e.dt)
        else:                                                                                          # (a)
            same = np.array_equal(placed.rows, rows)
            xl.check(got, base if same else flat(nat, e, placed.rows, f"{what}, rows of {layout}"), placed.win, what, e.dt)
    if B == 1 and e.strided:
        one_row(nat, e, what, base)
    return base


def one_row(nat, e, what, base=None):
    """(c): at one row x_row_stride is not read and selects no kernel."""
    rows = x_bits(e.lay, 1)
    base = flat(nat, e, rows, what) if base is None else base
    placed = xl.place(rows, "flat")
    dev = upload(placed.buf)
    for xs in ONE_ROW_STRIDES:
        xs = e.fin if xs is None else e.fin + 1 if xs == "fin + 1" else xs
        xl.check(launch(nat, e, 1, placed.win.ptr(dev.data_ptr()), xs), base, placed.win, f"{what}, one row, x_row_stride {xs}", e.dt)


# ================================================================================================ aqlm_hip_gemm_1x16_mfma
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("g", [8, 16])
def test_gemm_1x16_rows16(nat, g, dt):
    """gemm_variant 2: the 16-row blocks (gemm_rows16_body.h).  plan_rows16: 1792 features = 28 chunks, 4 per step up to 32 rows and
    2 above; 1024 features = 16 chunks, one per step up to 32 rows.  130 rows = a slab of 128 and one of 2 (X + 128 * xs)."""
    with tuning(nat, gemm_variant=2):
        for fin in (1792, 1024):
            e = e_gemm_1x16(nat, layer(1, 16, g, fin, M, dt, 130))
            for B in (1, 16, 17, 33, 65, 130):
                hold(nat, e, B, f"rows16 g{g} {fin}->{M} {dt}")


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("g", [8, 16])
def test_gemm_1x16_pipeline(nat, g, dt):
    """gemm_variant 3: the LDS-DMA pipeline.  plan_glds: 192 features = 3 chunks, no K split, the block writes y itself
    (gemm_mfma.hip, epilogue of gemm_1x16_glds_kernel); 1024 features = two K slices, fp32 partials, gemm_glds_finalize_kernel."""
    with tuning(nat, gemm_variant=3):
        for fin in (192, 1024):
            e = e_gemm_1x16(nat, layer(1, 16, g, fin, M, dt, 130))
            for B in (1, 17, 33, 81, 130):
                hold(nat, e, B, f"pipeline g{g} {fin}->{M} {dt}")


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("g", [8, 16])
def test_gemm_1x16_register_staged(nat, g, dt):
    """gemm_variant 1: the register-staged kernel, partials [K slice][M][Bpad] with Bpad = rows rounded up to 32, and gemm_finalize_kernel.
    X is read through a bounds-checked descriptor of the slab's extent ((rows - 1) * xs + in_features) * 2 bytes."""
    with tuning(nat, gemm_variant=1):
        e = e_gemm_1x16(nat, layer(1, 16, g, 256, M, dt, 130))
        for B in (1, 33, 65, 97, 130):
            hold(nat, e, B, f"register-staged g{g} 256->{M} {dt}")


@pytest.mark.parametrize("dt", DTYPES)
def test_gemm_1x16_scan(nat, dt):
    """The slice-scan kernel + its finalize (gemm_1x16_scan.hip): through aqlm_hip_gemm_1x16_mfma with gemm_variant 4 and through its own
    entry; 256 features is the smallest input the plan takes."""
    lay = layer(1, 16, 8, 256, M, dt, 17)
    for B in (1, 8, 17):
        base = hold(nat, e_scan(nat, lay), B, f"scan entry 256->{M} {dt}")
        with tuning(nat, gemm_variant=4):
            via = hold(nat, e_gemm_1x16(nat, lay), B, f"scan through gemm_1x16_mfma 256->{M} {dt}")
        assert np.array_equal(via, base), "gemm_variant 4 did not run the slice-scan kernel"


# ================================================================================================ aqlm_hip_gemm_kx8_mfma[_ws]
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("K", [1, 2])
def test_gemm_kx8_x_resident(nat, K, dt):
    """Default routing at <= 16 rows of 384 features: gemm_kx8_xres_kernel (xres_fits; three tiles, so never phased first).  A stride of
    0 is declined (xres_fits, try_phased: 0 < xs): the streaming kernel takes bcast."""
    e = e_gemm_kx8(nat, layer(K, 8, 8, 384, M, dt, 16))
    for B in (1, 2, 7, 16):
        assert e.ws(B) == 0
        hold(nat, e, B, f"x-resident {K}x8 384->{M} {dt}", bcast_declined=True)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("K", [1, 2])
def test_gemm_kx8_phased(nat, K, dt):
    """kx8_phase_tpb 1 .. 3 sends every <= 32-row call to gemm_kx8_xres_phased_kernel first; kx8_phase_quads 8 cuts the 17 quads of
    2176 features into three phases, the last one short.  <= 16 rows: one batch tile, 17+ rows: two."""
    e = e_gemm_kx8(nat, layer(K, 8, 8, 2176, M, dt, 32))
    for B in (7, 16, 17, 32):
        bases = []
        for tpb in (1, 2, 3):
            with tuning(nat, kx8_phase_quads=8, kx8_phase_tpb=tpb):
                bases.append(hold(nat, e, B, f"phased {K}x8 2176->{M} {dt}, {tpb} tiles per workgroup", bcast_declined=True))
        assert np.array_equal(bases[0], bases[1]) and np.array_equal(bases[0], bases[2])


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("K", [1, 2])
def test_gemm_kx8_streaming(nat, K, dt):
    """kx8_xres 0: gemm_kx8_rows16_kernel at every row count.  plan_kx8: 384 features = steps of 2 chunks, 1024 features = steps of
    4 chunks up to 32 rows."""
    with tuning(nat, kx8_xres=0):
        for fin in (384, 1024):
            e = e_gemm_kx8(nat, layer(K, 8, 8, fin, M, dt, 65))
            for B in (3, 17, 40, 65):
                hold(nat, e, B, f"streaming {K}x8 {fin}->{M} {dt}")


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("K", [1, 2])
def test_gemm_kx8_k_split(nat, K, dt):
    """49+ rows with a workspace of exactly the advertised size and kx8_ksplit 2: two K slices of 3 steps (768 features), one or two row
    tiles per block, fp32 partials + gemm_glds_finalize_kernel; 130 rows = a split slab of 128 and an unsplit one of 2 (X + 128 * xs).
    The no-workspace entry sums in another order: held to its own flat result."""
    lay = layer(K, 8, 8, 768, M, dt, 130)
    for B in (49, 130):
        for rt in (1, 2):
            with tuning(nat, kx8_ksplit=2, kx8_rt=rt):
                hold(nat, e_gemm_kx8(nat, lay), B, f"K split {K}x8 768->{M} {dt}, {rt} row tiles")
        hold(nat, e_gemm_kx8(nat, lay, workspace=False), B, f"no workspace {K}x8 768->{M} {dt}")


# ================================================================================================ 8x8
@pytest.mark.parametrize("dt", DTYPES)
def test_gemm_8x8(nat, dt):
    """gemm_8x8g32_rows16_kernel: 1, 2 and 4 batch tiles; 65 rows = a slab of 64 and one of 1 (X + 64 * xs)."""
    e = e_gemm_8x8(nat, layer(8, 8, 32, 2048, M, dt, 65))
    for B in (1, 3, 17, 33, 65):
        hold(nat, e, B, f"8x8 g32 2048->{M} {dt}")


@pytest.mark.parametrize("dt", DTYPES)
def test_gemv_8x8_lut_batch(nat, hk, dt):
    """aqlm_hip_gemv_8x8_lut_batch, canonical and planar codes: row b reads x + b * xs.  One row has its own case in
    test_one_row_ignores_the_stride."""
    lay, planar = lut_layer(hk, M, dt)
    for e in (e_lut_batch(nat, lay), e_lut_batch(nat, lay, planar)):
        for B in (2, 8):
            hold(nat, e, B, f"{LUT_IN}->{M} {dt}")


def lut_single_entries(nat, hk, dt):
    lay, planar = lut_layer(hk, M, dt)
    n = nat.lib.aqlm_hip_workspace_bytes(nat.OP_GEMV_8X8_LUT, LUT_G, M, LUT_IN)
    L = nat.lib
    args = lambda x, y: (lay.cb, lay.scales, lay.bias, x, y, M, LUT_IN, LUT_G, lay.dtid)
    mk = lambda name, call, ws, cells: entry(name, lay, lambda B: call, ws=lambda B: ws, cells=cells, strided=False)
    return [
        mk("aqlm_hip_gemv_8x8_lut", lambda x, xs, y, ys, ws, nb: L.aqlm_hip_gemv_8x8_lut(lay.codes, *args(x, y), ws, nb, stream()), n, False),
        mk("aqlm_hip_gemv_8x8_lut_fused", lambda x, xs, y, ys, ws, nb: L.aqlm_hip_gemv_8x8_lut_fused(lay.codes, *args(x, y), ws, nb, stream()), M * 8, True),
        mk("aqlm_hip_gemv_8x8_lut_planar", lambda x, xs, y, ys, ws, nb: L.aqlm_hip_gemv_8x8_lut_planar(planar.data_ptr(), *args(x, y), 0.0, ws, nb, 0, stream()),
           n, False),
        mk("aqlm_hip_gemv_8x8_lut_planar fused", lambda x, xs, y, ys, ws, nb: L.aqlm_hip_gemv_8x8_lut_planar(planar.data_ptr(), *args(x, y),
                                                                                                                planar.codebook_absmax, ws, nb, 1, stream()),
           M * 8, True),
    ]


@pytest.mark.parametrize("dt", DTYPES)
def test_gemv_8x8_lut_single_row(nat, hk, dt):
    """The single-row entries have no stride: a 16-byte aligned x at pointer & 31 == 16 gives the flat bits, a pointer that is not
    16-byte aligned is refused.  Two-kernel and single-kernel form, canonical and planar codes."""
    for e in lut_single_entries(nat, hk, dt):
        hold(nat, e, 1, f"{LUT_IN}->{M} {dt}")


# ================================================================================================ plain matvec entries
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("g", [8, 16])
def test_gemv_1x16(nat, g, dt):
    """aqlm_hip_gemv_1x16: 8 input groups = the fast kernel (gemv_body.h), 9 = the generic kernel.  7 rows = launches of 4 + 2 + 1 rows,
    each at x + done * xs.  Misaligned x: the generic kernel, whatever the shape."""
    for groups in (8, 9):
        e = e_gemv_1x16(nat, layer(1, 16, g, g * groups, M, dt, 8))
        for B in GEMV_BATCHES:
            hold(nat, e, B, f"g{g} {e.fin}->{M} {dt}")


@pytest.mark.parametrize("dt", DTYPES)
def test_gemv_kx8(nat, dt):
    """aqlm_hip_gemv_kx8: 1x8 / 2x8 g8 on the plain LDS kernel (kx8_mfma_min_rows 0, kx8_replicas 0), the replicated-LDS kernel at one
    row (kx8_replicas 2), 8x8 g32, and 4x8 g16 (no tuned instance: the generic kernel)."""
    for K in (1, 2):
        e = e_gemv_kx8(nat, layer(K, 8, 8, 64, M, dt, 8))
        with tuning(nat, kx8_mfma_min_rows=0, kx8_replicas=0):
            for B in GEMV_BATCHES:
                hold(nat, e, B, f"{K}x8 g8 64->{M} {dt}")
        with tuning(nat, kx8_replicas=2):
            hold(nat, e, 1, f"{K}x8 g8 64->{M} {dt} replicated")
    for K, g, fin in ((8, 32, 256), (4, 16, 64)):
        e = e_gemv_kx8(nat, layer(K, 8, g, fin, M, dt, 8))
        for B in GEMV_BATCHES:
            hold(nat, e, B, f"{K}x8 g{g} {fin}->{M} {dt}")


@pytest.mark.parametrize("dt", DTYPES)
def test_gemv_kx8_hands_rows_to_the_x_resident_kernel(nat, dt):
    """Default tuning, 3+ rows of 384 features: aqlm_hip_gemv_kx8 hands the call to aqlm_hip_gemm_kx8_mfma (kx8_mfma_min_rows 2), whose
    routing reads the stride; a misaligned x comes back AQLM_HIP_E_UNSUPPORTED from there and runs on the generic kernel."""
    for K in (1, 2):
        e = e_gemv_kx8(nat, layer(K, 8, 8, 384, M, dt, 16))
        for B in (3, 8):
            base = hold(nat, e, B, f"{K}x8 g8 384->{M} {dt}", bcast_declined=True)
            assert np.array_equal(base, flat(nat, e_gemm_kx8(nat, e.lay, workspace=False), x_bits(e.lay, B), "gemm_kx8_mfma"))


@pytest.mark.parametrize("dt", DTYPES)
def test_gemv_generic(nat, dt):
    e = e_gemv_generic(nat, layer(3, 5, 8, 64, M, dt, 8))
    for B in GEMV_BATCHES:
        hold(nat, e, B, f"3x5 g8 64->{M} {dt}")


# ================================================================================================ packed 1x16
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("entry_bytes", [3, 4])
def test_gemv_1x16_packed(nat, hk, entry_bytes, dt):
    """aqlm_hip_gemv_1x16_packed with the fused finalize and with packed_fused_finalize 0 (fp32 partials + finalize kernel),
    aqlm_hip_gemv_1x16_packed_cells, and aqlm_hip_gemv_1x16_packed_chain with the layer itself as the hinted next one.  The forms agree
    bit for bit."""
    lay, packed = packed_layer(nat, hk, M, dt, entry_bytes)
    n = lambda B: nat.lib.aqlm_hip_workspace_bytes(nat.OP_GEMV_1X16_PACKED, B, M, 64)
    for B in (1, 3, 8):
        what = f"64->{M} {dt}, {entry_bytes}-byte entries"
        fused = hold(nat, e_packed(nat, lay, packed), B, what + ", fused finalize")
        two = e_packed(nat, lay, packed)
        two.ws = n
        with tuning(nat, packed_fused_finalize=0):
            hold(nat, two, B, what + ", finalize kernel")
        assert np.array_equal(hold(nat, e_packed(nat, lay, packed, "packed_cells"), B, what), fused)
        assert np.array_equal(hold(nat, e_packed(nat, lay, packed, "packed_chain"), B, what), fused)


# ================================================================================================ _multi entries: one x, several segments
def lays_of(K, nbits, g, fin, dt, batch):
    lays = shared_x_layers(K, nbits, g, fin, dt, batch)
    assert tuple(lay.M for lay in lays) == SEGS and sum(SEGS) == TOTAL
    return lays


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("g", [8, 16])
def test_gemv_1x16_multi(nat, g, dt):
    e = e_gemv_1x16_multi(nat, lays_of(1, 16, g, 8 * g, dt, 8))
    for B in GEMV_BATCHES:
        hold(nat, e, B, f"g{g} {dt}")


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("K", [1, 2])
def test_gemv_kx8_multi(nat, K, dt):
    """One row: the shared-input LDS kernel; 4 rows: ONE launch of the X-resident MFMA kernel over the three layers, which declines a
    stride of 0 (xres_fits) -- bcast then runs layer by layer on the streaming kernel."""
    e = e_gemv_kx8_multi(nat, lays_of(K, 8, 8, 384, dt, 4))
    for B in (1, 4):
        hold(nat, e, B, f"{K}x8 {dt}", bcast_declined=True)


@pytest.mark.parametrize("dt", DTYPES)
def test_gemv_8x8_lut_multi(nat, hk, dt):
    """aqlm_hip_gemv_8x8_lut_multi (fp32 partials) and _planar_multi (single-kernel form), one row of x, no stride argument."""
    lays = lays_of(8, 8, LUT_G, LUT_IN, dt, 1)
    planars = [hk.planar_8x8_pack(lay.T["codes"], LUT_G, codebooks=lay.T["codebooks"]) for lay in lays]
    L, dtid = nat.lib, lays[0].dtid
    ns = sum(L.aqlm_hip_workspace_bytes(nat.OP_GEMV_8X8_LUT, LUT_G, lay.M, LUT_IN) for lay in lays)
    absmax = (ctypes.c_float * 3)(*[p.codebook_absmax for p in planars])
    multi = lambda x, xs, y, ys, ws, n: L.aqlm_hip_gemv_8x8_lut_multi(segment_array(nat, lays, y, ys), 3, x, LUT_IN, LUT_G, dtid, ws, n, stream())
    pmulti = lambda x, xs, y, ys, ws, n: L.aqlm_hip_gemv_8x8_lut_planar_multi(segment_array(nat, lays, y, ys, codes=[p.data_ptr() for p in planars]), absmax, 3,
                                                                            x, LUT_IN, LUT_G, dtid, ws, n, 1, stream())
    hold(nat, entry("aqlm_hip_gemv_8x8_lut_multi", lays, lambda B: multi, ws=lambda B: ns, strided=False), 1, dt)
    hold(nat, entry("aqlm_hip_gemv_8x8_lut_planar_multi", lays, lambda B: pmulti, ws=lambda B: TOTAL * 8, cells=True, strided=False), 1, dt)


def packed_multi_entry(nat, hk, dt, batch=3):
    lays = lays_of(1, 16, 8, 64, dt, batch)
    packs = []
    for lay in lays:
        with tuning(nat, packed_entry_bytes=4):
            packs.append(hk.prepack_1x16(lay.T["codes"], 8, codebooks=lay.T["codebooks"], uniform_only=True))
        assert packs[-1] is not None and packs[-1].desc.codebook_absmax > 0 and not packs[-1].desc.variable_geometry
    return e_packed_multi(nat, lays, packs)


@pytest.mark.parametrize("dt", DTYPES)
def test_gemv_1x16_packed_multi(nat, hk, dt):
    """aqlm_hip_gemv_1x16_packed_multi with the fused finalize: one row = the pipe kernel over all segments, 3 rows = the shared-input
    kernel."""
    e = packed_multi_entry(nat, hk, dt)
    for B in (1, 3):
        hold(nat, e, B, dt)


# ================================================================================================ (c) one row, every entry with a stride
def strided_entries(nat, hk, dt):
    lut, planar = lut_layer(hk, M, dt)
    pk, packed = packed_layer(nat, hk, M, dt, 4)
    return [e_gemm_1x16(nat, layer(1, 16, 8, 256, M, dt, 130)), e_scan(nat, layer(1, 16, 8, 256, M, dt, 17)),
            e_gemm_kx8(nat, layer(2, 8, 8, 384, M, dt, 16)), e_gemm_kx8(nat, layer(2, 8, 8, 384, M, dt, 16), workspace=False),
            e_gemm_8x8(nat, layer(8, 8, 32, 2048, M, dt, 65)), e_gemv_1x16(nat, layer(1, 16, 8, 64, M, dt, 8)),
            e_gemv_kx8(nat, layer(2, 8, 8, 64, M, dt, 8)), e_gemv_generic(nat, layer(3, 5, 8, 64, M, dt, 8)), e_lut_batch(nat, lut),
            e_lut_batch(nat, lut, planar), e_packed(nat, pk, packed), e_packed(nat, pk, packed, "packed_cells"),
            e_packed(nat, pk, packed, "packed_chain"), e_gemv_1x16_multi(nat, lays_of(1, 16, 8, 64, dt, 8)),
            e_gemv_kx8_multi(nat, lays_of(2, 8, 8, 384, dt, 4)), packed_multi_entry(nat, hk, dt)]


@pytest.mark.parametrize("dt", DTYPES)
def test_one_row_ignores_the_stride(nat, hk, dt):
    """At batch == 1, x_row_stride in_features, 0, 7, in_features + 1, -8 and 2^40 all give rc 0 and the flat bits, on every entry that
    takes a stride (torch reports arbitrary strides for a size-1 dimension, and `_flat_rows` passes them on).  Before the entries
    normalised the stride, the aqlm_hip_gemm_* entries returned AQLM_HIP_E_UNSUPPORTED at strides 7 and in_features + 1, and
    aqlm_hip_gemv_1x16 / _kx8 and their _multi forms ran the generic kernel -- whose bits equal the fast kernel's at these small
    shapes: test_one_row_stride_selects_no_kernel_where_the_kernels_differ has shapes that tell the two apart."""
    for e in strided_entries(nat, hk, dt):
        one_row(nat, e, f"{e.name} {dt}")


def test_one_row_stride_selects_no_kernel_where_the_kernels_differ(nat):
    """The fast matvec kernels and the generic kernel both sum in fp32 and round once, so their bits differ rarely: in none of the 45
    outputs of the small shapes above, which therefore cannot tell which kernel a one-row call ran.  At 512 features one output of
    these fp16 layers differs (asserted first: if a kernel change makes them agree, another shape has to be picked), and a one-row
    call at stride 7 or in_features + 1 must give the fast kernel's bits.  The library before the stride was ignored at one row gave
    the generic kernel's here.  1x8 / 2x8 g8 layers show no such output at any width up to 2048: on aqlm_hip_gemv_kx8[_multi] the
    route of those schemes is not observable through the result."""
    for e in (e_gemv_1x16(nat, layer(1, 16, 8, 512, M, "float16", 8)), e_gemv_1x16_multi(nat, lays_of(1, 16, 8, 512, "float16", 8)),
              e_gemv_kx8(nat, layer(8, 8, 32, 512, M, "float16", 8))):
        rows = x_bits(e.lay, 1)
        fast = flat(nat, e, rows, e.name)
        with tuning(nat, force_generic=1):
            generic = flat(nat, e, rows, e.name + ", force_generic")
        assert not np.array_equal(fast, generic), f"{e.name}: 512 features no longer tell the generic kernel from the fast one"
        one_row(nat, e, f"{e.name} 512->{e.M} float16", fast)


# ================================================================================================ (d) stride limits of the K x 8 route
def big_buffer(rows, xs):
    """`rows` ([B, fin] bit patterns) at stride `xs` in a device buffer of NaN patterns, written in place.  -> (buffer, x pointer)"""
    B, fin = rows.shape
    win = xl.Window("flat", B, fin, stride=xs)
    t = torch.full((8 + win.size,), xl.POISON, dtype=torch.int16, device=DEV)
    assert t.data_ptr() % 32 == 0
    buf, dev_rows = t[8:], torch.from_numpy(rows.view(np.int16)).to(DEV)
    for b in range(B):
        buf[win.row(b):win.row(b) + fin] = dev_rows[b]
    return buf, win.ptr(buf.data_ptr()), win


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("K", [1, 2])
def test_kx8_stride_limits(nat, K, dt):
    """xres_fits takes the X-resident kernel for 0 < xs < 2^22, try_phased the phased kernel for 0 < xs < 2^21; both form a row's address
    as a 24-bit by 8-bit multiply of the byte stride.  The last stride each guard accepts runs that kernel (the bits of the flat run of
    the same recipe), the first it declines runs the streaming kernel (the bits of the flat run under kx8_xres 0); each is held to the
    oracle.  Where two kernels give the same bits the case cannot tell which one ran; it still holds.  Buffers of 128 MiB of NaNs."""
    e = e_gemm_kx8(nat, layer(K, 8, 8, 384, M, dt, 16))                       # the x-resident recipe: 384 features, 16 rows, default tuning
    rows = x_bits(e.lay, 16)
    with tuning(nat, kx8_xres=0):
        streaming = flat(nat, e, rows, f"streaming {K}x8 384 {dt}")
    resident = flat(nat, e, rows, f"x-resident {K}x8 384 {dt}")
    for xs, want in (((1 << 22) - 8, resident), (1 << 22, streaming)):
        buf, x, win = big_buffer(rows, xs)
        assert buf.numel() * 2 <= 128 << 20
        xl.check(launch(nat, e, 16, x, xs), want, win, f"{K}x8 {dt}, 16 rows", dt)
        del buf
    e = e_gemm_kx8(nat, layer(K, 8, 8, 2176, M, dt, 32))                      # the phased recipe of the y file
    rows = x_bits(e.lay, 32)
    with tuning(nat, kx8_xres=0):
        streaming = flat(nat, e, rows, f"streaming {K}x8 2176 {dt}")
    with tuning(nat, kx8_phase_quads=8, kx8_phase_tpb=1):
        phased = flat(nat, e, rows, f"phased {K}x8 2176 {dt}")
        for xs, want in (((1 << 21) - 8, phased), (1 << 21, streaming)):
            buf, x, win = big_buffer(rows, xs)
            assert buf.numel() * 2 <= 128 << 20
            xl.check(launch(nat, e, 32, x, xs), want, win, f"{K}x8 {dt}, 32 rows, kx8_phase_tpb 1", dt)
            del buf


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("K", [1, 2])
def test_gemv_kx8_multi_at_the_last_token_stride(nat, K, dt):
    """hidden[:, -1, :] of a [4, 1024, 4096] tensor: a stride of 2^22, the first the shared-input X-resident launch declines."""
    e = e_gemv_kx8_multi(nat, lays_of(K, 8, 8, 384, dt, 4))
    rows = x_bits(e.lay, 4)
    buf, x, win = big_buffer(rows, 1 << 22)
    got = launch(nat, e, 4, x, 1 << 22)
    xl.check(got, got, win, e.name, dt)
    check_close(values(got, e.dtype), oracle(e, rows), e.dtype, f"{e.name} {K}x8 {dt}, xs 2^22")


# ================================================================================================ (e) rows past 4 GiB from x
@pytest.mark.parametrize("B", [128, 130])
def test_register_staged_rows_past_4_gib(nat, B):
    """gemm_variant 1, g8, 256 -> 45, fp16, x_row_stride 2^24 + 2^18: row 127 starts 4 327 997 440 bytes behind x.  The kernel forms a
    row's offset in 32 bits behind a bounds-checked descriptor whose extent the host clamps to 2^32 - 1, so a wrapped offset stays
    inside the buffer and reads NaNs or another row: a wrong kernel fails by value, not by a fault.  The host cuts such a slab into
    sub-slabs whose extent fits 32 bits (here 127 + 1 rows); 130 rows add the slab step X + 128 * xs, Y + 128 * ys.  One buffer of
    about 4.4 GB of NaNs, rows written in place, freed at the end.  Against the library before the cut every output was NaN, from
    row 0 on: with the extent clamped to 2^32 - 1 the offset 0xfffffff0, at which the kernel expects zeros for k past its slice, is
    in range for three of its four dwords (the descriptor checks dword by dword) and read the NaNs of a gap; and row 127 wrapped to
    offset 33 030 144, the gap between rows 0 and 1.  The cut keeps every extent <= 0xfffffff0."""
    xs = (1 << 24) + (1 << 18)
    with tuning(nat, gemm_variant=1):
        e = e_gemm_1x16(nat, layer(1, 16, 8, 256, M, "float16", 130))
        rows = x_bits(e.lay, B)
        base = flat(nat, e, rows, f"register-staged g8 256->{M}, {B} rows", y64=e.lay.y64[:B])
        assert 2 * 127 * xs > 1 << 32 > 2 * 126 * xs + 512
        buf, x, win = big_buffer(rows, xs)
        try:
            xl.check(launch(nat, e, B, x, xs), base, win, f"register-staged, {B} rows", "float16")
        finally:
            del buf
            torch.cuda.empty_cache()


# ================================================================================================ (f) refused before any launch
@pytest.mark.parametrize("dt", DTYPES)
def test_refused_strides(nat, hk, dt):
    """Two rows, a small real buffer; nothing is read past it because nothing runs.  A negative stride: AQLM_HIP_E_INVALID on every
    entry, from the one shared check (check_x_row_stride); 2^31 on the look-up-table batch entry, whose kernel takes the stride as
    an int: AQLM_HIP_E_INVALID."""
    for e in strided_entries(nat, hk, dt):
        rows = x_bits(e.lay, 2)
        placed = xl.place(rows, "flat")
        dev = upload(placed.buf)
        for xs in (-8, -e.fin, -1):
            msg = launch(nat, e, 2, placed.win.ptr(dev.data_ptr()), xs, rc_want=INVALID)
            assert "negative x_row_stride" in msg and e.name.split()[0].replace("_ws", "").replace("_cells", "").replace("_chain", "") in msg, msg
        if "lut_batch" in e.name:
            msg = launch(nat, e, 2, placed.win.ptr(dev.data_ptr()), 1 << 31, rc_want=INVALID)
            assert "x_row_stride" in msg, msg
