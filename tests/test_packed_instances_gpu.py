"""Instances of the packed 1x16 matvec (gemv_1x16_packed_body, aqlm_amd/csrc/packed_gemv_kernels.h) that ship in the library and that
no other GPU test runs:

  1. buffers packed with more than one x copy (`packed_xcopies` 2..4): the copy correction of the multi-row kernels, the reciprocal
     division of the 3-byte form, the XC-fold x fill, the slot -> j recovery of unpack and dequantise-from-packed, and the shared-input,
     routed and captured launches on such buffers;
  2. ring depths 4 and 8 at one row (`packed_prefetch`), at step counts that take the loop's remainder only, exactly one turn, one
     turn + 1 and at least two turns + 1;
  3. `packed_fill_rotate` = 0;
  4. the chain entry aqlm_hip_gemv_1x16_packed_chain with its prefetch waves (`packed_prefetch_waves`).

Random layers are oracle.aqlm_oracle.make_layer's, the reference is orc.dequantize_gemm in fp64, the tolerances are check_close and
check_rounded of tests/test_hip_parity.py; "same bits" is torch.equal on the raw 16-bit patterns.  Layers are built once per module
and shared by the cases; every tuning key a test sets is restored by `tuned` (tests/test_group_fold_gpu.py)."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import aqlm_oracle as orc
from tests import packed_model as pm
from tests.test_compact_window_host import COMPACT, FULL
from tests.test_group_fold_gpu import PackedLayer, bits, run_folded, tuned
from tests.test_hip_parity import DEV, check_close, check_rounded, tdtype, to_dev

pytestmark = pytest.mark.gpu


def _hk():
    assert torch.cuda.is_available(), "run with -m gpu on the MI355X box"
    from aqlm_amd.inference_kernels import hip_kernel

    return hip_kernel


def _native():
    from aqlm_amd import _native as native

    return native


def x_stride(in_groups):
    """pk_x_stride of packed_format.h, restated"""
    return ((in_groups + 1 + 11) & ~15) + 4


def max_x_copies(in_groups):
    return max(1, min(4, 4095 // x_stride(in_groups)))


def x_image_bytes(in_groups, copies):
    return ((copies - 1) * x_stride(in_groups) + in_groups + 1) * 16


_REFS = {}


class OracleLayer(PackedLayer):
    """A PackedLayer whose codes, codebook, scales, bias and input rows are make_layer's (so that the fp64 oracle applies), prepacked
    under the tuning keys given.  `x` / `y` are what PackedLayer.launch and run_folded use: row 0 and a one-row output."""

    def __init__(self, fin, fout, seed, dtype=torch.float16, rows=8, bias=True, codes_unsigned=None, relabel=True, uniform_only=False,
                 **keys):
        hk = _hk()
        self.key = (seed, fin, fout, dtype, rows, bias, codes_unsigned is not None)
        L = orc.make_layer(seed, fin, fout, 1, 16, 8, batch=rows, bias=bias, float_dtype=np.float16 if dtype == torch.float16 else "bfloat16")
        if codes_unsigned is not None:
            cu = np.asarray(codes_unsigned, dtype=np.int64).reshape(fout, fin // 8, 1)
            L = dict(L, codes=orc.pack_int_data(cu, 16), codes_unsigned=cu)
        T = to_dev(L, dtype)
        self.L, self.fin, self.fout, self.dtype = L, fin, fout, dtype
        self.codes, self.codebooks, self.scales, self.bias = T["codes"], T["codebooks"], T["scales"], T["bias"]
        self.xs = T["x"]
        self.x = self.xs[:1]
        self.y = torch.zeros((1, fout), device=DEV, dtype=dtype)
        self.cells = None
        with tuned(**keys):
            self.packed = hk.prepack_1x16(self.codes, 8, codebooks=self.codebooks, relabel=relabel, uniform_only=uniform_only)
        assert self.packed is not None and self.packed.desc.codebook_absmax > 0

    def y64(self):
        """fp64 oracle of all input rows, computed once per (layer data) and left unchanged"""
        if self.key not in _REFS:
            L = self.L
            _REFS[self.key] = orc.dequantize_gemm(L["x"], L["codes"], L["codebooks"], L["scales"], L["bias"])
        return _REFS[self.key]

    def run(self, x):
        return _hk().code1x16_matmat_packed(x, self.packed, self.codebooks, self.scales, self.bias)

    def layout(self):
        d = self.packed.desc
        groups = list(d.slice_groups)[:16] if d.variable_geometry else None
        return pm.layout(self.fout, self.fin // 8, int(d.waves), int(d.steps), int(d.entry_bytes), groups, d.relabelled)

    def cells_in_buffer(self):
        lay = self.layout()
        return self.packed.buf[lay["off_acc"]:lay["off_ent"]]


_LAYERS = {}


def layer(*args, **kw):
    """OracleLayer(*args, **kw), built once per module"""
    key = (args, tuple(sorted((k, v if not isinstance(v, np.ndarray) else id(v)) for k, v in kw.items())))
    if key not in _LAYERS:
        _LAYERS[key] = OracleLayer(*args, **kw)
    return _LAYERS[key]


def did(dtype):
    return _native().F16 if dtype == torch.float16 else _native().BF16


# ------------------------------------------------------------------ 1. buffers with several x copies
# inputs -> copies the format allows: 512, 1024, 2048, 4096: 4; 8192: 3; 11008: 2; 16384: 1 (the key is ignored).  1024 -> 300 has a
# ragged last row group (19 rows per group, 15 in the last), 512 -> 1000 several hundred rows.  bfloat16 on shapes of >= 300 rows:
# check_rounded wants 99.5 % of a row's outputs bit-equal to the rounded oracle, which 64 outputs can only meet with all of them.
# These all run one step per wave; 4096 -> 2200 at four waves per workgroup (pinned at repack) runs five, so the loops of the one-row
# and of the multi-row kernels take a whole turn and a remainder on entries that name copies (4 copies asked for only).
XC_SHAPES = [(512, 96, "float16"), (1024, 300, "float16"), (2048, 96, "float16"), (4096, 128, "float16"), (8192, 96, "float16"),
             (11008, 96, "float16"), (16384, 96, "float16"), (512, 1000, "float16"), (1024, 300, "bfloat16"), (512, 1000, "bfloat16"),
             (4096, 2200, "float16")]
ALLOWED = {512: 4, 1024: 4, 2048: 4, 4096: 4, 8192: 3, 11008: 2, 16384: 1}
XC_WAVES = {(4096, 2200): 4}
XC_CASES = [(fin, fout, dt, xc, eb) for fin, fout, dt in XC_SHAPES for xc in ((4,) if fin == 16384 or (fin, fout) in XC_WAVES else (2, 3, 4))
            for eb in (3, 4)]
XC_IDS = [f"{fin}-{fout}-{dt}-xc{xc}-eb{eb}" for fin, fout, dt, xc, eb in XC_CASES]


def xc_layer(fin, fout, dt, xc, eb, **kw):
    if (fin, fout) in XC_WAVES:
        kw = dict(kw, packed_waves=XC_WAVES[(fin, fout)])
    return layer(fin, fout, 5000 + fin + fout, tdtype(dt), packed_xcopies=xc, packed_entry_bytes=eb, **kw)


@pytest.mark.parametrize("fin,fout,dt,xc,eb", XC_CASES, ids=XC_IDS)
def test_x_copies_buffer_is_well_formed_and_lossless(fin, fout, dt, xc, eb):
    hk, native = _hk(), _native()
    lay = xc_layer(fin, fout, dt, xc, eb)
    packed, d = lay.packed, lay.packed.desc
    in_groups = fin // 8
    allowed = max_x_copies(in_groups)
    assert allowed == ALLOWED[fin]
    assert int(d.x_copies) == min(xc, allowed), f"{fin} inputs, {xc} copies asked for: the descriptor says {d.x_copies}"
    assert not d.variable_geometry and int(d.entry_bytes) == eb
    G = pm.decode_device_buffer(packed.buf.cpu().numpy(), fout, fin, int(d.waves), int(d.steps), eb, None, d.relabelled)
    j, copy = G["j"], G["copy"]
    assert G["spare_ok"], "the copy bits of an entry are not slot // stride"
    assert int(j.max()) == in_groups and int(copy[j == in_groups].max()) == 0, "a null entry names a copy other than 0"
    assert int(j[j != in_groups].max()) < in_groups and int(copy.max()) < int(d.x_copies)
    hist = np.bincount(copy[j != in_groups].ravel().astype(np.int64), minlength=4)
    print(f"x copies {fin}->{fout} {dt} asked {xc} got {d.x_copies} entry bytes {eb} waves {d.waves} steps {d.steps} "
          f"relabelled {int(d.relabelled)}: entries per copy {hist.tolist()}")
    if int(d.x_copies) > 1:
        assert int(hist[1:].sum()) > 0, "no entry names a copy other than 0: the buffer does not exercise the mechanism"
        assert int(hist[int(d.x_copies) - 1]) > 0, "the highest copy is never named: take another shape"
    assert int(d.steps) == (5 if (fin, fout) in XC_WAVES else 1)
    # the payload as the device holds it, walked like the kernel walks it, gives the codes back
    payload = ((j.astype(np.int64) + pm.XB) << 16) | G["code"]
    Pg = dict(M=fout, in_groups=in_groups, NW=int(d.waves), T=int(d.steps), RG=int(d.rows_per_group), ent=payload, mask=G["mask"],
              frow=G["frow"], winfo=G["winfo"], rowstart=G["rowstart"], geom=pm.Geometry(fout), old_of_new=G.get("old_of_new"))
    np.testing.assert_array_equal(pm.unpack(Pg), lay.L["codes_unsigned"][:, :, 0])
    # ... and so do the unpack kernel (both entry sizes: both j-recovery rules) and a re-attached descriptor
    assert torch.equal(hk.unpack_1x16(packed), lay.codes)
    again = hk.PackedCodes.from_buffer(packed.buf.clone())
    assert int(again.desc.x_copies) == int(d.x_copies)
    assert torch.equal(hk.unpack_1x16(again), lay.codes)
    # dequantise-from-packed: the bits of the dequantise from canonical codes
    for s in (None, lay.scales):
        W = hk.dequant_1x16_packed(packed, lay.codebooks, s)
        assert torch.equal(bits(W), bits(hk.code1x16_dequant(lay.codes, lay.codebooks, s))), f"scaled={s is not None}"
    # compact window exactly when the x image with all its copies fits it (4-byte entries, default ring depth)
    image = x_image_bytes(in_groups, int(d.x_copies))
    lds, win = native.packed_image(d, 1, did(lay.dtype))
    assert win == (COMPACT if eb == 4 and image <= COMPACT else FULL), f"x image of {image} bytes, window {win}"
    assert native.packed_image(d, 2, did(lay.dtype))[1] == 0   # more than one row: slice first, planes behind it


def test_x_image_sizes_at_the_window_edge():
    """1024 inputs: 3 copies are 6288 bytes (compact), 4 are 8400 (full; the limit is 8208); 2048 inputs with 2 copies: 8272 (full);
    512 inputs with 4 copies: 4304.  The buffers of these sizes are among the cases above and below."""
    assert (x_image_bytes(128, 3), x_image_bytes(128, 4), x_image_bytes(256, 2), x_image_bytes(64, 4)) == (6288, 8400, 8272, 4304)
    native = _native()
    for fin, fout, xc, window in ((1024, 300, 3, COMPACT), (1024, 300, 4, FULL), (2048, 96, 2, FULL), (512, 96, 4, COMPACT)):
        d = xc_layer(fin, fout, "float16", xc, 4).packed.desc
        assert int(d.x_copies) == xc and native.packed_image(d, 1)[1] == window, (fin, xc)


@pytest.mark.parametrize("fin,fout,dt,xc,eb", XC_CASES, ids=XC_IDS)
def test_x_copies_matvec(fin, fout, dt, xc, eb):
    hk = _hk()
    lay = xc_layer(fin, fout, dt, xc, eb)
    dtype, y64, x = lay.dtype, lay.y64(), lay.xs
    what = f"{fin}->{fout} {dt} x copies {lay.packed.desc.x_copies} entry bytes {eb}"

    def one_row(tag):
        y1 = lay.run(x[:1])
        m = check_close(y1.float().cpu().numpy(), y64[:1], dtype, f"{what} {tag}")
        exact = check_rounded(y1.float().cpu().numpy(), y64[:1], dtype, f"{what} {tag}")
        print(f"{what} {tag}: mean-rel {m:.3e}, {exact:.4f} of the outputs equal the rounded oracle")
        assert torch.equal(lay.run(torch.zeros_like(x[:1]))[0], lay.bias), f"{what} {tag}: zero x does not give the bias"
        for _ in range(10):
            assert torch.equal(bits(lay.run(x[:1])), bits(y1)), f"{what} {tag}: a repeat differs"
        return y1

    y1 = one_row("fused")
    hk.set_fused_finalize(False)
    try:
        one_row("two kernels")
    finally:
        hk.set_fused_finalize(True)
    # several rows per launch: every row has the bits of that row launched alone (the copy correction of the multi-row kernels,
    # and for 3-byte entries the reciprocal division that finds the copy)
    alone = [y1[0]] + [lay.run(x[r:r + 1].contiguous())[0] for r in range(1, 8)]
    for B in (2, 3, 5, 8):
        yb = lay.run(x[:B])
        check_close(yb.float().cpu().numpy(), y64[:B], dtype, f"{what}, {B} rows")
        for r in range(B):
            assert torch.equal(bits(yb[r]), bits(alone[r])), f"{what}: row {r} of a {B}-row launch differs from the row launched alone"


@pytest.mark.parametrize("rows", [1, 3])
@pytest.mark.parametrize("eb", [3, 4])
@pytest.mark.parametrize("copies", [(3, 3), (4, 1), (2, 3, 4)], ids=lambda c: "xc" + "".join(str(v) for v in c))
def test_shared_input_launch_on_several_x_copies(copies, eb, rows):
    """aqlm_hip_gemv_1x16_packed_multi of two and three layers: the bits of separate launches.  (At one row the pipelined kernel takes
    buffers of one x copy and 4-byte entries only: it must step aside here.)"""
    hk = _hk()
    fouts = (300, 128, 96)
    ls = [xc_layer(1024, fouts[k], "float16", xc, eb) for k, xc in enumerate(copies)]
    assert [int(l.packed.desc.x_copies) for l in ls] == list(copies) and max(copies) > 1
    x = ls[0].xs[:rows]
    outs = hk.code1x16_matmat_packed_multi(x, [l.packed for l in ls], [l.codebooks for l in ls], [l.scales for l in ls], [l.bias for l in ls])
    for k, (l, y) in enumerate(zip(ls, outs)):
        ref = l.run(x)
        assert torch.equal(bits(y), bits(ref)), f"segment {k} ({l.packed.desc.x_copies} x copies): differs from its own launch"
        check_close(y.float().cpu().numpy(), orc.dequantize_gemm(ls[0].L["x"][:rows], l.L["codes"], l.L["codebooks"], l.L["scales"], l.L["bias"]),
                    l.dtype, f"shared-input segment {k}")


ROUTED_IDS = [[0, 1], [2, 3], [1, 2], [3, 0], [0, 2]]   # top-2 over 5 tokens, every expert named


def routed_experts():
    """four experts of 512 -> 256, two packed with 4 x copies and two with 1; -> (layers, table, geometry)"""
    hk = _hk()
    if "routed" not in _LAYERS:
        ls = [layer(512, 256, 6100 + e, torch.float16, bias=False, uniform_only=True, packed_xcopies=(4 if e % 2 == 0 else 0)) for e in range(4)]
        assert [int(l.packed.desc.x_copies) for l in ls] == [4, 1, 4, 1]
        table, tail = hk.routed_packed_table([[(l.packed, l.codebooks, l.scales, None)] for l in ls], torch.device(DEV))
        _LAYERS["routed"] = (ls, table, [4, 1, 256, 512, 8, 2] + tail)
    return _LAYERS["routed"]


def routed_launch():
    ls, table, geometry = routed_experts()
    x = torch.cat([l.xs[:1] for l in ls] + [ls[0].xs[1:2]])   # 5 token rows
    ids = torch.tensor(ROUTED_IDS, device=DEV)
    return x, ids, torch.ops.aqlm.code1x16_moe_matmat_packed(x, ids, table, geometry, False)


def test_routed_launch_on_experts_of_mixed_x_copies():
    ls, _, _ = routed_experts()
    x, ids, y = routed_launch()
    assert tuple(y.shape) == (10, 1, 256)
    for p, e in enumerate(ids.view(-1).tolist()):
        ref = ls[e].run(x[p // 2].view(1, -1))
        assert torch.equal(bits(y[p, 0]), bits(ref[0])), f"pair {p} (expert {e}, {ls[e].packed.desc.x_copies} x copies)"
        check_close(y[p, 0].float().cpu().numpy()[None], orc.dequantize_gemm(x[p // 2].float().cpu().numpy()[None], ls[e].L["codes"],
                    ls[e].L["codebooks"], ls[e].L["scales"], None), ls[e].dtype, f"routed pair {p}")


@pytest.mark.parametrize("fold", [2, 4])
def test_captured_launches_on_four_x_copies(fold):
    """four layers of 512 -> 256 packed with 4 copies (x image 4304 bytes: the compact window, so they share a grouped launch) -- eager,
    captured and captured folded agree bit for bit (run_folded), and the node goes over to the folded kernel"""
    native = _native()
    ls = [layer(512, 256, 6200 + i, torch.float16, packed_xcopies=4) for i in range(4)]
    for i, l in enumerate(ls):
        assert int(l.packed.desc.x_copies) == 4 and native.packed_image(l.packed.desc, 1)[1] == COMPACT
        if i % 2:
            l.own_cells()
    assert len({int(l.packed.desc.waves) for l in ls}) == 1
    stats = run_folded(ls, fold)
    assert stats["merged"] == 3 and stats["nodes_added"] == 1 and stats["folded"] == 1
    for l in ls:
        check_close(l.y.float().cpu().numpy(), l.y64()[:1], l.dtype, "captured launch on 4 x copies")


# ------------------------------------------------------------------ 2. ring depths at one row
# 4096 inputs at four waves per workgroup (pinned at repack, labels and geometry as they are): out -> steps per wave, computed from the
# codes by the format model and asserted below.  For ring depth 4 that is the remainder alone (1, 2, 3), exactly one turn (4), one
# turn + 1 (5) and two turns + 1 and more (9, 19); for depth 8: remainder alone (1 .. 5), one turn (8), one turn + 1 (9), two + 3 (19).
# 4096 -> 37 has fewer rows than waves x 16.
RING_STEPS = {37: 1, 512: 2, 1024: 3, 1536: 4, 2200: 5, 3400: 8, 3900: 9, 9000: 19}


def test_ring_step_counts_cover_every_loop_path():
    steps = sorted(RING_STEPS.values())
    for pd in (4, 8):
        assert any(t < pd for t in steps) and pd in steps and pd + 1 in steps and any(t >= 2 * pd + 1 for t in steps), pd
    assert max(steps) <= 32   # the 3-byte form exists up to 32 steps per wave


@pytest.mark.parametrize("dt", ["float16", "bfloat16"])
@pytest.mark.parametrize("eb", [3, 4])
@pytest.mark.parametrize("fout", sorted(RING_STEPS))
def test_ring_depths_at_one_row(fout, eb, dt):
    native = _native()
    lay = layer(4096, fout, 4200 + fout, tdtype(dt), rows=1, relabel=False, uniform_only=True, packed_waves=4, packed_entry_bytes=eb)
    d = lay.packed.desc
    assert (int(d.waves), int(d.steps), int(d.entry_bytes)) == (4, RING_STEPS[fout], eb), f"4096 -> {fout}: {d.waves} waves x {d.steps} steps"
    assert not d.relabelled and not d.variable_geometry and int(d.x_copies) == 1
    y64, out = lay.y64(), {}
    for pd in (3, 4, 8):
        with tuned(packed_prefetch=pd):
            out[pd] = lay.run(lay.x)
            win = native.packed_image(d, 1, did(lay.dtype))[1]
        # deeper rings have no compact instance: the full window, and the bits of the compact launch
        assert win == (COMPACT if pd == 3 and eb == 4 else FULL), f"ring depth {pd}: window {win}"
        what = f"4096->{fout} {dt} entry bytes {eb} steps {d.steps} ring depth {pd}"
        m = check_close(out[pd].float().cpu().numpy(), y64, lay.dtype, what)
        exact = check_rounded(out[pd].float().cpu().numpy(), y64, lay.dtype, what)
        print(f"{what}: mean-rel {m:.3e}, exact {exact:.4f}")
    # a lane adds its steps in stream order whatever the depth
    for pd in (4, 8):
        assert torch.equal(bits(out[pd]), bits(out[3])), f"4096->{fout} {dt} entry bytes {eb}: ring depth {pd} differs from depth 3"
    assert native.get_tuning("packed_prefetch") == 0


# ------------------------------------------------------------------ 3. fill rotation off
@pytest.mark.parametrize("eb", [3, 4])
def test_fill_rotation_off_gives_the_same_bits(eb):
    native = _native()
    assert native.get_tuning("packed_fill_rotate") == 1
    for lay in (xc_layer(1024, 300, "float16", 3, eb), layer(4096, 1024, 4200 + 1024, torch.float16, rows=1, relabel=False, uniform_only=True,
                                                             packed_waves=4, packed_entry_bytes=eb)):
        for rows in (1, 3):
            if rows > lay.xs.shape[0]:
                continue
            want = lay.run(lay.xs[:rows])
            with tuned(packed_fill_rotate=0):
                got = lay.run(lay.xs[:rows])
            assert torch.equal(bits(got), bits(want)), f"{lay.fin}->{lay.fout} entry bytes {eb}, {rows} rows"
            check_close(got.float().cpu().numpy(), lay.y64()[:rows], lay.dtype, "fill rotation off")
    assert native.get_tuning("packed_fill_rotate") == 1


def test_fill_rotation_off_routed_launch():
    _, _, want = routed_launch()
    with tuned(packed_fill_rotate=0):
        _, _, got = routed_launch()
    assert torch.equal(bits(got), bits(want))


# ------------------------------------------------------------------ 4. the chain entry
def entry(name, lay, x, y, nxt=None, workspace=None):
    """aqlm_hip_gemv_1x16_packed (`name` "plain") or aqlm_hip_gemv_1x16_packed_chain ("chain"; `nxt` = (desc pointer or None, packed
    address, codebook address)) through the C ABI on the current stream -> return code"""
    native = _native()
    head = (ctypes.byref(lay.packed.desc), lay.packed.data_ptr(), lay.codebooks.data_ptr(), lay.scales.data_ptr(),
            None if lay.bias is None else lay.bias.data_ptr(), x.data_ptr(), y.data_ptr(), x.shape[0], x.stride(0), y.stride(0),
            did(lay.dtype), None if workspace is None else workspace.data_ptr(), 0 if workspace is None else workspace.numel() * 4)
    stream = torch.cuda.current_stream().cuda_stream
    if name == "plain":
        return native.lib.aqlm_hip_gemv_1x16_packed(*head, stream)
    return native.lib.aqlm_hip_gemv_1x16_packed_chain(*head, *(nxt or (None, None, None)), stream)


def hint_of(nxt_layer):
    """Whether the prefetch waves may be told about this next layer, worked out here from its layout: not for variable geometry and
    not where the whole-KiB requests would leave the buffer.  What the library decides is read from
    aqlm_hip_gemv_1x16_packed_chain_plan and compared with this (chain_against_plain)."""
    d, lay = nxt_layer.packed.desc, nxt_layer.layout()
    if d.variable_geometry:
        return "dropped (variable geometry)"
    bb = lay["ent_bytes"] // 256
    end = lay["off_ent"] + 255 * bb + (bb + 1023) // 1024 * 1024
    return "kept" if end <= lay["used"] else f"dropped ({bb} bytes per block, the last request would end {end - lay['used']} bytes past the buffer)"


def next_layers():
    """name -> the layer named as NEXT.  All float16: the hint reads bytes, and each is launched in its own type."""
    from tests.packed_model import zipf_codes

    if "next" not in _LAYERS:
        f16 = torch.float16
        cz8 = zipf_codes(1536, 256, 0.8, False, 7)
        nl = {
            "same shape 1024->512": layer(1024, 512, 7101, f16, rows=1),
            "same shape 4096->1024": layer(4096, 1024, 7102, f16, rows=1),
            "more waves": layer(1024, 512, 7103, f16, rows=1, packed_waves=8),
            "fewer waves": layer(1024, 512, 7104, f16, rows=1, packed_waves=2),
            "relabelled": layer(2048, 1536, 7105, f16, rows=1, codes_unsigned=cz8),
            "variable geometry": layer(2048, 1536, 7106, f16, rows=1, codes_unsigned=zipf_codes(1536, 256, 1.2, False, 7)),
            "3-byte entries": layer(1024, 512, 7107, f16, rows=1, relabel=False, packed_entry_bytes=3),
            "3-byte entries, relabelled": layer(2048, 1536, 7108, f16, rows=1, codes_unsigned=cz8, packed_entry_bytes=3),
        }
        d = {k: v.packed.desc for k, v in nl.items()}
        assert int(d["more waves"].waves) == 8 and int(d["fewer waves"].waves) == 2 and int(d["same shape 1024->512"].waves) not in (2, 8)
        assert d["relabelled"].relabelled and not d["relabelled"].variable_geometry and int(d["relabelled"].entry_bytes) == 4
        assert d["variable geometry"].variable_geometry
        assert int(d["3-byte entries"].entry_bytes) == 3 and not d["3-byte entries"].relabelled
        assert int(d["3-byte entries, relabelled"].entry_bytes) == 3 and d["3-byte entries, relabelled"].relabelled
        assert hint_of(nl["3-byte entries"]).startswith("dropped") and hint_of(nl["variable geometry"]).startswith("dropped")
        assert all(hint_of(v) == "kept" for k, v in nl.items() if k not in ("3-byte entries", "variable geometry"))
        for k, v in nl.items():
            print(f"chain: next layer '{k}' ({v.fin}->{v.fout}, {d[k].waves} waves x {d[k].steps} steps, {d[k].entry_bytes}-byte entries): hint {hint_of(v)}")
        _LAYERS["next"] = nl
    return _LAYERS["next"]


def chain_against_plain(A, rows, names, waves_keys=(-1, 0, 1, 7)):
    """Every (next layer, packed_prefetch_waves) on layer A with `rows` input rows: y has the bits of the plain entry, A's cells are
    zero afterwards and a plain call still gives those bits, the next layer's buffer is untouched and computes what it computed."""
    nl = next_layers()
    x = A.xs[:rows]
    want = torch.zeros((rows, A.fout), device=DEV, dtype=A.dtype)
    assert entry("plain", A, x, want) == 0, _native().last_error()
    check_close(want.float().cpu().numpy(), A.y64()[:rows], A.dtype, f"plain entry {A.fin}->{A.fout}")
    assert not bool(A.cells_in_buffer().any())
    for name in names:
        B = None if name == "null pointers" else nl[name]
        nxt = None if B is None else (ctypes.byref(B.packed.desc), B.packed.data_ptr(), B.codebooks.data_ptr())
        if B is not None:
            snapshot, b_before = B.packed.buf.clone(), B.run(B.x)
        for key in waves_keys:
            y = torch.full((rows, A.fout), 7.0, device=DEV, dtype=A.dtype)
            with tuned(packed_prefetch_waves=key):
                rc = entry("chain", A, x, y, nxt)
                plan = _native().packed_chain_plan(A.packed.desc, None if B is None else B.packed.desc, rows, did(A.dtype))
            assert rc == 0, f"next '{name}', prefetch waves {key}: {_native().last_error()}"
            # what the library says it launched: the hint kept exactly where this file's own reading of the layout keeps it, the
            # prefetch waves the key asks for (0 = 2) capped at 7 and at 16 - waves, a landing zone of 1 KiB each behind the image
            kept = B is not None and hint_of(B) == "kept"
            waves = min({-1: 0, 0: 2, 1: 1, 7: 7}[key], 16 - int(A.packed.desc.waves)) if kept else 0
            image = _native().packed_image(A.packed.desc, rows, did(A.dtype))[0]
            assert plan == (kept, waves, image + 1024 * waves), f"next '{name}', prefetch waves {key}, {rows} rows: the library reports {plan}"
            assert plan[2] <= 160 * 1024
            tag = f"{A.fin}->{A.fout} ({A.packed.desc.waves} waves) {A.dtype} {rows} rows, next '{name}', packed_prefetch_waves {key}"
            assert torch.equal(bits(y), bits(want)), f"{tag}: differs from aqlm_hip_gemv_1x16_packed"
            assert not bool(A.cells_in_buffer().any()), f"{tag}: accumulator cells not back at zero"
            again = torch.zeros_like(want)
            assert entry("plain", A, x, again) == 0 and torch.equal(bits(again), bits(want)), f"{tag}: a plain call afterwards differs"
        if B is not None:
            assert torch.equal(B.packed.buf, snapshot), f"next '{name}': its buffer was written"
            assert torch.equal(bits(B.run(B.x)), bits(b_before)), f"next '{name}': it no longer computes what it computed"
    B = nl[names[0]]   # a pointer missing: no hint, the plain call
    for nxt in ((ctypes.byref(B.packed.desc), None, B.codebooks.data_ptr()), (None, B.packed.data_ptr(), B.codebooks.data_ptr())):
        y = torch.zeros_like(want)
        assert entry("chain", A, x, y, nxt) == 0 and torch.equal(bits(y), bits(want))


CHAIN_NEXT = ["same shape 1024->512", "same shape 4096->1024", "more waves", "fewer waves", "relabelled", "variable geometry",
              "3-byte entries", "3-byte entries, relabelled", "null pointers"]


@pytest.mark.parametrize("rows", [1, 3])
@pytest.mark.parametrize("dt", ["float16", "bfloat16"])
@pytest.mark.parametrize("fin,fout", [(1024, 512), (4096, 1024)])
def test_chain_entry_has_the_bits_of_the_plain_entry(fin, fout, dt, rows):
    A = layer(fin, fout, 7000 + fin, tdtype(dt), rows=3)
    assert int(A.packed.desc.waves) <= 8   # room for every prefetch-wave count asked for (7 is capped at 16 - waves)
    chain_against_plain(A, rows, CHAIN_NEXT)


@pytest.mark.parametrize("eb", [3, 4])
@pytest.mark.parametrize("waves", [14, 16])
def test_chain_entry_on_a_layer_with_little_or_no_room_for_prefetch_waves(waves, eb):
    """14 waves: at most two prefetch waves (7 and the default are capped); 16 waves: none, the launch is the plain one"""
    A = layer(1024, 512, 7200 + waves, torch.float16, rows=3, packed_waves=waves, packed_entry_bytes=eb)
    assert int(A.packed.desc.waves) == waves and int(A.packed.desc.entry_bytes) == eb
    for rows in (1, 3):
        chain_against_plain(A, rows, ["same shape 1024->512", "relabelled", "3-byte entries, relabelled"])


def test_chain_entry_refuses_a_bad_next_layer_and_launches_nothing():
    native = _native()
    A, B = layer(1024, 512, 7000 + 1024, torch.float16, rows=3), next_layers()["same shape 1024->512"]
    x = A.xs[:1]
    bad = native.PackedDesc.from_ints(B.packed.desc.as_ints())
    bad.used_bytes += 1
    garbage = native.PackedDesc()
    good = ctypes.byref(B.packed.desc)
    for what, nxt in (("used_bytes off by one", (ctypes.byref(bad), B.packed.data_ptr(), B.codebooks.data_ptr())),
                      ("an empty descriptor", (ctypes.byref(garbage), B.packed.data_ptr(), B.codebooks.data_ptr())),
                      ("misaligned packed buffer", (good, B.packed.data_ptr() + 8, B.codebooks.data_ptr())),
                      ("misaligned codebook", (good, B.packed.data_ptr(), B.codebooks.data_ptr() + 8))):
        y = torch.full((1, A.fout), 7.0, device=DEV, dtype=A.dtype)
        assert entry("chain", A, x, y, nxt) == native.E_INVALID, what
        assert "next layer" in native.last_error()
        torch.cuda.synchronize()
        assert bool((y == 7.0).all()), f"{what}: the refused call wrote y"
        assert not bool(A.cells_in_buffer().any())
    y = torch.zeros((1, A.fout), device=DEV, dtype=A.dtype)
    assert entry("chain", A, x, y, (good, B.packed.data_ptr(), B.codebooks.data_ptr())) == 0
    assert torch.equal(bits(y), bits(A.run(x)))


@pytest.mark.parametrize("rows", [1, 3])
def test_chain_entry_with_the_two_kernel_finalize(rows):
    hk = _hk()
    A, B = layer(1024, 512, 7000 + 1024, torch.float16, rows=3), next_layers()["same shape 1024->512"]
    x = A.xs[:rows]
    nxt = (ctypes.byref(B.packed.desc), B.packed.data_ptr(), B.codebooks.data_ptr())
    ws = torch.empty((16 * rows * A.fout,), dtype=torch.float32, device=DEV)
    want, got = (torch.zeros((rows, A.fout), device=DEV, dtype=A.dtype) for _ in range(2))
    hk.set_fused_finalize(False)
    try:
        assert _native().packed_chain_plan(A.packed.desc, B.packed.desc, rows)[:2] == (False, 0)   # this form never prefetches
        assert entry("plain", A, x, want, workspace=ws) == 0, _native().last_error()
        for key in (-1, 0, 7):
            got.zero_()
            with tuned(packed_prefetch_waves=key):
                assert entry("chain", A, x, got, nxt, workspace=ws) == 0, _native().last_error()
            assert torch.equal(bits(got), bits(want)), f"prefetch waves {key}"
        assert entry("chain", A, x, got, nxt) == _native().E_INVALID   # the two-kernel form needs its workspace, named or not
    finally:
        hk.set_fused_finalize(True)
    assert _native().packed_chain_plan(A.packed.desc, B.packed.desc, rows)[:2] == (True, 2)
    check_close(want.float().cpu().numpy(), A.y64()[:rows], A.dtype, "two-kernel finalize through the chain entry")
    check_rounded(want.float().cpu().numpy(), A.y64()[:rows], A.dtype, "two-kernel finalize through the chain entry")
