"""The compact x window of the packed 1x16 matvec on the MI355X: one-row launches of layers whose x image
fits 8208 bytes keep x in a window of that size instead of 64 KiB, so that a workgroup of another layer fits the CU beside them.

  * parity at the window's edges: key on (`packed_compact_window` 0) against key forced off (1) -- the same bits -- and against the
    fp64 oracle under check_close of tests/test_hip_parity.py;
  * sixteen captured launches that may share CUs give the bits of the same launches issued eagerly, and leave the cells zero;
  * the image sizes the library reports agree with what the runtime says about its kernels (no launch)."""
import math

import numpy as np
import pytest

from oracle import aqlm_oracle as orc
from tests import packed_model as pm
from tests.packed_model import zipf_codes
from tests.test_compact_window_host import COMPACT, CU_LDS, FULL, desc, up
from tests.test_hip_parity import check_close, tdtype, to_dev

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hk():
    assert torch.cuda.is_available(), "run with -m gpu on the MI355X box"
    from aqlm_amd.inference_kernels import hip_kernel

    return hip_kernel


@pytest.fixture(autouse=True)
def default_key():
    from aqlm_amd import _native

    old = _native.get_tuning("packed_compact_window")
    yield
    _native.set_tuning("packed_compact_window", old)


# (in, out, dtype, bias, code law, window of the one-row launch)
EDGES = [
    (4096, 512, "float16", True, "uniform", COMPACT),     # x fills the window to its last byte: the null slot is the 16 bytes in front of the slice
    (4096, 512, "float16", False, "uniform", COMPACT),
    (4096, 512, "bfloat16", True, "uniform", COMPACT),
    (4096, 512, "bfloat16", False, "uniform", COMPACT),
    (4104, 512, "float16", True, "uniform", FULL),        # one input group too many: the full window
    (256, 512, "bfloat16", False, "uniform", COMPACT),
    (1024, 272, "float16", False, "uniform", COMPACT),    # 17 rows per group, the last groups ragged
    (1024, 1040, "bfloat16", True, "uniform", COMPACT),
    (2048, 1536, "float16", True, "relabelled", COMPACT),
    (2048, 1536, "bfloat16", False, "vargeom", COMPACT),
]


@pytest.mark.parametrize("fin,fout,dt,bias,law,window", EDGES)
def test_key_on_and_off_give_the_same_bits(hk, fin, fout, dt, bias, law, window):
    from aqlm_amd import _native

    dtype = tdtype(dt)
    L = orc.make_layer(9100 + fin + fout, fin, fout, 1, 16, 8, batch=1, bias=bias, float_dtype=np.float16 if dtype == torch.float16 else "bfloat16")
    if law != "uniform":   # the skewed code laws of tests/test_packed_dequant_gpu.py: Zipf 0.8 relabels, Zipf 1.2 also changes the geometry
        cu = zipf_codes(fout, fin // 8, 0.8 if law == "relabelled" else 1.2, False, 7)[:, :, None]
        L = dict(L, codes=orc.pack_int_data(cu, 16), codes_unsigned=cu)
    T = to_dev(L, dtype)
    packed = hk.prepack_1x16(T["codes"], 8, codebooks=T["codebooks"])
    assert packed is not None and packed.desc.entry_bytes == 4
    assert packed.desc.relabelled == (law != "uniform") and packed.desc.variable_geometry == (law == "vargeom")
    did = _native.F16 if dtype == torch.float16 else _native.BF16
    _native.set_tuning("packed_compact_window", 0)
    lds_on, win_on = _native.packed_image(packed.desc, 1, did)
    assert win_on == window == (COMPACT if (fin // 8 + 1) * 16 <= COMPACT else FULL)   # 4104 features say so: the full window
    y_on = hk.code1x16_matmat_packed(T["x"], packed, T["codebooks"], T["scales"], T["bias"])
    y_on2 = hk.code1x16_matmat_packed(T["x"], packed, T["codebooks"], T["scales"], T["bias"])
    _native.set_tuning("packed_compact_window", 1)
    lds_off, win_off = _native.packed_image(packed.desc, 1, did)
    assert win_off == FULL and (lds_on < lds_off) == (window == COMPACT)
    y_off = hk.code1x16_matmat_packed(T["x"], packed, T["codebooks"], T["scales"], T["bias"])
    assert torch.equal(y_on.view(torch.int16), y_off.view(torch.int16)) and torch.equal(y_on, y_on2)
    y64 = orc.dequantize_gemm(L["x"], L["codes"], L["codebooks"], L["scales"], L["bias"])
    check_close(y_on.float().cpu().numpy(), y64, dtype, f"compact window {fin}->{fout} {law}")
    if bias:   # zero input: every entry reads zeros, the null slot among them
        _native.set_tuning("packed_compact_window", 0)
        yz = hk.code1x16_matmat_packed(torch.zeros_like(T["x"]), packed, T["codebooks"], T["scales"], T["bias"])
        assert torch.equal(yz[0], T["bias"])


def test_sixteen_captured_launches_that_share_cus(hk):
    """1024 -> 1024 and 1024 -> 2048 alternating, every launch its own layer, x and y: captured with two chains in flight from the
    second launch on, so that workgroups of two layers meet on a CU; two replays; then every accumulator cell is zero."""
    from aqlm_amd import _native
    from tests.test_capture_overlap_gpu import PackedLayer, capture_window

    _native.set_tuning("packed_compact_window", 0)
    layers = [PackedLayer(1024, 1024 if i % 2 == 0 else 2048, 7000 + i) for i in range(16)]
    for l in layers:
        assert _native.packed_image(l.packed.desc, 1)[1] == COMPACT
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        for l in layers:
            l.launch(stream)
    stream.synchronize()
    want = [l.y.clone() for l in layers]
    assert all(bool(w.float().abs().sum() > 0) for w in want)
    for l in layers:
        l.y.zero_()
    torch.cuda.synchronize()
    _native.capture_overlap_stats(reset=True)
    graph = torch.cuda.CUDAGraph()
    with capture_window(2, min_run=1):
        with torch.cuda.graph(graph, stream=stream):
            for l in layers:
                l.launch(torch.cuda.current_stream())
    stats = _native.capture_overlap_stats()
    assert stats["api_failures"] == 0 and (stats["seen"], stats["relaxed"], stats["kept_window"]) == (16, 1, 14)
    with torch.cuda.stream(stream):
        graph.replay()
        graph.replay()
    stream.synchronize()
    for i, (l, w) in enumerate(zip(layers, want)):
        assert torch.equal(l.y, w), f"launch {i}: the captured replay differs from the eager pass"
        d = l.packed.desc
        lay = pm.layout(l.fout, l.fin // 8, int(d.waves), int(d.steps), 4, None, d.relabelled)
        cells = l.packed.buf[lay["off_acc"]:lay["off_ent"]]
        assert not bool(cells.any()), f"launch {i}: accumulator cells not zero after the replays"


def test_runtime_agrees_with_the_image_arithmetic():
    """No launch: hipOccupancyMaxActiveBlocksPerMultiprocessor on the kernels the two headline launches would run, each at its own
    block size.  The LDS a CU offers and the granule its allocations are rounded to are read off the runtime's answers (the largest
    request that still gets k workgroups, k = 1, 2, 3: all multiples of the granule), not assumed."""
    from aqlm_amd import _native

    assert torch.cuda.is_available()
    torch.cuda.init()
    a, b = desc(_native, 4096, 4096, 6, 6), desc(_native, 11008, 4096, 14, 6)
    _native.set_tuning("packed_compact_window", 0)
    (lds_a, win_a), (lds_b, win_b) = _native.packed_image(a), _native.packed_image(b)
    assert (win_a, win_b) == (COMPACT, COMPACT)

    def most(d, k):   # the largest dynamic LDS at which the runtime still lets k workgroups of the launch share a CU
        lo, hi = 0, CU_LDS
        while lo < hi:
            mid = (lo + hi + 1) // 2
            if _native.packed_image_blocks_per_cu(d, 1, _native.F16, mid) >= k:
                lo = mid
            else:
                hi = mid - 1
        return lo

    per_cu = most(a, 1)
    granule = math.gcd(per_cu, most(a, 2), most(a, 3), most(b, 2))
    print(f"runtime: {per_cu} bytes of LDS per CU, allocation granule {granule}; images {lds_a} + {lds_b}")
    assert per_cu == most(b, 1) and per_cu >= CU_LDS and granule >= 1
    assert up(lds_a, granule) + up(lds_b, granule) <= per_cu
    assert _native.packed_image_blocks_per_cu(a) >= 1 and _native.packed_image_blocks_per_cu(b) >= 1
    # a request of both images together is still granted a workgroup: the pair fits by the runtime's own account ...
    assert _native.packed_image_blocks_per_cu(a, 1, _native.F16, up(lds_a, granule) + up(lds_b, granule)) >= 1
    # ... and with the full window it does not: one workgroup per CU, as before
    _native.set_tuning("packed_compact_window", 1)
    full_a, full_b = _native.packed_image(a)[0], _native.packed_image(b)[0]
    assert _native.packed_image_blocks_per_cu(a) == 1 and _native.packed_image_blocks_per_cu(b) == 1
    assert up(full_a, granule) + up(full_b, granule) > per_cu
