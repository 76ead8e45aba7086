"""Folded grouped launches of the captured packed 1x16 matvec (aqlm_amd/csrc/group_fold.h; tuning key packed_group_fold): a node
of at least F launches runs as 256 / F workgroups per launch, each keeping its codebook slice and x in LDS and walking F row groups.

Every case makes its calls eagerly, then captured at the fold factor under test and replays the graph 20 times: y must be the bits
of the eager pass AND the bits of the same capture at packed_group_fold = 1, the accumulator cells must be zero afterwards (half
the layers bring their own cells, which are read; the others use the cells inside the packed buffer, which a last eager call
would trip over), and the `folded` counter of aqlm_hip_capture_overlap_stats_ex says how many nodes went over to the folded kernel.
Small prepacked 1x16g8 layers (512 inputs, 16 slices) unless a case needs a longer stream; runs relax and join from the second
launch on (packed_capture_min_run 1)."""
import contextlib
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

REPLAYS = 20
DTYPES = [torch.float16, torch.bfloat16]
FOLDS = [2, 4]


class PackedLayer:
    def __init__(self, fin, fout, seed, dtype=torch.float16, codes=None, bias=False, waves=0):
        from aqlm_amd import _native
        from aqlm_amd.inference_kernels import hip_kernel as hk

        dev = torch.device("cuda", 0)
        gen = torch.Generator(device=dev).manual_seed(seed)
        self.fin, self.fout, self.dtype = fin, fout, dtype
        if codes is None:
            codes = torch.randint(-32768, 32768, (fout, fin // 8, 1), generator=gen, device=dev, dtype=torch.int32).to(torch.int16)
        self.codes = codes
        self.codebooks = torch.randn((1, 65536, 1, 8), generator=gen, device=dev, dtype=torch.float32).to(dtype)
        self.scales = (0.5 + torch.rand((fout,), generator=gen, device=dev, dtype=torch.float32)).to(dtype)
        self.bias = torch.randn((fout,), generator=gen, device=dev, dtype=torch.float32).to(dtype) if bias else None
        self.x = torch.randn((1, fin), generator=gen, device=dev, dtype=torch.float32).to(dtype)
        self.y = torch.zeros((1, fout), device=dev, dtype=dtype)
        self.cells = None  # caller-owned accumulator cells (own_cells())
        old = _native.get_tuning("packed_waves")
        _native.set_tuning("packed_waves", waves)  # waves per workgroup at repack (0 = the repack's choice)
        try:
            self.packed = hk.prepack_1x16(self.codes, 8, codebooks=self.codebooks)
        finally:
            _native.set_tuning("packed_waves", old)
        assert self.packed is not None and self.packed.desc.codebook_absmax > 0

    def own_cells(self):
        if self.cells is None:
            self.cells = torch.zeros((self.fout,), dtype=torch.int64, device=self.x.device)
        return self

    def launch(self, stream, x=None):
        from aqlm_amd import _native

        x = self.x if x is None else x
        head = (ctypes.byref(self.packed.desc), self.packed.data_ptr(), self.codebooks.data_ptr(), self.scales.data_ptr(),
                None if self.bias is None else self.bias.data_ptr(), x.data_ptr(), self.y.data_ptr(), x.shape[0], x.stride(0),
                self.y.stride(0), _native.F16 if self.dtype == torch.float16 else _native.BF16)
        if self.cells is None:
            rc = _native.lib.aqlm_hip_gemv_1x16_packed(*head, None, 0, stream.cuda_stream)
        else:
            rc = _native.lib.aqlm_hip_gemv_1x16_packed_cells(*head, self.cells.data_ptr(), self.cells.numel() * 8, stream.cuda_stream)
        _native.check(rc)


_LAYERS = {}


def layers(dtype, shape, n, **kw):
    """`n` independent layers of one shape (built once per dtype, shape and options, shared by the cases); every second one brings
    its own accumulator cells"""
    have = _LAYERS.setdefault((dtype, shape, tuple(sorted(kw.items()))), [])
    while len(have) < n:
        layer = PackedLayer(shape[0], shape[1], 700 + 37 * len(have) + shape[1], dtype, **kw)
        have.append(layer.own_cells() if len(have) % 2 else layer)
    return have[:n]


@contextlib.contextmanager
def tuned(**keys):
    from aqlm_amd import _native

    old = {k: _native.get_tuning(k) for k in keys}
    for k, v in keys.items():
        _native.set_tuning(k, v)
    try:
        yield
    finally:
        for k, v in old.items():
            _native.set_tuning(k, v)


def bits(t):
    return t.view(torch.int16)


def captured(program, ls, fold, window, merge):
    """the program captured at `fold`, replayed; -> (bit patterns of every y, counters of the capture)"""
    from aqlm_amd import _native

    for l in ls:
        l.y.zero_()
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    with tuned(packed_capture_window=window, packed_capture_merge=merge, packed_capture_min_run=1, packed_group_fold=fold):
        _native.capture_overlap_stats(reset=True)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            program(torch.cuda.current_stream())
        stats = _native.capture_overlap_stats()
    with torch.cuda.stream(stream):
        for _ in range(REPLAYS):
            graph.replay()
    stream.synchronize()
    assert stats["api_failures"] == 0 and stats["merge_refused"] == 0, _native.last_error()
    return [bits(l.y).clone() for l in ls], stats


def run_folded(ls, fold, window=1, merge=8, program=None):
    """Eager, captured at fold 1, captured at `fold`: the three must agree bit for bit, and the cells must be back at zero.
    -> counters of the folded capture."""
    ls = list(ls)
    program = program or (lambda s: [l.launch(s) for l in ls])
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        program(stream)
    stream.synchronize()
    want = [bits(l.y).clone() for l in ls]
    assert all(bool((w != 0).any()) for w in want)
    plain, stats1 = captured(program, ls, 1, window, merge)
    assert stats1["folded"] == 0
    got, stats = captured(program, ls, fold, window, merge)
    for i, (g, p, w) in enumerate(zip(got, plain, want)):
        assert torch.equal(g, w), f"layer {i}: the folded capture differs from the eager pass"
        assert torch.equal(g, p), f"layer {i}: the folded capture differs from the capture at packed_group_fold = 1"
    for i, l in enumerate(ls):
        if l.cells is not None:
            assert not bool(l.cells.any()), f"layer {i}: accumulator cells not back at zero"
    with torch.cuda.stream(stream):  # the cells inside the packed buffers: a cell left dirty would show in the next call
        program(stream)
    stream.synchronize()
    for i, (l, w) in enumerate(zip(ls, want)):
        assert torch.equal(bits(l.y), w), f"layer {i}: an eager call after the replays differs (cells inside the packed buffer)"
    assert (stats["seen"], stats["merged"], stats["nodes_added"]) == (stats1["seen"], stats1["merged"], stats1["nodes_added"])
    return stats


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("fold", FOLDS)
@pytest.mark.parametrize("shape", [(512, 256), (512, 512)])
@pytest.mark.parametrize("members", [2, 3, 6, 8])
def test_member_counts_and_fold_factors(members, shape, fold, dtype):
    ls = layers(dtype, shape, members)
    stats = run_folded(ls, fold)  # one chain, one node of `members` launches
    assert stats["merged"] == members - 1 and stats["nodes_added"] == 1
    assert stats["folded"] == (1 if members >= fold else 0)  # a node with fewer members than F is not folded


# 512 -> 130: 9 rows per group, so group 14 holds 4 rows and group 15 none; 512 -> 250: the last group is short; 512 -> 1000: several
# hundred rows.  A later pass has fewer rows, or none, than the one before it, and at 512 inputs (4 codes per row and slice on
# average) a few per cent of the (row, slice) buckets are empty.
@pytest.mark.parametrize("fold", FOLDS)
@pytest.mark.parametrize("fout", [130, 250, 1000])
def test_short_and_empty_passes(fout, fold):
    ls = layers(torch.float16, (512, fout), 4)
    rg = int(ls[0].packed.desc.rows_per_group)
    assert rg * 16 >= fout and (fout != 130 or (rg == 9 and fout - 14 * rg == 4 and fout - 15 * rg < 0))
    stats = run_folded(ls, fold)
    assert stats["folded"] == 1


# The loop's remainder path in a later pass: streams of T = 3 steps per wave (a multiple of the ring depth: no remainder) and of
# T = 4 (one turn of the loop, then one step of remainder); the small layers above have T = 1 (remainder only).  4096 inputs give a
# row 8-9 lane-steps per slice; four waves per workgroup are asked for at repack so that the streams are long enough.
@pytest.mark.parametrize("fold", FOLDS)
@pytest.mark.parametrize("fout,multiple", [(1024, True), (1536, False)])
def test_ring_remainder_in_later_passes(fout, multiple, fold):
    ls = layers(torch.float16, (4096, fout), 4, waves=4)
    steps = int(ls[0].packed.desc.steps)
    assert all(int(l.packed.desc.steps) == steps and int(l.packed.desc.waves) == 4 for l in ls)
    assert steps >= 3 and (steps % 3 == 0) == multiple, f"4096 -> {fout}: {steps} steps per wave"
    assert int(layers(torch.float16, (512, 256), 1)[0].packed.desc.steps) < 3
    stats = run_folded(ls, fold)
    assert stats["folded"] == 1


@pytest.mark.parametrize("dtype", DTYPES)
def test_bias(dtype):
    ls = layers(dtype, (512, 320), 4, bias=True)
    assert run_folded(ls, 2)["folded"] == 1
    assert run_folded(ls, 4)["folded"] == 1


@pytest.mark.parametrize("fold", FOLDS)
def test_non_finite_x_poisons_its_own_rows_only(fold):
    ls = layers(torch.float16, (512, 250), 4)
    bad = ls[2]
    x = bad.x.clone()
    x[0, 5] = float("nan")
    x[0, 301] = float("inf")
    stats = run_folded(ls, fold, program=lambda s: [l.launch(s, x=x if l is bad else None) for l in ls])
    assert stats["folded"] == 1
    assert bool(torch.isnan(bad.y).all())
    assert all(bool(torch.isfinite(l.y).all()) for l in ls if l is not bad)


@pytest.mark.parametrize("fold", FOLDS)
def test_variable_geometry_members_keep_the_unfolded_kernel(fold):
    from tests.packed_model import zipf_codes

    dtype = torch.float16
    fin, fout = 2048, 1536  # (the shape and code law tests/test_compact_window_gpu.py shows to change the geometry)
    dev = torch.device("cuda", 0)
    key = "variable geometry"
    if key not in _LAYERS:
        # launches share a node only at one block size and LDS image: the layers of a kind carry the same codes -- one geometry
        gen = torch.Generator(device=dev).manual_seed(78)
        cu = torch.randint(-32768, 32768, (fout, fin // 8, 1), generator=gen, device=dev, dtype=torch.int32).to(torch.int16)
        u = [PackedLayer(fin, fout, 810 + i, dtype, codes=cu.clone()) for i in range(8)]
        cz = torch.from_numpy(zipf_codes(fout, fin // 8, 1.2, False, 7)[:, :, None].astype("int64")).to(dev)
        v = [PackedLayer(fin, fout, 910 + i, dtype, codes=(cz - (cz >= 32768) * 65536).to(torch.int16)) for i in range(2)]
        _LAYERS[key] = (u, v)
    u, v = _LAYERS[key]
    assert all(l.packed.desc.variable_geometry for l in v) and not any(l.packed.desc.variable_geometry for l in u)
    assert len({int(l.packed.desc.waves) for l in u}) == 1 and len({int(l.packed.desc.waves) for l in v}) == 1
    # one chain: u0..u3 share a node (folded), v0 cannot join it, v1 joins v0 (variable geometry: never folded), u4..u7 a third node
    ls = u[:4] + v + u[4:]
    stats = run_folded(ls, fold)
    assert (stats["seen"], stats["merged"], stats["nodes_added"], stats["folded"]) == (10, 7, 3, 2)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("fold", FOLDS)
def test_two_shapes_alternating_fold_both_chains(fold, dtype):
    a, b = layers(dtype, (512, 256), 4), layers(dtype, (512, 320), 4)
    ls = [l for pair in zip(a, b) for l in pair]
    stats = run_folded(ls, fold, window=2, merge=4)  # A0 B0 open two nodes, the others join their own shape's
    assert (stats["seen"], stats["merged"], stats["nodes_added"], stats["folded"]) == (8, 6, 2, 2)


@pytest.mark.parametrize("fold", FOLDS)
def test_shared_x(fold):
    ls = layers(torch.float16, (512, 512), 6)
    assert run_folded(ls, fold)["folded"] == 1  # every member its own x
    shared = ls[1].x
    stats = run_folded(ls, fold, program=lambda s: [l.launch(s, x=shared if i in (1, 2, 4) else None) for i, l in enumerate(ls)])
    assert stats["folded"] == 1 and stats["merged"] == 5


def test_more_rows_in_a_group_than_threads_stays_unfolded():
    # The folded kernel finalizes one row per thread.  128 -> 16384: 1024 rows per group at about one lane-step per row and slice,
    # so the streams run two steps on eight waves -- 512 threads for 1024 rows.
    ls = layers(torch.float16, (128, 16384), 3)
    d = ls[0].packed.desc
    assert int(d.rows_per_group) > 64 * int(d.waves), f"{d.rows_per_group} rows per group, {d.waves} waves"
    stats = run_folded(ls, 2)
    assert stats["merged"] == 2 and stats["folded"] == 0
