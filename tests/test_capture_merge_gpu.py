"""Captured packed 1x16 matvecs that share a graph node (include/aqlm_hip.h, "Grouped launches"; tuning key packed_capture_merge).
Every case makes the same calls eagerly and under capture, replays the graph 20 times and compares bit for bit; what the planner
decided is read from aqlm_hip_capture_overlap_stats_ex: `merged` launches joined a node, `nodes_added` added one of their own.
Small prepacked 1x16g8 layers as in tests/test_capture_overlap_gpu.py (512 -> 256 / 320 / 512, 16 slices), float16 and bfloat16;
runs relax (and join) from their second launch on."""
import contextlib
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

REPLAYS = 20
DTYPES = [torch.float16, torch.bfloat16]


class PackedLayer:
    def __init__(self, fin, fout, seed, dtype=torch.float16, codes=None):
        from aqlm_amd.inference_kernels import hip_kernel as hk

        dev = torch.device("cuda", 0)
        gen = torch.Generator(device=dev).manual_seed(seed)
        self.fin, self.fout, self.dtype = fin, fout, dtype
        if codes is None:
            codes = torch.randint(-32768, 32768, (fout, fin // 8, 1), generator=gen, device=dev, dtype=torch.int32).to(torch.int16)
        self.codes = codes
        self.codebooks = torch.randn((1, 65536, 1, 8), generator=gen, device=dev, dtype=torch.float32).to(dtype)
        self.scales = (0.5 + torch.rand((fout,), generator=gen, device=dev, dtype=torch.float32)).to(dtype)
        self.x = torch.randn((1, fin), generator=gen, device=dev, dtype=torch.float32).to(dtype)
        self.y = torch.zeros((1, fout), device=dev, dtype=dtype)
        self.packed = hk.prepack_1x16(self.codes, 8, codebooks=self.codebooks)
        assert self.packed is not None and self.packed.desc.codebook_absmax > 0

    def launch(self, stream, x=None, y=None, cells=None):
        from aqlm_amd import _native

        x = self.x if x is None else x
        y = self.y if y is None else y
        head = (ctypes.byref(self.packed.desc), self.packed.data_ptr(), self.codebooks.data_ptr(), self.scales.data_ptr(), None,
                x.data_ptr(), y.data_ptr(), x.shape[0], x.stride(0), y.stride(0), _native.F16 if self.dtype == torch.float16 else _native.BF16)
        if cells is None:
            rc = _native.lib.aqlm_hip_gemv_1x16_packed(*head, None, 0, stream.cuda_stream)
        else:
            rc = _native.lib.aqlm_hip_gemv_1x16_packed_cells(*head, cells.data_ptr(), cells.numel() * 8, stream.cuda_stream)
        _native.check(rc)


_LAYERS = {}


def layers(dtype, shape, n, first_seed=0):
    """`n` independent layers of one shape (built once per dtype and shape, shared by the cases)"""
    have = _LAYERS.setdefault((dtype, shape), [])
    while len(have) < n:
        have.append(PackedLayer(shape[0], shape[1], 500 + 31 * len(have) + shape[1] + first_seed, dtype))
    return have[:n]


def run_both(program, outputs):
    """Eager first, then captured and replayed; asserts that every replay leaves the bits of the eager pass, that the counters add
    up and that no rewrite of a node was refused; returns the counters of the capture."""
    from aqlm_amd import _native

    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        program(stream)
    stream.synchronize()
    want = [t.clone() for t in outputs()]
    for t in outputs():
        t.zero_()
    torch.cuda.synchronize()
    _native.capture_overlap_stats(reset=True)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        program(torch.cuda.current_stream())
    stats = _native.capture_overlap_stats()
    with torch.cuda.stream(stream):
        for _ in range(REPLAYS):
            graph.replay()
    stream.synchronize()
    for i, (g, w) in enumerate(zip(outputs(), want)):
        assert bool(w.float().abs().sum() > 0) or w.dtype == torch.int64
        assert torch.equal(g, w), f"output {i} of the captured replay differs from the eager pass"
    assert stats["api_failures"] == 0 and stats["merge_refused"] == 0, _native.last_error()
    assert stats["seen"] == stats["relaxed"] + stats["kept_conflict"] + stats["kept_window"] + stats["runs_broken"]
    assert stats["merged"] <= stats["kept_window"] and stats["nodes_added"] == stats["seen"] - stats["merged"]
    return stats


@contextlib.contextmanager
def capture(window, merge, min_run=1):
    from aqlm_amd import _native

    keys = ("packed_capture_window", "packed_capture_merge", "packed_capture_min_run")
    old = [_native.get_tuning(k) for k in keys]
    for k, v in zip(keys, (window, merge, min_run)):
        _native.set_tuning(k, v)
    try:
        yield
    finally:
        for k, v in zip(keys, old):
            _native.set_tuning(k, v)


def pick(stats, *names):
    return tuple(stats[n] for n in names)


@pytest.mark.parametrize("dtype", DTYPES)
def test_eight_layers_of_one_shape_share_two_nodes(dtype):
    ls = layers(dtype, (512, 256), 8)
    with capture(2, 4):  # two nodes open the run; the other six join them in turn, oldest node first
        stats = run_both(lambda s: [l.launch(s) for l in ls], lambda: [l.y for l in ls])
    assert pick(stats, "seen", "runs_broken", "relaxed", "kept_window", "merged", "nodes_added") == (8, 1, 1, 6, 6, 2)
    with capture(2, 3):  # groups of three: 3 + 3, then a third node that the eighth launch joins
        stats = run_both(lambda s: [l.launch(s) for l in ls], lambda: [l.y for l in ls])
    assert pick(stats, "seen", "merged", "nodes_added") == (8, 5, 3)


@pytest.mark.parametrize("dtype", DTYPES)
def test_alternating_shapes_never_share_a_node(dtype):
    a, b = layers(dtype, (512, 256), 6), layers(dtype, (512, 320), 6)
    ls = [l for pair in zip(a, b) for l in pair]
    with capture(2, 4):  # A0 B0 open; A1..A3 and B1..B3 join; A4 and B4 wait for the full nodes; A5 and B5 join those
        stats = run_both(lambda s: [l.launch(s) for l in ls], lambda: [l.y for l in ls])
    assert pick(stats, "seen", "runs_broken", "relaxed", "merged", "nodes_added") == (12, 1, 1, 8, 4)
    with capture(1, 4):  # a single chain: the neighbour is always the other shape
        stats = run_both(lambda s: [l.launch(s) for l in ls], lambda: [l.y for l in ls])
    assert pick(stats, "seen", "relaxed", "merged", "nodes_added") == (12, 0, 0, 12)


@pytest.mark.parametrize("dtype", DTYPES)
def test_variable_geometry_layers_join_only_their_own_instance(dtype):
    from tests.packed_model import zipf_codes

    fin, fout = 2048, 1536  # (the shape and code law tests/test_compact_window_gpu.py shows to change the geometry)
    dev = torch.device("cuda", 0)
    # Launches share a node only at one block size and LDS image, and at this size the repack picks the waves per workgroup by the
    # layer's codes.  So the layers of a kind carry the same codes -- one geometry -- with their own codebooks, scales, x and y.
    gen = torch.Generator(device=dev).manual_seed(77)
    cu = torch.randint(-32768, 32768, (fout, fin // 8, 1), generator=gen, device=dev, dtype=torch.int32).to(torch.int16)
    u = [PackedLayer(fin, fout, 800 + i, dtype, codes=cu.clone()) for i in range(3)]
    cz = torch.from_numpy(zipf_codes(fout, fin // 8, 1.2, False, 7)[:, :, None].astype("int64")).to(dev)
    v = [PackedLayer(fin, fout, 900 + i, dtype, codes=(cz - (cz >= 32768) * 65536).to(torch.int16)) for i in range(2)]
    assert all(l.packed.desc.variable_geometry for l in v) and not any(l.packed.desc.variable_geometry for l in u)
    assert len({int(l.packed.desc.waves) for l in u}) == 1 and len({int(l.packed.desc.waves) for l in v}) == 1
    ls = [u[0], u[1], v[0], v[1], u[2]]
    with capture(1, 4):  # one chain: u1 joins u0, v0 cannot, v1 joins v0, u2 cannot
        stats = run_both(lambda s: [l.launch(s) for l in ls], lambda: [l.y for l in ls])
    assert pick(stats, "seen", "merged", "nodes_added") == (5, 2, 3)
    ls = [u[0], v[0], u[1], v[1], u[2]]
    with capture(2, 4):  # two chains: each kind finds its own node
        stats = run_both(lambda s: [l.launch(s) for l in ls], lambda: [l.y for l in ls])
    assert pick(stats, "seen", "relaxed", "merged", "nodes_added") == (5, 1, 3, 2)


def test_hazards_keep_a_launch_out_of_the_node():
    dtype = torch.float16
    a, c, d = layers(dtype, (512, 256), 3)
    y2 = torch.zeros_like(a.y)
    with capture(1, 4):  # the same layer twice: the cells inside its packed buffer are shared; a third layer joins the second node
        stats = run_both(lambda s: [a.launch(s), a.launch(s, y=y2), c.launch(s)], lambda: [a.y, y2, c.y])
    assert pick(stats, "seen", "kept_conflict", "merged", "nodes_added") == (3, 1, 1, 2)
    cells = torch.zeros((256,), dtype=torch.int64, device=a.x.device)
    with capture(1, 4):  # caller's cells shared by two layers, a third with the library's own
        stats = run_both(lambda s: [a.launch(s, cells=cells), c.launch(s, cells=cells), d.launch(s)], lambda: [a.y, c.y, d.y, cells])
    assert pick(stats, "seen", "kept_conflict", "merged", "nodes_added") == (3, 1, 1, 2)
    p, q, r = layers(dtype, (512, 512), 3)
    yq = torch.zeros_like(q.y)
    with capture(2, 4):  # y of one launch is x of a later one
        stats = run_both(lambda s: [p.launch(s), r.launch(s), q.launch(s, x=p.y, y=yq)], lambda: [p.y, r.y, yq])
    assert pick(stats, "seen", "relaxed", "kept_conflict", "merged", "nodes_added") == (3, 1, 1, 0, 3)


def test_nothing_joins_a_node_from_before_a_broken_run():
    dtype = torch.float16
    a, b, c, d = layers(dtype, (512, 256), 4)
    mid = torch.zeros_like(a.y)

    def program(s):
        a.launch(s)
        b.launch(s)
        torch.add(a.y, 1.0, out=mid)  # a foreign node
        c.launch(s)
        d.launch(s)

    with capture(1, 4):
        stats = run_both(program, lambda: [a.y, b.y, c.y, d.y, mid])
    assert pick(stats, "seen", "runs_broken", "merged", "nodes_added") == (4, 2, 2, 2)
    side = torch.cuda.Stream()
    other = torch.zeros((64,), device=a.x.device)

    def waits(s):
        other.zero_()
        a.launch(s)
        b.launch(s)
        side.wait_stream(s)
        with torch.cuda.stream(side):
            other.add_(1.0)
        s.wait_stream(side)  # the capturing stream now also waits for the side stream's node
        c.launch(s)
        d.launch(s)

    with capture(1, 4):
        stats = run_both(waits, lambda: [a.y, b.y, c.y, d.y, other])
    assert pick(stats, "seen", "runs_broken", "merged", "nodes_added") == (4, 2, 2, 2)


def test_key_at_one_is_the_graph_without_grouped_launches():
    dtype = torch.float16
    a, b = layers(dtype, (512, 256), 3), layers(dtype, (512, 320), 3)
    ls = [l for pair in zip(a, b) for l in pair]
    with capture(2, 1):  # the counters tests/test_capture_overlap_gpu.py states for this program
        stats = run_both(lambda s: [l.launch(s) for l in ls], lambda: [l.y for l in ls])
    assert pick(stats, "seen", "runs_broken", "relaxed", "kept_window", "merged", "nodes_added") == (6, 1, 1, 4, 0, 6)
    with capture(1, 1):
        stats = run_both(lambda s: [l.launch(s) for l in ls], lambda: [l.y for l in ls])
    assert pick(stats, "seen", "runs_broken", "relaxed", "kept_window", "merged", "nodes_added") == (6, 0, 0, 6, 0, 6)
    with capture(2, 4, min_run=8):  # a run shorter than packed_capture_min_run: nothing relaxed, nothing joined
        stats = run_both(lambda s: [l.launch(s) for l in ls], lambda: [l.y for l in ls])
    assert pick(stats, "seen", "relaxed", "merged", "nodes_added") == (6, 0, 0, 6)


@pytest.mark.parametrize("dtype", DTYPES)
def test_window_of_one_is_a_chain_of_groups(dtype):
    ls = layers(dtype, (512, 320), 8)
    with capture(1, 4):
        stats = run_both(lambda s: [l.launch(s) for l in ls], lambda: [l.y for l in ls])
    assert pick(stats, "seen", "relaxed", "merged", "nodes_added") == (8, 0, 6, 2)


def test_the_same_program_captured_twice():
    ls = layers(torch.float16, (512, 256), 8)
    with capture(2, 4):
        first = run_both(lambda s: [l.launch(s) for l in ls], lambda: [l.y for l in ls])  # (its graph is gone when it returns)
        second = run_both(lambda s: [l.launch(s) for l in ls], lambda: [l.y for l in ls])
    assert first == second and first["merged"] == 6
