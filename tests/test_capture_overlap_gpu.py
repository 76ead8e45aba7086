"""Packed 1x16 matvecs captured into a hipGraph are ordered by the memory they touch (include/aqlm_hip.h, "Capture overlap").
Every case makes the same calls eagerly and under capture, replays the graph 20 times, compares bit for bit, and reads
aqlm_hip_capture_overlap_stats for what the planner decided.  Small prepacked 1x16g8 layers (512 -> 256 / 320 / 512): 16 slices,
the accumulator cells inside the packed buffer and the single-kernel finalize, like the large ones."""
import contextlib
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

REPLAYS = 20


class PackedLayer:
    def __init__(self, fin, fout, seed, rows=1):
        from aqlm_amd.inference_kernels import hip_kernel as hk

        dev = torch.device("cuda", 0)
        gen = torch.Generator(device=dev).manual_seed(seed)
        self.fin, self.fout, self.rows = fin, fout, rows
        self.codes = torch.randint(-32768, 32768, (fout, fin // 8, 1), generator=gen, device=dev, dtype=torch.int32).to(torch.int16)
        self.codebooks = torch.randn((1, 65536, 1, 8), generator=gen, device=dev, dtype=torch.float32).half()
        self.scales = (0.5 + torch.rand((fout,), generator=gen, device=dev, dtype=torch.float32)).half()
        self.x = torch.randn((rows, fin), generator=gen, device=dev, dtype=torch.float32).half()
        self.y = torch.zeros((rows, fout), device=dev, dtype=torch.float16)
        self.packed = hk.prepack_1x16(self.codes, 8, codebooks=self.codebooks)
        assert self.packed is not None and self.packed.desc.codebook_absmax > 0

    def launch(self, stream, x=None, y=None, cells=None):
        from aqlm_amd import _native

        x = self.x if x is None else x
        y = self.y if y is None else y
        head = (ctypes.byref(self.packed.desc), self.packed.data_ptr(), self.codebooks.data_ptr(), self.scales.data_ptr(), None,
                x.data_ptr(), y.data_ptr(), x.shape[0], x.stride(0), y.stride(0), _native.F16)
        if cells is None:
            rc = _native.lib.aqlm_hip_gemv_1x16_packed(*head, None, 0, stream.cuda_stream)
        else:
            rc = _native.lib.aqlm_hip_gemv_1x16_packed_cells(*head, cells.data_ptr(), cells.numel() * 8, stream.cuda_stream)
        _native.check(rc)


@pytest.fixture(scope="module")
def layers():
    assert torch.cuda.is_available()
    shapes = [(512, 256), (512, 320), (512, 256), (512, 320), (512, 256), (512, 320)]
    return [PackedLayer(fin, fout, 100 + i) for i, (fin, fout) in enumerate(shapes)]


def run_both(program, outputs):
    """`program(stream)` makes the calls; `outputs()` lists the tensors they leave.  Eager first, then captured and replayed;
    returns the planner's counters for the capture.  Asserts that every replay leaves the bits of the eager pass."""
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
    got = outputs()
    assert len(got) == len(want)
    with torch.cuda.stream(stream):
        for _ in range(REPLAYS):
            graph.replay()
    stream.synchronize()
    for i, (g, w) in enumerate(zip(got, want)):
        assert torch.equal(g, w), f"output {i} of the captured replay differs from the eager pass"
    assert stats["api_failures"] == 0, _native.last_error()
    assert stats["seen"] == stats["relaxed"] + stats["kept_conflict"] + stats["kept_window"] + stats["runs_broken"]
    return stats


@contextlib.contextmanager
def capture_window(n, min_run=1):
    """The cases below that count launches are stated for a window of 4 and for runs that relax from their second launch on; the
    library's defaults are a smaller window and runs that relax nothing until they are 8 launches long (capture_overlap.h)."""
    from aqlm_amd import _native

    old = _native.get_tuning("packed_capture_window"), _native.get_tuning("packed_capture_min_run")
    _native.set_tuning("packed_capture_window", n)
    _native.set_tuning("packed_capture_min_run", min_run)
    try:
        yield
    finally:
        _native.set_tuning("packed_capture_window", old[0])
        _native.set_tuning("packed_capture_min_run", old[1])


@pytest.fixture(autouse=True)
def relax_from_the_second_launch():
    """Every case runs with packed_capture_min_run = 1 unless it asks for the defaults itself."""
    from aqlm_amd import _native

    old = _native.get_tuning("packed_capture_min_run")
    _native.set_tuning("packed_capture_min_run", 1)
    yield
    _native.set_tuning("packed_capture_min_run", old)


@pytest.mark.parametrize("rows", [1, 2])
def test_independent_layers_are_relaxed(layers, rows):
    ls = layers[:4] if rows == 1 else [PackedLayer(512, 256 if i % 2 == 0 else 320, 200 + i, rows=2) for i in range(4)]
    with capture_window(4):
        stats = run_both(lambda s: [l.launch(s) for l in ls], lambda: [l.y for l in ls])
    assert (stats["seen"], stats["relaxed"], stats["runs_broken"]) == (4, 3, 1)


def test_true_chain_is_kept(layers):
    a, b = PackedLayer(512, 512, 300), layers[0]
    yb = torch.zeros_like(b.y)

    def program(s):
        a.launch(s)
        b.launch(s, x=a.y, y=yb)

    stats = run_both(program, lambda: [a.y, yb])
    assert (stats["seen"], stats["relaxed"], stats["kept_conflict"]) == (2, 0, 1)


def test_same_layer_twice_is_kept(layers):
    a = layers[0]
    y2 = torch.zeros_like(a.y)

    def program(s):
        a.launch(s)
        a.launch(s, y=y2)  # its own y, but the cells inside the packed buffer are shared

    stats = run_both(program, lambda: [a.y, y2])
    assert (stats["relaxed"], stats["kept_conflict"]) == (0, 1)
    stats = run_both(lambda s: [a.launch(s), a.launch(s)], lambda: [a.y])  # and with the same y
    assert (stats["relaxed"], stats["kept_conflict"]) == (0, 1)


def test_shared_caller_cells_are_kept(layers):
    a, b = layers[0], layers[1]
    cells = torch.zeros((max(a.fout, b.fout),), dtype=torch.int64, device=a.x.device)
    stats = run_both(lambda s: [a.launch(s, cells=cells), b.launch(s, cells=cells)], lambda: [a.y, b.y, cells])
    assert (stats["seen"], stats["relaxed"], stats["kept_conflict"]) == (2, 0, 1)
    own = torch.zeros_like(cells)  # each its own cells: the packed buffers are only read, nothing is shared
    stats = run_both(lambda s: [a.launch(s, cells=cells), b.launch(s, cells=own)], lambda: [a.y, b.y, cells, own])
    assert (stats["relaxed"], stats["kept_conflict"]) == (1, 0)


def test_output_aliasing_an_earlier_input_is_kept(layers):
    a, b = layers[0], layers[2]  # both 512 -> 256
    x0 = a.x.clone()
    xa = torch.zeros_like(a.x)
    yb = xa[:, :256]  # b writes into what a reads

    def program(s):
        xa.copy_(x0)  # (a torch node: every replay starts from the same x)
        a.launch(s, x=xa)
        b.launch(s, y=yb)

    stats = run_both(program, lambda: [a.y, xa])
    assert (stats["seen"], stats["relaxed"], stats["kept_conflict"]) == (2, 0, 1)


def test_torch_ops_break_a_run_and_see_all_of_it(layers):
    a, b, c, d = layers[:4]
    mid = torch.zeros_like(a.y)
    total = torch.zeros((1,), dtype=torch.float32, device=a.x.device)

    def program(s):
        a.launch(s)
        b.launch(s)
        torch.add(a.y, 1.0, out=mid)  # a foreign node between two launches
        c.launch(s)
        d.launch(s)
        total.copy_((a.y.float().sum() + b.y.float().sum() + c.y.float().sum() + d.y.float().sum()).reshape(1))

    stats = run_both(program, lambda: [a.y, b.y, c.y, d.y, mid, total])
    assert (stats["seen"], stats["relaxed"], stats["runs_broken"]) == (4, 2, 2)


def test_window_bounds_the_launches_in_flight(layers):
    from aqlm_amd import _native

    with capture_window(4):  # the fifth and sixth of six independent launches wait for the first and second
        stats = run_both(lambda s: [l.launch(s) for l in layers], lambda: [l.y for l in layers])
    assert (stats["seen"], stats["runs_broken"], stats["relaxed"], stats["kept_window"]) == (6, 1, 3, 2)
    # the default window, as the library ships it: two chains
    assert _native.get_tuning("packed_capture_window") == 2
    stats = run_both(lambda s: [l.launch(s) for l in layers], lambda: [l.y for l in layers])
    assert (stats["seen"], stats["runs_broken"], stats["relaxed"], stats["kept_window"]) == (6, 1, 1, 4)


def test_defaults_leave_short_runs_in_stream_order(layers):
    """As shipped, a run relaxes nothing before it is 8 launches long: q/k/v-sized runs give the graph stream order gives (a graph
    with branches costs host time for every node), a stack of linears overlaps from its ninth launch on."""
    from aqlm_amd import _native

    more = layers + [PackedLayer(512, 256, 400 + i) for i in range(4)]
    _native.set_tuning("packed_capture_min_run", 8)  # (the autouse fixture puts its value back)
    assert _native.get_tuning("packed_capture_window") == 2
    stats = run_both(lambda s: [l.launch(s) for l in more[:3]], lambda: [l.y for l in more[:3]])
    assert (stats["seen"], stats["runs_broken"], stats["relaxed"], stats["kept_window"]) == (3, 1, 0, 2)
    stats = run_both(lambda s: [l.launch(s) for l in more], lambda: [l.y for l in more])
    assert (stats["seen"], stats["runs_broken"], stats["relaxed"], stats["kept_window"]) == (10, 1, 1, 8)


def test_window_of_one_is_stream_order(layers):
    with capture_window(1):
        stats = run_both(lambda s: [l.launch(s) for l in layers[:4]], lambda: [l.y for l in layers[:4]])
    assert (stats["seen"], stats["relaxed"]) == (4, 0)


def test_event_wait_breaks_a_run(layers):
    a, b = layers[0], layers[1]
    side = torch.cuda.Stream()
    other = torch.zeros((64,), device=a.x.device)

    def program(s):
        a.launch(s)
        side.wait_stream(s)
        with torch.cuda.stream(side):
            other.add_(1.0)
        s.wait_stream(side)  # the capturing stream now also waits for the side stream's node
        b.launch(s)

    def fresh(s):
        other.zero_()
        program(s)

    stats = run_both(fresh, lambda: [a.y, b.y, other])
    assert (stats["seen"], stats["relaxed"], stats["runs_broken"]) == (2, 0, 2)
