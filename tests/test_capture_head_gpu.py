"""Regrouping the head of a run of captured packed 1x16 matvecs (capture_overlap.h, "Regrouping the head"; tuning key
packed_capture_head).  Every case makes the same calls eagerly, captures them with the key off and with the key on, replays each
graph 20 times and compares bit for bit: the regrouped capture must leave the bits of the eager pass and of the capture with the
key off, and the callers' accumulator cells must be back at zero.  What happened is read from aqlm_hip_capture_overlap_stats_ex:
`head_regrouped` runs, `head_moved` launches that gave up a node of their own, `head_refused` scripts that stopped early.
Layers of 512 -> 256 and 512 -> 320 as in tests/test_capture_overlap_gpu.py (16 rows per group); every second layer brings its own
cells.  Defaults unless a case says otherwise: window 2, merge 4, min_run 8, the default fold."""
import pytest
import torch

from tests.test_group_fold_gpu import PackedLayer, bits, layers, tuned

pytestmark = pytest.mark.gpu

REPLAYS = 20
DTYPES = [torch.float16, torch.bfloat16]
A, B = (512, 256), (512, 320)
CLASSIC = ("seen", "relaxed", "kept_conflict", "kept_window", "runs_broken", "api_failures")
DEFAULTS = dict(packed_capture_window=2, packed_capture_merge=4, packed_capture_min_run=8, packed_group_fold=0)


def captured(program, outputs, head, keys):
    """the program captured at packed_capture_head = `head`, replayed; -> (bit patterns of the outputs, counters of the capture)"""
    from aqlm_amd import _native

    for t in outputs():
        t.zero_()
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    with tuned(**dict(DEFAULTS, **keys, packed_capture_head=head)):
        _native.capture_overlap_stats(reset=True)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            program(torch.cuda.current_stream())
        stats = _native.capture_overlap_stats()
    with torch.cuda.stream(stream):
        for _ in range(REPLAYS):
            graph.replay()
    stream.synchronize()
    assert stats["api_failures"] == 0 and stats["merge_refused"] == 0 and stats["head_refused"] == 0, _native.last_error()
    assert stats["seen"] == stats["relaxed"] + stats["kept_conflict"] + stats["kept_window"] + stats["runs_broken"]
    return [bits(t).clone() for t in outputs()], stats


def run_head(ls, program=None, outputs=None, **keys):
    """Eager, captured with the key off, captured with the key on.  -> (counters with the key on, counters with the key off)"""
    ls = list(ls)
    program = program or (lambda s: [l.launch(s) for l in ls])
    outputs = outputs or (lambda: [l.y for l in ls])
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        program(stream)
    stream.synchronize()
    want = [bits(t).clone() for t in outputs()]
    assert all(bool((w != 0).any()) for w in want)
    plain, off = captured(program, outputs, 0, keys)
    assert (off["head_regrouped"], off["head_moved"]) == (0, 0)
    got, on = captured(program, outputs, 1, keys)
    for i, (g, p, w) in enumerate(zip(got, plain, want)):
        assert torch.equal(g, w), f"output {i}: the regrouped capture differs from the eager pass"
        assert torch.equal(g, p), f"output {i}: the regrouped capture differs from the capture at packed_capture_head = 0"
    for i, l in enumerate(ls):
        if l.cells is not None:
            assert not bool(l.cells.any()), f"layer {i}: accumulator cells not back at zero"
    with torch.cuda.stream(stream):  # the cells inside the packed buffers: a cell left dirty would show in the next call
        program(stream)
    stream.synchronize()
    for i, (t, w) in enumerate(zip(outputs(), want)):
        assert torch.equal(bits(t), w), f"output {i}: an eager call after the replays differs (cells inside the packed buffer)"
    return on, off


def pick(stats, *names):
    return tuple(stats[n] for n in names)


def alternating(dtype, n):
    a, b = layers(dtype, A, (n + 1) // 2), layers(dtype, B, n // 2)
    return [(a if i % 2 == 0 else b)[i // 2] for i in range(n)]


@pytest.mark.parametrize("dtype", DTYPES)
def test_eight_alternating_launches_become_two_folded_nodes(dtype):
    on, off = run_head(alternating(dtype, 8))
    assert pick(on, "head_regrouped", "head_moved", "folded") == (1, 6, 2)
    assert pick(on, *CLASSIC) == pick(off, *CLASSIC) == (8, 0, 0, 7, 1, 0)


def test_seven_launches_are_left_alone():
    on, off = run_head(alternating(torch.float16, 7))
    assert on == off and on["head_regrouped"] == 0


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_ten_launch_program_of_the_overlap_tests(dtype):
    a, b = layers(dtype, A, 7), layers(dtype, B, 3)
    ls = [a[0], b[0], a[1], b[1], a[2], b[2], a[3], a[4], a[5], a[6]]  # A B A B A B A A | A A
    on, off = run_head(ls)
    assert pick(on, "seen", "runs_broken", "relaxed", "kept_window") == (10, 1, 1, 8)
    assert pick(on, *CLASSIC) == pick(off, *CLASSIC)
    # groups {A0 A1 A2 A3} {B0 B1 B2} {A4}; the ninth launch is relaxed, the tenth joins the third node
    assert pick(on, "head_regrouped", "head_moved", "folded", "merged") == (1, 5, 1, 1)


@pytest.mark.parametrize("n", [16, 24])
def test_longer_stacks_regroup_their_head_once(n):
    on, off = run_head(alternating(torch.float16, n))
    assert pick(on, "head_regrouped", "head_moved") == (1, 6)
    assert pick(on, *CLASSIC) == pick(off, *CLASSIC) and on["merged"] == off["merged"]
    assert on["folded"] == n // 4  # every node of the step holds four launches


def test_hazards_in_the_head_leave_it_as_issued():
    dtype = torch.float16
    ls = alternating(dtype, 9)
    again = ls[:3] + [ls[0]] + ls[3:]  # the same layer twice (its y, and its cells, are written twice)
    on, off = run_head(again, outputs=lambda: [l.y for l in ls])
    assert on["head_regrouped"] == 0 and on["kept_conflict"] == 1 and pick(on, *CLASSIC) == pick(off, *CLASSIC)
    # a y that aliases an earlier x: launch 5 writes into what launch 1 reads
    x0 = ls[0].x.clone()
    xa = torch.zeros_like(x0)

    def program(s):
        xa.copy_(x0)  # (a torch node: every replay starts from the same x)
        for i, l in enumerate(ls[:8]):
            if i == 0:
                l.launch(s, x=xa)
            elif i == 4:  # 512 -> 256, into the first half of xa
                y, l.y = l.y, xa[:, :256]
                try:
                    l.launch(s)
                finally:
                    l.y = y
            else:
                l.launch(s)

    outs = lambda: [l.y for i, l in enumerate(ls[:8]) if i != 4] + [xa]  # noqa: E731
    on, off = run_head(ls[:8], program=program, outputs=outs)
    assert on["head_regrouped"] == 0 and on["kept_conflict"] == 1 and pick(on, *CLASSIC) == pick(off, *CLASSIC)


def test_a_torch_op_starts_the_head_over():
    ls = alternating(torch.float16, 14)
    mid = torch.zeros_like(ls[0].y)

    def program(s):
        for l in ls[:5]:
            l.launch(s)
        torch.add(ls[0].y, 1.0, out=mid)  # a foreign node
        for l in ls[5:]:
            l.launch(s)

    on, off = run_head(ls, program=program, outputs=lambda: [l.y for l in ls] + [mid])
    assert pick(on, "runs_broken", "head_regrouped", "head_moved") == (2, 1, 6)  # only the second run
    assert pick(on, *CLASSIC) == pick(off, *CLASSIC)


def test_variable_geometry_and_three_byte_members_keep_a_node_each():
    from aqlm_amd import _native
    from tests.packed_model import zipf_codes

    dtype = torch.float16
    dev = torch.device("cuda", 0)
    fin, fout = 2048, 1536  # (the shape and code law tests/test_compact_window_gpu.py shows to change the geometry)
    cz = torch.from_numpy(zipf_codes(fout, fin // 8, 1.2, False, 7)[:, :, None].astype("int64")).to(dev)
    v = PackedLayer(fin, fout, 920, dtype, codes=(cz - (cz >= 32768) * 65536).to(torch.int16))
    assert v.packed.desc.variable_geometry
    with tuned(packed_entry_bytes=3):
        t = PackedLayer(512, 256, 930, dtype).own_cells()
    assert int(t.packed.desc.entry_bytes) == 3
    a = layers(dtype, A, 6)
    ls = [a[0], v, a[1], t, a[2], a[3], a[4], a[5]]
    on, off = run_head(ls)
    # groups {a0 a1 a2 a3} {v} {t} {a4 a5}: v keeps its node, t moves into the third node as the launch it was, four nodes go
    assert pick(on, "head_regrouped", "head_moved", "folded") == (1, 4, 1)
    assert pick(on, *CLASSIC) == pick(off, *CLASSIC)
    assert _native.get_tuning("packed_entry_bytes") == 0


def test_window_of_one_regroups_and_stays_a_chain():
    on, off = run_head(alternating(torch.float16, 12), packed_capture_window=1)
    assert pick(on, "head_regrouped", "head_moved", "relaxed") == (1, 6, 0)
    assert pick(on, *CLASSIC) == pick(off, *CLASSIC)


def test_merge_of_one_regroups_nothing():
    on, off = run_head(alternating(torch.float16, 10), packed_capture_merge=1)
    assert on == off and on["head_regrouped"] == 0 and on["merged"] == 0


@pytest.mark.parametrize("dtype", DTYPES)
def test_three_launches_at_min_run_three_share_an_unfolded_node(dtype):
    on, off = run_head(layers(dtype, A, 3), packed_capture_min_run=3)
    assert pick(on, "head_regrouped", "head_moved", "folded") == (1, 2, 0)
    assert pick(on, *CLASSIC) == pick(off, *CLASSIC) == (3, 0, 0, 2, 1, 0)


def test_more_rows_in_a_group_than_threads_stays_unfolded():
    ls = layers(torch.float16, (128, 16384), 4)  # (tests/test_group_fold_gpu.py: 1024 rows per group on 512 threads)
    d = ls[0].packed.desc
    assert int(d.rows_per_group) > 64 * int(d.waves), f"{d.rows_per_group} rows per group, {d.waves} waves"
    on, off = run_head(ls, packed_capture_min_run=4)
    assert pick(on, "head_regrouped", "head_moved", "folded") == (1, 3, 0)


def test_the_same_program_captured_twice():
    ls = alternating(torch.float16, 10)
    first, _ = run_head(ls)
    second, _ = run_head(ls)
    assert first == second and first["head_regrouped"] == 1
