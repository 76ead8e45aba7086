"""The layout harness (tests/y_layout.py) on numpy stand-ins for an entry: one that keeps the contract and four that break it the way
an address mistake in a kernel or its launch code would.  `check` / `check_workspace` must accept the first and reject each of the
others, naming the region that was hit -- the evidence that tests/test_y_layout_gpu.py would fail on a subtly wrong kernel, without
running a broken kernel on a GPU."""
import numpy as np
import pytest

from tests import y_layout as yl

BATCH = 3
SHAPES = [48, 45, 46, 47]      # M & 3 = 0 .. 3, as in the GPU tests


def result(batch, M):
    """What the stand-ins compute: distinct bit patterns, none of them the sentinel."""
    r = (np.arange(batch * M, dtype=np.uint32) * 7 + 0x0101).astype(np.uint16).reshape(batch, M)
    assert not (r == yl.SENTINEL).any()
    return r


def entry_ok(buf, y, ys, batch, M, ws=None, ws_at=0, ws_bytes=0):
    """y[b * ys + m] for m < M; the workspace used up to its last advertised byte."""
    r = result(batch, M)
    for b in range(batch):
        buf[y + b * ys:y + b * ys + M] = r[b]
    if ws is not None:
        ws[ws_at:ws_at + ws_bytes] = 0xC3


def entry_stride_is_m(buf, y, ys, batch, M, **kw):
    """The slab offset computed with M where ys belongs."""
    r = result(batch, M)
    for b in range(batch):
        buf[y + b * M:y + b * M + M] = r[b]


def entry_no_tail_guard(buf, y, ys, batch, M, **kw):
    """The last tile of a row stores four elements although M % 4 of them exist."""
    r = result(batch, M)
    for b in range(batch):
        buf[y + b * ys:y + b * ys + M] = r[b]
        last = M // 4 * 4
        if last < M:
            buf[y + b * ys + last:y + b * ys + last + 4] = np.resize(r[b, last:], 4)


def entry_writes_in_front(buf, y, ys, batch, M, **kw):
    entry_ok(buf, y, ys, batch, M)
    buf[y - 1] = 0x1234


def entry_overruns_workspace(buf, y, ys, batch, M, ws=None, ws_at=0, ws_bytes=0):
    """A workspace formula that forgot a padded tile: one byte past the advertised size."""
    entry_ok(buf, y, ys, batch, M, ws, ws_at, ws_bytes)
    ws[ws_at + ws_bytes] = 0xC3


def run(entry, layout, M, batch=BATCH, ws_bytes=0):
    win = yl.Window(layout, batch, M)
    buf = yl.new_buffer(win)
    ws = yl.Workspace(ws_bytes)
    wbuf = yl.new_workspace(ws)
    entry(buf, win.start, win.ys, batch, M, ws=wbuf, ws_at=ws.start, ws_bytes=ws_bytes)
    return buf, wbuf


@pytest.mark.parametrize("M", SHAPES)
def test_layouts_are_what_the_table_says(M):
    expect = {"flat": (0, M), "gap4": (0, M + 4), "odd": (0, M + 1), "off1": (2, M + 4), "off2": (4, M + 6), "off3": (6, M + 3)}
    assert list(yl.LAYOUTS) == list(expect)
    for layout, (ptr7, ys) in expect.items():
        win = yl.Window(layout, BATCH, M)
        assert (win.ys, win.ptr(4096) & 7) == (ys, ptr7)
        assert win.size == yl.PAD + ptr7 // 2 + (BATCH - 1) * ys + M + yl.PAD
        assert int(win.inside().sum()) == BATCH * M
        assert win.region(0) == win.region(win.start - 1) == "front pad" and win.region(win.size - 1) == "back pad"
        assert win.region(win.start) == "row 0" and win.region(win.row(BATCH - 1) + M - 1) == f"row {BATCH - 1}"
        assert win.region(win.row(BATCH - 1) + M) == "back pad"
        if ys > M:
            assert win.region(win.row(0) + M) == "gap behind row 0"


@pytest.mark.parametrize("M", SHAPES)
@pytest.mark.parametrize("layout", list(yl.LAYOUTS))
def test_the_correct_entry_is_accepted(layout, M):
    base = yl.windows(run(entry_ok, "flat", M)[0], "flat", BATCH, M)
    np.testing.assert_array_equal(base, result(BATCH, M))
    buf, wbuf = run(entry_ok, layout, M, ws_bytes=4 * BATCH * M)
    got = yl.check(buf, layout, BATCH, M, base, "stand-in")
    np.testing.assert_array_equal(got, base)
    yl.check_workspace(wbuf, 4 * BATCH * M, "stand-in")


@pytest.mark.parametrize("M", SHAPES)
@pytest.mark.parametrize("layout", [k for k in yl.LAYOUTS if k != "flat"])
def test_row_written_at_b_times_m_is_rejected(layout, M):
    base = result(BATCH, M)
    yl.check(run(entry_stride_is_m, "flat", M)[0], "flat", BATCH, M, base)     # invisible in the layout the Python wrappers pass
    with pytest.raises(AssertionError) as e:
        yl.check(run(entry_stride_is_m, layout, M)[0], layout, BATCH, M, base, "stride")
    assert "gap behind row 0" in str(e.value), str(e.value)    # row 1 starts ys - M elements early


@pytest.mark.parametrize("layout", list(yl.LAYOUTS))
@pytest.mark.parametrize("M", [45, 46, 47])
def test_four_element_store_on_a_ragged_row_is_rejected(layout, M):
    base = result(BATCH, M)
    with pytest.raises(AssertionError) as e:
        yl.check(run(entry_no_tail_guard, layout, M)[0], layout, BATCH, M, base, "tail")
    msg = str(e.value)
    if layout == "flat":   # no gap: the spill lands in the next row (overwritten again by that row's own store) and in the back pad
        assert "back pad" in msg, msg
    else:
        assert "gap behind row 0" in msg, msg


def test_four_element_store_is_fine_where_rows_are_whole():
    for layout in yl.LAYOUTS:
        yl.check(run(entry_no_tail_guard, layout, 48)[0], layout, BATCH, 48, result(BATCH, 48))


@pytest.mark.parametrize("layout", list(yl.LAYOUTS))
def test_element_in_the_front_pad_is_rejected(layout):
    with pytest.raises(AssertionError) as e:
        yl.check(run(entry_writes_in_front, layout, 46)[0], layout, BATCH, 46, result(BATCH, 46), "front")
    assert "front pad" in str(e.value) and "(y + -1)" in str(e.value), str(e.value)


def test_byte_past_the_advertised_workspace_is_rejected():
    n = 4 * BATCH * 45
    buf, wbuf = run(entry_overruns_workspace, "off1", 45, ws_bytes=n)
    yl.check(buf, "off1", BATCH, 45, result(BATCH, 45))                         # y itself is right
    with pytest.raises(AssertionError) as e:
        yl.check_workspace(wbuf, n, "ws")
    assert "behind the workspace" in str(e.value) and "(0 behind its end)" in str(e.value), str(e.value)
    wbuf[yl.WS_PAD + n] = yl.WS_SENTINEL
    wbuf[yl.WS_PAD - 1] = 0
    with pytest.raises(AssertionError, match="in front of the workspace"):
        yl.check_workspace(wbuf, n, "ws")


def test_cells_must_be_zero_at_rest():
    ws = yl.Workspace(8 * 45)
    cells = yl.new_workspace(ws, zero_inside=True)
    yl.check_workspace(cells, 8 * 45, "cells", zero_at_rest=True)
    cells[ws.start + 8 * 44 + 3] = 1            # the last cell keeps a count
    with pytest.raises(AssertionError, match="not zero at rest.*cell 44"):
        yl.check_workspace(cells, 8 * 45, "cells", zero_at_rest=True)
    yl.check_workspace(cells, 8 * 45, "cells")   # ... which only the zero-at-rest check sees


def test_wrong_values_inside_the_windows_are_rejected():
    buf, _ = run(entry_ok, "odd", 47)
    base = result(BATCH, 47)
    base[2, 46] ^= 1
    with pytest.raises(AssertionError, match="first at row 2, column 46"):
        yl.check(buf, "odd", BATCH, 47, base)
