"""The read-side layout harness (tests/x_layout.py) on numpy stand-ins for an entry: one that keeps the x contract and five that break
it the way an address mistake in a kernel or its launch code would.  Each stand-in computes fp32 row dot products from the buffer.
`check` must accept the first in every layout and reject each of the others in at least one named layout, through a NaN output or
a value mismatch -- the evidence that tests/test_x_layout_gpu.py would fail on a subtly wrong kernel, without running a broken kernel
on a GPU.  One class of mistake cannot reach an output at all (a padded row that is loaded from the wrong place and never stored):
the stand-ins load through a tape and `check_reads` names the region that was touched."""
import numpy as np
import pytest

from tests import x_layout as xl

BATCH, FIN, M = 5, 64, 6
TILE = 4            # the stand-ins take rows four at a time, as the matvec kernels do; rows past the batch are computed, not stored


def rows_bits(batch=BATCH, fin=FIN):
    """Distinct small fp16 values (k / 64, exact in fp16 and in the fp32 sums), none of them the poison."""
    v = ((np.arange(batch * fin) * 37 + 11) % 251 - 125).astype(np.float32) / 64
    return v.astype(np.float16).view(np.uint16).reshape(batch, fin)


W = (((np.arange(FIN * M) * 13 + 5) % 17 - 8).astype(np.float32) / 8).reshape(FIN, M)


class Tape:
    """The buffer as fp16, every load recorded as (first element, count)."""

    def __init__(self, buf):
        self.a, self.reads = buf.view(np.float16), []

    def load(self, first, count):
        self.reads.append((int(first), int(count)))
        v = np.full(count, np.nan, dtype=np.float32)          # behind the buffer: more poison
        got = self.a[first:first + count]
        v[:got.size] = got
        return v


def entry_ok(tape, x, xs, batch, fin, row_of=None, base=None, extra=0, clamp=None, bits=None):
    """y[b] = x[b * xs : b * xs + fin] @ W in fp32, in tiles of TILE rows; a padded row re-reads row batch - 1.  The keyword arguments
    are the mistakes of the broken stand-ins."""
    clamp = batch - 1 if clamp is None else clamp
    base = x if base is None else base
    y = np.zeros((batch, W.shape[1]), dtype=np.float32)
    for b0 in range(0, batch, TILE):
        for b in range(b0, b0 + TILE):
            r = b if b < batch else clamp
            byte = 2 * (r * (xs if row_of is None else row_of))
            if bits is not None:
                byte &= (1 << bits) - 1
            v = tape.load(base + byte // 2, fin + extra)
            acc = v[:fin] @ W
            if extra:
                acc = acc + v[fin:] @ W[:extra]
            if b < batch:
                y[b] = acc
    return y


def entry_stride_is_fin(tape, x, xs, batch, fin):
    """in_features where the stride belongs."""
    return entry_ok(tape, x, xs, batch, fin, row_of=fin)


def entry_ignores_offset(offset):
    """Reads from the allocation's aligned start, not from the pointer it was given."""
    return lambda tape, x, xs, batch, fin: entry_ok(tape, x, xs, batch, fin, base=x - offset)


def entry_reads_past_the_row(tape, x, xs, batch, fin):
    """One 16-byte piece past the end of each row, accumulated."""
    return entry_ok(tape, x, xs, batch, fin, extra=8)


def entry_clamps_to_batch(tape, x, xs, batch, fin):
    """Rows >= batch clamped to row `batch`, not batch - 1."""
    return entry_ok(tape, x, xs, batch, fin, clamp=batch)


def entry_truncates(bits):
    """The byte offset of a row kept to `bits` bits."""
    return lambda tape, x, xs, batch, fin: entry_ok(tape, x, xs, batch, fin, bits=bits)


def run(entry, layout, batch=BATCH, fin=FIN):
    placed = xl.place(rows_bits(batch, fin), layout)
    tape = Tape(placed.buf)
    return entry(tape, placed.win.start, placed.win.xs, batch, fin), placed, tape


def flat_of(placed):
    """The correct stand-in on the same (materialised) rows in the flat layout."""
    flat = xl.place(placed.rows, "flat")
    return entry_ok(Tape(flat.buf), flat.win.start, flat.win.xs, *placed.rows.shape)


def rejected(entry, layout, **kw):
    got, placed, _ = run(entry, layout, **kw)
    with pytest.raises(AssertionError) as e:
        xl.check(got, flat_of(placed), placed.win, "stand-in")
    return str(e.value)


def accepted(entry, layout, **kw):
    got, placed, tape = run(entry, layout, **kw)
    xl.check(got, flat_of(placed), placed.win, "stand-in")
    return placed, tape


@pytest.mark.parametrize("fin", [64, 256])
def test_layouts_are_what_the_table_says(fin):
    expect = {"flat": (0, fin), "gap8": (0, fin + 8), "slice": (8, 3 * fin + 40), "bcast": (0, 0), "overlap": (0, 8), "odd": (0, fin + 1),
              "off1": (1, fin + 4), "off2": (2, fin + 6), "off4": (4, fin + 3)}
    assert list(xl.LAYOUTS) == list(expect)
    assert xl.POISON == 0x7FFF and xl.PAD == 24
    assert np.isnan(np.array([xl.POISON], dtype=np.uint16).view(np.float16)[0])                                   # fp16
    assert np.isnan((np.array([xl.POISON], dtype=np.uint32) << 16).view(np.float32)[0])                          # bf16
    assert xl.nan_mask(np.array([0x7FFF, 0x7C00, 0x3C00], np.uint16), "float16").tolist() == [True, False, False]
    assert xl.nan_mask(np.array([0x7FFF, 0x7F80, 0x3F80], np.uint16), "bfloat16").tolist() == [True, False, False]
    for layout, (offset, xs) in expect.items():
        win = xl.Window(layout, BATCH, fin)
        assert (win.xs, win.ptr(4096 + 16) & 31) == (xs, 2 * offset)
        assert win.size == xl.PAD + offset + (BATCH - 1) * xs + fin + xl.PAD
        assert int(win.inside().sum()) == (fin if xs == 0 else (BATCH - 1) * min(xs, fin) + fin)
        assert win.region(0) == win.region(win.start - 1) == "front pad" and win.region(win.size - 1) == "back pad"
        assert win.region(win.start) == "row 0" and win.region(win.row(BATCH - 1) + fin) == "back pad"
        if xs > fin:
            assert win.region(win.row(0) + fin) == "gap behind row 0" and win.region(win.row(1)) == "row 1"
        aligned = offset % 8 == 0 and xs % 8 == 0
        assert aligned == (layout not in xl.MISALIGNED)
    assert xl.Window("slice", BATCH, fin).ptr(4096 + 16) & 31 == 16
    assert xl.Window("flat", 16, 384, stride=(1 << 22) - 8).xs == (1 << 22) - 8


@pytest.mark.parametrize("layout", list(xl.LAYOUTS))
def test_placed_buffer_is_poison_outside_the_windows(layout):
    rows = rows_bits()
    placed = xl.place(rows, layout)
    inside = placed.win.inside()
    assert (placed.buf[~inside] == xl.POISON).all() and not (placed.buf[inside] == xl.POISON).any()
    assert (placed.buf[:xl.PAD] == xl.POISON).all() and (placed.buf[-xl.PAD:] == xl.POISON).all()
    for b in range(BATCH):
        np.testing.assert_array_equal(placed.buf[placed.win.row(b):placed.win.row(b) + FIN], placed.rows[b])
    if layout == "bcast":
        assert (placed.rows == rows[0]).all()
    elif layout == "overlap":
        np.testing.assert_array_equal(placed.rows[1, :FIN - 8], placed.rows[0, 8:])      # the rows share their elements
    else:
        assert placed.rows is not None and np.array_equal(placed.rows, rows)


@pytest.mark.parametrize("batch", [1, 4, 5])
@pytest.mark.parametrize("layout", list(xl.LAYOUTS))
def test_the_correct_entry_is_accepted(layout, batch):
    placed, tape = accepted(entry_ok, layout, batch=batch)
    xl.check_reads(tape.reads, placed.win, "stand-in")
    want = placed.rows.view(np.float16).astype(np.float32) @ W
    np.testing.assert_array_equal(flat_of(placed), want)


@pytest.mark.parametrize("layout,region", [("gap8", "gap behind row 0"), ("slice", "gap behind row 0"), ("odd", "gap behind row 0"),
                                           ("off1", "gap behind row 0"), ("bcast", "back pad"), ("overlap", "back pad")])
def test_in_features_where_the_stride_belongs_is_rejected(layout, region):
    accepted(entry_stride_is_fin, "flat")                    # invisible in the layout the Python wrappers pass
    msg = rejected(entry_stride_is_fin, layout)
    win = xl.Window(layout, BATCH, FIN)
    assert "are NaN, first at row 1" in msg, msg             # row 1 is read at x + in_features: it meets the poison behind row 0 ...
    if layout == "overlap":                                  # ... or, 56 elements late in the stream, the poison behind the last row
        assert win.region(win.start + FIN) == f"row {BATCH - 1}" and win.region(win.start + 2 * FIN - 1) == region
    else:
        assert win.region(win.start + FIN + (FIN if layout == "slice" else 0)) == region
        assert win.region(win.start + 2 * FIN - 1) in (region, "row 1")


@pytest.mark.parametrize("layout", ["slice", "off1", "off2", "off4"])
def test_ignored_pointer_offset_is_rejected(layout):
    offset = xl.LAYOUTS[layout][0]
    for other in ("flat", "gap8", "bcast", "overlap", "odd"):          # offset 0: nothing to ignore
        accepted(entry_ignores_offset(xl.LAYOUTS[other][0]), other)
    msg = rejected(entry_ignores_offset(offset), layout)
    assert "are NaN, first at row 0, column 0" in msg, msg
    win = xl.Window(layout, BATCH, FIN)
    assert win.region(win.start - offset) == "front pad"


@pytest.mark.parametrize("layout,first,region", [("flat", 0, "row 1"), ("gap8", 0, "gap behind row 0"), ("slice", 0, "gap behind row 0"),
                                                  ("bcast", 0, "back pad"), ("overlap", BATCH - 1, "back pad"), ("odd", 0, "gap behind row 0")])
def test_piece_past_the_end_of_a_row_is_rejected(layout, first, region):
    msg = rejected(entry_reads_past_the_row, layout)
    win = xl.Window(layout, BATCH, FIN)
    assert win.region(win.row(first) + FIN) == region
    if region.startswith("row"):        # flat: the piece is the next row's head -- wrong values; only the last row meets the back pad
        assert "differ from the flat layout's, first at row 0" in msg or f"are NaN, first at row {BATCH - 1}" in msg, msg
        assert win.region(win.row(BATCH - 1) + FIN) == "back pad"
    elif layout == "overlap":           # the piece lies inside the stream for every row but the last: wrong values there, NaN in the last
        assert f"are NaN, first at row {BATCH - 1}" in msg, msg
    else:
        assert "are NaN, first at row 0" in msg, msg


@pytest.mark.parametrize("layout,region", [("flat", "back pad"), ("gap8", "back pad"), ("slice", "region behind the buffer"),
                                           ("odd", "back pad"), ("overlap", "back pad")])
def test_padded_row_clamped_to_row_batch_is_rejected_by_its_reads(layout, region):
    """Rows >= batch of the last tile are computed and never stored: loading them from row `batch` changes no output, so `check`
    cannot see it (nor can the GPU test: there the mistake is a read behind the buffer).  The tape does."""
    placed, tape = accepted(entry_clamps_to_batch, layout)
    with pytest.raises(AssertionError) as e:
        xl.check_reads(tape.reads, placed.win, "clamp")
    assert f"in the {region}" in str(e.value), str(e.value)
    placed, tape = accepted(entry_clamps_to_batch, layout, batch=TILE)       # a whole tile: nothing is padded
    xl.check_reads(tape.reads, placed.win, "clamp")
    placed, tape = accepted(entry_clamps_to_batch, "bcast")                  # stride 0: row `batch` is row 0
    xl.check_reads(tape.reads, placed.win, "clamp")


@pytest.mark.parametrize("layout,bits,row,region", [("slice", 10, 3, "gap behind row 0"), ("gap8", 9, 4, "row 0"), ("flat", 9, 4, "row 0"),
                                                     ("odd", 9, 4, "row 0")])
def test_row_offset_truncated_to_n_bits_is_rejected(layout, bits, row, region):
    """A 32-bit row offset wraps at 4 GiB; the same mistake with `bits` bits wraps inside a buffer of a few hundred bytes.  The wrapped
    row is read from an earlier row or from the gap behind it."""
    win = xl.Window(layout, BATCH, FIN)
    for b in range(BATCH):
        assert (2 * b * win.xs >= 1 << bits) == (b >= row), (b, win.xs)      # `row` is the first row whose offset wraps
    wrapped = win.start + ((2 * row * win.xs) & ((1 << bits) - 1)) // 2
    assert win.region(wrapped) == region
    accepted(entry_truncates(bits), layout, batch=row)                       # invisible while every offset fits
    msg = rejected(entry_truncates(bits), layout)
    if region.startswith("gap"):
        assert f"are NaN, first at row {row}" in msg, msg
    else:
        assert f"first at row {row}" in msg, msg
    accepted(entry_truncates(bits), "bcast")                                 # stride 0: nothing to wrap
    accepted(entry_truncates(32), layout)


def test_every_broken_stand_in_is_rejected_somewhere_and_the_correct_one_nowhere():
    broken = {"stride": entry_stride_is_fin, "past": entry_reads_past_the_row, "wrap": entry_truncates(9)}
    for layout in xl.LAYOUTS:
        accepted(entry_ok, layout)
        broken["offset"] = entry_ignores_offset(xl.LAYOUTS[layout][0])
    hits = {name: [] for name in list(broken) + ["offset", "clamp"]}
    for layout in xl.LAYOUTS:
        broken["offset"] = entry_ignores_offset(xl.LAYOUTS[layout][0])
        for name, entry in broken.items():
            got, placed, _ = run(entry, layout)
            try:
                xl.check(got, flat_of(placed), placed.win, name)
            except AssertionError:
                hits[name].append(layout)
        got, placed, tape = run(entry_clamps_to_batch, layout)
        try:
            xl.check_reads(tape.reads, placed.win, "clamp")
        except AssertionError:
            hits["clamp"].append(layout)
    assert all(hits.values()), hits
    assert "flat" not in hits["stride"] and "flat" not in hits["offset"]     # what the rest of the suite passes shows neither
    assert set(hits["offset"]) == {"slice", "off1", "off2", "off4"}


def test_wrong_values_are_rejected():
    got, placed, _ = run(entry_ok, "gap8")
    want = flat_of(placed)
    want[2, 3] = np.nextafter(want[2, 3], np.float32(np.inf))
    with pytest.raises(AssertionError, match="first at row 2, column 3"):
        xl.check(got, want, placed.win)
    bits = np.array([[0x3C00, 0x7FFF]], dtype=np.uint16)
    with pytest.raises(AssertionError, match="are NaN, first at row 0, column 1"):
        xl.check(bits, bits, xl.Window("flat", 1, FIN), dt="bfloat16")
