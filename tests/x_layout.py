"""Layout harness of the dense forward entries, read side: WHERE an entry reads x, the mirror of tests/y_layout.py.

An entry of include/aqlm_hip.h takes ``x`` and ``x_row_stride`` (elements) and promises to read the ``batch`` windows
``[b * xs, b * xs + in_features)`` behind ``x`` and nothing else of it.  A read cannot be seen, but what was read can: the harness
puts the rows into a larger 16-bit buffer in which every element outside the union of the windows is 0x7FFF -- a NaN in fp16 and in
bf16 alike -- with 24 such elements on either side, and ``check`` holds the result of the call to two statements:

  (a) no output is NaN: nothing outside the windows reached a sum (a padded row that is computed and never stored does not count);
  (b) the outputs equal, bit for bit, what the same entry gave for the same values in the ``flat`` layout (xs == in_features).

``bcast`` (stride 0: every row is row 0) and ``overlap`` (stride 8 < in_features) are legal inputs -- ``x.expand(B, -1)`` and
``t.unfold(0, fin, 8)`` reach the C ABI uncopied.  Their rows are not free: ``place`` returns the materialised [batch, fin] rows, which
the oracle and the flat baseline use.

Plain helper module: numpy only (tests/test_x_layout_host.py); the device tests upload ``Placed.buf``."""
import types

import numpy as np

PAD = 24            # poison elements on either side of the union of the x windows
POISON = 0x7FFF     # fp16: exponent 0x1f, mantissa 0x3ff; bf16: exponent 0xff, mantissa 0x7f -- a NaN in both
BASE_MOD32 = 16     # address of buffer element 0, mod 32: PAD elements (48 bytes) behind it lie on a 32-byte boundary

# name -> (pointer offset in elements from that boundary, stride as a function of in_features)
LAYOUTS = {
    "flat": (0, lambda fin: fin),             # what a fresh contiguous tensor passes
    "gap8": (0, lambda fin: fin + 8),         # the smallest legal gap
    "slice": (8, lambda fin: 3 * fin + 40),   # a column slice of a wider tensor, pointer & 31 == 16
    "bcast": (0, lambda fin: 0),              # x.expand(B, -1)
    "overlap": (0, lambda fin: 8),            # t.unfold(0, fin, 8)
    "odd": (0, lambda fin: fin + 1),          # misaligned rows: the plain gemv entries only
    "off1": (1, lambda fin: fin + 4),         # pointer & 15 == 2
    "off2": (2, lambda fin: fin + 6),         # pointer & 15 == 4
    "off4": (4, lambda fin: fin + 3),         # pointer & 15 == 8
}
ALIGNED = ("gap8", "slice", "overlap")        # 16-byte aligned pointer, stride % 8 == 0, 0 < stride: below every routing limit
MISALIGNED = ("odd", "off1", "off2", "off4")


class Window:
    """Where the rows of x lie in a buffer of `size` 16-bit elements: row b at [start + b * xs, start + b * xs + fin).  `stride`
    overrides the layout's (the stride-limit cases)."""

    def __init__(self, layout, batch, fin, stride=None):
        offset, xs = LAYOUTS[layout]
        self.layout, self.batch, self.fin = layout, int(batch), int(fin)
        self.offset = offset
        self.xs = int(xs(self.fin) if stride is None else stride)
        assert self.xs >= 0
        self.start = PAD + offset
        self.size = self.start + (self.batch - 1) * self.xs + self.fin + PAD

    def row(self, b):
        return self.start + b * self.xs

    def ptr(self, base_ptr):
        """Address of x[0, 0] in a buffer that starts at `base_ptr` (== BASE_MOD32 mod 32)."""
        assert base_ptr % 32 == BASE_MOD32, base_ptr
        p = base_ptr + 2 * self.start
        assert p % 32 == 2 * self.offset
        return p

    def region(self, i):
        """Name of the region element i of the buffer belongs to."""
        if i < self.start:
            return "front pad"
        if i >= self.row(self.batch - 1) + self.fin:
            return "back pad"
        if self.xs == 0:
            return "row 0"
        b, c = divmod(i - self.start, self.xs)
        if c < self.fin:
            return f"row {min(b, self.batch - 1)}"     # overlapping rows: the last row that starts at or before i
        return f"gap behind row {b}"

    def inside(self):
        """Boolean mask over the buffer: True inside the union of the windows."""
        m = np.zeros(self.size, dtype=bool)
        for b in range(self.batch):
            m[self.row(b):self.row(b) + self.fin] = True
        return m


def place(rows, layout, stride=None):
    """`rows`: [batch, fin] bit patterns (uint16).  -> Placed(buf, win, rows): the poison-filled buffer with the rows written into their
    windows, the window, and the [batch, fin] rows the entry is to see -- `rows` itself, except for the layouts whose windows share
    elements: bcast shows row 0 `batch` times, overlap shows the windows of the stream rows.reshape(-1)."""
    rows = np.ascontiguousarray(rows, dtype=np.uint16)
    batch, fin = rows.shape
    win = Window(layout, batch, fin, stride)
    buf = np.full(win.size, POISON, dtype=np.uint16)
    if batch > 1 and win.xs < fin:
        n = (batch - 1) * win.xs + fin
        buf[win.start:win.start + n] = rows.reshape(-1)[:n]
        seen = np.stack([buf[win.row(b):win.row(b) + fin] for b in range(batch)])
    else:
        for b in range(batch):
            buf[win.row(b):win.row(b) + fin] = rows[b]
        seen = rows
    assert not (seen == POISON).any()
    return types.SimpleNamespace(buf=buf, win=win, rows=seen)


def nan_mask(a, dt=None):
    """NaNs of a float array, or of 16-bit patterns of storage type `dt` ("float16" / "bfloat16")."""
    a = np.asarray(a)
    if a.dtype.kind == "f":
        return np.isnan(a)
    a = a.view(np.uint16)
    exp, man = (0x7C00, 0x03FF) if dt == "float16" else (0x7F80, 0x007F)
    return ((a & exp) == exp) & ((a & man) != 0)


def check(got, baseline, win, what="", dt=None):
    """(a) no output is NaN, (b) `got` equals `baseline` ([batch, M]: the entry's own result on the same rows in the flat layout) bit
    for bit.  Floats are compared as their bit patterns.  Returns got."""
    got, want = np.asarray(got), np.asarray(baseline)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    where = f"{what} [{win.layout}, {win.batch} x {win.fin}, x + {win.offset}, xs {win.xs}]"
    bad = np.argwhere(nan_mask(got, dt))
    if bad.size:
        b, m = (int(v) for v in bad[0])
        raise AssertionError(f"{where}: {bad.shape[0]} of {got.size} outputs are NaN, first at row {b}, column {m}: row {b} was not read "
                             f"from its window [{win.row(b)}, {win.row(b) + win.fin}) of the buffer alone")
    bits = (lambda a: a.view(np.uint32)) if got.dtype == np.float32 else (lambda a: a.view(np.uint16) if a.dtype.itemsize == 2 else a)
    bad = np.argwhere(bits(got) != bits(want))
    if bad.size:
        b, m = (int(v) for v in bad[0])
        raise AssertionError(f"{where}: {bad.shape[0]} of {got.size} outputs differ from the flat layout's, first at row {b}, column {m}: "
                             f"{got[b, m]!r}, flat {want[b, m]!r}")
    return got


def check_reads(reads, win, what=""):
    """`reads`: [(first element, count)] of the buffer a host stand-in loaded.  Every one of them must lie inside the windows; the
    first that does not is named by its region.  (Only a model can be asked this: a GPU read leaves no trace.)"""
    inside = win.inside()
    for first, count in reads:
        for i in range(first, first + count):
            if i < 0 or i >= win.size or not inside[i]:
                name = win.region(i) if 0 <= i < win.size else "region behind the buffer" if i > 0 else "region in front of the buffer"
                raise AssertionError(f"{what} [{win.layout}, {win.batch} x {win.fin}, xs {win.xs}]: element {i} (x + {i - win.start}) was read, "
                                     f"in the {name}")
