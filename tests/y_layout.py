"""Layout harness of the dense forward entries: WHERE an entry writes, not what.

An entry of include/aqlm_hip.h takes ``y`` and ``y_row_stride`` (elements) and promises to write the ``batch`` windows
``[b * ys, b * ys + M)`` behind ``y`` and nothing else, for any 2-byte aligned ``y`` and any ``ys >= M``.  The harness puts such a
window into a larger int16 buffer filled with a sentinel (0x5A5A, 24 elements of padding on either side, as
tests/test_dequant_exact_gpu.py does for W), and ``check`` holds the buffer to two statements after the call, both bit for bit:

  (a) every element outside the windows -- the front pad, every gap between two rows, the back pad -- still is the sentinel;
  (b) the windows hold what the same entry wrote, on the same inputs and tuning, in the ``flat`` layout (ys == M, aligned).

The same is done for a workspace: exactly the advertised number of bytes, 16-byte aligned, sentinels in front and behind; and for
the zero-at-rest accumulator cells of the single-kernel finalizes (``zero_at_rest``).

Plain helper module: numpy only, the buffers may be numpy arrays (tests/test_y_layout_host.py) or torch tensors on the device."""
import numpy as np

PAD = 24            # sentinel elements on either side of the y windows
SENTINEL = 0x5A5A
WS_PAD = 64         # sentinel bytes on either side of a workspace (a multiple of 16: the workspace stays 16-byte aligned)
WS_SENTINEL = 0x5A

# name -> (offset of the first element from an 8-byte aligned address, in elements; ys - M)
LAYOUTS = {
    "flat": (0, 0),   # what the Python wrappers pass
    "gap4": (0, 4),   # the 8-byte store with gaps between the rows where M % 4 == 0
    "odd": (0, 1),    # ys & 3 != 0
    "off1": (1, 4),   # pointer & 7 == 2
    "off2": (2, 6),   # pointer & 7 == 4, ys & 3 == 2
    "off3": (3, 3),   # pointer & 7 == 6
}


class Window:
    """Where the rows of y lie in a buffer of `size` int16 elements: row b at [start + b * ys, start + b * ys + M)."""

    def __init__(self, layout, batch, M):
        offset, extra = LAYOUTS[layout]
        self.layout, self.batch, self.M = layout, int(batch), int(M)
        self.ys = self.M + extra
        self.start = PAD + offset          # PAD elements are 48 bytes: the element at PAD is as aligned as the buffer (>= 16 bytes)
        self.size = self.start + (self.batch - 1) * self.ys + self.M + PAD

    def row(self, b):
        return self.start + b * self.ys

    def ptr(self, base_ptr):
        """Address of y[0, 0] in a buffer that starts at `base_ptr` (which must be 8-byte aligned)."""
        assert base_ptr % 8 == 0, base_ptr
        p = base_ptr + 2 * self.start
        assert p % 8 == 2 * LAYOUTS[self.layout][0]
        return p

    def region(self, i):
        """Name of the region element i of the buffer belongs to."""
        if i < self.start:
            return "front pad"
        b, c = divmod(i - self.start, self.ys)
        if b >= self.batch or (b == self.batch - 1 and c >= self.M):
            return "back pad"
        return f"row {b}" if c < self.M else f"gap behind row {b}"

    def inside(self):
        """Boolean mask over the buffer: True inside the windows."""
        m = np.zeros(self.size, dtype=bool)
        for b in range(self.batch):
            m[self.row(b):self.row(b) + self.M] = True
        return m


def _host(buf, dtype):
    """A numpy view / copy of `buf` (numpy array or torch tensor, any device) as `dtype`."""
    if not isinstance(buf, np.ndarray):
        buf = buf.detach().cpu().numpy()
    return np.ascontiguousarray(buf).reshape(-1).view(dtype)


def new_buffer(win):
    """Sentinel-filled host buffer for `win` (the device tests build theirs with torch.full((win.size,), SENTINEL, int16))."""
    return np.full(win.size, SENTINEL, dtype=np.uint16)


def windows(buf, layout, batch, M):
    """The [batch, M] bit patterns (uint16) the windows of `buf` hold."""
    win = Window(layout, batch, M)
    a = _host(buf, np.uint16)
    assert a.size == win.size, (a.size, win.size)
    return np.stack([a[win.row(b):win.row(b) + M] for b in range(batch)])


def check(buf, layout, batch, M, baseline, what=""):
    """(a) nothing outside the `batch` windows of `layout` was written, (b) the windows equal `baseline` ([batch, M] bit patterns, the
    entry's own result in the `flat` layout).  Both bit for bit.  Returns the windows."""
    win = Window(layout, batch, M)
    a = _host(buf, np.uint16)
    assert a.size == win.size, (what, a.size, win.size)
    outside = ~win.inside()
    hit = np.flatnonzero(outside & (a != SENTINEL))
    if hit.size:
        i = int(hit[0])
        raise AssertionError(f"{what} [{layout}, {batch} x {M}, ys {win.ys}]: {hit.size} elements outside the y windows were written, first "
                             f"at buffer index {i} (y + {i - win.start}) in the {win.region(i)}: 0x{int(a[i]):04x}")
    got = np.stack([a[win.row(b):win.row(b) + M] for b in range(batch)])
    want = _host(baseline, np.uint16).reshape(batch, M)
    bad = np.argwhere(got != want)
    if bad.size:
        b, m = (int(v) for v in bad[0])
        raise AssertionError(f"{what} [{layout}, {batch} x {M}, ys {win.ys}]: {bad.shape[0]} of {got.size} outputs differ from the flat "
                             f"layout's, first at row {b}, column {m}: 0x{int(got[b, m]):04x}, flat 0x{int(want[b, m]):04x}")
    return got


# ---------------------------------------------------------------------------------------------------------------- workspaces
class Workspace:
    """`nbytes` bytes of workspace at [WS_PAD, WS_PAD + nbytes) of a buffer of `size` bytes, sentinel bytes around them."""

    def __init__(self, nbytes):
        self.nbytes = int(nbytes)
        self.start = WS_PAD
        self.size = self.start + self.nbytes + WS_PAD

    def ptr(self, base_ptr):
        assert base_ptr % 16 == 0, base_ptr
        return base_ptr + self.start

    def fill(self, buf, zero_inside=False):
        """Sentinels everywhere (numpy array or torch uint8 tensor); zeros inside for accumulator cells."""
        buf[:] = WS_SENTINEL
        if zero_inside:
            buf[self.start:self.start + self.nbytes] = 0


def new_workspace(ws, zero_inside=False):
    buf = np.empty(ws.size, dtype=np.uint8)
    ws.fill(buf, zero_inside)
    return buf


def check_workspace(buf, nbytes, what="", zero_at_rest=False):
    """Nothing in front of or behind the `nbytes` advertised bytes was written; `zero_at_rest`: and the bytes themselves are all zero
    again (the accumulator cells of the single-kernel finalizes)."""
    ws = Workspace(nbytes)
    a = _host(buf, np.uint8)
    assert a.size == ws.size, (what, a.size, ws.size)
    end = ws.start + ws.nbytes
    for name, lo, hi in (("behind the workspace", end, ws.size), ("in front of the workspace", 0, ws.start)):
        hit = np.flatnonzero(a[lo:hi] != WS_SENTINEL)
        if hit.size:
            i = lo + int(hit[0])
            raise AssertionError(f"{what}: {hit.size} bytes {name} of {nbytes} bytes were written, first at byte {i - ws.start} of it "
                                 f"({i - end} behind its end): 0x{int(a[i]):02x}")
    if zero_at_rest:
        hit = np.flatnonzero(a[ws.start:end])
        if hit.size:
            raise AssertionError(f"{what}: the cells are not zero at rest after the call: {hit.size} bytes set inside the workspace, first "
                                 f"at byte {int(hit[0])} (cell {int(hit[0]) // 8})")
