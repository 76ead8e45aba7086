"""The LDS image of a packed 1x16 launch as aqlm_hip_gemv_1x16_packed_image reports it -- no GPU: descriptors are built by the numpy
model's layout (tests/packed_model.py) and the entry reads them on the host.

One-row launches of layers whose x image fits 8208 bytes take the compact x window, so that two layers' workgroups share a CU
(DESIGN.md section 4.3); everything else keeps the image it had.  The sizes are restated here from the map in
packed_gemv_kernels.h (PackedLds) and must agree with the library byte for byte."""
import ctypes

import pytest

from tests import packed_model as pm

COMPACT, FULL, SLICE = 8208, 65520, 65536
CU_LDS = 160 * 1024


@pytest.fixture(scope="module")
def native():
    from aqlm_amd import _native

    return _native


@pytest.fixture(autouse=True)
def default_keys(native):
    keys = ("packed_compact_window", "packed_prefetch")
    old = [native.get_tuning(k) for k in keys]
    yield
    for k, v in zip(keys, old):
        native.set_tuning(k, v)


def desc(native, fout, fin, waves, steps, x_copies=1, entry_bytes=4, groups=None):
    lay = pm.layout(fout, fin // 8, waves, steps, entry_bytes, groups, False)
    g = (ctypes.c_uint8 * 32)(*(groups or [16] * 16))
    return native.PackedDesc(pm.MAGIC, pm.VERSION, fout, fin, 4, waves, steps, entry_bytes, lay["used"], x_copies, 1.5,
                             native.PACKED_VARGEOM if groups else 0, lay["RG"], g)


def up(v, a):
    return (v + a - 1) // a * a


def full_image(RG):
    """x first behind the 64 KiB window: row starts in whole KiB, colend and xmax for 16 waves (the image every launch had)."""
    return up(FULL + SLICE + up((RG + 1) * 4, 1024) + (RG + 1) * 4 + 16 * 256, 16) + 64


def compact_image(RG, waves):
    """... behind the compact window: row starts in the 256-byte pieces of their DMA, colend for the waves of the stream."""
    return up(COMPACT + SLICE + up((RG + 1) * 4, 256) + (RG + 1) * 4 + waves * 256, 16) + 64


def slice_first_image(in_groups, RG, rows):
    return up(SLICE + rows * (in_groups + 1) * 16 + up((RG + 1) * 4, 1024) + rows * (RG + 1) * 4 + rows * 16 * 256, 16) + rows * 64


# (out, in, waves, steps, x copies, entry bytes) -> window
CASES = [
    ((4096, 4096, 6, 6, 1, 4), COMPACT),      # x fills the window to its last byte
    ((11008, 4096, 14, 6, 1, 4), COMPACT),
    ((14336, 4096, 14, 8, 1, 4), COMPACT),
    ((512, 256, 4, 1, 1, 4), COMPACT),
    ((272, 1024, 4, 1, 1, 4), COMPACT),
    ((512, 4104, 6, 2, 1, 4), FULL),          # one input group too many
    ((4096, 8192, 14, 6, 1, 4), FULL),
    ((512, 1024, 4, 2, 2, 4), COMPACT),       # two copies of x: (132 + 129) * 16 = 4176 bytes
    ((512, 1024, 4, 2, 4, 4), FULL),          # four: (3 * 132 + 129) * 16 = 8400
    ((4096, 4096, 6, 6, 2, 4), FULL),
    ((4096, 4096, 6, 6, 1, 3), FULL),         # 3-byte entries have no compact instance
    ((57344, 256, 8, 4, 1, 4), 0),            # 3584 rows per group: slice first
]


@pytest.mark.parametrize("shape,window", CASES)
def test_compact_window_is_chosen_exactly_when_x_fits(native, shape, window):
    fout, fin, waves, steps, xc, eb = shape
    d = desc(native, fout, fin, waves, steps, xc, eb)
    RG = (fout + 15) // 16
    want = {COMPACT: compact_image(RG, waves), FULL: full_image(RG), 0: slice_first_image(fin // 8, RG, 1)}[window]
    for dt in (native.F16, native.BF16):
        assert native.packed_image(d, 1, dt) == (want, window)
    assert want <= CU_LDS
    # the key forced off: the image every launch had before, and so for more than one row whatever the key says
    rows2 = (slice_first_image(fin // 8, RG, 2), 0)
    assert native.packed_image(d, 2) == rows2
    native.set_tuning("packed_compact_window", 1)
    assert native.packed_image(d, 1) == ((full_image(RG), FULL) if window else (want, 0))
    assert native.packed_image(d, 2) == rows2
    native.set_tuning("packed_compact_window", 0)
    native.set_tuning("packed_prefetch", 4)   # deeper rings have no compact instance
    assert native.packed_image(d, 1) == ((full_image(RG), FULL) if window else (want, 0))


def test_variable_geometry_takes_the_compact_window(native):
    groups = [17, 15] + [16] * 14
    d = desc(native, 512, 2048, 4, 2, groups=groups)
    RG = (512 + 14) // 15
    assert d.rows_per_group == RG
    assert native.packed_image(d, 1) == (compact_image(RG, 4), COMPACT)
    native.set_tuning("packed_prefetch", 4)   # the variable-geometry kernel runs ring depth 3 at one row whatever the key says
    assert native.packed_image(d, 1) == (compact_image(RG, 4), COMPACT)
    native.set_tuning("packed_compact_window", 1)
    assert native.packed_image(d, 1) == (full_image(RG), FULL)


@pytest.mark.parametrize("wide", [(11008, 14), (14336, 14)])
def test_headline_pairs_fit_one_cu_together(native, wide):
    """4096 -> 4096 beside 4096 -> 11008 (and beside 4096 -> 14336): the two images, each rounded up to the allocation granule,
    fit a CU's 160 KiB -- for every granule from 128 bytes to 2 KiB, 1280 among them (the GPU test takes what the runtime answers)."""
    a = native.packed_image(desc(native, 4096, 4096, 6, 6))[0]
    b = native.packed_image(desc(native, wide[0], 4096, wide[1], 6))[0]
    assert (a, b) == (compact_image(256, 6), compact_image((wide[0] + 15) // 16, wide[1]))
    for granule in (128, 256, 512, 1024, 1280, 2048):
        assert up(a, granule) + up(b, granule) <= CU_LDS, granule
    assert 2 * full_image(256) > CU_LDS   # what kept a second workgroup off the CU


def test_rejections(native):
    L = native.lib
    d = desc(native, 512, 256, 4, 1)
    lds, win = ctypes.c_size_t(0), ctypes.c_uint32(0)
    for rows, dt in ((0, native.F16), (9, native.F16), (1, 7)):
        assert L.aqlm_hip_gemv_1x16_packed_image(ctypes.byref(d), rows, dt, 0, ctypes.byref(lds), ctypes.byref(win), None) == native.E_INVALID
    assert L.aqlm_hip_gemv_1x16_packed_image(None, 1, native.F16, 0, ctypes.byref(lds), ctypes.byref(win), None) == native.E_INVALID
    bad = native.PackedDesc.from_ints(d.as_ints())
    bad.used_bytes += 1
    assert L.aqlm_hip_gemv_1x16_packed_image(ctypes.byref(bad), 1, native.F16, 0, None, None, None) == native.E_INVALID
    assert "descriptor" in native.last_error()
    assert L.aqlm_hip_gemv_1x16_packed_image(ctypes.byref(d), 1, native.F16, 0, None, None, None) == 0
