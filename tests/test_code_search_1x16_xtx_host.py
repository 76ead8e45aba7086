"""The calibrated code search of 1x16 layers (aqlm_hip_code_search_1x16_xtx behind aqlm.tuning.find_optimal_codes_calibrated), the parts
that need no GPU: the symbols and the ABI version, the route predicate, the numpy model of the kernel's arithmetic
(tests/x16_xtx_model.py) driven group by group against the torch route and the reference's codes on fixture case ``a``
(tests/golden/code_update_xtx_golden.npz: 1x16 g8, 32 x 64, beam 1), the calls that keep the torch route, and the argument checks of
the C entry on host buffers (every such call returns before a launch)."""
import ctypes
import itertools
import os
import re

import numpy as np
import pytest
import torch

from tests import x16_xtx_model as model
from tests.test_code_search_xtx_host import golden, torch_route

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("aqlm_hip_code_search_1x16_xtx_supported", "aqlm_hip_code_search_1x16_xtx_workspace_bytes", "aqlm_hip_code_search_1x16_xtx")


def test_symbols_are_declared_bound_and_exported_and_the_abi_version_stays():
    from aqlm_amd import _native as nat
    from aqlm_amd.inference_kernels import hip_kernel as hk

    text = open(os.path.join(ROOT, "include", "aqlm_hip.h")).read()
    assert int(re.search(r"#define AQLM_HIP_CODE_SEARCH_1X16_XTX_MAX_BEAM (\d+)", text).group(1)) == 8 == hk.CODE_SEARCH_1X16_XTX_MAX_BEAM
    declared = set(re.findall(r"\b(aqlm_hip_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S)))
    raw = ctypes.CDLL(nat.LIB_PATH)
    for name in NEW:
        assert name in declared and name in nat.SIGNATURES and hasattr(raw, name), name
    assert nat.lib.aqlm_hip_abi_version() == nat.ABI_VERSION == 9
    fn, size = nat.lib.aqlm_hip_code_search_1x16_xtx_supported, nat.lib.aqlm_hip_code_search_1x16_xtx_workspace_bytes
    for out, g, beam, pin in ((1, 8, 1, 1), (64, 16, 8, 8), (4096, 8, 8, 1), (14336, 16, 3, 3), (64, 8, 4, 8)):
        assert fn(out, g, beam, pin) == 1 and size(out, g, beam, pin) >= 2048 + 8 * out * beam * pin
    for out, g, beam, pin in ((0, 8, 4, 1), (64, 4, 4, 1), (64, 32, 4, 1), (64, 8, 0, 1), (64, 8, 9, 1), (64, 8, 4, 0), (64, 8, 4, 9)):
        assert fn(out, g, beam, pin) == 0 and size(out, g, beam, pin) == 0
    assert hk.code_search_1x16_xtx_supported(64, 8, 8, 8) and not hk.code_search_1x16_xtx_supported(64, 8, 9)


def test_route_predicate_is_a_pure_table(monkeypatch):
    import aqlm.tuning as tuning

    takes = tuning.takes_code_search_kernel_1x16_xtx
    monkeypatch.setattr(tuning, "CODE_SEARCH_KERNEL", True)
    for g, beam in itertools.product((8, 16), range(1, 9)):
        assert takes(16, 1, 1, g, beam, True, True, True) is True
    # each condition switched off alone
    for off in ((8, 1, 1, 8, 4, True, True, True), (16, 2, 1, 8, 4, True, True, True), (16, 0, 1, 8, 4, True, True, True),
                (16, 1, 2, 8, 4, True, True, True), (16, 1, 1, 4, 4, True, True, True), (16, 1, 1, 32, 4, True, True, True),
                (16, 1, 1, 8, 0, True, True, True), (16, 1, 1, 8, 9, True, True, True), (16, 1, 1, 8, 16, True, True, True),
                (16, 1, 1, 8, 4, False, True, True), (16, 1, 1, 8, 4, True, False, True), (16, 1, 1, 8, 4, True, True, False)):
        assert takes(*off) is False, off
    monkeypatch.setattr(tuning, "CODE_SEARCH_KERNEL", False)
    assert takes(16, 1, 1, 8, 4, True, True, True) is False


def test_model_driven_group_by_group_equals_the_torch_route_and_the_reference_on_case_a():
    c = golden("a")
    assert c["shape"] == (32, 64, 1, 16, 1, 8) and c["beam"] == 1
    codes, tied = model.search_layer(c["XTX"].numpy(), c["target"].numpy(), c["books"].reshape(65536, 8).numpy(), c["prev"].numpy(),
                                     c["scales"].reshape(-1).numpy(), c["beam"], c["group_order"], np.float64, c["near"])
    assert not tied.any(), "the generator discards a seed with a near tie on any row, by the test the model applies"
    differ = (torch.from_numpy(codes) != torch_route("a", torch.float64)).any(-1).any(-1).numpy()
    assert not differ.any(), f"{int(differ.sum())} rows differ from the torch route"
    assert np.array_equal(codes, c["expected"].numpy()), "and so the model reproduces the reference's codes"


def test_the_model_step_orders_ties_and_nans_as_a_stable_sort_does():
    rng = np.random.default_rng(0)
    flat = rng.standard_normal(5000).astype(np.float32)
    flat[100] = flat[7] = flat[4000] = flat.min()
    assert np.array_equal(model._first(flat, 9), np.argsort(flat, kind="stable")[:9])
    flat[10:] = np.nan
    assert np.array_equal(model._first(flat, 12), np.argsort(flat, kind="stable")[:12])


@pytest.mark.parametrize("beam", [1, 9])
def test_host_tensors_and_a_beam_of_9_keep_the_torch_route(monkeypatch, beam):
    import aqlm.tuning as tuning
    from aqlm_amd.inference_kernels import hip_kernel as hk
    from aqlm_amd.utils import pack_int_data

    monkeypatch.setattr(hk, "code_search_1x16_xtx_step", lambda *a, **k: pytest.fail("the kernel entry was called"))
    c = golden("a", torch.float32)
    stored = pack_int_data(c["prev"], 16)
    assert stored.dtype == torch.int16
    got = tuning.find_optimal_codes_calibrated(c["XTX"], c["target"], c["books"].half(), stored, c["scales"].half(), beam_size=beam,
                                               dim_order=[0])
    assert got.dtype == torch.int16 and got.shape == stored.shape
    found = got.to(torch.int64) % 65536
    if beam == 1:
        assert torch.equal(found, c["expected"])  # the fixture's values are exact in fp16
    else:  # a wider beam may only lower the objective the fixture's codes reach
        from aqlm_amd.utils import _dequantize_weight

        d = golden("a")
        reached = float(tuning.calibrated_error(_dequantize_weight(found, d["books"], d["scales"]), d["target"], d["XTX"]))
        fixture = float(tuning.calibrated_error(_dequantize_weight(d["expected"], d["books"], d["scales"]), d["target"], d["XTX"]))
        assert reached <= fixture * (1 + 1e-6)


def test_the_step_wrapper_refuses_host_tensors():
    from aqlm_amd.inference_kernels import hip_kernel as hk

    with pytest.raises(ValueError, match="on the GPU"):
        hk.code_search_1x16_xtx_step(torch.zeros((1, 4, 8)), torch.zeros((1, 4)), torch.zeros((1, 4, 1), dtype=torch.int16), torch.zeros((8, 8)),
                                     torch.zeros((65536,)), torch.zeros((65536, 8), dtype=torch.float16), None, 2)


def test_c_entry_refuses_bad_arguments_before_any_launch():
    from aqlm_amd import _native as nat

    buf = ctypes.create_string_buffer(1 << 17)
    p = (ctypes.addressof(buf) + 15) // 16 * 16
    args = lambda **kw: [kw.get(n, d) for n, d in (  # noqa: E731
        ("t", p), ("tps", 64 * 8), ("trs", 8), ("loss", p + 4096), ("codes_in", p + 8192), ("h", p + 12288), ("q", p + 16384), ("cb", p + 20480),
        ("dt", nat.F16), ("scales", p + 32770), ("out", 64), ("g", 8), ("beam", 4), ("pin", 1), ("loss_out", p + 36864),
        ("codes_out", p + 40962), ("source", p + 45057), ("delta", p + 49152), ("t_out", p + 57344), ("ws", p + 65536), ("ws_bytes", 0),
        ("stream", None))]
    call = nat.lib.aqlm_hip_code_search_1x16_xtx
    # every call below is refused; the last complaint in line is the size of the workspace, which is how a call that is fine up to there shows
    assert call(*args()) == nat.E_INVALID and "workspace of 0 bytes" in nat.last_error()
    need = nat.lib.aqlm_hip_code_search_1x16_xtx_workspace_bytes(64, 8, 4, 1)
    assert call(*args(ws_bytes=need - 1)) == nat.E_INVALID and f"where {need} bytes are needed" in nat.last_error()
    for null in ("t", "loss", "codes_in", "h", "q", "cb", "loss_out", "codes_out", "source", "delta", "ws"):
        assert call(*args(**{null: None})) == nat.E_INVALID and "null pointer" in nat.last_error(), null
    assert call(*args(t=None, g=4)) == nat.E_INVALID and "null pointer" in nat.last_error(), "null pointers come first"
    assert call(*args(scales=None, t_out=None)) == nat.E_INVALID and "workspace of 0 bytes" in nat.last_error()  # both may be NULL
    for name, addr in (("cb", p + 20480 + 8), ("t", p + 2), ("loss", p + 4098), ("codes_in", p + 8193), ("h", p + 12289), ("q", p + 16388),
                       ("scales", p + 32771), ("loss_out", p + 36866), ("codes_out", p + 40961), ("delta", p + 49154), ("t_out", p + 57346),
                       ("ws", p + 65544)):
        assert call(*args(**{name: addr})) == nat.E_INVALID and "misaligned" in nat.last_error(), name
    assert call(*args(cb=p + 20480 + 8, out=0)) == nat.E_INVALID and "misaligned" in nat.last_error(), "alignment comes before the sizes"
    for bad in ({"out": 0}, {"out": -3}, {"g": 0}, {"trs": 4}, {"pin": 4, "tps": 4}):
        assert call(*args(**bad)) == nat.E_INVALID and "bad sizes" in nat.last_error(), bad
    assert call(*args(out=0, dt=nat.F32)) == nat.E_INVALID, "sizes come before the dtype"
    assert call(*args(dt=nat.F32, g=4, trs=4)) == nat.E_UNSUPPORTED and "float16 and bfloat16" in nat.last_error(), "the dtype comes before the scheme"
    for bad in ({"g": 4}, {"g": 32, "trs": 32}, {"beam": 9}, {"beam": 0}, {"pin": 0}, {"pin": 9}):
        assert call(*args(**bad)) == nat.E_UNSUPPORTED and "shape outside" in nat.last_error(), bad
