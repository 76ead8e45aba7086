"""The calibrated code search (aqlm.tuning.find_optimal_codes_calibrated, aqlm_hip_code_search_kx8_xtx), the parts that need no GPU:
the torch route against the reference's codes (tests/golden/code_update_xtx_golden.npz, written by tools/gen_code_update_xtx_golden.py),
the numpy model of the kernel's arithmetic (tests/kx8_xtx_model.py) driven group by group against the torch route in float64, the
objective, the route predicate, the argument checks of the Python functions and of the C entry (on host buffers: every such call
returns before a launch), and ``update_codes_calibrated_`` on a host layer."""
import ctypes
import functools
import itertools
import json
import os
import re

import numpy as np
import pytest
import torch

from tests import kx8_xtx_model as model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("aqlm_hip_code_search_kx8_xtx_supported", "aqlm_hip_code_search_kx8_xtx_workspace_bytes", "aqlm_hip_code_search_kx8_xtx")
CASES = ("a", "b1", "b4", "c", "d", "e")
KX8_CASES = ("b1", "b4", "c", "e")


@functools.lru_cache(maxsize=None)
def golden(case, dtype=torch.float64):
    """The tensors of one case from the fixture's integer-coded arrays (tools/gen_code_update_xtx_golden.py documents the coding)."""
    z = np.load(os.path.join(ROOT, "tests", "golden", "code_update_xtx_golden.npz"))
    meta = json.loads(str(z["meta"]))
    info = meta["cases"][case]
    name = info["layer"]
    out_features, in_features, K, nbits, ogs, g = meta["layers"][name]["shape"]
    if nbits == 16:
        books = (z[f"{name}_codebook_hi_k"][:, None].astype(np.float64) + z[f"{name}_codebook_lo_k"][None, :].astype(np.float64)).reshape(1, 65536, ogs, g)
    else:
        books = z[f"{name}_codebook_k"].astype(np.float64)
    books = books * meta["grid"]
    near = (z[f"{name}_prev_codes"].astype(np.int64) + z[f"{name}_near_shift"].astype(np.int64)) % books.shape[1]
    unscaled = sum(books[c][near[..., c]] for c in range(K)).transpose(0, 2, 1, 3).reshape(out_features, in_features)
    unscaled = unscaled + z[f"{name}_noise_k"].astype(np.float64) * meta["grid"]
    factors = 2.0 ** z[f"{name}_scale_exp"].astype(np.float64)
    x = z[f"{name}_x_k"].astype(np.float64)
    XTX = (x.T @ x + 16 * np.eye(in_features)).astype(np.float32)  # integers below 2^24: float32 holds them exactly
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dtype)  # noqa: E731
    return {"XTX": t(XTX), "books": t(books), "target": t(unscaled * np.repeat(factors, ogs)[:, None]), "scales": t(factors).reshape(-1, 1, 1, 1),
            "prev": torch.from_numpy(z[f"{name}_prev_codes"].astype(np.int64)), "expected": torch.from_numpy(z[f"{case}_expected"].astype(np.int64)),
            "beam": info["beam_size"], "group_order": info["group_order"], "dim_order": info["dim_order"],
            "shape": (out_features, in_features, K, nbits, ogs, g), "near": meta["near"]}


@functools.lru_cache(maxsize=None)
def torch_route(case, dtype):
    import aqlm.tuning as tuning

    c = golden(case, dtype)
    return tuning.find_optimal_codes_calibrated(c["XTX"], c["target"], c["books"], c["prev"], c["scales"], beam_size=c["beam"],
                                                group_order=c["group_order"], dim_order=c["dim_order"])


def test_the_fixture_holds_the_cases_of_the_issue():
    shapes = {case: (golden(case)["shape"], golden(case)["beam"]) for case in CASES}
    assert shapes == {"a": ((32, 64, 1, 16, 1, 8), 1), "b1": ((64, 128, 2, 8, 1, 8), 1), "b4": ((64, 128, 2, 8, 1, 8), 4),
                      "c": ((32, 128, 4, 8, 1, 16), 2), "d": ((32, 64, 2, 8, 2, 8), 2), "e": ((32, 256, 8, 8, 1, 32), 4)}
    c = golden("c")
    assert sorted(c["group_order"]) == list(range(8)) and c["group_order"] != list(range(8)) and len(c["dim_order"]) == 8
    assert len({tuple(o) for o in c["dim_order"]}) > 1 and all(sorted(o) == [0, 1, 2, 3] for o in c["dim_order"])
    for case in CASES:
        share = float((golden(case)["expected"] != golden(case)["prev"]).any(-1).float().mean())
        assert 0 < share < 1, case
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "code_update_xtx_golden.npz")) < 100 * 1024


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["fp32", "fp64"])
@pytest.mark.parametrize("case", CASES)
def test_torch_route_equals_the_reference_code_for_code(case, dtype):
    c = golden(case, dtype)
    got = torch_route(case, dtype)
    assert got.shape == c["prev"].shape and got.dtype == c["prev"].dtype
    differ = int((got != c["expected"]).any(-1).any(-1).sum())
    assert differ == 0, f"{differ} output groups differ from the reference's codes"


@pytest.mark.parametrize("case", KX8_CASES)
def test_model_driven_group_by_group_equals_the_torch_route_in_float64(case):
    c = golden(case)
    _, _, K, _, _, g = c["shape"]
    codes, tied = model.search_layer(c["XTX"].numpy(), c["target"].numpy(), c["books"].reshape(K, 256, g).numpy(), c["prev"].numpy(),
                                     c["scales"].reshape(-1).numpy(), c["beam"], c["group_order"], c["dim_order"], np.float64, c["near"])
    assert not tied.any(), "the generator discards a seed with a near tie on any row, by the test the model applies"
    differ = (torch.from_numpy(codes) != torch_route(case, torch.float64)).any(-1).any(-1).numpy()
    assert not differ.any(), f"{int(differ.sum())} rows differ from the torch route"
    assert np.array_equal(codes, c["expected"].numpy()), "and so the model reproduces the reference's codes"


@pytest.mark.parametrize("case", CASES)
def test_the_objective_does_not_rise(case):
    import aqlm.tuning as tuning
    from aqlm_amd.utils import _dequantize_weight

    c = golden(case)
    before = float(tuning.calibrated_error(_dequantize_weight(c["prev"], c["books"], c["scales"]), c["target"], c["XTX"]))
    after = float(tuning.calibrated_error(_dequantize_weight(torch_route(case, torch.float64), c["books"], c["scales"]), c["target"], c["XTX"]))
    print(f"case {case}: calibrated error {before:.6g} -> {after:.6g}")
    assert after <= before
    error = (_dequantize_weight(c["prev"], c["books"], c["scales"]) - c["target"])
    assert before == pytest.approx(float(torch.einsum("oi,ij,oj->", error, c["XTX"], error)), rel=1e-12)


def test_wrap_around_form_and_dtype_of_the_codes_are_kept():
    import aqlm.tuning as tuning
    from aqlm_amd.utils import pack_int_data

    c = golden("b4", torch.float32)
    stored = pack_int_data(c["prev"], 8)
    assert stored.dtype == torch.int8 and bool((stored < 0).any())
    got = tuning.find_optimal_codes_calibrated(c["XTX"], c["target"], c["books"], stored, c["scales"], beam_size=4)
    assert got.dtype == torch.int8 and got.shape == stored.shape and torch.equal(got.to(torch.int64) % 256, c["expected"])
    without = tuning.find_optimal_codes_calibrated(c["XTX"], c["target"], c["books"], c["prev"], None, beam_size=1)
    assert without.shape == c["prev"].shape  # scales may be None


SCHEMES = ((1, 8, 1, 8), (2, 8, 1, 8), (4, 8, 1, 16), (8, 8, 1, 32), (3, 8, 1, 8), (9, 8, 1, 8), (0, 8, 1, 8), (2, 8, 2, 8), (2, 8, 1, 4),
           (2, 8, 1, 64), (2, 16, 1, 8), (1, 16, 1, 8), (1, 16, 1, 16))
TAKEN = SCHEMES[:5]


def test_route_predicate_is_a_pure_table(monkeypatch):
    import aqlm.tuning as tuning

    for switch in (True, False):
        monkeypatch.setattr(tuning, "CODE_SEARCH_KERNEL", switch)
        for scheme in SCHEMES:
            for beam in (1, 4, 16, 17, 0):
                for on_gpu, dtypes_ok, supported in itertools.product((False, True), repeat=3):
                    want = switch and scheme in TAKEN and 1 <= beam <= 16 and on_gpu and dtypes_ok and supported
                    assert tuning.takes_code_search_kernel_kx8_xtx(*scheme, beam, on_gpu, dtypes_ok, supported) is want
    monkeypatch.setattr(tuning, "CODE_SEARCH_KERNEL", True)
    assert tuning.takes_code_search_kernel_kx8_xtx(2, 8, 1, 8, 8, True, True, True) is True
    for host, books_fp32, beam, ogs in ((True, False, 8, 1), (False, True, 8, 1), (False, False, 17, 1), (False, False, 8, 2)):
        assert tuning.takes_code_search_kernel_kx8_xtx(2, 8, ogs, 8, beam, not host, not books_fp32, True) is False


def test_host_tensors_never_reach_the_kernel_entry(monkeypatch):
    import aqlm.tuning as tuning
    from aqlm_amd.inference_kernels import hip_kernel as hk
    from aqlm_amd.utils import pack_int_data

    real = hk.code_search_kx8_xtx_step
    monkeypatch.setattr(hk, "code_search_kx8_xtx_step", lambda *a, **k: pytest.fail("the kernel entry was called for host tensors"))
    c = golden("b1", torch.float32)
    got = tuning.find_optimal_codes_calibrated(c["XTX"], c["target"], c["books"].half(), pack_int_data(c["prev"], 8), c["scales"].half(), beam_size=1)
    assert torch.equal(got.to(torch.int64) % 256, c["expected"])  # the fixture's values are exact in fp16
    with pytest.raises(ValueError, match="on the GPU"):
        real(torch.zeros((1, 4, 8)), torch.zeros((1, 4)), torch.zeros((1, 4, 2), dtype=torch.int8), torch.zeros((8, 8)),
             torch.zeros((2, 256)), torch.zeros((2, 256, 8), dtype=torch.float16), None, 2)


def test_bad_arguments_raise():
    import aqlm.tuning as tuning

    c = golden("b1", torch.float32)
    call = lambda **kw: tuning.find_optimal_codes_calibrated(kw.pop("XTX", c["XTX"]), c["target"], c["books"], c["prev"], c["scales"], **kw)  # noqa: E731
    with pytest.raises(NotImplementedError, match="sparsity_regularizer"):
        call(sparsity_regularizer=0.1)
    with pytest.raises(TypeError):
        call(max_update_fraction=0.5)
    for bad in (dict(group_order=[0] * 16), dict(group_order=list(range(15))), dict(dim_order=[0, 0]), dict(dim_order=[[0, 1]] * 15),
                dict(dim_order=[[0, 1]] * 15 + [[1, 1]]), dict(XTX=c["XTX"][:, :64]), dict(XTX=c["XTX"][:64, :64]), dict(beam_size=0)):
        with pytest.raises(ValueError):
            call(**bad)
    with pytest.raises(ValueError, match="one layer"):
        tuning.find_optimal_codes_calibrated(c["XTX"], c["target"][:, :64], c["books"], c["prev"], c["scales"])


def test_symbols_are_declared_bound_and_exported_and_the_abi_version_stays():
    from aqlm_amd import _native as nat
    from aqlm_amd.inference_kernels import hip_kernel as hk

    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "aqlm_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(aqlm_hip_[a-z0-9_]+)\s*\(", text))
    raw = ctypes.CDLL(nat.LIB_PATH)
    for name in NEW:
        assert name in declared and name in nat.SIGNATURES and hasattr(raw, name), name
    assert nat.lib.aqlm_hip_abi_version() == nat.ABI_VERSION == 9
    fn = nat.lib.aqlm_hip_code_search_kx8_xtx_supported
    for out, K, g, beam, pin in ((1, 1, 8, 1, 1), (64, 2, 8, 16, 16), (4096, 8, 32, 8, 1), (14336, 4, 16, 3, 3), (64, 2, 8, 4, 16)):
        assert fn(out, K, g, beam, pin) == 1
    for out, K, g, beam, pin in ((0, 2, 8, 4, 1), (64, 0, 8, 4, 1), (64, 9, 8, 4, 1), (64, 2, 4, 4, 1), (64, 2, 64, 4, 1), (64, 2, 8, 0, 1),
                                 (64, 2, 8, 17, 1), (64, 2, 8, 4, 0), (64, 2, 8, 4, 17)):
        assert fn(out, K, g, beam, pin) == 0
    assert nat.lib.aqlm_hip_code_search_kx8_xtx_workspace_bytes(4096, 8, 32, 16) == 0
    assert hk.code_search_kx8_xtx_supported(64, 2, 8, 16, 16) and not hk.code_search_kx8_xtx_supported(64, 2, 8, 17)


def test_c_entry_refuses_bad_arguments_before_any_launch():
    from aqlm_amd import _native as nat

    buf = ctypes.create_string_buffer(1 << 17)
    p = (ctypes.addressof(buf) + 15) // 16 * 16
    order = lambda *v: (ctypes.c_int * len(v))(*v)  # noqa: E731
    args = lambda **kw: [kw.get(n, d) for n, d in (  # noqa: E731
        ("t", p), ("tps", 64 * 8), ("trs", 8), ("loss", p + 4096), ("codes_in", p + 8193), ("h", p + 12288), ("q", p + 16384), ("cb", p + 20480),
        ("dt", nat.F16), ("scales", p + 32770), ("out", 64), ("K", 2), ("g", 8), ("beam", 4), ("pin", 1), ("order", None), ("loss_out", p + 36864),
        ("codes_out", p + 40961), ("source", p + 45057), ("delta", p + 49152), ("t_out", p + 57344), ("ws", None), ("ws_bytes", 0), ("stream", None))]
    call = nat.lib.aqlm_hip_code_search_kx8_xtx
    # every call below is refused; the last complaint in line is dim_order, which is how a call that is fine up to there shows
    fine = {"order": order(0, 0)}
    assert call(*args(**fine)) == nat.E_INVALID and "permutation" in nat.last_error()
    for null in ("t", "loss", "codes_in", "h", "q", "cb", "loss_out", "codes_out", "source", "delta"):
        assert call(*args(**{null: None})) == nat.E_INVALID and "null pointer" in nat.last_error(), null
    assert call(*args(t=None, g=4, K=9)) == nat.E_INVALID and "null pointer" in nat.last_error(), "null pointers come first"
    assert call(*args(scales=None, t_out=None, **fine)) == nat.E_INVALID and "permutation" in nat.last_error()  # both may be NULL
    for name, addr in (("cb", p + 20480 + 8), ("t", p + 2), ("loss", p + 4098), ("h", p + 12289), ("q", p + 16386), ("scales", p + 32771),
                       ("loss_out", p + 36866), ("delta", p + 49154), ("t_out", p + 57346)):
        assert call(*args(**{name: addr})) == nat.E_INVALID and "misaligned" in nat.last_error(), name
    assert call(*args(cb=p + 20480 + 8, out=0)) == nat.E_INVALID and "misaligned" in nat.last_error(), "alignment comes before the sizes"
    for bad in ({"out": 0}, {"out": -3}, {"g": 0}, {"trs": 4}, {"pin": 4, "tps": 4}):
        assert call(*args(**bad)) == nat.E_INVALID and "bad sizes" in nat.last_error(), bad
    assert call(*args(out=0, dt=nat.F32)) == nat.E_INVALID, "sizes come before the dtype"
    assert call(*args(dt=nat.F32, K=9)) == nat.E_UNSUPPORTED and "float16 and bfloat16" in nat.last_error(), "the dtype comes before the scheme"
    for bad in ({"g": 4}, {"K": 9}, {"K": 0}, {"beam": 17}, {"beam": 0}, {"pin": 0}, {"pin": 17}, {"g": 64, "trs": 64}):
        assert call(*args(**bad)) == nat.E_UNSUPPORTED and "shape outside" in nat.last_error(), bad
    assert call(*args(K=9, order=order(0, 0))) == nat.E_UNSUPPORTED, "the scheme comes before dim_order"
    for K, bad in ((2, (0, 0)), (2, (0, 2)), (2, (-1, 0)), (3, (2, 2, 1)), (1, (1,))):
        assert call(*args(K=K, order=order(*bad))) == nat.E_INVALID and "permutation" in nat.last_error(), bad


def test_update_codes_calibrated_on_a_host_layer_moves_the_version_counter():
    import aqlm.tuning as tuning
    from aqlm import QuantizedLinear
    from aqlm_amd.utils import pack_int_data

    c = golden("b1", torch.float32)
    layer = QuantizedLinear(128, 64, 8, 1, 2, 8, bias=False, dtype=torch.float32)
    with torch.no_grad():
        layer.codes.copy_(pack_int_data(c["prev"], 8))
        layer.codebooks.copy_(c["books"])
        layer.scales.copy_(c["scales"])
    before, version = float(tuning.calibrated_error(layer, c["target"], c["XTX"])), layer.codes._version
    holder = layer.codes
    changed = tuning.update_codes_calibrated_(layer, c["target"], c["XTX"], beam_size=1)
    assert layer.codes is holder and layer.codes._version > version
    assert int(changed) == int((c["expected"] != c["prev"]).any(-1).sum()) and torch.equal(layer.codes.to(torch.int64) % 256, c["expected"])
    assert float(tuning.calibrated_error(layer, c["target"], c["XTX"])) < before
    with pytest.raises(NotImplementedError):
        tuning.update_codes_calibrated_(layer, c["target"], c["XTX"], sparsity_regularizer=1.0)
    layer._moe_expert = True
    with pytest.raises(TypeError, match="expert"):
        tuning.update_codes_calibrated_(layer, c["target"], c["XTX"])
    with pytest.raises(TypeError):
        tuning.update_codes_calibrated_(torch.nn.Linear(8, 8), c["target"], c["XTX"])
