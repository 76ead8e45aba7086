"""aqlm_hip_code_search_kx8 (the beam search that re-chooses the codes of K x 8 layers), the parts that need no GPU: the C ABI
(symbols, the support and workspace queries, the argument checks on host buffers in their documented order -- every such call
returns before a launch), the route predicate as a truth table, and the numpy model of the entry's arithmetic
(tests/kx8_search_model.py) against the reference's codes (tests/golden/code_update_golden.npz, cases d, e, f) and, on inputs of a
dyadic grid where float32 and float64 compute the same numbers, against the torch route in float64."""
import ctypes
import functools
import itertools
import json
import os
import re

import numpy as np
import pytest
import torch

from tests import kx8_search_model as model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("aqlm_hip_code_search_kx8_supported", "aqlm_hip_code_search_kx8_workspace_bytes", "aqlm_hip_code_search_kx8")
# K, g, beam_size
DYADIC = [(2, 8, 8), (3, 8, 16), (1, 8, 4), (4, 16, 4), (8, 32, 8), (2, 16, 3)]
TIE_CAP = 0.15


# ---------------------------------------------------------------------------------------------------------------------------
# 1. symbols and queries
# ---------------------------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_bound_and_exported_and_the_abi_version_stays():
    from aqlm_amd import _native as nat

    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "aqlm_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(aqlm_hip_[a-z0-9_]+)\s*\(", text))
    raw = ctypes.CDLL(nat.LIB_PATH)
    for name in NEW:
        assert name in declared and name in nat.SIGNATURES and hasattr(raw, name), name
    assert nat.lib.aqlm_hip_abi_version() == nat.ABI_VERSION == 9
    assert int(re.search(r"#define AQLM_HIP_CODE_SEARCH_KX8_MAX_BEAM (\d+)", text).group(1)) == 16
    from aqlm_amd.inference_kernels import hip_kernel

    assert hasattr(torch.ops.aqlm, "code_search_kx8") and hip_kernel.CODE_SEARCH_KX8_MAX_BEAM == 16
    for fn in ("code_search_kx8_supported", "code_search_kx8"):
        assert callable(getattr(hip_kernel, fn))


def test_supported_and_workspace_queries():
    from aqlm_amd import _native as nat
    from aqlm_amd.inference_kernels import hip_kernel as hk

    fn = nat.lib.aqlm_hip_code_search_kx8_supported
    for out, fin, K, g, beam in ((1, 8, 1, 8, 1), (3, 40, 2, 8, 8), (67, 72, 3, 8, 16), (64, 512, 4, 16, 4), (64, 1024, 8, 32, 8),
                                 (4096, 4096, 2, 8, 16), (14336, 4096, 8, 32, 1), (4096, 14336, 1, 8, 4), (64, 96, 5, 32, 7)):
        assert fn(out, fin, K, g, beam) == 1, (out, fin, K, g, beam)
    for K in (0, 9, -1):
        assert fn(64, 256, K, 8, 4) == 0, K
    for g in (4, 12, 64, 0, -8):
        assert fn(64, 192, 2, g, 4) == 0, g
    for beam in (0, 17, -1, 256):
        assert fn(64, 256, 2, 8, beam) == 0, beam
    assert fn(64, 60, 2, 8, 4) == 0 and fn(64, 72, 2, 16, 4) == 0 and fn(64, 48, 8, 32, 4) == 0  # in_features % g
    assert fn(0, 64, 2, 8, 4) == 0 and fn(64, 0, 2, 8, 4) == 0 and fn(-1, 64, 2, 8, 4) == 0
    assert fn(1 << 15, 1 << 19, 2, 8, 4) == 0 and fn((1 << 15) - 1, 1 << 19, 2, 8, 4) == 1  # 2^31 groups / 2^31 - 2^16
    assert hk.code_search_kx8_supported(64, 256, 2, 8, 16) and not hk.code_search_kx8_supported(64, 256, 2, 8, 17)
    ws = nat.lib.aqlm_hip_code_search_kx8_workspace_bytes
    for groups, K, g, beam in ((1, 1, 8, 1), (2048, 2, 8, 8), (2097152, 8, 32, 16), (0, 2, 8, 4), (2048, 9, 8, 4)):
        assert ws(groups, K, g, beam) == 0  # |C|^2 comes from the registers that hold the candidates: no workspace


# ---------------------------------------------------------------------------------------------------------------------------
# 2. argument checks, on dummy host pointers: every call returns before a launch
# ---------------------------------------------------------------------------------------------------------------------------
def test_argument_checks_report_the_documented_codes_in_the_documented_order():
    from aqlm_amd import _native as nat

    buf = ctypes.create_string_buffer(1 << 17)
    p = (ctypes.addressof(buf) + 15) // 16 * 16
    order = lambda *v: (ctypes.c_int * len(v))(*v)  # noqa: E731
    args = lambda **kw: [kw.get(n, d) for n, d in (  # noqa: E731
        ("ref", p), ("rt", nat.F32), ("stride", 256), ("scales", p + 4098), ("cb", p + 8192), ("dt", nat.F16), ("prev", p + 16385), ("out", 64),
        ("in", 256), ("K", 2), ("g", 8), ("beam", 4), ("order", None), ("ids", None), ("ids64", 0), ("n", 2048), ("codes", p + 24577),
        ("scores", p + 32772), ("ws", None), ("ws_bytes", 0), ("stream", None))]
    call = nat.lib.aqlm_hip_code_search_kx8
    # every call below is refused; the last complaint in line is dim_order, which is how a call that is fine up to there shows
    fine_up_to_the_order = {"order": order(0, 0)}
    assert call(*args(**fine_up_to_the_order)) == nat.E_INVALID and "permutation" in nat.last_error()
    for null in ("ref", "cb", "prev", "codes"):
        assert call(*args(**{null: None})) == nat.E_INVALID and "null pointer" in nat.last_error(), null
    assert call(*args(ref=None, g=12, n=0, K=0)) == nat.E_INVALID and "null pointer" in nat.last_error(), "null pointers come first"
    # scales, group_ids, scores_out and the workspace may be NULL
    assert call(*args(scales=None, scores=None, **fine_up_to_the_order)) == nat.E_INVALID and "permutation" in nat.last_error()
    misaligned = (("ref", p + 2, {}), ("ref", p + 1, {"rt": nat.F16}), ("scales", p + 4097, {}), ("cb", p + 8192 + 8, {}), ("scores", p + 32770, {}),
                  ("ids", p + 65536 + 2, {"n": 7}), ("ids", p + 65536 + 4, {"n": 7, "ids64": 1}))
    for name, addr, more in misaligned:
        assert call(*args(**{name: addr}, **more)) == nat.E_INVALID and "misaligned" in nat.last_error(), name
    # a 16-bit reference is 2-byte aligned, int8 codes have no alignment
    assert call(*args(ref=p + 2, rt=nat.BF16, prev=p + 16387, codes=p + 24579, **fine_up_to_the_order)) == nat.E_INVALID \
        and "permutation" in nat.last_error()
    assert call(*args(cb=p + 8192 + 8, out=0)) == nat.E_INVALID and "misaligned" in nat.last_error(), "alignment comes before the sizes"
    for bad in ({"out": 0}, {"in": 0}, {"g": 0}, {"in": 252}, {"out": -3}):
        assert call(*args(**bad)) == nat.E_INVALID and "bad sizes" in nat.last_error(), bad
    assert call(*args(stride=248)) == nat.E_INVALID and "row stride" in nat.last_error()
    for n in (0, -1, 2047, 2049):  # without group_ids the call covers the layer
        assert call(*args(n=n)) == nat.E_INVALID and "bad sizes" in nat.last_error(), n
    assert call(*args(ids=p + 65536, n=0)) == nat.E_INVALID and "bad sizes" in nat.last_error()
    assert call(*args(ids=p + 65536, n=5, **fine_up_to_the_order)) == nat.E_INVALID and "permutation" in nat.last_error()
    assert call(*args(out=0, rt=7)) == nat.E_INVALID, "sizes come before the dtypes"
    for rt in (3, -1):
        assert call(*args(rt=rt)) == nat.E_UNSUPPORTED and "float32" in nat.last_error(), rt
    assert call(*args(dt=nat.F32)) == nat.E_UNSUPPORTED and "float16 and bfloat16" in nat.last_error(), "the codebooks are fp16 / bf16"
    assert call(*args(rt=5, dt=nat.F32)) == nat.E_UNSUPPORTED and "float32 (dtype id 5)" in nat.last_error(), "the reference's dtype comes first"
    assert call(*args(dt=nat.F32, K=9)) == nat.E_UNSUPPORTED and "float16 and bfloat16" in nat.last_error(), "dtypes come before the scheme"
    for bad in ({"K": 0}, {"K": 9}, {"K": -2}, {"g": 4, "n": 4096}, {"g": 64, "n": 256}, {"beam": 0}, {"beam": 17}, {"beam": -1}):
        assert call(*args(**bad)) == nat.E_UNSUPPORTED and "shape outside" in nat.last_error(), bad
    huge = {"out": 1 << 15, "in": 1 << 19, "stride": 1 << 19, "n": 1 << 31}
    assert call(*args(**huge)) == nat.E_UNSUPPORTED and "shape outside" in nat.last_error()
    assert call(*args(ids=p + 65536, n=1 << 31)) == nat.E_UNSUPPORTED and "shape outside" in nat.last_error()
    assert call(*args(K=9, order=order(0, 0))) == nat.E_UNSUPPORTED, "the scheme comes before dim_order"
    for K, bad in ((2, (0, 0)), (2, (0, 2)), (2, (-1, 0)), (3, (0, 1, 3)), (3, (2, 2, 1)), (1, (1,))):
        assert call(*args(K=K, order=order(*bad))) == nat.E_INVALID and "permutation" in nat.last_error(), bad


def test_the_python_entry_checks_its_arguments_before_the_library_is_called():
    from aqlm_amd.inference_kernels import hip_kernel as hk

    reference = torch.zeros((4, 32))
    books, prev = torch.zeros((2, 256, 8), dtype=torch.float16), torch.zeros((16, 2), dtype=torch.int8)
    with pytest.raises(ValueError, match="on the GPU"):
        hk.code_search_kx8(reference, None, books, prev, 8, 4)
    with pytest.raises(ValueError, match="permutation"):
        hk.code_search_kx8(reference, None, books, prev, 8, 4, dim_order=[0, 0])


# ---------------------------------------------------------------------------------------------------------------------------
# 3. the predicate
# ---------------------------------------------------------------------------------------------------------------------------
SCHEMES = ((1, 8, 1, 8), (2, 8, 1, 8), (4, 8, 1, 16), (8, 8, 1, 32), (3, 8, 1, 8), (9, 8, 1, 8), (0, 8, 1, 8), (2, 8, 2, 8), (2, 8, 1, 4),
           (2, 8, 1, 64), (2, 16, 1, 8), (1, 16, 1, 8), (1, 16, 1, 16), (2, 12, 1, 8))
TAKEN = SCHEMES[:5]


def test_route_predicate_is_a_pure_table(monkeypatch):
    import aqlm.tuning as tuning

    assert tuning.CODE_SEARCH_KERNEL is True
    for switch in (True, False):
        monkeypatch.setattr(tuning, "CODE_SEARCH_KERNEL", switch)
        for scheme in SCHEMES:
            for beam in (1, 4, 8, 16, 17, 0):
                for on_gpu, dtypes_ok, supported in itertools.product((False, True), repeat=3):
                    want = switch and scheme in TAKEN and 1 <= beam <= 16 and on_gpu and dtypes_ok and supported
                    got = tuning.takes_code_search_kernel_kx8(*scheme, beam, on_gpu, dtypes_ok, supported)
                    assert got is want, (scheme, beam, on_gpu, dtypes_ok, supported)
                    # the 1x16 predicate is what it was on the same rows, and the two are never true together
                    old = tuning.takes_code_search_kernel(*scheme, on_gpu, dtypes_ok, supported)
                    assert old is (switch and scheme in ((1, 16, 1, 8), (1, 16, 1, 16)) and on_gpu and dtypes_ok and supported)
                    assert not (got and old)
    monkeypatch.setattr(tuning, "CODE_SEARCH_KERNEL", True)
    base = [2, 8, 1, 8, 8, True, True, True]
    assert tuning.takes_code_search_kernel_kx8(*base) is True
    for i, other in enumerate((9, 16, 2, 4, 17, False, False, False)):  # flipping any one argument flips the result
        flipped = list(base)
        flipped[i] = other
        assert tuning.takes_code_search_kernel_kx8(*flipped) is False, i
    monkeypatch.setattr(tuning, "CODEBOOK_GRAD_KERNEL", False)  # the switch of the gradient kernels is another switch
    assert tuning.takes_code_search_kernel_kx8(*base) is True


def test_host_tensors_and_fp32_parameters_keep_the_torch_route(monkeypatch):
    """On this side of the predicate nothing changed: a host call never reaches the kernel's Python entry."""
    import aqlm.tuning as tuning
    from aqlm_amd.inference_kernels import hip_kernel as hk

    monkeypatch.setattr(hk, "code_search_kx8", lambda *a, **k: pytest.fail("the kernel entry was called for host tensors"))
    c = model.dyadic_case(2, 8, out_features=4, groups_per_row=8)
    from aqlm_amd.utils import pack_int_data

    prev = pack_int_data(torch.from_numpy(c["prev"]).reshape(4, 8, 2), 8)
    for dtype in (torch.float32, torch.float16):
        got = tuning.find_optimal_codes(torch.from_numpy(c["reference"]), torch.from_numpy(c["codebooks"]).reshape(2, 256, 1, 8).to(dtype), prev,
                                        torch.from_numpy(c["scales"]).reshape(-1, 1, 1, 1).to(dtype), beam_size=4)
        want, _, tied = model.search(c["reference"], c["scales"], c["codebooks"], c["prev"], 8, 4)
        assert not tied.any() and torch.equal(got.to(torch.int64).reshape(-1, 2) % 256, torch.from_numpy(want))


# ---------------------------------------------------------------------------------------------------------------------------
# 4. the model against the reference's codes
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["d", "e", "f"])
def test_model_reproduces_the_reference_code_for_code(case):
    z = np.load(os.path.join(ROOT, "tests", "golden", "code_update_golden.npz"))
    meta = json.loads(str(z["meta"]))
    info = meta["cases"][case]
    name = info["layer"]
    out_features, in_features, K, nbits, ogs, g = meta["layers"][name]["shape"]
    assert (nbits, ogs) == (8, 1) and (K, g) == {"d": (2, 8), "e": (2, 8), "f": (4, 16)}[case]
    books = (z[f"{name}_codebook_k"].astype(np.float32) * np.float32(meta["grid"])).reshape(K, 256, g)
    target = z[f"{name}_reference_k"].astype(np.float32) * np.float32(meta["grid"])
    scales = (2.0 ** z[f"{name}_scale_exp"].astype(np.float32)).reshape(-1)
    prev = z[f"{name}_prev_codes"].astype(np.int64).reshape(-1, K)
    expected = z[f"{case}_expected"].astype(np.int64).reshape(-1, K)
    options = info["options"]
    assert options.get("beam_size", 1) == {"d": 1, "e": 4, "f": 2}[case] and options.get("dim_order") == ([2, 0, 3, 1] if case == "f" else None)
    codes, score, _ = model.search(target, scales, books, prev, g, options.get("beam_size", 1), options.get("dim_order"))
    assert codes.shape == expected.shape and int(codes.min()) >= 0 and int(codes.max()) <= 255
    assert np.array_equal(codes, expected), f"{int((codes != expected).any(-1).sum())} groups differ"
    assert 0.3 <= float((codes != prev).any(-1).mean()) <= 0.7
    # with two codebooks the score is the squared distance the returned codes leave (every sum is exact on the fixture's grid); with
    # more, the position-wise residues of a beam step make it the distance of a hypothesis that may have moved to another position
    if K == 2:
        r = model.quotient(target, scales, g, np.float64)
        left = r - sum(books[c][codes[:, c]].astype(np.float64) for c in range(K))
        assert np.array_equal(score.astype(np.float64), (left * left).sum(-1))


# ---------------------------------------------------------------------------------------------------------------------------
# 5. the model on the dyadic grid: float32 is exact there, and the codes are the torch route's
# ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _dyadic(K, g, beam):
    c = model.dyadic_case(K, g)
    return c, model.search(c["reference"], c["scales"], c["codebooks"], c["prev"], g, beam)


@pytest.mark.parametrize("K,g,beam", DYADIC)
def test_float32_and_float64_compute_the_same_scores_on_the_dyadic_generator(K, g, beam):
    c, (codes, score, tied) = _dyadic(K, g, beam)
    assert c["reference"].shape == (64, 32 * g) and codes.shape == (2048, K)
    codes64, score64, tied64 = model.search(c["reference"], c["scales"], c["codebooks"], c["prev"], g, beam, dtype=np.float64)
    assert score.dtype == np.float32 and score64.dtype == np.float64
    assert np.array_equal(score.astype(np.float64), score64), "the inputs are exact in float32: both precisions give the same bits"
    assert np.array_equal(codes, codes64) and np.array_equal(tied, tied64)
    assert float(np.abs(score64).max()) / model.GRID ** 2 < 2 ** 24


@pytest.mark.parametrize("K,g,beam", DYADIC)
def test_model_equals_the_torch_route_in_float64_on_every_group_without_an_exact_tie(K, g, beam):
    import aqlm.tuning as tuning

    c, (codes, _, tied) = _dyadic(K, g, beam)
    share, changed = float(tied.mean()), float((codes != c["prev"]).any(-1).mean())
    print(f"{K}x8 g{g} beam {beam}: {100 * share:.2f} % of the groups have an exact tie among the best keep + 1 scores of some step, "
          f"{100 * changed:.1f} % change code")
    assert share <= TIE_CAP, "a condition on the inputs"
    assert changed >= 0.3, "the inputs must not pass on an identity"
    r = torch.from_numpy(model.quotient(c["reference"], c["scales"], g, np.float64))
    want = tuning._beam_codes_torch(r, torch.from_numpy(c["codebooks"]).double(), torch.from_numpy(c["prev"]), beam, list(range(K)),
                                    tuning.CODE_SEARCH_CHUNK_VALUES).numpy()
    differ = (codes != want).any(-1) & ~tied
    assert not differ.any(), f"{int(differ.sum())} groups without a tie differ from the torch route"
