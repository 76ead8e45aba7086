"""Residual k-means initialisation of AQLM layers, the parts that need no GPU: the C ABI of aqlm_hip_kmeans_assign / _update (symbols,
the support and workspace queries, the argument checks on host buffers in their documented order), the route predicate as a truth
table, the torch route of ``aqlm.tuning.fit_kmeans`` / ``init_aq_kmeans`` against what the reference's own functions produced
(tests/golden/kmeans_golden.npz, written by tools/gen_kmeans_golden.py: seeds whose float64 margins stay above 1e-4 of the score scale,
so the expected codes hold on any BLAS), ``init_layer_kmeans_`` on a host layer, tests/kmeans_model.py against exact rational
arithmetic, and the code object of kmeans.hip (10 kernels, no scratch)."""
import ctypes
import itertools
import json
import os
import re
import shutil
import subprocess
from fractions import Fraction

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import kmeans_model as model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
ISA_FLAGS = ["-O3", "-std=c++17", "--offload-arch=gfx950", "-fPIC", "-ffp-contract=fast", "-mllvm",
             "-amdgpu-kernarg-preload-count=14", "--cuda-device-only", "-S"]  # the Makefile's flags
NEW = ("aqlm_hip_kmeans_supported", "aqlm_hip_kmeans_workspace_bytes", "aqlm_hip_kmeans_assign", "aqlm_hip_kmeans_update")


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
    eps = float(re.search(r"#define AQLM_HIP_KMEANS_EPS ([0-9.e+-]+)", text).group(1))
    assert eps == nat.KMEANS_EPS and eps <= 2.0 ** -17
    from aqlm_amd.inference_kernels import hip_kernel  # noqa: F401  (registers the ops)

    assert hasattr(torch.ops.aqlm, "kmeans_assign") and hasattr(torch.ops.aqlm, "kmeans_update_")
    for fn in ("kmeans_supported", "kmeans_assign", "kmeans_update"):
        assert callable(getattr(hip_kernel, fn))
    assert hip_kernel.KMEANS_EPS == eps


def test_supported_query():
    from aqlm_amd import _native as nat
    from aqlm_amd.inference_kernels import hip_kernel as hk

    fn = nat.lib.aqlm_hip_kmeans_supported
    for n, k, d in ((1, 128, 8), (2085, 256, 16), (2097152, 65536, 8), (2**31 - 1, 384, 16), (129, 65408, 8), (7, 4096, 16)):
        assert fn(n, k, d) == 1, (n, k, d)
    for d in (4, 12, 32, 0, -8):
        assert fn(1000, 256, d) == 0, d
    for k in (64, 200, 65664, 0, -128, 127, 129, 65536 + 128):
        assert fn(1000, k, 8) == 0, k
    for n in (0, 2**31, -1, 2**40):
        assert fn(n, 256, 8) == 0, n
    assert hk.kmeans_supported(1000, 256, 8) and not hk.kmeans_supported(1000, 256, 32) and not hk.kmeans_supported(0, 256, 8)


def test_workspace_is_the_documented_formula():
    from aqlm_amd import _native as nat

    ws = nat.lib.aqlm_hip_kmeans_workspace_bytes
    for n, k, d in itertools.product((1, 2085, 2**31 - 1), (128, 256, 384, 4096, 65536), (8, 16)):
        assert ws(n, k, d) == 256 + k * 4 + k * d * 4, (n, k, d)  # header, |C_c|^2 in fp32, two fp16 images of the centroids
    assert ws(0, 256, 8) == 0 and ws(2**31, 256, 8) == 0 and ws(100, 200, 8) == 0 and ws(100, 256, 12) == 0 and ws(100, 65664, 8) == 0


# ---------------------------------------------------------------------------------------------------------------------------
# 2. argument checks, on dummy host pointers: every call returns before the device is touched
# ---------------------------------------------------------------------------------------------------------------------------
def test_assign_checks_report_the_documented_codes_in_the_documented_order():
    from aqlm_amd import _native as nat

    buf = ctypes.create_string_buffer(1 << 17)
    p = (ctypes.addressof(buf) + 15) // 16 * 16
    need = nat.lib.aqlm_hip_kmeans_workspace_bytes(300, 256, 8)
    args = lambda **kw: [kw.get(n, d) for n, d in (  # noqa: E731
        ("data", p), ("n", 300), ("cent", p + 16384), ("k", 256), ("d", 8), ("absmax", 3.5), ("codes", p + 32768 + 4), ("sums", p + 40960 + 8),
        ("counts", p + 65536 + 4), ("ws", p + 81920), ("ws_bytes", need), ("stream", None))]
    call = nat.lib.aqlm_hip_kmeans_assign
    for null in ("data", "cent", "codes", "ws"):
        assert call(*args(**{null: None})) == nat.E_INVALID and "null pointer" in nat.last_error(), null
    for lone in ("sums", "counts"):  # both or neither
        assert call(*args(**{lone: None})) == nat.E_INVALID and "null pointer" in nat.last_error(), lone
    assert call(*args(data=None, d=12, n=0)) == nat.E_INVALID and "null pointer" in nat.last_error(), "null pointers come first"
    misaligned = (("data", p + 8), ("data", p + 4), ("cent", p + 16384 + 8), ("codes", p + 32768 + 2), ("sums", p + 40960 + 4),
                  ("counts", p + 65536 + 2), ("ws", p + 81920 + 8))
    for name, addr in misaligned:
        assert call(*args(**{name: addr})) == nat.E_INVALID and "misaligned" in nat.last_error(), name
    assert call(*args(cent=p + 16384 + 8, n=0)) == nat.E_INVALID and "misaligned" in nat.last_error(), "alignment comes before the sizes"
    for bad in ({"n": 0}, {"n": -4}, {"k": 0}, {"d": 0}, {"d": -8}, {"absmax": -1.0}, {"absmax": float("inf")}, {"absmax": float("nan")}):
        assert call(*args(**bad)) == nat.E_INVALID and "bad sizes" in nat.last_error(), bad
    assert call(*args(n=0, d=12)) == nat.E_INVALID, "sizes come before the shape"
    for bad in ({"d": 4}, {"d": 12}, {"d": 32}, {"k": 64}, {"k": 200}, {"k": 65664}, {"n": 2**31}):
        assert call(*args(**bad)) == nat.E_UNSUPPORTED and "shape outside" in nat.last_error(), bad
    assert call(*args(d=32, ws_bytes=0)) == nat.E_UNSUPPORTED, "the shape comes before the workspace"
    assert call(*args(ws_bytes=need - 4)) == nat.E_INVALID and f"{need} bytes are needed" in nat.last_error()
    # sums_out and counts_out NULL together, and data_absmax 0, are valid arguments: the first complaint is the next one in line
    assert call(*args(sums=None, counts=None, absmax=0.0, ws_bytes=0)) == nat.E_INVALID and "bytes are needed" in nat.last_error()


def test_update_checks_report_the_documented_codes_in_the_documented_order():
    from aqlm_amd import _native as nat

    buf = ctypes.create_string_buffer(1 << 16)
    p = (ctypes.addressof(buf) + 15) // 16 * 16
    args = lambda **kw: [kw.get(n, d) for n, d in (  # noqa: E731
        ("sums", p + 8), ("counts", p + 20480 + 4), ("n", 300), ("k", 256), ("d", 8), ("absmax", 3.5), ("cent", p + 32768 + 4), ("stream", None))]
    call = nat.lib.aqlm_hip_kmeans_update
    for null in ("sums", "counts", "cent"):
        assert call(*args(**{null: None})) == nat.E_INVALID and "null pointer" in nat.last_error(), null
    for name, addr in (("sums", p + 4), ("counts", p + 20480 + 2), ("cent", p + 32768 + 2)):
        assert call(*args(**{name: addr})) == nat.E_INVALID and "misaligned" in nat.last_error(), name
    assert call(*args(sums=p + 4, k=0)) == nat.E_INVALID and "misaligned" in nat.last_error(), "alignment comes before the sizes"
    for bad in ({"n": 0}, {"k": 0}, {"d": 0}, {"absmax": -2.0}, {"absmax": float("nan")}):
        assert call(*args(**bad)) == nat.E_INVALID and "bad sizes" in nat.last_error(), bad
    for bad in ({"d": 12}, {"k": 200}, {"n": 2**31}):
        assert call(*args(**bad)) == nat.E_UNSUPPORTED and "shape outside" in nat.last_error(), bad


# ---------------------------------------------------------------------------------------------------------------------------
# 3. the predicate
# ---------------------------------------------------------------------------------------------------------------------------
def test_route_predicate_is_a_pure_table(monkeypatch):
    import aqlm.tuning as tuning

    assert tuning.KMEANS_KERNEL is True
    sizes = (16, 64, 128, 200, 256, 384, 4096, 65536, 65664, 131072)
    for switch in (True, False):
        monkeypatch.setattr(tuning, "KMEANS_KERNEL", switch)
        for k, dim, on_gpu, dtype, ogs in itertools.product(sizes, (4, 8, 12, 16, 32), (False, True),
                                                            (torch.float32, torch.float16, torch.bfloat16, torch.float64), (1, 2)):
            want = switch and k in (128, 256, 384, 4096, 65536) and dim in (8, 16) and on_gpu and dtype == torch.float32 and ogs == 1
            assert tuning.takes_kmeans_kernel(k, dim, on_gpu, dtype, ogs) is want, (switch, k, dim, on_gpu, dtype, ogs)
    monkeypatch.setattr(tuning, "KMEANS_KERNEL", True)
    assert tuning.takes_kmeans_kernel(256, 8, True, torch.float32) is True  # out_group_size defaults to 1
    # the switches of the other kernels are other switches
    monkeypatch.setattr(tuning, "CODE_SEARCH_KERNEL", False)
    monkeypatch.setattr(tuning, "CODEBOOK_GRAD_KERNEL", False)
    assert tuning.takes_kmeans_kernel(65536, 16, True, torch.float32, 1) is True


# ---------------------------------------------------------------------------------------------------------------------------
# 4. the torch route against the reference's results
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden():
    z = np.load(os.path.join(ROOT, "tests", "golden", "kmeans_golden.npz"))
    return z, json.loads(str(z["meta"]))


def _summation_bound(points: np.ndarray, membership: np.ndarray, k: int) -> np.ndarray:
    """[k, d]: count * 2^-24 * mean|x_t| = 2^-24 * the sum of |x_t| over the cluster's points."""
    total = np.zeros((k, points.shape[1]), dtype=np.float64)
    np.add.at(total, membership.astype(np.int64), np.abs(points.astype(np.float64)))
    return total * 2.0 ** -24


@pytest.mark.parametrize("case", ["a", "b"])
def test_fit_kmeans_torch_route_reproduces_the_reference(golden, case):
    import aqlm.tuning as tuning

    z, meta = golden
    info = meta["cases"][case]
    data, rows = torch.from_numpy(z[f"{case}_data"]), torch.from_numpy(z[f"{case}_rows"])
    k = info["k"]
    assert tuple(data.shape) == {"a": (512, 8), "b": (384, 16)}[case] and k == {"a": 32, "b": 16}[case]
    assert info["iterations"] == 7 if case == "a" else info["iterations"] > 1
    assert torch.equal(torch.randperm(data.shape[0], generator=torch.Generator().manual_seed(info["seed"]))[:k], rows)
    before = data.clone()
    centroids, codes, restored, iterations = tuning.fit_kmeans(data, k, initial_centroids=data[rows], return_iterations=True, **info["options"])
    assert torch.equal(data, before) and centroids.dtype == torch.float32 and codes.dtype == torch.int64
    assert iterations == info["iterations"]
    assert np.array_equal(codes.numpy(), z[f"{case}_codes"]), f"{int((codes.numpy() != z[f'{case}_codes']).sum())} points differ"
    bound = _summation_bound(z[f"{case}_data"], z[f"{case}_update_codes"], k)
    assert np.all(np.abs(centroids.numpy().astype(np.float64) - z[f"{case}_centroids"]) <= bound)
    assert torch.equal(restored, centroids[codes])
    # the same start drawn from a generator; three return values without return_iterations
    drawn = tuning.fit_kmeans(data, k, generator=torch.Generator().manual_seed(info["seed"]), **info["options"])
    assert len(drawn) == 3 and torch.equal(drawn[0], centroids) and torch.equal(drawn[1], codes)
    again, rebuilt = tuning.find_nearest_cluster(data, centroids)
    assert torch.equal(again, codes) and torch.equal(rebuilt, restored)


def test_init_aq_kmeans_torch_route_reproduces_the_reference(golden, monkeypatch):
    import aqlm.tuning as tuning

    z, meta = golden
    info = meta["cases"]["c"]
    out_features, in_features, K, ogs, g, size = info["shape"]
    assert (out_features, in_features, K, ogs, g, size) == (32, 64, 2, 1, 8, 16)
    weight = torch.from_numpy(z["c_weight"])
    steps = []
    step = tuning._kmeans_step
    monkeypatch.setattr(tuning, "_kmeans_step", lambda *a: (steps.append(1), step(*a))[1])
    before = weight.clone()
    codes, books = tuning.init_aq_kmeans(weight, num_codebooks=K, out_group_size=ogs, in_group_size=g, codebook_size=size,
                                         max_iter=info["max_iter"], generator=torch.Generator().manual_seed(info["seed"]))
    assert torch.equal(weight, before), "the weight is not written"
    assert codes.dtype == torch.int64 and tuple(codes.shape) == (32, 8, 2) and books.dtype == torch.float32 and tuple(books.shape) == (2, 16, 1, 8)
    assert len(steps) == info["iterations"]
    assert np.array_equal(codes.numpy(), z["c_codes"])
    residue = z["c_weight"].reshape(32, 8, 8).reshape(256, 8).astype(np.float32).copy()
    for c in range(K):
        bound = _summation_bound(residue, z["c_codes"][..., c].reshape(-1), size)
        assert np.all(np.abs(books[c].reshape(size, g).numpy().astype(np.float64) - z["c_codebooks"][c].reshape(size, g)) <= bound), c
        residue -= z["c_codebooks"][c].reshape(size, g)[z["c_codes"][..., c].reshape(-1)]


def test_a_non_finite_value_raises_and_the_options_not_offered_raise():
    import aqlm.tuning as tuning

    data = torch.randn(64, 8, generator=torch.Generator().manual_seed(0))
    for bad in (float("nan"), float("inf"), float("-inf")):
        poisoned = data.clone()
        poisoned[17, 3] = bad
        with pytest.raises(ValueError, match="non-finite"):
            tuning.fit_kmeans(poisoned, 4)
        with pytest.raises(ValueError, match="non-finite"):
            tuning.find_nearest_cluster(poisoned, data[:4])
        with pytest.raises(ValueError, match="non-finite"):
            tuning.init_aq_kmeans(poisoned, num_codebooks=1, out_group_size=1, in_group_size=8, codebook_size=4)
    for name, value in (("greedy_init", True), ("use_faiss", True), ("devices", [torch.device("cpu")])):
        with pytest.raises(NotImplementedError, match=name):
            tuning.fit_kmeans(data, 4, **{name: value})
        with pytest.raises(NotImplementedError, match=name):
            tuning.init_aq_kmeans(data, num_codebooks=1, out_group_size=1, in_group_size=8, codebook_size=4, **{name: value})
    with pytest.raises(TypeError, match="bogus"):
        tuning.fit_kmeans(data, 4, bogus=1)
    with pytest.raises(TypeError, match="bogus"):
        tuning.init_aq_kmeans(data, num_codebooks=1, out_group_size=1, in_group_size=8, codebook_size=4, bogus=1)
    with pytest.raises(ValueError):
        tuning.fit_kmeans(data, 4, initial_centroids=data[:5])
    with pytest.raises(ValueError):
        tuning.init_aq_kmeans(data[:, :6], num_codebooks=1, out_group_size=1, in_group_size=8, codebook_size=4)
    # a cluster that loses all its points keeps its centroid; g = 32 and out_group_size 2 are served (by the torch route)
    far = torch.cat([data[:3], torch.full((1, 8), 1e6)])
    centroids, codes, _ = tuning.fit_kmeans(data, 4, max_iter=3, initial_centroids=far)
    assert torch.equal(centroids[3], far[3]) and int((codes == 3).sum()) == 0
    wide = torch.randn(16, 64, generator=torch.Generator().manual_seed(1))
    for ogs, g in ((1, 32), (2, 8)):
        codes, books = tuning.init_aq_kmeans(wide, num_codebooks=2, out_group_size=ogs, in_group_size=g, codebook_size=8, max_iter=4,
                                             generator=torch.Generator().manual_seed(2))
        assert tuple(codes.shape) == (16 // ogs, 64 // g, 2) and tuple(books.shape) == (2, 8, ogs, g) and int(codes.max()) < 8


# ---------------------------------------------------------------------------------------------------------------------------
# 5. init_layer_kmeans_ on host layers
# ---------------------------------------------------------------------------------------------------------------------------
def _host_layer():
    import aqlm

    layer = aqlm.QuantizedLinear(128, 64, 8, 1, 2, 8, bias=True, dtype=torch.float32)
    with torch.no_grad():
        layer.codebooks.zero_()
        layer.codes.zero_()
        layer.scales.fill_(1.0)
        layer.bias.copy_(torch.linspace(-1, 1, 64))
    return layer


def test_init_layer_kmeans_writes_in_place_and_the_next_forward_uses_the_result():
    import aqlm.tuning as tuning
    from aqlm_amd.utils import _dequantize_weight, unpack_int_data

    layer = _host_layer()
    weight = torch.randn(64, 128, generator=torch.Generator().manual_seed(3)) * torch.linspace(0.5, 2.0, 64)[:, None]
    x = torch.randn(3, 128, generator=torch.Generator().manual_seed(4))
    with torch.no_grad():
        layer(x)  # whatever derived state a forward builds exists before the parameters change
    params = (layer.codes, layer.codebooks, layer.scales)
    versions = [p._version for p in params]
    error = tuning.init_layer_kmeans_(layer, weight, max_iter=5, generator=torch.Generator().manual_seed(5))
    assert (layer.codes, layer.codebooks, layer.scales) == params or all(a is b for a, b in zip((layer.codes, layer.codebooks, layer.scales), params))
    assert all(p._version > v for p, v in zip(params, versions))
    assert layer.codes.dtype == torch.int8 and layer.codebooks.dtype == torch.float32 and not layer.codes.requires_grad
    assert torch.equal(layer.scales.flatten(), weight.norm(dim=-1) + 1e-9)
    dequantised = _dequantize_weight(unpack_int_data(layer.codes, 8), layer.codebooks, layer.scales)
    with torch.no_grad():
        y = layer(x)
    assert torch.allclose(y, F.linear(x, dequantised, layer.bias), rtol=1e-5, atol=1e-4)
    got = float((weight - dequantised).square().sum() / weight.square().sum())
    assert error.dim() == 0 and abs(float(error) - got) <= 1e-5 and 0.0 < got < 0.5, (float(error), got)


def test_init_layer_kmeans_refuses_what_update_codes_refuses():
    import aqlm.tuning as tuning
    from aqlm_amd.moe import QuantizedMixtralExperts
    from aqlm_amd.sharded import ShardedQuantizedLinear

    layer = _host_layer()
    weight = torch.randn(64, 128, generator=torch.Generator().manual_seed(3))
    for name in ("greedy_init", "use_faiss", "devices"):
        with pytest.raises(NotImplementedError, match=name):
            tuning.init_layer_kmeans_(layer, weight, **{name: True})
    with pytest.raises(ValueError):
        tuning.init_layer_kmeans_(layer, weight[:, :64])
    layer._moe_expert = True
    with pytest.raises(TypeError, match="QuantizedLinear.*expert"):
        tuning.init_layer_kmeans_(layer, weight)
    assert int(layer.codes.abs().sum()) == 0, "nothing was written"
    for cls in (QuantizedMixtralExperts, ShardedQuantizedLinear):
        module = cls.__new__(cls)
        torch.nn.Module.__init__(module)
        with pytest.raises(TypeError, match=cls.__name__):
            tuning.init_layer_kmeans_(module, weight)
    with pytest.raises(TypeError, match="Linear"):
        tuning.init_layer_kmeans_(torch.nn.Linear(8, 8), weight)
    with torch.inference_mode():
        frozen = _host_layer()
    with pytest.raises(RuntimeError, match="inference tensor"):
        tuning.init_layer_kmeans_(frozen, weight)


# ---------------------------------------------------------------------------------------------------------------------------
# 6. the numpy model against exact rational arithmetic
# ---------------------------------------------------------------------------------------------------------------------------
def test_model_is_exact_rational_arithmetic_on_a_handful_of_points():
    assert [model.exponent(v) for v in (1.0, 1.99, 2.0, 0.75, 3.5, 0.0, 1e-45, 2.0 ** -126)] == [0, 0, 1, -1, 1, -126, -126, -126]
    assert model.shift(1, 1.0) == 40 and model.shift(5, 1.0) == 40 and model.shift(2**22, 1.0) == 40 and model.shift(2**22 + 1, 1.0) == 39
    assert model.shift(2**31 - 1, 1.0) == 31 and model.shift(2085, 3.5) == 39 and model.shift(2085, 0.3) == 42
    rng = np.random.default_rng(0)
    data = rng.normal(size=(7, 8)).astype(np.float32)
    absmax = np.float32(np.abs(data).max())
    n = data.shape[0]
    s = model.shift(n, absmax)
    half = np.float32(2.0 ** -(s + 1))
    data[0, :4] = [3 * half, 5 * half, -3 * half, -5 * half]  # ties: 1.5, 2.5 -> 2, 2; -1.5, -2.5 -> -2, -2
    assert model.quantise(data, n, absmax)[0, :4].tolist() == [2, 2, -2, -2]
    indices = np.array([2, 0, 2, 2, 5, 0, 2])
    sums, counts = model.sums_and_counts(data, indices, 6, absmax)
    exact = [[Fraction(0)] * 8 for _ in range(6)]
    for row, c in zip(data, indices):
        for t, v in enumerate(row):
            q = round(Fraction(float(v)) * Fraction(2) ** s)  # round(Fraction) rounds ties to even
            exact[c][t] += q
    assert [[int(v) for v in row] for row in exact] == sums.tolist() and counts.tolist() == [2, 0, 4, 0, 0, 1]
    old = rng.normal(size=(6, 8)).astype(np.float32)
    old[1, 0], old[3, 1] = np.float32("nan"), np.float32(-0.0)
    new = model.update(old, sums, counts, n, absmax)
    for c in range(6):
        for t in range(8):
            if counts[c] == 0:
                assert new[c, t].view(np.uint32) == old[c, t].view(np.uint32)
            else:  # int / int is correctly rounded to a double; one more rounding to fp32
                want = np.float32(float(Fraction(int(sums[c][t]), int(counts[c]) * 2 ** s)))
                assert new[c, t].view(np.uint32) == want.view(np.uint32), (c, t)
                assert abs(Fraction(float(new[c, t])) - sum(Fraction(float(data[i, t])) for i in np.flatnonzero(indices == c)) / int(counts[c])) \
                    <= Fraction(1, 2 ** 24) * abs(Fraction(float(new[c, t]))) + Fraction(1, 2 ** (s - 1))
    # a rejected point joins nothing
    poisoned = data.copy()
    poisoned[1, 2], poisoned[4, 0] = np.float32("nan"), np.float32("inf")
    poisoned[6, 7] = np.float32(2) * absmax
    assert model.accepted(poisoned, absmax).tolist() == [True, False, True, True, False, True, False]
    keep = np.array([0, 2, 3, 5])
    sums_p, counts_p = model.sums_and_counts(poisoned, indices, 6, absmax)
    part = np.zeros((6, 8), dtype=np.int64)
    np.add.at(part, indices[keep], model.quantise(data[keep], n, absmax))
    assert np.array_equal(sums_p, part) and counts_p.tolist() == [1, 0, 3, 0, 0, 0]


# ---------------------------------------------------------------------------------------------------------------------------
# 7. the code object
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_code_object_holds_the_kernels_without_scratch(tmp_path):
    out = tmp_path / "kmeans.s"
    subprocess.run([HIPCC] + ISA_FLAGS + [os.path.join(ROOT, "aqlm_amd", "csrc", "kmeans.hip"), "-o", str(out)], check=True,
                   stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=900)
    text = out.read_text()
    pattern = r"_ZN4aqlm\d+kmeans_(?:absmax|split|assign|update)_kernel\w+"
    names = set(re.findall(rf"^\s+\.name:\s+({pattern})", text, re.M))
    # the maximum, the split for d 8 / 16, the assignment for d 8 / 16 x (no sums, direct adds, LDS pre-reduction), the update
    assert len(names) == 10 and sum("assign" in n for n in names) == 6 and sum("split" in n for n in names) == 2, names
    seen = 0
    for m in re.finditer(rf"\.name:\s+({pattern})(.*?)(?=\n  - |\Z)", text, re.S):
        assert re.search(r"\.private_segment_fixed_size:\s+0\b", m.group(2)), m.group(1)
        assert re.search(r"\.vgpr_spill_count:\s+0\b", m.group(2)) and re.search(r"\.sgpr_spill_count:\s+0\b", m.group(2)), m.group(1)
        seen += 1
    assert seen == 10
    assert "cmpswap" not in text, "every atomic is a native add or max, no compare-and-swap loop"
    for name in names:
        body = re.split(rf"^{name}:", text, maxsplit=1, flags=re.M)[1].split(".Lfunc_end", 1)[0]
        assert not re.search(r"\bscratch_(load|store)", body), f"{name}: scratch access"
        mfma = len(re.findall(r"\bv_mfma_f32_32x32x16_f16\b", body))
        if "assign" in name:
            # four point tiles per centroid tile: hi and lo of the centroids at d 8, hi.hi + hi.lo + lo.hi at d 16
            assert mfma == (8 if "ILi8E" in name else 12), f"{name}: {mfma} MFMAs"
            mode = int(re.search(r"ILi\d+ELi(\d)E", name).group(1))
            assert ("global_atomic_add_x2" in body) == (mode != 0), name  # 64-bit integer adds to memory
            assert ("ds_add_u64" in body) == (mode == 2), name            # ... and to LDS on the pre-reduced path only
        else:
            assert mfma == 0, name
