"""aqlm_hip_kmeans_assign / aqlm_hip_kmeans_update and the k-means initialisation built on them, on the MI355X.  The oracle of the
assignment is a float64 brute force over all centroids, computed in chunks on the device, of ``S(n, c) = |C_c|^2 - 2 <x_n, C_c>``.
The accuracy contract is held as include/aqlm_hip.h states it, with the documented epsilon (2^-17):
  * every point whose float64 margin between the best and the second best exceeds 2 E(n), E(n) = eps (|x_n|^2 + max |C_c|^2), must
    equal the float64 argmin exactly;
  * every other point (the near-tie class) must score within 2 E(n) of the minimum;
  * the near-tie class may hold at most 2 % of the points -- a condition on eps, not a tolerance.
The sums, the counts and the update are held bit for bit to tests/kmeans_model.py.  Cases use 2085 points unless stated; the seeded
inputs and their oracle are computed once per configuration."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import kmeans_model as model

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
POINTS = 2085
SIGMA = {8: 0.3, 16: 0.65}  # noise on the planted centroid


@pytest.fixture(scope="module")
def hk():
    from aqlm_amd.inference_kernels import hip_kernel

    return hip_kernel


def oracle(x, centroids, chunk=512):
    """x [N, d] float64, centroids [k, d] float64 -> (argmin, minimum, margin to the second best) in float64."""
    norms = centroids.square().sum(-1)
    best = torch.empty((x.shape[0],), dtype=torch.int64, device=x.device)
    low = torch.empty((x.shape[0],), dtype=torch.float64, device=x.device)
    margin = torch.empty_like(low)
    for a in range(0, x.shape[0], chunk):
        scores = norms[None] - 2 * (x[a:a + chunk] @ centroids.T)
        values, indices = scores.topk(2, dim=-1, largest=False, sorted=True)
        best[a:a + chunk], low[a:a + chunk], margin[a:a + chunk] = indices[:, 0], values[:, 0], values[:, 1] - values[:, 0]
    return best, low, margin


def tolerance(x, centroids, eps):
    return eps * (x.square().sum(-1) + centroids.square().sum(-1).max())


def hold_to_contract(got, x, centroids, eps, expect=None, what=""):
    """The three conditions of the module docstring for the indices ``got`` [N] of the points ``x``; ``expect``: a precomputed
    ``oracle(x, centroids)``.  Returns the share of the near-tie class."""
    best, low, margin = oracle(x, centroids) if expect is None else expect
    E = tolerance(x, centroids, eps)
    near = margin <= 2 * E
    share = float(near.double().mean())
    score = centroids.square().sum(-1)[got] - 2 * (x * centroids[got]).sum(-1)
    wrong = int(((got != best) & ~near).sum())
    excess = float(((score - low) / (2 * E)).max())
    print(f"{what}: near-tie class {100 * share:.3f} % of {x.shape[0]} points, {wrong} separated points differ from the float64 argmin, "
          f"{int((got != best).sum())} differ in all, worst (score - min) / 2E = {excess:.4f}")
    assert share <= 0.02, f"{what}: {100 * share:.2f} % of the points lie within 2 E of a tie"
    assert wrong == 0, f"{what}: {wrong} points with a float64 margin above 2 E differ from the float64 argmin"
    assert excess <= 1.0, f"{what}: a chosen centroid scores {excess:.3f} x 2 E above the minimum"
    return share


@functools.lru_cache(maxsize=None)
def case(d, k, kind, n=POINTS):
    """Seeded inputs (seed 1000 d + k) and their float64 oracle.  ``gauss``: points and centroids N(0, 1); ``planted``: points = a random
    centroid + sigma N(0, 1); ``lloyd``: the centroids are the means after one float64 Lloyd step from N(0, 1) centroids.  Nothing in
    the result is written by a test."""
    gen = torch.Generator().manual_seed(1000 * d + k)
    data = torch.randn((n, d), generator=gen)
    centroids = torch.randn((k, d), generator=gen)
    if kind == "planted":
        data = centroids[torch.randint(0, k, (n,), generator=gen)] + SIGMA[d] * torch.randn((n, d), generator=gen)
    data, centroids = data.to(DEV), centroids.to(DEV)
    if kind == "lloyd":
        first = oracle(data.double(), centroids.double())[0]
        means = centroids.double().clone().index_reduce_(0, first, data.double(), "mean", include_self=False)
        centroids = means.float()
    c = {"data": data, "centroids": centroids, "x64": data.double(), "c64": centroids.double(), "absmax": float(data.abs().max())}
    c["oracle"] = oracle(c["x64"], c["c64"])
    return c


def assign(hk, c, **kw):
    codes, sums, counts = hk.kmeans_assign(kw.pop("data", c["data"]), kw.pop("centroids", c["centroids"]), kw.pop("absmax", c["absmax"]), **kw)
    assert codes.dtype == torch.int32
    return codes.to(torch.int64), sums, counts


# ---------------------------------------------------------------------------------------------------------------------------
# 1. the assignment contract
# ---------------------------------------------------------------------------------------------------------------------------
CONTRACT = [(d, k, kind) for d in (8, 16) for k in (128, 256, 384, 4096, 65536) for kind in ("gauss", "planted", "lloyd")
            if not (k == 65536 and kind == "lloyd")]


@pytest.mark.parametrize("d,k,kind", CONTRACT)
def test_indices_equal_the_float64_argmin_outside_the_near_tie_class(hk, d, k, kind):
    c = case(d, k, kind)
    got, sums, counts = assign(hk, c)
    assert got.shape == (POINTS,) and int(got.min()) >= 0 and int(got.max()) < k
    assert sums.dtype == torch.int64 and tuple(sums.shape) == (k, d) and counts.dtype == torch.int32 and int(counts.sum()) == POINTS
    hold_to_contract(got, c["x64"], c["c64"], hk.KMEANS_EPS, c["oracle"], f"d {d}, k {k}, {kind} centroids")
    alone = assign(hk, c, with_sums=False)
    assert torch.equal(alone[0], got) and alone[1].numel() == 0 and alone[2].numel() == 0, "the index does not depend on the sums"


def test_many_blocks_of_points_per_workgroup(hk):
    """More blocks of 128 points than the LDS pre-reduced launch has workgroups: a workgroup walks several blocks and flushes once."""
    n, k, d = 128 * 1024 + 8965, 256, 8
    c = case(d, k, "gauss", n=n)
    got, sums, counts = assign(hk, c)
    hold_to_contract(got, c["x64"], c["c64"], hk.KMEANS_EPS, c["oracle"], f"{n} points")
    want_sums, want_counts = model.sums_and_counts(c["data"].cpu().numpy(), got.cpu().numpy(), k, c["absmax"])
    assert np.array_equal(sums.cpu().numpy(), want_sums) and np.array_equal(counts.cpu().numpy(), want_counts)


# ---------------------------------------------------------------------------------------------------------------------------
# 2. edges of the tiling
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [8, 16])
@pytest.mark.parametrize("k", [128, 384])
def test_winners_at_both_ends_of_every_waves_range(hk, d, k):
    c = case(d, k, "gauss")
    ends = torch.tensor([e for w in range(4) for e in (w * k // 4, (w + 1) * k // 4 - 1)], device=DEV)
    for n in (1, 31, 127, 128, 129, 257):
        for shift in range(0, 8, 3):
            planted = ends[(torch.arange(n, device=DEV) + shift) % 8]
            data = c["centroids"][planted].contiguous()
            got, _, counts = assign(hk, c, data=data, absmax=float(data.abs().max()))
            assert got.shape == (n,) and torch.equal(got, planted), (n, shift, got.tolist()[:16])
            assert torch.equal(counts.to(torch.int64), torch.bincount(planted, minlength=k))


# ---------------------------------------------------------------------------------------------------------------------------
# 3. ties, order and magnitudes
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,k", [(8, 128), (16, 4096), (8, 65536), (16, 65536)])
def test_equal_scores_give_the_smallest_index_and_the_last_index_comes_back(hk, d, k):
    c = case(d, k, "gauss")
    centroids = c["centroids"].clone()
    twins = (5, 70000 % k, k - 1)
    assert len(set(twins)) == 3
    centroids[twins[1]] = centroids[twins[2]] = centroids[5]
    gen = torch.Generator().manual_seed(3)
    rows = [centroids[t] for t in twins] + [centroids[0], centroids[k - 2]]
    rows += [centroids[5] + 1e-3 * torch.randn((d,), generator=gen).to(DEV) for _ in range(27)]
    got = hk.kmeans_assign(torch.stack(rows).contiguous(), centroids, 8.0, with_sums=False)[0]
    assert got.dtype == torch.int32 and got.tolist() == [5, 5, 5, 0, k - 2] + [5] * 27
    # the last centroid, distinct again: 65535 is 65535 in int32, not -1
    got = hk.kmeans_assign(c["centroids"][k - 1:].contiguous(), c["centroids"], 8.0, with_sums=False)[0]
    assert got.tolist() == [k - 1]


@pytest.mark.parametrize("d,k", [(8, 256), (16, 384), (8, 65536)])
def test_powers_of_two_do_not_change_the_indices(hk, d, k):
    c = case(d, k, "planted")
    got = assign(hk, c, with_sums=False)[0]
    for factor in (2.0 ** -30, 2.0 ** 30):
        scaled = assign(hk, c, data=c["data"] * factor, centroids=c["centroids"] * factor, absmax=c["absmax"] * factor, with_sums=False)[0]
        assert torch.equal(scaled, got), factor


# ---------------------------------------------------------------------------------------------------------------------------
# 4. sums, counts and rejected points
# ---------------------------------------------------------------------------------------------------------------------------
def raw_assign(hk, data, centroids, absmax, codes, sums, counts):
    """The entry on caller-owned buffers."""
    from aqlm_amd import _native as nat

    n, d, k = data.shape[0], data.shape[1], centroids.shape[0]
    ws = hk._workspace(data.device, int(nat.lib.aqlm_hip_kmeans_workspace_bytes(n, k, d)))
    rc = nat.lib.aqlm_hip_kmeans_assign(data.data_ptr(), n, centroids.data_ptr(), k, d, absmax, codes.data_ptr(), sums.data_ptr(),
                                        counts.data_ptr(), ws.data_ptr(), ws.numel() * 4, torch.cuda.current_stream().cuda_stream)
    nat.check(rc, "kmeans_assign")


SUMS = [(8, 256), (16, 256), (8, 1024), (16, 4096), (8, 65536)]  # LDS pre-reduced: the first three (64 KiB of sums at k 1024); direct: the others


@pytest.mark.parametrize("d,k", SUMS)
def test_sums_and_counts_equal_the_model_bit_for_bit(hk, d, k):
    c = case(d, k, "planted")
    got, sums, counts = assign(hk, c)
    want_sums, want_counts = model.sums_and_counts(c["data"].cpu().numpy(), got.cpu().numpy(), k, c["absmax"])
    assert np.array_equal(sums.cpu().numpy(), want_sums) and np.array_equal(counts.cpu().numpy(), want_counts)
    assert int(want_counts.max()) > 1 or k == 65536, "clusters of several points"
    again = assign(hk, c)
    assert torch.equal(again[0], got) and torch.equal(again[1], sums) and torch.equal(again[2], counts), "a second call, identical bits"
    # a pre-filled buffer is overwritten, not added to
    codes = torch.full((POINTS,), -7, dtype=torch.int32, device=DEV)
    filled, filled_counts = torch.full((k, d), 1 << 40, dtype=torch.int64, device=DEV), torch.full((k,), 99, dtype=torch.int32, device=DEV)
    raw_assign(hk, c["data"], c["centroids"], c["absmax"], codes, filled, filled_counts)
    assert torch.equal(codes.to(torch.int64), got) and torch.equal(filled, sums) and torch.equal(filled_counts, counts)
    # a larger data_absmax is a coarser unit: the model follows
    wide = assign(hk, c, absmax=c["absmax"] * 5)
    want_sums, want_counts = model.sums_and_counts(c["data"].cpu().numpy(), got.cpu().numpy(), k, c["absmax"] * 5)
    assert torch.equal(wide[0], got) and np.array_equal(wide[1].cpu().numpy(), want_sums) and np.array_equal(wide[2].cpu().numpy(), want_counts)


@pytest.mark.parametrize("d,k", [(8, 256), (16, 4096)])
def test_rejected_points_get_an_index_and_join_no_sum(hk, d, k):
    c = case(d, k, "planted")
    clean = assign(hk, c)[0]
    data = c["data"].clone()
    bad = [3, 128 + 31, 2084]
    data[bad[0], 1] = float("nan")
    data[bad[1], d - 1] = float("-inf")
    data[bad[2], 0] = 2 * c["absmax"]
    got, sums, counts = assign(hk, c, data=data)
    assert int(got.min()) >= 0 and int(got.max()) < k
    keep = torch.ones((POINTS,), dtype=torch.bool, device=DEV)
    keep[bad] = False
    assert torch.equal(got[keep], clean[keep]), "no other row changes"
    keep = keep.cpu().numpy()
    want_sums, want_counts = model.sums_and_counts(c["data"].cpu().numpy()[keep], got.cpu().numpy()[keep], k, c["absmax"], n=POINTS)
    assert np.array_equal(sums.cpu().numpy(), want_sums) and np.array_equal(counts.cpu().numpy(), want_counts)
    assert int(counts.sum()) == POINTS - 3
    whole, whole_counts = model.sums_and_counts(data.cpu().numpy(), got.cpu().numpy(), k, c["absmax"])
    assert np.array_equal(whole, want_sums) and np.array_equal(whole_counts, want_counts), "the model rejects the same rows"
    # the finite row above data_absmax is searched like any other
    x = data[bad[2]:].double()
    hold_to_contract(got[bad[2]:], x, c["c64"], hk.KMEANS_EPS, None, "the row above data_absmax")


@pytest.mark.parametrize("d,k", [(8, 256), (16, 128), (8, 65536)])
def test_update_equals_the_model_and_empty_clusters_keep_their_bits(hk, d, k):
    rng = np.random.default_rng(d + k)
    n = 5000
    data = rng.normal(size=(n, d)).astype(np.float32)
    absmax = float(np.abs(data).max())
    indices = rng.integers(0, k - 40, size=(n,))  # the last 40 clusters are empty
    sums, counts = model.sums_and_counts(data, indices, k, absmax)
    old = rng.normal(size=(k, d)).astype(np.float32)
    old[k - 1].view(np.uint32)[:] = 0x7FC12345  # a NaN with a payload
    old[k - 2] = np.float32(-0.0)
    want = model.update(old, sums, counts, n, absmax)
    centroids = torch.from_numpy(old).to(DEV)
    hk.kmeans_update_(centroids, torch.from_numpy(sums).to(DEV), torch.from_numpy(counts).to(DEV), n, absmax)
    assert np.array_equal(centroids.cpu().numpy().view(np.uint32), want.view(np.uint32))
    empty = counts == 0
    assert empty[k - 40:].all() and np.array_equal(want[empty].view(np.uint32), old[empty].view(np.uint32))
    fresh = hk.kmeans_update(torch.from_numpy(old).to(DEV), torch.from_numpy(sums).to(DEV), torch.from_numpy(counts).to(DEV), n, absmax)
    assert torch.equal(fresh.view(torch.int32), centroids.view(torch.int32))
    # the mean of the points themselves, to one rounding of the fixed-point terms and one of the result
    mean = np.zeros((k, d))
    np.add.at(mean, indices, data.astype(np.float64))
    full = ~empty
    mean[full] /= counts[full][:, None]
    assert np.all(np.abs(want[full] - mean[full]) <= 2.0 ** -24 * np.abs(mean[full]) + 2.0 ** -(model.shift(n, absmax) + 1))


# ---------------------------------------------------------------------------------------------------------------------------
# 5. the fit
# ---------------------------------------------------------------------------------------------------------------------------
def _summation_bound(points, membership, k):
    """[k, d] float64: count * 2^-24 * mean|x_t| = 2^-24 * the sum of |x_t| over the cluster's points."""
    total = torch.zeros((k, points.shape[1]), dtype=torch.float64, device=points.device)
    return total.index_add_(0, membership, points.double().abs()) * 2.0 ** -24


def test_lloyd_iterations_lower_the_objective_and_agree_with_the_torch_route(hk, monkeypatch):
    import aqlm.tuning as tuning

    n, k, d = 4096, 256, 8
    gen = torch.Generator().manual_seed(77)
    data = torch.randn((n, d), generator=gen).to(DEV)
    start = data[torch.randperm(n, generator=gen)[:k].to(DEV)].clone()
    x64 = data.double()
    calls = []
    real = hk.kmeans_assign
    monkeypatch.setattr(hk, "kmeans_assign", lambda *a, **kw: (calls.append(1), real(*a, **kw))[1])
    previous = None
    for iterations in range(1, 7):
        centroids, indices, restored = tuning.fit_kmeans(data, k, max_iter=iterations, initial_centroids=start)
        assert torch.equal(restored, centroids[indices]) and indices.dtype == torch.int64
        objective = float((x64 - centroids.double()[indices]).square().sum())
        slack = float(2 * tolerance(x64, centroids.double(), hk.KMEANS_EPS).sum())
        print(f"{iterations} iterations: objective {objective:.4f} (slack {slack:.4f})")
        assert previous is None or objective <= previous + slack, (iterations, objective, previous)
        previous = objective
    assert len(calls) == sum(i + 1 for i in range(1, 7)), "the kernel took every assignment"
    # one iteration on both routes
    first_kernel, _ = tuning.find_nearest_cluster(data, start)
    after_kernel = tuning.fit_kmeans(data, k, max_iter=1, initial_centroids=start)[0]
    monkeypatch.setattr(tuning, "KMEANS_KERNEL", False)
    calls.clear()
    first_torch, _ = tuning.find_nearest_cluster(data, start)
    after_torch = tuning.fit_kmeans(data, k, max_iter=1, initial_centroids=start)[0]
    assert not calls, "the switch sends the calls through the torch route"
    _, _, margin = oracle(x64, start.double())
    near = margin <= 2 * tolerance(x64, start.double(), hk.KMEANS_EPS)
    assert float(near.double().mean()) <= 0.02 and torch.equal(first_kernel[~near], first_torch[~near])
    same = torch.ones((k,), dtype=torch.bool, device=DEV)
    differ = first_kernel != first_torch
    same[first_kernel[differ]] = False
    same[first_torch[differ]] = False
    print(f"{int(differ.sum())} points differ between the routes, {int(same.sum())} of {k} clusters have identical members")
    assert int(same.sum()) >= k - 2 * int(near.sum())
    bound = _summation_bound(data, first_kernel, k)
    assert ((after_kernel.double() - after_torch.double()).abs() <= bound)[same].all()


@pytest.mark.parametrize("scheme", ["2x8", "1x16"])
def test_init_aq_kmeans_on_the_kernel_route(hk, monkeypatch, scheme):
    """``init_aq_kmeans`` of a 64 x 128 weight as 2x8 g8 (two codebooks of 256) and as 1x16 g8 (one codebook of 65536 for 1024 groups,
    with ``max_points_per_centroid`` so that the subsample path runs; every group is its own centroid).  The relative error ``||W -
    W_q||^2 / ||W||^2`` of the kernel route may exceed the mean of the torch route's over five seeds by three times their spread (max -
    min).  Measured on the MI355X (profiles/kmeans.json, "residual_init"): 2x8 g8 -- kernel route 3.509e-2 at seed 0, torch route mean
    3.545e-2 with a spread of 1.556e-3 over seeds 0 to 4; 1x16 g8 -- 0 on both routes for every seed (1024 groups, each its own
    centroid: the first convergence check stops the fit on the exact points)."""
    import aqlm.tuning as tuning
    from aqlm_amd.utils import _dequantize_weight

    K, size, options = {"2x8": (2, 256, {"max_iter": 10}), "1x16": (1, 65536, {"max_iter": 3, "max_points_per_centroid": 1})}[scheme]
    weight = torch.randn((64, 128), generator=torch.Generator().manual_seed(5)).to(DEV)

    def run(seed):
        codes, books = tuning.init_aq_kmeans(weight, num_codebooks=K, out_group_size=1, in_group_size=8, codebook_size=size,
                                             generator=torch.Generator().manual_seed(seed), **options)
        error = float((weight - _dequantize_weight(codes, books, None)).square().sum() / weight.square().sum())
        return codes, books, error

    calls = []
    real = hk.kmeans_assign
    monkeypatch.setattr(hk, "kmeans_assign", lambda *a, **kw: (calls.append(1), real(*a, **kw))[1])
    codes, books, error = run(0)
    assert calls, "the kernel route ran"
    assert codes.dtype == torch.int64 and tuple(codes.shape) == (64, 16, K) and books.dtype == torch.float32
    assert tuple(books.shape) == (K, size, 1, 8) and int(codes.min()) >= 0 and int(codes.max()) < size
    residue = weight.reshape(64, 16, 8).reshape(1024, 8).clone()
    for c in range(K):  # re-assigning every residue reproduces the codes
        again, restored = tuning.find_nearest_cluster(residue, books[c].reshape(size, 8))
        assert torch.equal(again, codes[..., c].reshape(-1)), c
        residue -= restored
    monkeypatch.setattr(tuning, "KMEANS_KERNEL", False)
    calls.clear()
    errors = [run(seed)[2] for seed in range(5)]
    assert not calls
    mean, spread = sum(errors) / 5, max(errors) - min(errors)
    print(f"{scheme}: kernel route {error:.6e} (seed 0), torch route mean {mean:.6e} spread {spread:.6e} over five seeds")
    assert error <= mean + 3 * spread


def test_init_layer_kmeans_rebuilds_the_derived_state_of_a_gpu_layer(hk, monkeypatch):
    import aqlm
    import aqlm.tuning as tuning
    from aqlm_amd.utils import _dequantize_weight, unpack_int_data

    fin, fout, g = 64, 128, 8
    layer = aqlm.QuantizedLinear(fin, fout, g, 1, 1, 16, bias=True, device=DEV, dtype=torch.float16)
    gen = torch.Generator().manual_seed(9)
    with torch.no_grad():
        layer.codes.copy_(torch.randint(-32768, 32768, (fout, fin // g, 1), generator=gen).to(torch.int16))
        layer.codebooks.copy_(torch.randn((1, 65536, 1, g), generator=gen))
        layer.scales.copy_(torch.rand((fout, 1, 1, 1), generator=gen) + 0.5)
        layer.bias.copy_(torch.randn((fout,), generator=gen) * 0.1)
    xs = {rows: torch.randn((rows, fin), generator=gen).to(torch.float16).to(DEV) for rows in (1, 32)}
    with torch.no_grad():
        before = {rows: layer(x) for rows, x in xs.items()}  # the derived state of the old parameters exists
    weight = (torch.randn((fout, fin), generator=gen) * torch.linspace(0.5, 2.0, fout)[:, None]).to(DEV)
    calls = []
    real = hk.kmeans_assign
    monkeypatch.setattr(hk, "kmeans_assign", lambda *a, **kw: (calls.append(1), real(*a, **kw))[1])
    params = (layer.codes, layer.codebooks, layer.scales)
    versions = [p._version for p in params]
    error = tuning.init_layer_kmeans_(layer, weight, max_iter=3, generator=torch.Generator().manual_seed(1))
    assert calls, "the kernel route ran"
    assert all(a is b for a, b in zip((layer.codes, layer.codebooks, layer.scales), params)) and all(p._version > v for p, v in zip(params, versions))
    assert layer.codes.dtype == torch.int16 and layer.codebooks.dtype == torch.float16 and error.is_cuda and float(error) < 1e-6
    with torch.no_grad():
        w64 = _dequantize_weight(unpack_int_data(layer.codes, 16), layer.codebooks.double(), layer.scales.double())
        assert float((w64 - weight.double()).norm() / weight.double().norm()) < 2.0 ** -9, "every group is its own centroid, rounded to fp16"
        for rows, x in xs.items():
            got = layer(x)
            exact = F.linear(x.double(), w64, layer.bias.double())
            bound = 2.0 ** -10 * exact.abs() + 2.0 ** -13 * F.linear(x.double().abs(), w64.abs(), layer.bias.double().abs())
            assert ((got.double() - exact).abs() <= bound).all(), f"{rows} rows against the torch definition"
            assert not torch.equal(got, before[rows])
    state = {name: value.clone() for name, value in layer.state_dict().items()}
    other = aqlm.QuantizedLinear(fin, fout, g, 1, 1, 16, bias=True, device=DEV, dtype=torch.float16)
    other.load_state_dict(state)
    with torch.no_grad():
        assert all(torch.equal(other.state_dict()[name], value) for name, value in state.items())
        assert torch.equal(other(xs[32]), layer(xs[32]))


def test_the_switch_and_unsupported_shapes_take_the_torch_route(hk, monkeypatch):
    import aqlm.tuning as tuning

    def fail(*a, **kw):
        raise AssertionError("the kernel route ran")

    monkeypatch.setattr(hk, "kmeans_assign", fail)
    monkeypatch.setattr(hk, "kmeans_update", fail)
    gen = torch.Generator().manual_seed(2)
    weight = torch.randn((64, 128), generator=gen).to(DEV)
    # g = 32 and out_group_size 2 whatever the switch says; 2x8 g8 with the switch off
    tuning.init_aq_kmeans(weight, num_codebooks=1, out_group_size=1, in_group_size=32, codebook_size=128, max_iter=2, generator=gen)
    tuning.init_aq_kmeans(weight, num_codebooks=1, out_group_size=2, in_group_size=8, codebook_size=128, max_iter=2, generator=gen)
    tuning.fit_kmeans(weight.reshape(-1, 8), 64, max_iter=2, generator=gen)  # k = 64 is not a multiple of 128
    tuning.fit_kmeans(weight.reshape(-1, 8).double(), 128, max_iter=2, generator=gen)
    with pytest.raises(AssertionError, match="kernel route"):
        tuning.fit_kmeans(weight.reshape(-1, 8), 128, max_iter=2, generator=gen)
    monkeypatch.setattr(tuning, "KMEANS_KERNEL", False)
    centroids, indices, _ = tuning.fit_kmeans(weight.reshape(-1, 8), 128, max_iter=2, generator=gen)
    assert centroids.is_cuda and indices.dtype == torch.int64
    poisoned = weight.clone()
    poisoned[3, 3] = float("nan")
    for switch in (True, False):
        monkeypatch.setattr(tuning, "KMEANS_KERNEL", switch)
        with pytest.raises(ValueError, match="non-finite"):
            tuning.fit_kmeans(poisoned.reshape(-1, 8), 128, max_iter=2)
