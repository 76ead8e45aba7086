"""aqlm_hip_code_search_1x16 and the code update built on it, on the MI355X.  The oracle is a float64 brute force over all 65536
codewords, computed in chunks on the device, of the scores ``S(n, c) = |C_c|^2 - 2 <r_n, C_c>`` with ``r_n`` the fp32 quotient of the
definition (include/aqlm_hip.h).  The accuracy contract is held as stated there, with the documented epsilon (2^-17):
  * every group whose float64 margin between the best and the second best exceeds 2 E(n), E(n) = eps (|r_n|^2 + max |C_c|^2),
    must equal the float64 argmin exactly;
  * every other group (the near-tie class) must score within 2 E(n) of the minimum;
  * the near-tie class may hold at most 2 % of the groups -- a condition on eps, not a tolerance.
Cases use 2048 groups (out 64, in 32 g) unless stated; the seeded inputs and their oracle are computed once per configuration."""
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
ENTRIES = 65536
SIGMA = {8: 0.3, 16: 0.65}  # noise on the planted codeword: 30-60 % of the groups change code in float64 (asserted)


@pytest.fixture(scope="module")
def hk():
    from aqlm_amd.inference_kernels import hip_kernel

    return hip_kernel


def _unsigned(codes):
    return codes.to(torch.int64) % ENTRIES


def quotient(reference, scales):
    """r of the definition: widened to fp32, an IEEE division (taken on the host), as float64 [out, in]."""
    r = reference.detach().float().cpu()
    if scales is not None:
        r = r / scales.detach().float().cpu().reshape(-1, 1)
    return r.double().to(reference.device)


def oracle(r, codebook, chunk=512):
    """r [N, g] float64, codebook [65536, g] float64 -> (argmin, minimum, margin to the second best) in float64."""
    norms = codebook.square().sum(-1)
    best = torch.empty((r.shape[0],), dtype=torch.int64, device=r.device)
    low = torch.empty((r.shape[0],), dtype=torch.float64, device=r.device)
    margin = torch.empty_like(low)
    for a in range(0, r.shape[0], chunk):
        scores = norms[None] - 2 * (r[a:a + chunk] @ codebook.T)
        values, indices = scores.topk(2, dim=-1, largest=False, sorted=True)
        best[a:a + chunk], low[a:a + chunk], margin[a:a + chunk] = indices[:, 0], values[:, 0], values[:, 1] - values[:, 0]
    return best, low, margin


def tolerance(r, codebook, eps):
    return eps * (r.square().sum(-1) + codebook.square().sum(-1).max())


def hold_to_contract(got, r, codebook, eps, expect=None, what=""):
    """The three conditions of the module docstring for the codes ``got`` (unsigned, [N]) of the groups ``r``; ``expect``: a
    precomputed ``oracle(r, codebook)``.  Returns the share of the near-tie class."""
    best, low, margin = oracle(r, codebook) if expect is None else expect
    E = tolerance(r, codebook, eps)
    near = margin <= 2 * E
    share = float(near.double().mean())
    score = codebook.square().sum(-1)[got] - 2 * (r * codebook[got]).sum(-1)
    wrong = int(((got != best) & ~near).sum())
    excess = float(((score - low) / (2 * E)).max())
    print(f"{what}: near-tie class {100 * share:.3f} % of {r.shape[0]} groups, {wrong} separated groups differ from the float64 argmin, "
          f"{int((got != best).sum())} differ in all, worst (score - min) / 2E = {excess:.4f}")
    assert share <= 0.02, f"{what}: {100 * share:.2f} % of the groups lie within 2 E of a tie"
    assert wrong == 0, f"{what}: {wrong} groups with a float64 margin above 2 E differ from the float64 argmin"
    assert excess <= 1.0, f"{what}: a chosen code scores {excess:.3f} x 2 E above the minimum"
    return share


@functools.lru_cache(maxsize=None)
def case(g, dtype, ref_dtype, out=64, groups_per_row=32, seed=0):
    """Seeded inputs -- codebook N(0, 1) rounded to the storage dtype, r = C[random code] + sigma N(0, 1), scales in [0.5, 1.5] with
    every third one negative -- and their float64 oracle.  Nothing in the result is written by a test."""
    gen = torch.Generator().manual_seed(1000 * g + seed)
    codebook = torch.randn((ENTRIES, g), generator=gen).to(dtype)
    planted = torch.randint(0, ENTRIES, (out, groups_per_row), generator=gen)
    r = codebook[planted].float() + SIGMA[g] * torch.randn((out, groups_per_row, g), generator=gen)
    scales = torch.rand((out,), generator=gen) + 0.5
    scales[::3] *= -1
    scales = scales.to(dtype)
    reference = (r * scales.float()[:, None, None]).reshape(out, groups_per_row * g).to(ref_dtype)
    c = {"codebook": codebook.to(DEV), "scales": scales.to(DEV), "reference": reference.to(DEV), "planted": planted.to(DEV).flatten(),
         "g": g, "out": out, "in": groups_per_row * g}
    c["cb64"] = c["codebook"].double()
    c["r"] = quotient(c["reference"], c["scales"]).reshape(-1, g)
    c["oracle"] = oracle(c["r"], c["cb64"])
    return c


def search(hk, c, **kw):
    return _unsigned(hk.code_search_1x16(kw.pop("reference", c["reference"]), kw.pop("scales", c["scales"]), c["codebook"], c["g"], **kw))


# ---------------------------------------------------------------------------------------------------------------------------
# 1. parity
# ---------------------------------------------------------------------------------------------------------------------------
PARITY = [(8, torch.float16, torch.float32), (8, torch.bfloat16, torch.float32), (16, torch.float16, torch.float32),
          (16, torch.bfloat16, torch.float32), (8, torch.float16, torch.float16), (8, torch.bfloat16, torch.bfloat16)]


@pytest.mark.parametrize("g,dtype,ref_dtype", PARITY, ids=lambda v: str(v).replace("torch.", ""))
def test_codes_equal_the_float64_argmin_outside_the_near_tie_class(hk, g, dtype, ref_dtype):
    c = case(g, dtype, ref_dtype)
    changed = float((c["oracle"][0] != c["planted"]).double().mean())
    print(f"g {g}: {100 * changed:.1f} % of the groups change code in float64")
    assert 0.30 <= changed <= 0.60, "the inputs must not pass on an identity"
    got = search(hk, c)
    assert got.shape == (2048,) and int(got.min()) >= 0 and int(got.max()) < ENTRIES
    hold_to_contract(got, c["r"], c["cb64"], hk.CODE_SEARCH_EPS, c["oracle"], f"g {g} {dtype} codebook, {ref_dtype} reference")
    assert torch.equal(got, search(hk, c)), "a second call gives the same codes"


# ---------------------------------------------------------------------------------------------------------------------------
# 2. edges of the tiling
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("g", [8, 16])
@pytest.mark.parametrize("out,groups_per_row", [(1, 1), (3, 5), (67, 9)])
def test_layers_that_fill_no_tile(hk, g, out, groups_per_row):
    c = case(g, torch.float16, torch.float32, out=out, groups_per_row=groups_per_row, seed=out)
    got = search(hk, c)
    assert got.shape == (out * groups_per_row,)
    hold_to_contract(got, c["r"], c["cb64"], hk.CODE_SEARCH_EPS, c["oracle"], f"{out} x {groups_per_row} groups of {g}")


@pytest.mark.parametrize("g", [8, 16])
def test_group_id_lists_of_every_tile_remainder(hk, g):
    c = case(g, torch.float16, torch.float32)
    full = search(hk, c)
    gen = torch.Generator().manual_seed(g)
    for n in (1, 31, 32, 33, 63, 64, 65, 257):
        ids = torch.randperm(2048, generator=gen)[:n].to(DEV)
        got = search(hk, c, group_ids=ids)
        assert got.shape == (n,)
        expect = tuple(t[ids] for t in c["oracle"])
        hold_to_contract(got, c["r"][ids], c["cb64"], hk.CODE_SEARCH_EPS, expect, f"g {g}, {n} group ids")
        assert torch.equal(got, full[ids]), "a group's code does not depend on the call it is searched in"


# ---------------------------------------------------------------------------------------------------------------------------
# 3. ties and extremes
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("g,dtype", [(8, torch.float16), (16, torch.bfloat16)], ids=["g8-fp16", "g16-bf16"])
def test_equal_scores_give_the_smallest_index_and_the_ends_of_the_codebook_come_back(hk, g, dtype):
    c = case(g, dtype, torch.float32)
    codebook = c["codebook"].clone()
    codebook[40000] = codebook[123]
    gen = torch.Generator().manual_seed(3)
    rows = [codebook[123].float(), codebook[0].float(), codebook[ENTRIES - 1].float(), codebook[40000].float()]
    rows += [codebook[123].float() + 1e-3 * torch.randn((g,), generator=gen).to(DEV) for _ in range(28)]
    reference = torch.stack(rows).reshape(1, 32 * g).contiguous()
    got = hk.code_search_1x16(reference, None, codebook, g)
    assert got.dtype == torch.int16 and got.shape == (32,)
    assert int(got[1]) == 0 and int(got[2]) == -1, "codeword 65535 is stored as -1"
    want = torch.full((32,), 123, dtype=torch.int64, device=DEV)
    want[1], want[2] = 0, ENTRIES - 1
    assert torch.equal(_unsigned(got), want), _unsigned(got).tolist()


@pytest.mark.parametrize("g,dtype", [(8, torch.bfloat16), (16, torch.float16)], ids=["g8-bf16", "g16-fp16"])
def test_the_search_is_idempotent_on_dequantised_weights(hk, g, dtype):
    c = case(g, dtype, torch.float32)
    assert torch.unique(c["codebook"].float(), dim=0).shape[0] == ENTRIES, "a duplicate-free codebook"
    codes = torch.cat([c["planted"][:2046], torch.tensor([0, ENTRIES - 1], device=DEV)])
    weight = (c["codebook"][codes].float().reshape(64, 32, g) * c["scales"].float()[:, None, None]).reshape(64, 32 * g)
    assert torch.equal(search(hk, c, reference=weight), codes)
    assert torch.equal(search(hk, c, reference=weight.to(dtype)), codes), "the weights as the layer would hold them"


# ---------------------------------------------------------------------------------------------------------------------------
# 4. addressing
# ---------------------------------------------------------------------------------------------------------------------------
def test_group_ids_of_both_widths_in_any_order_and_ids_outside_the_layer(hk):
    c = case(8, torch.float16, torch.float32)
    full = search(hk, c)
    ids = torch.randperm(2048, generator=torch.Generator().manual_seed(9))[:300]
    ids = torch.cat([ids.sort(descending=True).values, ids[:20]]).to(DEV)  # descending, then repeats
    a = search(hk, c, group_ids=ids)
    b = search(hk, c, group_ids=ids.to(torch.int32))
    assert torch.equal(a, b) and torch.equal(a, full[ids])
    for width in (torch.int64, torch.int32):
        mixed = torch.tensor([5, -1, 2047, 2048, 0, 2**31 - 1, -(2**31), 77], dtype=width, device=DEV)
        out = torch.full((8,), 12345, dtype=torch.int16, device=DEV)
        back = hk.code_search_1x16(c["reference"], c["scales"], c["codebook"], 8, group_ids=mixed, codes_out=out)
        assert back is out
        inside = torch.tensor([0, 2, 4, 7], device=DEV)
        outside = torch.tensor([1, 3, 5, 6], device=DEV)
        assert torch.equal(out[outside], torch.full((4,), 12345, dtype=torch.int16, device=DEV)), "a slot of an id outside the layer is not written"
        assert torch.equal(_unsigned(out[inside]), full[mixed[inside].long()])
    huge = torch.tensor([2**40, -(2**40), 3], dtype=torch.int64, device=DEV)
    out = torch.full((3,), -7, dtype=torch.int16, device=DEV)
    hk.code_search_1x16(c["reference"], c["scales"], c["codebook"], 8, group_ids=huge, codes_out=out)
    assert out[:2].tolist() == [-7, -7] and int(_unsigned(out[2:])[0]) == int(full[3])


@pytest.mark.parametrize("ref_dtype", [torch.float32, torch.float16], ids=["fp32", "fp16"])
def test_a_column_slice_of_a_wider_tensor_and_null_scales(hk, ref_dtype):
    c = case(8, torch.float16, ref_dtype)
    wide = torch.full((64, 256 + 40), float("nan"), dtype=ref_dtype, device=DEV)
    wide[:, 24:24 + 256] = c["reference"]
    view = wide[:, 24:24 + 256]
    assert not view.is_contiguous() and view.stride(0) == 296
    assert torch.equal(search(hk, c, reference=view), search(hk, c))
    odd = wide[:, 3:3 + 256]  # groups that start at no 16-byte boundary
    odd.copy_(c["reference"])
    assert torch.equal(search(hk, c, reference=odd), search(hk, c))
    # a view with another column stride (here a transpose) is served too, by the kernel route of the API as well
    import aqlm.tuning as tuning

    turned = c["reference"].t().contiguous().t()
    assert turned.stride(1) != 1 and torch.equal(turned, c["reference"])
    assert torch.equal(search(hk, c, reference=turned), search(hk, c))
    prev = torch.zeros((64, 32, 1), dtype=torch.int16, device=DEV)
    books, scales = c["codebook"].reshape(1, ENTRIES, 1, 8), c["scales"].reshape(-1, 1, 1, 1)
    assert torch.equal(_unsigned(tuning.find_optimal_codes(turned, books, prev, scales)).flatten(), search(hk, c))
    ones = torch.ones((64,), dtype=torch.float16, device=DEV)
    a = hk.code_search_1x16(c["reference"], None, c["codebook"], 8)
    b = hk.code_search_1x16(c["reference"], ones, c["codebook"], 8)
    assert torch.equal(a, b), "scales NULL and scales of ones: identical bits"
    hold_to_contract(_unsigned(a), quotient(c["reference"], None).reshape(-1, 8), c["cb64"], hk.CODE_SEARCH_EPS, None, "no scales")


# ---------------------------------------------------------------------------------------------------------------------------
# 5. non-finite input
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("g,dtype", [(8, torch.float16), (16, torch.bfloat16)], ids=["g8-fp16", "g16-bf16"])
def test_non_finite_groups_return_and_keep_their_previous_codes(hk, g, dtype):
    import aqlm.tuning as tuning

    c = case(g, dtype, torch.float32)
    reference = c["reference"].clone()
    reference[5, 3 * g + 2] = float("nan")
    reference[9, 30 * g + g - 1] = float("-inf")
    reference[11, 7 * g] = 3.0e38  # finite, beyond the kernel's stated range (2^100): the update keeps the previous code
    reference[13, 2 * g + 1] = -1.0e27  # finite, far beyond fp16, inside the range: the scaled split serves it
    bad = torch.tensor([5 * 32 + 3, 9 * 32 + 30], device=DEV)
    raw = search(hk, c, reference=reference)
    torch.cuda.synchronize()
    assert int(raw.min()) >= 0 and int(raw.max()) < ENTRIES
    prev = torch.randint(-32768, 32768, (64, 32, 1), generator=torch.Generator().manual_seed(4)).to(torch.int16).to(DEV)
    new = tuning.find_optimal_codes(reference, c["codebook"].reshape(1, ENTRIES, 1, g), prev, c["scales"].reshape(-1, 1, 1, 1))
    assert new.dtype == torch.int16 and new.shape == prev.shape
    flat_new, flat_prev = new.flatten(), prev.flatten()
    assert torch.equal(flat_new[bad], flat_prev[bad]), "a group with a NaN or an Inf keeps its previous code"
    keep = torch.ones((2048,), dtype=torch.bool, device=DEV)
    keep[bad] = False
    keep[11 * 32 + 7] = False
    keep[13 * 32 + 2] = False
    got = _unsigned(flat_new)
    assert torch.equal(got[keep], search(hk, c)[keep]), "every other group is what the clean layer gives"
    hold_to_contract(got[keep], c["r"][keep], c["cb64"], hk.CODE_SEARCH_EPS, tuple(t[keep] for t in c["oracle"]), "beside non-finite groups")
    assert int(flat_new[11 * 32 + 7]) == int(flat_prev[11 * 32 + 7]), "a group beyond 2^100 keeps its previous code"
    assert 0 <= int(raw[11 * 32 + 7]) < ENTRIES
    # the group of magnitude 1e27: the scaled split keeps it in the operand format, its code scores within 2 E of the float64 minimum
    # (E grows with |r|^2: at this magnitude the best codewords are all within 2 E of one another, so the score is the check)
    big = torch.tensor([13 * 32 + 2], device=DEV)
    r_big = quotient(reference, c["scales"]).reshape(-1, g)[big]
    _, low, _ = oracle(r_big, c["cb64"])
    score = c["cb64"].square().sum(-1)[got[big]] - 2 * (r_big * c["cb64"][got[big]]).sum(-1)
    excess = float((score - low) / (2 * tolerance(r_big, c["cb64"], hk.CODE_SEARCH_EPS)))
    print(f"group of magnitude 1e27: (score - min) / 2E = {excess:.3e}, code {int(got[big])} (raw {int(raw[big])})")
    assert excess <= 1.0 and int(got[big]) == int(raw[big]) and int(got[big]) != int(_unsigned(flat_prev[big]))


# ---------------------------------------------------------------------------------------------------------------------------
# 6. the API on the device
# ---------------------------------------------------------------------------------------------------------------------------
def _separated(c, hk):
    """The parity inputs with every group near a tie (float64 margin <= 8 E) moved onto its best codeword: both routes must then
    agree code for code."""
    best, _, margin = c["oracle"]
    near = margin <= 8 * tolerance(c["r"], c["cb64"], hk.CODE_SEARCH_EPS)
    r = torch.where(near[:, None], c["cb64"][best], c["r"]).float().reshape(c["out"], -1, c["g"])
    return (r * c["scales"].float()[:, None, None]).reshape(c["out"], c["in"]).contiguous()


@pytest.mark.parametrize("g,dtype", [(8, torch.float16), (16, torch.bfloat16)], ids=["g8-fp16", "g16-bf16"])
def test_find_optimal_codes_equals_the_torch_route(hk, monkeypatch, g, dtype):
    import aqlm.tuning as tuning

    c = case(g, dtype, torch.float32)
    reference = _separated(c, hk)
    books, scales = c["codebook"].reshape(1, ENTRIES, 1, g), c["scales"].reshape(-1, 1, 1, 1)
    prev = torch.where(c["planted"] >= 32768, c["planted"] - ENTRIES, c["planted"]).to(torch.int16).reshape(64, 32, 1)
    calls = []
    real = hk.code_search_1x16
    monkeypatch.setattr(hk, "code_search_1x16", lambda *a, **k: (calls.append(k.get("group_ids")), real(*a, **k))[1])
    results = {}
    for name, options in (("full", {}), ("beam", {"beam_size": 4}), ("fraction", {"max_update_fraction": 0.25}),
                          ("trust", {"max_update_fraction": 0.25, "trust_ratio": 0.05})):
        monkeypatch.setattr(tuning, "CODE_SEARCH_KERNEL", True)
        calls.clear()
        got = tuning.find_optimal_codes(reference, books, prev, scales, **options)
        assert len(calls) == 1, "the kernel took the search"
        assert (calls[0] is None) == ("max_update_fraction" not in options)
        assert calls[0] is None or calls[0].numel() == 512, "the kernel is called with the selected groups only"
        again = tuning.find_optimal_codes(reference, books, prev, scales, **options)
        assert torch.equal(got, again), "two calls, identical bits"
        monkeypatch.setattr(tuning, "CODE_SEARCH_KERNEL", False)
        calls.clear()
        want = tuning.find_optimal_codes(reference, books, prev, scales, **options)
        assert not calls, "the switch sends the call through the torch route"
        assert got.dtype == torch.int16 and got.shape == prev.shape
        assert torch.equal(got, want), f"{name}: {int((got != want).sum())} codes differ from the torch route"
        results[name] = int((got != prev).sum())
    print("groups changed:", results)
    assert results["full"] == results["beam"] > results["fraction"] > results["trust"] > 1
    assert results["fraction"] <= 512


def test_update_codes_rebuilds_every_derived_copy(hk, monkeypatch):
    """A 1x16 layer that was prepacked (its canonical codes dropped), has served forwards, trained a step and built the inverted
    index of its codes: after ``update_codes_`` the codes are back and new, a 1-row forward, a 32-row forward and a training step's
    gradients carry the bits of a freshly built layer that holds the new codes, they agree with the torch definition on the new
    codes, and the index is a new object."""
    import aqlm
    import aqlm.tuning as tuning
    import aqlm_amd.inference as inf
    from aqlm_amd.checkpoint import prepack_model
    from aqlm_amd.utils import _dequantize_weight, unpack_int_data

    monkeypatch.setattr(inf, "PREPACK_MIN_CODES", 100_000)
    fin, fout, dtype, g = 2048, 512, torch.float16, 8
    gen = torch.Generator().manual_seed(21)

    def build(codes, codebooks, scales, bias, pack):
        m = aqlm.QuantizedLinear(fin, fout, g, 1, 1, 16, bias=True, device=DEV, dtype=dtype)
        with torch.no_grad():
            m.codes.copy_(codes); m.codebooks.copy_(codebooks); m.scales.copy_(scales); m.bias.copy_(bias)  # noqa: E702
        if pack:
            assert prepack_model(torch.nn.ModuleDict({"l": m}))["prepacked_layers"] == 1 and m._codes_dropped
        return m

    codes = torch.randint(-32768, 32768, (fout, fin // g, 1), generator=gen).to(torch.int16)
    codebooks = torch.randn((1, ENTRIES, 1, g), generator=gen)
    scales, bias = torch.rand((fout, 1, 1, 1), generator=gen) + 0.5, torch.randn((fout,), generator=gen) * 0.1
    layer = build(codes, codebooks, scales, bias, pack=True)
    xs = {rows: torch.randn((rows, fin), generator=gen).to(dtype).to(DEV) for rows in (1, 32)}
    wy = torch.randn((32, fout), generator=gen).to(dtype).to(DEV)
    with torch.no_grad():
        before = layer(xs[1])
    assert layer._codes_dropped

    def target(seed):
        noise = torch.randn((fout, fin), generator=torch.Generator().manual_seed(seed)).to(DEV)
        with torch.no_grad():
            w = _dequantize_weight(unpack_int_data(layer._canonical_codes(), 16), layer.codebooks.float(), layer.scales.float())
        return w + 0.3 * layer.scales.float().reshape(-1, 1) * noise

    def check(tag):
        fresh = build(layer.codes.detach().cpu(), layer.codebooks.detach().cpu(), layer.scales.detach().cpu(), layer.bias.detach().cpu(),
                      pack=False)
        with torch.no_grad():
            w64 = _dequantize_weight(unpack_int_data(layer.codes, 16), layer.codebooks.double(), layer.scales.double())
            for rows, x in xs.items():
                got, want = layer(x), fresh(x)
                exact = F.linear(x.double(), w64, layer.bias.double())
                # one rounding of the output to fp16 (2^-11 |y|) after fp32 sums of 2048 exact products (at most 2048 * 2^-24 of the
                # summed magnitudes); a single stale code moves y by far more
                bound = 2.0 ** -10 * exact.abs() + 2.0 ** -13 * F.linear(x.double().abs(), w64.abs(), layer.bias.double().abs())
                assert ((got.double() - exact).abs() <= bound).all(), f"{tag}: {rows} rows against the torch definition"
                assert ((want.double() - exact).abs() <= bound).all()
        return fresh

    # (a) dropped codes come back first, the forward follows the new codes
    reference = target(1)
    old = layer._canonical_codes().clone()
    changed = tuning.update_codes_(layer, reference)
    assert not layer._codes_dropped and tuple(layer.codes.shape) == (fout, fin // g, 1)
    expected = tuning.find_optimal_codes(reference, layer.codebooks.detach(), old, layer.scales.detach())
    assert torch.equal(layer.codes, expected)
    share = int(changed) / (fout * fin // g)
    assert changed.is_cuda and changed.dim() == 0 and int(changed) == int((expected != old).sum()) and 0.3 <= share <= 0.6, share
    check("after the first update")
    with torch.no_grad():
        assert not torch.equal(layer(xs[1]), before)

    # (b) a training step builds the index; the next update replaces it and the gradients follow the new codes
    params = tuning.make_trainable(torch.nn.ModuleDict({"l": layer}))
    assert len(params) == 2
    (layer(xs[32]) * wy).sum().backward()
    index = layer.codebook_grad_index()
    assert layer._grad_index is not None and layer.codebook_grad_index() is index
    param, version = layer.codes, layer.codes._version
    changed = tuning.update_codes_(layer, target(2))
    assert layer.codes is param and layer.codes._version > version and int(changed) > 0
    fresh = check("after the second update")
    assert layer.codebook_grad_index() is not index, "the inverted index follows the new codes"
    tuning.make_trainable(torch.nn.ModuleDict({"l": fresh}))
    for m in (layer, fresh):
        m.codebooks.grad = m.scales.grad = None
        (m(xs[32]) * wy).sum().backward()
    assert torch.equal(layer.codebooks.grad, fresh.codebooks.grad) and torch.equal(layer.scales.grad, fresh.scales.grad)
    # the torch definition in float64: each term carries the fp16 rounding of dW (2^-11), the output one more; normwise 2^-9 is
    # four times that
    cb64 = layer.codebooks.detach().double().requires_grad_(True)
    s64 = layer.scales.detach().double().requires_grad_(True)
    y = F.linear(xs[32].double(), _dequantize_weight(_unsigned(layer.codes.detach()), cb64, s64), layer.bias.detach().double())
    (y * wy.double()).sum().backward()
    for got, exact, what in ((layer.codebooks.grad, cb64.grad, "codebook"), (layer.scales.grad, s64.grad, "scale")):
        rel = float((got.double() - exact).norm() / exact.norm())
        print(f"{what} gradient after the update: relative error {rel:.2e}")
        assert rel <= 2.0 ** -9, f"{what} gradient: {rel}"
