"""aqlm_hip_code_search_kx8 and the code update built on it, on the MI355X.  The entry is held to its own arithmetic BIT FOR BIT: the
oracle is tests/kx8_search_model.py (numpy, float32, one IEEE operation per product and per sum in the order include/aqlm_hip.h
states), run on the host on exactly the values the kernel reads.  Codes must be equal on every group and the returned scores must
carry the same bits -- a fused multiply-add or another summation order shows there.  Where the kernel route is compared with the
torch route (another arithmetic), the inputs lie on a dyadic grid on which every fp32 sum is exact, and groups with an exact tie
among the best keep + 1 scores of some step are left out (at most 15 % of the groups: a condition on the inputs).
Cases use 2048 groups (out 64, 32 groups per row) unless stated; seeded inputs and their model results are computed once per
configuration and never written."""
import functools
import itertools
import json
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import kx8_search_model as model

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TIE_CAP = 0.15


@pytest.fixture(scope="module")
def hk():
    from aqlm_amd.inference_kernels import hip_kernel

    return hip_kernel


def stored(codes):
    """unsigned codes -> the int8 the checkpoint stores"""
    codes = torch.as_tensor(codes).to(torch.int64)
    return torch.where(codes >= 128, codes - 256, codes).to(torch.int8)


def unsigned(codes):
    return codes.to(torch.int64) % 256


def bits(x):
    return torch.as_tensor(x).contiguous().view(torch.int32)


@functools.lru_cache(maxsize=None)
def case(K, g, dtype, ref_dtype, out=64, groups_per_row=32, seed=0):
    """Seeded Gaussian inputs, off any grid: codebooks N(0, 1) rounded to the storage dtype, r = the sum of planted codewords + 0.35
    N(0, 1), the previous codes = the planted ones with one code of every second group drawn anew, scales in [0.5, 1.5] with every
    third one negative.  Host tensors (what the model reads, widened exactly) and their device copies."""
    gen = torch.Generator().manual_seed(10000 * K + 100 * g + seed)
    books = torch.randn((K, 256, g), generator=gen).to(dtype)
    N = out * groups_per_row
    planted = torch.randint(0, 256, (N, K), generator=gen)
    r = sum(books[c][planted[:, c]].float() for c in range(K)) + 0.35 * torch.randn((N, g), generator=gen)
    prev = planted.clone()
    moved = torch.nonzero(torch.rand((N,), generator=gen) < 0.5).flatten()
    prev[moved, torch.randint(0, K, (moved.numel(),), generator=gen)] = torch.randint(0, 256, (moved.numel(),), generator=gen)
    scales = torch.rand((out,), generator=gen) + 0.5
    scales[::3] *= -1
    scales = scales.to(dtype)
    reference = (r.reshape(out, groups_per_row, g) * scales.float()[:, None, None]).reshape(out, groups_per_row * g).to(ref_dtype)
    return {"K": K, "g": g, "out": out, "in": groups_per_row * g, "N": N, "books": books, "scales": scales, "reference": reference,
            "prev": prev, "d_books": books.to(DEV), "d_scales": scales.to(DEV), "d_reference": reference.to(DEV), "d_prev": stored(prev).to(DEV)}


def _np(t):
    return t.float().numpy()


@functools.lru_cache(maxsize=None)
def expected(K, g, dtype, ref_dtype, beam, order=None, out=64, groups_per_row=32, seed=0, scaled=True):
    c = case(K, g, dtype, ref_dtype, out, groups_per_row, seed)
    return model.search(_np(c["reference"]), _np(c["scales"]) if scaled else None, _np(c["books"]), c["prev"].numpy(), g, beam,
                        None if order is None else list(order))


def run(hk, c, beam, **kw):
    codes, scores = hk.code_search_kx8(kw.pop("reference", c["d_reference"]), kw.pop("scales", c["d_scales"]), c["d_books"],
                                       kw.pop("prev", c["d_prev"]), c["g"], beam, return_scores=True, **kw)
    return codes, scores


def hold_to_model(got, want, what):
    codes, scores = got
    want_codes, want_scores, _ = want
    assert codes.dtype == torch.int8 and scores.dtype == torch.float32
    differ = int((unsigned(codes).cpu() != torch.from_numpy(want_codes)).any(-1).sum())
    off = int((bits(scores.cpu()) != bits(torch.from_numpy(want_scores))).sum())
    print(f"{what}: {differ} of {codes.shape[0]} groups differ from the model, {off} scores differ in their bits")
    assert differ == 0, f"{what}: {differ} groups differ from the model"
    assert off == 0, f"{what}: {off} scores are not the model's bits"


# ---------------------------------------------------------------------------------------------------------------------------
# 1. bit for bit against the model
# ---------------------------------------------------------------------------------------------------------------------------
SCHEMES = [(1, 8, 1), (1, 8, 4), (2, 8, 1), (2, 8, 8), (3, 8, 16), (4, 16, 4), (8, 32, 8), (2, 16, 3)]


@pytest.mark.parametrize("wide_reference", [True, False], ids=["ref-fp32", "ref-16bit"])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("K,g,beam", SCHEMES)
def test_codes_and_scores_equal_the_model_bit_for_bit(hk, K, g, beam, dtype, wide_reference):
    ref_dtype = torch.float32 if wide_reference else dtype
    c = case(K, g, dtype, ref_dtype)
    want = expected(K, g, dtype, ref_dtype, beam)
    changed = float((want[0] != c["prev"].numpy()).any(-1).mean())
    print(f"{K}x8 g{g} beam {beam}: {100 * changed:.1f} % of the groups change code")
    assert changed >= 0.30, "the inputs must not pass on an identity"
    got = run(hk, c, beam)
    assert got[0].shape == (2048, K) and got[1].shape == (2048,)
    hold_to_model(got, want, f"{K}x8 g{g} beam {beam}, {dtype} codebooks, {ref_dtype} reference")
    again = run(hk, c, beam)
    assert torch.equal(got[0], again[0]) and torch.equal(bits(got[1]), bits(again[1])), "two calls give identical bits"
    assert torch.equal(hk.code_search_kx8(c["d_reference"], c["d_scales"], c["d_books"], c["d_prev"], g, beam), got[0]), "without scores"


# ---------------------------------------------------------------------------------------------------------------------------
# 2. the reference's codes through the API on the device
# ---------------------------------------------------------------------------------------------------------------------------
def _golden_case(name_of_case):
    from aqlm_amd.utils import pack_int_data

    z = np.load(os.path.join(ROOT, "tests", "golden", "code_update_golden.npz"))
    meta = json.loads(str(z["meta"]))
    info = meta["cases"][name_of_case]
    name = info["layer"]
    out_features, in_features, K, nbits, ogs, g = meta["layers"][name]["shape"]
    books = torch.from_numpy(z[f"{name}_codebook_k"].astype(np.float32) * meta["grid"])
    target = torch.from_numpy(z[f"{name}_reference_k"].astype(np.float32) * meta["grid"])
    scales = torch.from_numpy(2.0 ** z[f"{name}_scale_exp"].astype(np.float32)).reshape(-1, 1, 1, 1)
    prev = pack_int_data(torch.from_numpy(z[f"{name}_prev_codes"].astype(np.int64)), nbits)
    want = pack_int_data(torch.from_numpy(z[f"{name_of_case}_expected"].astype(np.int64)), nbits)
    options = {k: v for k, v in info["options"].items() if k not in ("admitted", "changed_share")}
    return target, books, prev, scales, options, want


def _spy(hk, monkeypatch):
    calls = []
    real = hk.code_search_kx8
    monkeypatch.setattr(hk, "code_search_kx8", lambda *a, **k: (calls.append(k.get("group_ids")), real(*a, **k))[1])
    return calls


@pytest.mark.parametrize("name", ["d", "e", "f"])
def test_golden_cases_through_find_optimal_codes_on_the_device(hk, monkeypatch, name):
    import aqlm.tuning as tuning

    target, books, prev, scales, options, want = _golden_case(name)
    assert books.half().float().equal(books) and scales.half().float().equal(scales), "the fixture's values are exact in fp16"
    calls = _spy(hk, monkeypatch)
    got = tuning.find_optimal_codes(target.to(DEV), books.half().to(DEV), prev.to(DEV), scales.half().to(DEV), **options)
    assert len(calls) == 1 and calls[0] is None, "the kernel took the search, for every group"
    assert got.dtype == torch.int8 and torch.equal(got.cpu(), want), f"{int((got.cpu() != want).any(-1).sum())} groups differ"


# ---------------------------------------------------------------------------------------------------------------------------
# 3. dim_order
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", list(itertools.permutations(range(3))), ids=lambda o: "".join(map(str, o)))
def test_every_order_of_three_codebooks(hk, order):
    c = case(3, 8, torch.float16, torch.float32, out=16, groups_per_row=32)
    want = expected(3, 8, torch.float16, torch.float32, 4, order, out=16, groups_per_row=32)
    hold_to_model(run(hk, c, 4, dim_order=list(order)), want, f"3x8 g8 beam 4 in the order {order}")


def test_an_order_of_eight_codebooks(hk):
    order = (5, 2, 7, 0, 3, 6, 1, 4)
    c = case(8, 32, torch.bfloat16, torch.float32, out=16, groups_per_row=16)
    want = expected(8, 32, torch.bfloat16, torch.float32, 3, order, out=16, groups_per_row=16)
    hold_to_model(run(hk, c, 3, dim_order=list(order)), want, f"8x8 g32 beam 3 in the order {order}")
    natural = expected(8, 32, torch.bfloat16, torch.float32, 3, None, out=16, groups_per_row=16)
    assert (natural[0] != want[0]).any(), "the order matters on these inputs"


# ---------------------------------------------------------------------------------------------------------------------------
# 4. edges of the work distribution
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,g,beam", [(2, 8, 8), (4, 16, 4)])
@pytest.mark.parametrize("out,groups_per_row", [(1, 1), (3, 5), (67, 9)])
def test_layers_that_fill_no_tile(hk, K, g, beam, out, groups_per_row):
    c = case(K, g, torch.float16, torch.float32, out=out, groups_per_row=groups_per_row, seed=out)
    want = expected(K, g, torch.float16, torch.float32, beam, out=out, groups_per_row=groups_per_row, seed=out)
    got = run(hk, c, beam)
    assert got[0].shape == (out * groups_per_row, K)
    hold_to_model(got, want, f"{out} x {groups_per_row} groups, {K}x8 g{g}")


def test_group_ids_of_both_widths_any_order_repeats_and_every_list_length(hk):
    c = case(2, 8, torch.float16, torch.float32)
    want = expected(2, 8, torch.float16, torch.float32, 8)
    full = run(hk, c, 8)
    gen = torch.Generator().manual_seed(5)
    for n in (1, 2, 3, 4, 5, 7, 8, 63, 64, 65, 255, 257):
        ids = torch.randperm(2048, generator=gen)[:n]
        ids = torch.cat([ids, ids[: n // 3]])  # shuffled, then repeats
        for width in (torch.int64, torch.int32):
            got = run(hk, c, 8, group_ids=ids.to(width).to(DEV))
            assert got[0].shape == (ids.numel(), 2)
            hold_to_model(got, tuple(t[ids.numpy()] for t in want), f"{ids.numel()} group ids, {width}")
            assert torch.equal(got[0], full[0][ids.to(DEV)]), "a group's codes do not depend on the call it is searched in"


def test_ids_outside_the_layer_leave_their_slot_untouched(hk):
    c = case(2, 8, torch.float16, torch.float32)
    full = run(hk, c, 8)[0]
    for width in (torch.int64, torch.int32):
        mixed = torch.tensor([5, -1, 2047, 2048, 0, 2**31 - 1, -(2**31), 77], dtype=width, device=DEV)
        out = torch.full((8, 2), 93, dtype=torch.int8, device=DEV)
        back = hk.code_search_kx8(c["d_reference"], c["d_scales"], c["d_books"], c["d_prev"], 8, 8, group_ids=mixed, codes_out=out)
        assert back is out
        inside, outside = torch.tensor([0, 2, 4, 7], device=DEV), torch.tensor([1, 3, 5, 6], device=DEV)
        assert torch.equal(out[outside], torch.full((4, 2), 93, dtype=torch.int8, device=DEV)), "a slot of an id outside the layer is not written"
        assert torch.equal(out[inside], full[mixed[inside].long()])
    huge = torch.tensor([2**40, -(2**40), 3], dtype=torch.int64, device=DEV)
    out = torch.full((3, 2), -7, dtype=torch.int8, device=DEV)
    hk.code_search_kx8(c["d_reference"], c["d_scales"], c["d_books"], c["d_prev"], 8, 8, group_ids=huge, codes_out=out)
    assert out[:2].flatten().tolist() == [-7] * 4 and torch.equal(out[2], full[3])


# ---------------------------------------------------------------------------------------------------------------------------
# 5. the tie rule
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
def test_equal_scores_go_to_the_smaller_flat_index(hk, dtype):
    """Codebook 1 holds the same row at 7 and at 200.  Searched last, the two candidates tie on the one position: 7.  Searched first
    with two hypotheses kept, they become positions 0 (code 7) and 1 (code 200) with identical residues, so on the last step every
    candidate ties across the two positions: the lower position, whose codes hold 7.  Targets on rows 0 and 255 bring both ends of a
    codebook back."""
    c = case(2, 8, dtype, torch.float32)
    books = c["books"].clone()
    books[1, 200] = books[1, 7]
    first = torch.tensor([3, 0, 255, 31] * 8)
    second = torch.tensor([7, 200, 7, 200, 0, 255, 0, 255] * 4)
    reference = (books[0][first].float() + books[1][second].float()).reshape(1, 32 * 8).contiguous()
    wrong = torch.full((32,), 9)
    # codebook 1 last, from previous codes that are right there; codebook 1 first, from previous codes that are right in codebook 0
    for prev, order in ((torch.stack([wrong, second], dim=1), None), (torch.stack([first, wrong], dim=1), [1, 0])):
        for beam in (1, 2, 16):
            want = model.search(reference.numpy(), None, _np(books), prev.numpy(), 8, beam, order)
            got = hk.code_search_kx8(reference.to(DEV), None, books.to(DEV), stored(prev).to(DEV), 8, beam, dim_order=order, return_scores=True)
            hold_to_model(got, want, f"duplicated rows, beam {beam}, order {order}")
            codes = unsigned(got[0]).cpu()
            assert torch.equal(codes[:, 0], first), codes[:, 0].tolist()
            assert torch.equal(codes[:, 1], torch.where(second == 200, torch.tensor(7), second)), codes[:, 1].tolist()
            assert set(got[0].cpu().flatten().tolist()) >= {0, -1}, "codes 0 and 255 (stored as -1) both come back"


def test_a_codebook_of_equal_rows_ties_every_candidate_of_a_position(hk):
    """Every row of codebook 1 is the same: on its step all 256 candidates of a position tie, far more keys reach the bound than a
    wave has lanes, and the best of them are the smallest flat indices (so a kept hypothesis holds one of the codes 0 .. beam - 1)."""
    c = case(3, 8, torch.float16, torch.float32, out=8, groups_per_row=16)
    books = c["books"].clone()
    books[1, :] = books[1, 0]
    for beam, order in ((16, None), (5, [1, 2, 0]), (8, [0, 2, 1])):
        want = model.search(_np(c["reference"]), _np(c["scales"]), _np(books), c["prev"].numpy(), 8, beam, order)
        assert want[2].all(), "every group has exact ties"
        got = hk.code_search_kx8(c["d_reference"], c["d_scales"], books.to(DEV), c["d_prev"], 8, beam, dim_order=order, return_scores=True)
        hold_to_model(got, want, f"equal rows, beam {beam}, order {order}")
        assert int(unsigned(got[0])[:, 1].max()) < beam, "one of the smallest codes of the tied codebook: the hypotheses a step keeps"


# ---------------------------------------------------------------------------------------------------------------------------
# 6. addressing
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wide_reference", [True, False], ids=["ref-fp32", "ref-fp16"])
def test_a_column_slice_of_a_wider_tensor_and_null_scales(hk, wide_reference):
    ref_dtype = torch.float32 if wide_reference else torch.float16
    c = case(2, 8, torch.float16, ref_dtype)
    base = run(hk, c, 8)
    wide = torch.full((64, 256 + 40), float("nan"), dtype=ref_dtype, device=DEV)
    wide[:, 24:24 + 256] = c["d_reference"]
    view = wide[:, 24:24 + 256]
    assert not view.is_contiguous() and view.stride(0) == 296
    got = run(hk, c, 8, reference=view)
    assert torch.equal(got[0], base[0]) and torch.equal(bits(got[1]), bits(base[1]))
    odd = wide[:, 3:3 + 256]  # groups that start at no 16-byte boundary
    odd.copy_(c["d_reference"])
    got = run(hk, c, 8, reference=odd)
    assert torch.equal(got[0], base[0]) and torch.equal(bits(got[1]), bits(base[1]))
    turned = c["d_reference"].t().contiguous().t()  # another column stride: copied first
    assert turned.stride(1) != 1
    assert torch.equal(run(hk, c, 8, reference=turned)[0], base[0])
    ones = torch.ones((64,), dtype=torch.float16, device=DEV)
    a, b = run(hk, c, 8, scales=None), run(hk, c, 8, scales=ones)
    assert torch.equal(a[0], b[0]) and torch.equal(bits(a[1]), bits(b[1])), "scales NULL and scales of ones: identical bits"
    hold_to_model(a, expected(2, 8, torch.float16, ref_dtype, 8, scaled=False), "no scales")


# ---------------------------------------------------------------------------------------------------------------------------
# 7. non-finite input
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,g,beam,dtype", [(2, 8, 8, torch.float16), (4, 16, 4, torch.bfloat16)], ids=["2x8g8-fp16", "4x8g16-bf16"])
def test_non_finite_groups_return_and_keep_their_previous_codes(hk, K, g, beam, dtype):
    import aqlm.tuning as tuning

    c = case(K, g, dtype, torch.float32)
    reference = c["d_reference"].clone()
    reference[5, 3 * g + 2] = float("nan")
    reference[9, 30 * g + g - 1] = float("-inf")
    reference[11, 7 * g] = 3.0e38
    reference[13, 2 * g + 1] = -2.0 ** 61  # finite, beyond the kernel's stated range (2^60)
    bad = torch.tensor([5 * 32 + 3, 9 * 32 + 30, 11 * 32 + 7, 13 * 32 + 2], device=DEV)
    clean = run(hk, c, beam)
    raw = run(hk, c, beam, reference=reference)
    torch.cuda.synchronize()
    assert raw[0].shape == (2048, K) and raw[0].dtype == torch.int8  # (any int8 is a code in 0 .. 255)
    keep = torch.ones((2048,), dtype=torch.bool, device=DEV)
    keep[bad] = False
    assert torch.equal(raw[0][keep], clean[0][keep]) and torch.equal(bits(raw[1][keep]), bits(clean[1][keep])), \
        "the neighbours of a non-finite group carry the bits of a run without it"
    books, scales = c["d_books"].reshape(K, 256, 1, g), c["d_scales"].reshape(-1, 1, 1, 1)
    prev = c["d_prev"].reshape(64, 32, K)
    new = tuning.find_optimal_codes(reference, books, prev, scales, beam_size=beam).reshape(2048, K)
    assert new.dtype == torch.int8
    assert torch.equal(new[bad], c["d_prev"][bad]), "a group with a NaN, an Inf or an element of 2^60 or more keeps its previous codes"
    assert torch.equal(new[keep], clean[0][keep]), "every other group is what the clean layer gives"


# ---------------------------------------------------------------------------------------------------------------------------
# 8. the API on the device against the torch route
# ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def dyadic(K, g, beam):
    c = model.dyadic_case(K, g)
    codes, _, tied = model.search(c["reference"], c["scales"], c["codebooks"], c["prev"], g, beam)
    return c, codes, tied


def _dyadic_tensors(c):
    K, g = c["K"], c["g"]
    books = torch.from_numpy(c["codebooks"]).reshape(K, 256, 1, g)
    scales = torch.from_numpy(c["scales"]).reshape(-1, 1, 1, 1)
    assert books.half().float().equal(books) and scales.half().float().equal(scales)
    prev = stored(torch.from_numpy(c["prev"])).reshape(c["out"], -1, K)
    return torch.from_numpy(c["reference"]).to(DEV), books.half().to(DEV), prev.to(DEV), scales.half().to(DEV)


@pytest.mark.parametrize("K,g,beam", [(2, 8, 8), (8, 32, 4)])
def test_find_optimal_codes_equals_the_torch_route(hk, monkeypatch, K, g, beam):
    import aqlm.tuning as tuning
    from aqlm_amd.utils import _dequantize_weight

    c, model_codes, tied = dyadic(K, g, beam)
    share = float(tied.mean())
    print(f"{K}x8 g{g} beam {beam}: {100 * share:.2f} % of the groups have an exact tie")
    assert share <= TIE_CAP, "a condition on the inputs"
    reference, books, prev, scales = _dyadic_tensors(c)
    untied = torch.from_numpy(~tied).to(DEV)
    calls = _spy(hk, monkeypatch)
    # the selection: the tenth of the groups furthest from the target, in that order (float64 on the grid: exact)
    weight = _dequantize_weight(unsigned(prev), books.double(), scales.double())
    distance = (reference.double() - weight).reshape(64, 32, g).square().sum(-1).flatten()
    count = math.ceil(0.1 * 2048)
    ranked = distance.argsort(descending=True, stable=True)
    threshold = distance[ranked[count - 1]]

    def both(**options):
        monkeypatch.setattr(tuning, "CODE_SEARCH_KERNEL", True)
        calls.clear()
        got = tuning.find_optimal_codes(reference, books, prev, scales, beam_size=beam, **options)
        assert len(calls) == 1, "the kernel took the search"
        ids = calls[0]
        assert torch.equal(got, tuning.find_optimal_codes(reference, books, prev, scales, beam_size=beam, **options)), "two calls, identical bits"
        monkeypatch.setattr(tuning, "CODE_SEARCH_KERNEL", False)
        calls.clear()
        want = tuning.find_optimal_codes(reference, books, prev, scales, beam_size=beam, **options)
        assert not calls, "the switch sends the call through the torch route"
        assert got.dtype == torch.int8 and got.shape == prev.shape
        differ = (got != want).any(-1).flatten() & untied
        assert not differ.any(), f"{options}: {int(differ.sum())} groups without a tie differ from the torch route"
        return got.reshape(2048, K), ids

    full, ids = both()
    assert ids is None
    assert torch.equal(unsigned(full).cpu()[~tied], torch.from_numpy(model_codes)[~tied]) and torch.equal(unsigned(full).cpu(), torch.from_numpy(model_codes))
    part, ids = both(max_update_fraction=0.1)
    assert ids is not None and ids.numel() == count and ids.unique().numel() == count, "the kernel is called with the selected groups only"
    assert bool((distance[ids] >= threshold).all()), "... which are the groups furthest from the target"
    changed = (part != prev.reshape(2048, K)).any(-1)
    assert 0 < int(changed.sum()) <= count and torch.equal(part[ids], full[ids])
    rest = torch.ones((2048,), dtype=torch.bool, device=DEV)
    rest[ids] = False
    assert not changed[rest].any()
    # a trust ratio midway between two cumulative norms of the selected changes, ahead of the first selected group with a tie (so
    # that both routes add up the same changes)
    tied_selected = torch.nonzero(~untied[ids]).flatten()
    horizon = int(tied_selected[0]) if tied_selected.numel() else count
    middle = (min(horizon, count) - 2) // 2
    assert middle >= 1 and middle + 1 < horizon
    new_weight = _dequantize_weight(unsigned(part).reshape(64, 32, K), books.double(), scales.double())
    change = (new_weight - weight).reshape(64, 32, g).square().sum(-1).flatten()[ids]
    cumulative = change.cumsum(0).sqrt()
    assert float(cumulative[middle + 1]) > float(cumulative[middle]), "a threshold strictly between two cumulative norms"
    ratio = float((cumulative[middle] + cumulative[middle + 1]) / 2 / weight.norm())
    trusted, ids_again = both(max_update_fraction=0.1, trust_ratio=ratio)
    assert torch.equal(ids_again, ids)
    admitted = ids[: middle + 2]  # (the change that crosses the threshold is the last one admitted)
    assert torch.equal(trusted[admitted], part[admitted]), "the admitted changes"
    beyond = torch.ones((2048,), dtype=torch.bool, device=DEV)
    beyond[admitted] = False
    assert torch.equal(trusted[beyond], prev.reshape(2048, K)[beyond]), "everything after them keeps its codes"


def test_beam_17_and_out_group_size_2_take_the_torch_route(hk, monkeypatch):
    import aqlm.tuning as tuning

    calls = _spy(hk, monkeypatch)
    c = model.dyadic_case(2, 8)
    want, _, tied = model.search(c["reference"], c["scales"], c["codebooks"], c["prev"], 8, 17)
    assert float(tied.mean()) <= TIE_CAP
    reference, books, prev, scales = _dyadic_tensors(c)
    got = tuning.find_optimal_codes(reference, books, prev, scales, beam_size=17)
    assert not calls, "beam_size 17 is outside the kernel"
    assert torch.equal(unsigned(got).reshape(2048, 2).cpu()[~tied], torch.from_numpy(want)[~tied])
    target, books, prev, scales, options, expected_codes = _golden_case("g")
    assert books.shape[2] == 2
    got = tuning.find_optimal_codes(target.to(DEV), books.half().to(DEV), prev.to(DEV), scales.half().to(DEV), **options)
    assert not calls, "out_group_size 2 is outside the kernel"
    assert torch.equal(got.cpu(), expected_codes)


def test_update_codes_then_a_forward_call(hk, monkeypatch):
    """A 2x8 g8 layer on the device: ``update_codes_`` runs the kernel, the count it returns is the model's, and the next forward
    calls follow the new codes -- they agree with ``F.linear`` on the weight dequantised from them within the bound the 1x16 test
    of this kind uses."""
    import aqlm
    import aqlm.tuning as tuning
    from aqlm_amd.utils import _dequantize_weight

    fin, fout, dtype, g, K = 2048, 64, torch.float16, 8, 2
    c = case(K, g, dtype, torch.float32, out=fout, groups_per_row=fin // g, seed=3)
    layer = aqlm.QuantizedLinear(fin, fout, g, 1, K, 8, bias=True, device=DEV, dtype=dtype)
    gen = torch.Generator().manual_seed(17)
    with torch.no_grad():
        layer.codes.copy_(c["d_prev"].reshape(fout, fin // g, K))
        layer.codebooks.copy_(c["d_books"].reshape(K, 256, 1, g))
        layer.scales.copy_(c["d_scales"].reshape(-1, 1, 1, 1))
        layer.bias.copy_(torch.randn((fout,), generator=gen) * 0.1)
    xs = {rows: torch.randn((rows, fin), generator=gen).to(dtype).to(DEV) for rows in (1, 32)}
    with torch.no_grad():
        before = layer(xs[1])
    calls = _spy(hk, monkeypatch)
    want = expected(K, g, dtype, torch.float32, 4, out=fout, groups_per_row=fin // g, seed=3)
    param, version = layer.codes, layer.codes._version
    changed = tuning.update_codes_(layer, c["d_reference"], beam_size=4)
    assert len(calls) == 1 and layer.codes is param and layer.codes._version > version
    assert torch.equal(unsigned(layer.codes).reshape(-1, K).cpu(), torch.from_numpy(want[0]))
    count = int((want[0] != c["prev"].numpy()).any(-1).sum())
    assert changed.is_cuda and changed.dim() == 0 and int(changed) == count and count >= 0.3 * c["N"]
    with torch.no_grad():
        w64 = _dequantize_weight(unsigned(layer.codes), layer.codebooks.double(), layer.scales.double())
        for rows, x in xs.items():
            got = layer(x)
            exact = F.linear(x.double(), w64, layer.bias.double())
            bound = 2.0 ** -10 * exact.abs() + 2.0 ** -13 * F.linear(x.double().abs(), w64.abs(), layer.bias.double().abs())
            worst = float(((got.double() - exact).abs() / bound).max())
            print(f"{rows} rows after the update: worst error / bound = {worst:.3f}")
            assert worst <= 1.0, f"{rows} rows against the torch definition on the new codes"
        assert not torch.equal(layer(xs[1]), before)
