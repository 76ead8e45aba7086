"""aqlm_hip_code_search_kx8_xtx and the calibrated code update built on it, on the MI355X.  One launch is held to its own arithmetic
BIT FOR BIT: the oracle is tests/kx8_xtx_model.py (numpy, float32, one IEEE operation per product and per sum in the order
include/aqlm_hip.h states) on exactly the values the kernel reads -- codes, sources and the bits of loss, delta and t.  The whole call
(kernel route) is compared with the torch route in float64: rows may differ only where the float64 arithmetic shows, at some step of
that row, two adjacent scores among the best beam_size + 1 closer than 2^-18 times that step's largest |score|, and at most 5 % of
the rows may differ at all.  Seeded inputs and their model results are computed once per configuration."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import kx8_xtx_model as model

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
OUT = 64
DIFFER_CAP = 0.05


@pytest.fixture(scope="module")
def hk():
    from aqlm_amd.inference_kernels import hip_kernel

    return hip_kernel


def stored(codes):
    codes = torch.as_tensor(codes).to(torch.int64)
    return torch.where(codes >= 128, codes - 256, codes).to(torch.int8)


def bits(x):
    return torch.as_tensor(x).contiguous().view(torch.int32)


@functools.lru_cache(maxsize=None)
def layer(K, g, dtype, fin=64, out=OUT, seed=0):
    """Seeded Gaussian inputs, off any grid (the planted-codes recipe of tests/test_code_search_kx8_gpu.py::case): codebooks N(0, 1)
    rounded to the storage dtype, W_ref = scaled sums of planted codewords + 0.35 N(0, 1), previous codes = the planted ones with one
    code of every second group drawn anew, scales in [0.5, 1.5] with every third one negative, XTX = X^T X / n of a seeded correlated X
    plus a small non-symmetric part."""
    gen = torch.Generator().manual_seed(20000 * K + 100 * g + seed)
    ng = fin // g
    books = torch.randn((K, 256, g), generator=gen).to(dtype)
    planted = torch.randint(0, 256, (out, ng, K), generator=gen)
    r = sum(books[c][planted[..., c]].float() for c in range(K)) + 0.35 * torch.randn((out, ng, g), generator=gen)
    prev = planted.clone().reshape(-1, K)
    moved = torch.nonzero(torch.rand((out * ng,), generator=gen) < 0.5).flatten()
    prev[moved, torch.randint(0, K, (moved.numel(),), generator=gen)] = torch.randint(0, 256, (moved.numel(),), generator=gen)
    prev = prev.reshape(out, ng, K)
    scales = torch.rand((out,), generator=gen) + 0.5
    scales[::3] *= -1
    scales = scales.to(dtype)
    reference = (r * scales.float()[:, None, None]).reshape(out, fin)
    X = torch.randn((4 * fin, fin), generator=gen)
    X = X + 0.6 * X.roll(1, 1)
    XTX = X.T @ X / X.shape[0] + 0.02 * torch.randn((fin, fin), generator=gen)
    return {"K": K, "g": g, "fin": fin, "books": books, "scales": scales, "reference": reference, "prev": prev, "XTX": XTX.contiguous()}


@functools.lru_cache(maxsize=None)
def step_case(K, g, beam, dtype, positions, out=OUT, rows=None):
    """The inputs of one launch for group 1 of ``layer``: position b holds the previous codes with the codes of group 0 shifted by b (so
    the positions differ), its T slice and its loss, all float32 values formed in float64.  ``rows``: "equal" makes the 256 rows of every
    codebook one row (the shift then changes no weight: the positions are equal too), "pairs" makes row 2i + 1 a copy of row 2i."""
    c = dict(layer(K, g, dtype, out=out))
    if rows is not None:
        c["books"] = c["books"].clone()
        if rows == "equal":
            c["books"][:] = c["books"][:, :1]
        else:
            c["books"][:, 1::2] = c["books"][:, 0::2]
    books, s = c["books"].double(), c["scales"].double()
    XTX = c["XTX"].double()
    t, loss = [], []
    for b in range(positions):
        codes = c["prev"].clone()
        codes[:, 0, :] = (codes[:, 0, :] + 7 * b) % 256
        weight = sum(books[k][codes[..., k]] for k in range(K)).reshape(out, -1) * s[:, None]
        error = c["reference"].double() - weight
        T = error @ XTX
        t.append(T[:, g:2 * g])
        loss.append((T * error).sum(-1))
    H = c["XTX"][g:2 * g, g:2 * g].contiguous()
    q = torch.from_numpy(model.group_q(c["books"].float().numpy(), H.numpy(), np.float64)).float()
    codes_in = c["prev"][None, :, 1, :].expand(positions, out, K).contiguous()
    return {"t": torch.stack(t).float().contiguous(), "loss": torch.stack(loss).float().contiguous(), "codes_in": codes_in, "H": H, "q": q,
            "books": c["books"], "scales": c["scales"]}


@functools.lru_cache(maxsize=None)
def expected(K, g, beam, dtype, positions, scaled=True, order=None, out=OUT, rows=None):
    c = step_case(K, g, beam, dtype, positions, out, rows)
    return model.step(c["t"].numpy(), c["loss"].numpy(), c["codes_in"].numpy(), c["H"].numpy(), c["q"].numpy(), c["books"].float().numpy(),
                      c["scales"].float().numpy() if scaled else None, beam, None if order is None else list(order))


def launch(hk, c, beam, t=None, scaled=True, order=None):
    return hk.code_search_kx8_xtx_step(c["t"].to(DEV) if t is None else t, c["loss"].to(DEV), stored(c["codes_in"]).to(DEV), c["H"].to(DEV),
                                       c["q"].to(DEV), c["books"].to(DEV), c["scales"].to(DEV) if scaled else None, beam, dim_order=order,
                                       return_t=True)


def hold_to_model(got, want, what, rows=None):
    rows = slice(None) if rows is None else rows
    assert got.codes.dtype == torch.int8 and got.source.dtype == torch.uint8 and got.loss.dtype == torch.float32
    report = {"codes": int(((got.codes.cpu().to(torch.int64) % 256) != torch.from_numpy(want["codes"]))[:, rows].sum()),
              "source": int((got.source.cpu().to(torch.int64) != torch.from_numpy(want["source"]))[:, rows].sum())}
    for name in ("loss", "delta", "t"):
        report[name] = int((bits(getattr(got, name).cpu()) != bits(torch.from_numpy(want[name])))[:, rows].sum())
    print(f"{what}: entries that differ from the model {report}")
    assert not any(report.values()), f"{what}: {report}"


SCHEMES = [(1, 8, 1), (1, 8, 4), (2, 8, 1), (2, 8, 8), (3, 8, 16), (4, 16, 4), (8, 32, 8), (2, 16, 3)]


# positions_in 1 (the first group of a call) and beam_size (every later group); at beam_size 1 the two are one launch
LAUNCHES = [(K, g, beam, positions) for K, g, beam in SCHEMES for positions in sorted({1, beam})]


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("K,g,beam,positions", LAUNCHES)
def test_one_launch_equals_the_model_bit_for_bit(hk, K, g, beam, positions, dtype):
    c, want = step_case(K, g, beam, dtype, positions), expected(K, g, beam, dtype, positions)
    changed = float((want["codes"][0] != (c["codes_in"][0].numpy() % 256)).any(-1).mean())
    print(f"{K}x8 g{g} beam {beam}, {positions} positions: {100 * changed:.1f} % of the rows change a code")
    assert changed >= 0.30, "the inputs must not pass on an identity"
    got = launch(hk, c, beam)
    assert got.codes.shape == (beam, OUT, K) and got.delta.shape == (beam, OUT, g) and got.t.shape == (beam, OUT, g)
    hold_to_model(got, want, f"{K}x8 g{g} beam {beam} {dtype}, {positions} positions")
    again = launch(hk, c, beam)
    for name in ("loss", "delta", "t"):
        assert torch.equal(bits(getattr(got, name)), bits(getattr(again, name))), "two calls give identical bits"
    assert torch.equal(got.codes, again.codes) and torch.equal(got.source, again.source)


def test_strided_view_no_scales_and_dim_order(hk):
    K, g, beam, dtype = 2, 8, 8, torch.float16
    c = step_case(K, g, beam, dtype, beam)
    wide = torch.full((beam, OUT, 40), float("nan"), device=DEV)
    wide[:, :, 16:24] = c["t"].to(DEV)
    hold_to_model(launch(hk, c, beam, t=wide[:, :, 16:24]), expected(K, g, beam, dtype, beam), "t as a view of a wider buffer")
    hold_to_model(launch(hk, c, beam, scaled=False), expected(K, g, beam, dtype, beam, scaled=False), "scales NULL")
    c3 = step_case(3, 8, 16, dtype, 16)
    hold_to_model(launch(hk, c3, 16, order=[2, 0, 1]), expected(3, 8, 16, dtype, 16, order=(2, 0, 1)), "dim_order 2, 0, 1")


@pytest.mark.parametrize("poison", [float("nan"), float("inf"), float("-inf")])
def test_non_finite_inputs_stay_in_range_and_leave_the_other_rows_alone(hk, poison):
    K, g, beam, dtype = 2, 8, 8, torch.float16
    c = dict(step_case(K, g, beam, dtype, beam))
    t, loss = c["t"].clone(), c["loss"].clone()
    t[3, 5, 2] = poison
    loss[1, 9] = poison
    c["t"], c["loss"] = t, loss
    got = launch(hk, c, beam)
    torch.cuda.synchronize()
    assert int(got.source.max()) < beam
    others = [r for r in range(OUT) if r not in (5, 9)]
    hold_to_model(got, expected(K, g, beam, dtype, beam), f"rows beside the {poison} ones", rows=others)


@pytest.mark.parametrize("where", ["H", "q"])
@pytest.mark.parametrize("poison", [float("nan"), float("inf")])
def test_non_finite_H_or_q_still_gives_codes_and_sources_in_range(hk, where, poison):
    """Every row reads H and q, so no row keeps the model's bits: the call returns, sources stay below positions_in (int8 codes cover
    0 .. 255 by construction) and a second call gives the same result."""
    K, g, beam, dtype = 2, 8, 8, torch.float16
    c = dict(step_case(K, g, beam, dtype, beam))
    bad = c[where].clone()
    bad[1, 3] = poison
    bad[0, 0] = -poison
    c[where] = bad
    got = launch(hk, c, beam)
    torch.cuda.synchronize()
    assert got.codes.shape == (beam, OUT, K) and got.source.shape == (beam, OUT)
    assert int(got.source.max()) < beam
    again = launch(hk, c, beam)
    assert torch.equal(got.codes, again.codes) and torch.equal(got.source, again.source), "still a function of the arguments"


# ---------------------------------------------------------------------------------------------------------------------------
# exact ties: both ways of the selection (kx8_select_body.h) with equal keys, and the scores they pass on
# ---------------------------------------------------------------------------------------------------------------------------
TIES = ([(K, 8, beam, positions, torch.float16) for K in (2, 3) for beam in (4, 16) for positions in (1, 4)]
        + [(2, 32, 16, 4, torch.float16), (3, 8, 4, 4, torch.bfloat16)])
TIE_IDS = [f"{K}x8-g{g}-beam{beam}-p{positions}-{'bf16' if dtype == torch.bfloat16 else 'fp16'}" for K, g, beam, positions, dtype in TIES]


@pytest.mark.parametrize("K,g,beam,positions,dtype", TIES, ids=TIE_IDS)
def test_codebooks_of_equal_rows_tie_every_candidate(hk, K, g, beam, positions, dtype):
    """Every key of a step has the same score (the 256 candidates of a position, and the positions among themselves): far more than 64
    reach the bound, so every step goes the general way, and rank i is flat index i -- position 0, code i."""
    c, want = step_case(K, g, beam, dtype, positions, 8, "equal"), expected(K, g, beam, dtype, positions, out=8, rows="equal")
    assert bool((c["q"] == c["q"][:, :1]).all()) and bool((c["t"] == c["t"][:1]).all()) and bool((c["loss"] == c["loss"][:1]).all())
    ranks = np.broadcast_to(np.arange(beam)[:, None], (beam, 8))
    assert (want["codes"][:, :, :K - 1] == 0).all() and (want["codes"][:, :, K - 1] == ranks).all() and (want["source"] == 0).all(), \
        "the inputs tie: the model's stable sort keeps flat indices 0 .. beam_size - 1 on every step"
    assert (bits(want["loss"]) == bits(want["loss"])[:1]).all()
    hold_to_model(launch(hk, c, beam), want, f"{K}x8 g{g} beam {beam} {dtype}, {positions} positions, equal rows")


@pytest.mark.parametrize("K,g,beam,positions,dtype", TIES, ids=TIE_IDS)
def test_rows_equal_in_pairs_tie_inside_the_counting_way(hk, K, g, beam, positions, dtype):
    """Candidates 2i and 2i + 1 of every position have the same score: the few keys within the bound hold exact ties, which the
    count on the full key gives to the smaller flat index."""
    c, want = step_case(K, g, beam, dtype, positions, 8, "pairs"), expected(K, g, beam, dtype, positions, out=8, rows="pairs")
    assert bool((c["q"][:, 1::2] == c["q"][:, 0::2]).all()) and bool((c["books"][:, 1::2] == c["books"][:, 0::2]).all())
    pairs = bits(want["loss"]).numpy().reshape(beam // 2, 2, 8)
    print(f"{int((pairs[:, 0] == pairs[:, 1]).sum())} of {pairs[:, 0].size} adjacent survivors of the last step have equal scores")
    assert (pairs[:, 0] == pairs[:, 1]).any(), "the inputs must tie among the survivors"
    hold_to_model(launch(hk, c, beam), want, f"{K}x8 g{g} beam {beam} {dtype}, {positions} positions, rows equal in pairs")


# ---------------------------------------------------------------------------------------------------------------------------
# the whole call: kernel route against the torch route in float64
# ---------------------------------------------------------------------------------------------------------------------------
CALLS = [(2, 8, 128, 64, 4, torch.float16, False), (2, 8, 128, 64, 8, torch.bfloat16, False), (1, 8, 128, 64, 4, torch.float16, False),
         (4, 16, 128, 32, 2, torch.float16, True), (8, 32, 256, 32, 4, torch.float16, False), (3, 8, 64, 64, 16, torch.float16, False)]


@functools.lru_cache(maxsize=None)
def call_case(K, g, fin, out, beam, dtype, shuffled):
    import aqlm.tuning as tuning

    c = layer(K, g, dtype, fin, out, seed=1)
    ng = fin // g
    rng = np.random.default_rng(5)
    group_order = [int(j) for j in rng.permutation(ng)] if shuffled else None
    dim_order = [[int(k) for k in rng.permutation(K)] for _ in range(ng)] if shuffled else None
    books4, scales4 = c["books"].reshape(K, 256, 1, g), c["scales"].reshape(-1, 1, 1, 1)
    want = tuning.find_optimal_codes_calibrated(c["XTX"].double(), c["reference"].double(), books4.double(), c["prev"], scales4.double(),
                                                beam_size=beam, group_order=group_order, dim_order=dim_order)
    _, near = model.search_layer(c["XTX"].numpy(), c["reference"].numpy(), c["books"].float().numpy(), c["prev"].numpy(), c["scales"].float().numpy(),
                                 beam, group_order, dim_order, np.float64, model.NEAR)
    return c, books4, scales4, group_order, dim_order, want, near


@pytest.mark.parametrize("K,g,fin,out,beam,dtype,shuffled", CALLS)
def test_kernel_route_against_the_torch_route_in_float64(hk, monkeypatch, K, g, fin, out, beam, dtype, shuffled):
    import aqlm.tuning as tuning
    from aqlm_amd.utils import _dequantize_weight

    c, books4, scales4, group_order, dim_order, want, near = call_case(K, g, fin, out, beam, dtype, shuffled)
    calls = []
    real = hk.code_search_kx8_xtx_step
    monkeypatch.setattr(hk, "code_search_kx8_xtx_step", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    args = (c["XTX"].to(DEV), c["reference"].to(DEV), books4.to(DEV), stored(c["prev"]).to(DEV), scales4.to(DEV))
    results, default = {}, tuning.CALIBRATED_BLOCK_GROUPS
    assert default > 1
    for block in (default, 1):
        monkeypatch.setattr(tuning, "CALIBRATED_BLOCK_GROUPS", block)
        got = tuning.find_optimal_codes_calibrated(*args, beam_size=beam, group_order=group_order, dim_order=dim_order)
        assert got.dtype == torch.int8 and got.shape == c["prev"].shape
        results[block] = got.cpu().to(torch.int64) % 256
    assert len(calls) == 2 * (fin // g), "one launch per input group"
    got = results[default]
    differ = (got != want).any(-1).any(-1).numpy()
    print(f"{K}x8 g{g} {out} x {fin} beam {beam}: {int(differ.sum())} rows differ from float64, {int(near.sum())} rows have a near tie, "
          f"{int((differ & ~near).sum())} differ without one")
    assert not (differ & ~near).any(), f"{int((differ & ~near).sum())} rows without a near tie differ from the float64 torch route"
    assert differ.mean() <= DIFFER_CAP
    blocks_differ = (results[1] != got).any(-1).any(-1).numpy()
    assert not (blocks_differ & ~near).any(), "a block size of 1 group and the default agree outside the near-tie set"
    XTX, ref = c["XTX"].double(), c["reference"].double()
    before = float(tuning.calibrated_error(_dequantize_weight(c["prev"], books4.double(), scales4.double()), ref, XTX))
    after = float(tuning.calibrated_error(_dequantize_weight(got, books4.double(), scales4.double()), ref, XTX))
    print(f"calibrated error {before:.6g} -> {after:.6g}")
    assert after <= before


def test_update_codes_calibrated_on_a_gpu_layer_rebuilds_the_derived_copies(hk):
    import aqlm.tuning as tuning
    from aqlm import QuantizedLinear
    from aqlm_amd.utils import _dequantize_weight

    K, g, fin, out = 2, 8, 128, 64
    c = layer(K, g, torch.float16, fin, out, seed=1)
    m = QuantizedLinear(fin, out, g, 1, K, 8, bias=False, device=DEV, dtype=torch.float16)
    with torch.no_grad():
        m.codes.copy_(stored(c["prev"]))
        m.codebooks.copy_(c["books"].reshape(K, 256, 1, g))
        m.scales.copy_(c["scales"].reshape(-1, 1, 1, 1))
        x = torch.randn((3, fin), generator=torch.Generator().manual_seed(3)).half().to(DEV)
        m(x)  # derived copies exist before the update
        XTX, ref = c["XTX"].to(DEV), c["reference"].to(DEV)
        before, version, holder = float(tuning.calibrated_error(m, ref, XTX)), m.codes._version, m.codes
        changed = int(tuning.update_codes_calibrated_(m, ref, XTX, beam_size=4))
        assert m.codes is holder and m.codes._version > version and changed > 0
        assert changed == int((m.codes.cpu() != stored(c["prev"])).any(-1).sum())
        dense = _dequantize_weight(m.codes.to(torch.int64) % 256, m.codebooks.float(), m.scales.float())
        y, want = m(x).float(), F.linear(x.float(), dense)
        assert float((y - want).abs().max()) <= 2e-3 * float(want.abs().max()) + 1e-3
        assert float(tuning.calibrated_error(m, ref, XTX)) < before
