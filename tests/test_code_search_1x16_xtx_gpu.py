"""aqlm_hip_code_search_1x16_xtx and the calibrated code update of 1x16 layers built on it, on the MI355X.  One call of the entry is held
to its own arithmetic BIT FOR BIT: the oracle is tests/x16_xtx_model.py (numpy, float32, one IEEE operation per product and per sum in
the order include/aqlm_hip.h states) on exactly the values the kernel reads -- codes, sources and the bits of loss, delta and t.  The
matrix unit only filters, so codebooks whose scores differ by less than the scan resolves (equal rows, rows equal in pairs, rows one
unit in the last place apart) must come out in the model's order too.  The whole call (kernel route) is compared with the torch
route in float64: rows may differ only where the float64 arithmetic shows two adjacent scores among a group's best beam_size + 1
closer than 2^-18 times that group's largest |score|, and at most 5 % of the rows may differ at all.  Seeded inputs and their model
results are computed once per configuration."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import x16_xtx_model as model
from tests.test_code_search_xtx_host import golden

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
OUT = 64
SIZE = 65536
DIFFER_CAP = 0.05


@pytest.fixture(scope="module")
def hk():
    from aqlm_amd.inference_kernels import hip_kernel

    return hip_kernel


def stored(codes):
    codes = torch.as_tensor(codes).to(torch.int64)
    return torch.where(codes >= SIZE // 2, codes - SIZE, codes).to(torch.int16)


def bits(x):
    return torch.as_tensor(x).contiguous().view(torch.int32)


@functools.lru_cache(maxsize=None)
def layer(g, dtype, fin=64, out=OUT, seed=0):
    """The planted-codes recipe of tests/test_code_search_xtx_gpu.py::layer with one codebook of 65536 entries: codebook N(0, 1) rounded
    to the storage dtype, W_ref = scaled planted codewords + 0.35 N(0, 1), previous codes = the planted ones with the code of every
    second group drawn anew, scales in [0.5, 1.5] with every third one negative, XTX = X^T X / n of a seeded correlated X plus a small
    non-symmetric part."""
    gen = torch.Generator().manual_seed(777 + 100 * g + seed)
    ng = fin // g
    book = torch.randn((SIZE, g), generator=gen).to(dtype)
    planted = torch.randint(0, SIZE, (out, ng), generator=gen)
    r = book[planted].float() + 0.35 * torch.randn((out, ng, g), generator=gen)
    prev = planted.clone().reshape(-1)
    moved = torch.nonzero(torch.rand((out * ng,), generator=gen) < 0.5).flatten()
    prev[moved] = torch.randint(0, SIZE, (moved.numel(),), generator=gen)
    prev = prev.reshape(out, ng, 1)
    scales = torch.rand((out,), generator=gen) + 0.5
    scales[::3] *= -1
    scales = scales.to(dtype)
    reference = (r * scales.float()[:, None, None]).reshape(out, fin)
    X = torch.randn((4 * fin, fin), generator=gen)
    X = X + 0.6 * X.roll(1, 1)
    XTX = X.T @ X / X.shape[0] + 0.02 * torch.randn((fin, fin), generator=gen)
    return {"g": g, "fin": fin, "book": book, "scales": scales, "reference": reference, "prev": prev, "XTX": XTX.contiguous()}


def step_inputs(c, prev, positions):
    """The inputs of one call for group 1 of layer ``c`` with previous codes ``prev``: position b holds ``prev`` with the code of group 0
    shifted by 7 b (so the positions differ), its T slice and its loss, float32 values formed in float64."""
    g, out = c["g"], prev.shape[0]
    book, s, XTX = c["book"].double(), c["scales"].double(), c["XTX"].double()
    t, loss = [], []
    for b in range(positions):
        codes = prev.clone()
        codes[:, 0, 0] = (codes[:, 0, 0] + 7 * b) % SIZE
        error = c["reference"].double() - book[codes[..., 0]].reshape(out, -1) * s[:, None]
        T = error @ XTX
        t.append(T[:, g:2 * g])
        loss.append((T * error).sum(-1))
    H = c["XTX"][g:2 * g, g:2 * g].contiguous()
    q = torch.from_numpy(model.group_q(c["book"].float().numpy(), H.numpy(), np.float64)).float()
    codes_in = prev[None, :, 1, :].expand(positions, out, 1).contiguous()
    return {"t": torch.stack(t).float().contiguous(), "loss": torch.stack(loss).float().contiguous(), "codes_in": codes_in, "H": H, "q": q,
            "book": c["book"], "scales": c["scales"]}


@functools.lru_cache(maxsize=None)
def step_case(g, dtype, positions, out=OUT, rows=None):
    """``rows``: "equal" makes the 65536 rows of the codebook one row (the shift then changes no weight: the positions are equal too),
    "pairs" makes row 2i + 1 a copy of row 2i, "ulp" makes it that copy with element 0 moved by one unit in the last place of the
    storage dtype."""
    c = dict(layer(g, dtype, out=out))
    if rows is not None:
        book = c["book"].clone()
        if rows == "equal":
            book[:] = book[:1]
        else:
            book[1::2] = book[0::2]
            if rows == "ulp":
                book[1::2, 0] = (book[1::2, 0].contiguous().view(torch.int16) + 1).view(dtype)
        c["book"] = book
    return step_inputs(c, c["prev"], positions)


def run_model(c, beam, scaled=True):
    return model.step(c["t"].numpy(), c["loss"].numpy(), c["codes_in"].numpy(), c["H"].numpy(), c["q"].numpy(), c["book"].float().numpy(),
                      c["scales"].float().numpy() if scaled else None, beam)


@functools.lru_cache(maxsize=None)
def expected(g, beam, dtype, positions, scaled=True, out=OUT, rows=None):
    return run_model(step_case(g, dtype, positions, out, rows), beam, scaled)


def launch(hk, c, beam, t=None, scaled=True, return_t=True):
    return hk.code_search_1x16_xtx_step(c["t"].to(DEV) if t is None else t, c["loss"].to(DEV), stored(c["codes_in"]).to(DEV), c["H"].to(DEV),
                                        c["q"].to(DEV), c["book"].to(DEV), c["scales"].to(DEV) if scaled else None, beam, return_t=return_t)


def hold_to_model(got, want, what, rows=None):
    rows = slice(None) if rows is None else rows
    assert got.codes.dtype == torch.int16 and got.source.dtype == torch.uint8 and got.loss.dtype == torch.float32
    report = {"codes": int(((got.codes[..., 0].cpu().to(torch.int64) % SIZE) != torch.from_numpy(want["codes"]))[:, rows].sum()),
              "source": int((got.source.cpu().to(torch.int64) != torch.from_numpy(want["source"]))[:, rows].sum())}
    for name in ("loss", "delta", "t"):
        report[name] = int((bits(getattr(got, name).cpu()) != bits(torch.from_numpy(want[name])))[:, rows].sum())
    print(f"{what}: entries that differ from the model {report}")
    assert not any(report.values()), f"{what}: {report}"


LAUNCHES = [(g, beam, positions) for g in (8, 16) for beam, positions in ((1, 1), (4, 1), (4, 4), (8, 8))]


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("g,beam,positions", LAUNCHES)
def test_one_call_equals_the_model_bit_for_bit(hk, g, beam, positions, dtype):
    c, want = step_case(g, dtype, positions), expected(g, beam, dtype, positions)
    changed = float((want["codes"][0] != (c["codes_in"][0, :, 0].numpy() % SIZE)).mean())
    print(f"1x16 g{g} beam {beam}, {positions} positions: {100 * changed:.1f} % of the rows change their code")
    assert changed >= 0.30, "the inputs must not pass on an identity"
    got = launch(hk, c, beam)
    assert got.codes.shape == (beam, OUT, 1) and got.delta.shape == (beam, OUT, g) and got.t.shape == (beam, OUT, g)
    hold_to_model(got, want, f"1x16 g{g} beam {beam} {dtype}, {positions} positions")
    again = launch(hk, c, beam)
    for name in ("loss", "delta", "t"):
        assert torch.equal(bits(getattr(got, name)), bits(getattr(again, name))), "two calls give identical bits"
    assert torch.equal(got.codes, again.codes) and torch.equal(got.source, again.source)


@pytest.mark.parametrize("out", [5, 131])
def test_partial_tiles_and_more_than_one_block_of_columns(hk, out):
    g, beam, dtype = 8, 4, torch.float16
    hold_to_model(launch(hk, step_case(g, dtype, beam, out), beam), expected(g, beam, dtype, beam, out=out), f"out = {out}: {4 * out} columns")


def test_strided_view_no_scales_and_return_t(hk):
    g, beam, dtype = 8, 4, torch.float16
    c, want = step_case(g, dtype, beam), expected(g, beam, dtype, beam)
    wide = torch.full((beam, OUT, 40), float("nan"), device=DEV)
    wide[:, :, 16:24] = c["t"].to(DEV)
    hold_to_model(launch(hk, c, beam, t=wide[:, :, 16:24]), want, "t as a view of a wider buffer")
    hold_to_model(launch(hk, c, beam, scaled=False), expected(g, beam, dtype, beam, scaled=False), "scales NULL")
    bare = launch(hk, c, beam, return_t=False)
    assert bare.t is None
    hold_to_model(bare._replace(t=torch.from_numpy(want["t"])), want, "t_out NULL")


# ---------------------------------------------------------------------------------------------------------------------------
# codebooks that defeat a lazy filter: scores that differ by nothing, or by less than the scan resolves
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
def test_a_codebook_of_equal_rows_ties_every_candidate(hk, dtype):
    g, beam = 8, 4
    c, want = step_case(g, dtype, beam, 16, "equal"), expected(g, beam, dtype, beam, out=16, rows="equal")
    assert bool((c["q"] == c["q"][:1]).all()) and bool((c["t"] == c["t"][:1]).all()) and bool((c["loss"] == c["loss"][:1]).all())
    ranks = np.broadcast_to(np.arange(beam)[:, None], (beam, 16))
    assert (want["codes"] == ranks).all() and (want["source"] == 0).all(), "the inputs tie: a stable sort keeps flat indices 0 .. 3"
    assert (bits(want["loss"]) == bits(want["loss"])[:1]).all()
    hold_to_model(launch(hk, c, beam), want, f"g{g} beam {beam} {dtype}, equal rows")


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
def test_rows_equal_in_pairs_go_to_the_smaller_index(hk, dtype):
    g, beam = 8, 4
    c, want = step_case(g, dtype, beam, 16, "pairs"), expected(g, beam, dtype, beam, out=16, rows="pairs")
    pairs = bits(want["loss"]).numpy().reshape(beam // 2, 2, 16)
    print(f"{int((pairs[:, 0] == pairs[:, 1]).sum())} of {pairs[:, 0].size} adjacent survivors have equal scores")
    assert (pairs[:, 0] == pairs[:, 1]).any(), "the inputs must tie among the survivors"
    hold_to_model(launch(hk, c, beam), want, f"g{g} beam {beam} {dtype}, rows equal in pairs")


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
def test_rows_one_unit_in_the_last_place_apart_come_in_model_order(hk, dtype):
    g, beam = 8, 4
    c, want = step_case(g, dtype, beam, 16, "ulp"), expected(g, beam, dtype, beam, out=16, rows="ulp")
    twins = (want["codes"][0::2] // 2 == want["codes"][1::2] // 2) & (want["source"][0::2] == want["source"][1::2])
    print(f"{int(twins.sum())} of {twins.size} adjacent survivors are the two rows of one pair")
    assert twins.any(), "the inputs must put both rows of a pair among the survivors"
    hold_to_model(launch(hk, c, beam), want, f"g{g} beam {beam} {dtype}, rows one ulp apart")


# ---------------------------------------------------------------------------------------------------------------------------
# magnitudes
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what", ["loss x 2^12", "t x 2^-12"])
def test_magnitudes_of_loss_and_t(hk, what):
    g, beam, dtype = 8, 4, torch.float16
    c = dict(step_case(g, dtype, beam))
    if what.startswith("loss"):
        c["loss"] = c["loss"] * 4096.0  # the base swamps the group's contribution
    else:
        c["t"] = c["t"] * (1.0 / 4096.0)
    hold_to_model(launch(hk, c, beam), run_model(c, beam), what)


def test_a_previous_code_that_is_already_optimal_is_kept_with_a_zero_delta(hk):
    g, beam, dtype = 8, 4, torch.float16
    c = layer(g, dtype)
    best = expected(g, beam, dtype, 1)["codes"][0]  # the optimum of every row from position 0
    prev = c["prev"].clone()
    rows = list(range(0, OUT, 4))
    prev[rows, 1, 0] = torch.from_numpy(best)[rows]
    case = step_inputs(c, prev, 1)
    want = run_model(case, beam)
    assert (want["codes"][0][rows] == best[rows]).all() and (want["source"][0][rows] == 0).all(), "the optimum stays the optimum"
    assert (bits(want["delta"])[0][rows] == 0).all(), "and its weight change is +0 in every element"
    got = launch(hk, case, beam)
    hold_to_model(got, want, "previous codes already optimal on every fourth row")
    assert bool((bits(got.delta.cpu())[0][rows] == 0).all())


# ---------------------------------------------------------------------------------------------------------------------------
# non-finite inputs
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("poison", [float("nan"), float("inf"), float("-inf")])
def test_non_finite_t_or_loss_stays_in_range_and_leaves_the_other_rows_alone(hk, poison):
    g, beam, dtype = 8, 4, torch.float16
    c = dict(step_case(g, dtype, beam))
    t, loss = c["t"].clone(), c["loss"].clone()
    t[3, 5, 2] = poison
    loss[1, 9] = poison
    c["t"], c["loss"] = t, loss
    got = launch(hk, c, beam)
    torch.cuda.synchronize()
    assert int(got.source.max()) < beam and got.codes.shape == (beam, OUT, 1)
    others = [r for r in range(OUT) if r not in (5, 9)]
    hold_to_model(got, expected(g, beam, dtype, beam), f"rows beside the {poison} ones", rows=others)


@pytest.mark.parametrize("where", ["H", "q"])
@pytest.mark.parametrize("poison", [float("nan"), float("inf")])
def test_non_finite_H_or_q_still_gives_codes_and_sources_in_range(hk, where, poison):
    """Every row reads H and every row's bound reads max|q|: each candidate goes the exact way.  The call returns, sources stay below
    positions_in (int16 codes cover 0 .. 65535 by construction), a second call gives the same result, and with one poisoned q entry
    the rows stay the model's (the model reads the same q)."""
    g, beam, dtype = 8, 4, torch.float16
    c = dict(step_case(g, dtype, beam))
    bad = c[where].clone()
    if where == "H":
        bad[1, 3] = poison
    else:
        bad[12345] = poison
    c[where] = bad
    got = launch(hk, c, beam)
    torch.cuda.synchronize()
    assert got.codes.shape == (beam, OUT, 1) and int(got.source.max()) < beam
    again = launch(hk, c, beam)
    assert torch.equal(got.codes, again.codes) and torch.equal(got.source, again.source), "still a function of the arguments"
    if where == "q":
        assert not bool((c["codes_in"] % SIZE == 12345).any())
        hold_to_model(got, run_model(c, beam), f"q[12345] = {poison}")


# ---------------------------------------------------------------------------------------------------------------------------
# the whole call: kernel route against the torch route in float64
# ---------------------------------------------------------------------------------------------------------------------------
CALLS = [(8, 1), (8, 4), (16, 4)]


@functools.lru_cache(maxsize=None)
def call_case(g, beam):
    import aqlm.tuning as tuning

    c = layer(g, torch.float16, 32, OUT)
    book4, scales4 = c["book"].reshape(1, SIZE, 1, g), c["scales"].reshape(-1, 1, 1, 1)
    want = tuning.find_optimal_codes_calibrated(c["XTX"].double(), c["reference"].double(), book4.double(), c["prev"], scales4.double(), beam_size=beam)
    _, near = model.search_layer(c["XTX"].numpy(), c["reference"].numpy(), c["book"].float().numpy(), c["prev"].numpy(), c["scales"].float().numpy(),
                                 beam, None, np.float64, model.NEAR)
    return c, book4, scales4, want, near


@pytest.mark.parametrize("g,beam", CALLS)
def test_kernel_route_against_the_torch_route_in_float64(hk, monkeypatch, g, beam):
    import aqlm.tuning as tuning
    from aqlm_amd.utils import _dequantize_weight

    c, book4, scales4, want, near = call_case(g, beam)
    calls = []
    real = hk.code_search_1x16_xtx_step
    monkeypatch.setattr(hk, "code_search_1x16_xtx_step", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    got = tuning.find_optimal_codes_calibrated(c["XTX"].to(DEV), c["reference"].to(DEV), book4.to(DEV), stored(c["prev"]).to(DEV), scales4.to(DEV),
                                               beam_size=beam)
    assert got.dtype == torch.int16 and got.shape == c["prev"].shape
    assert len(calls) == 32 // g, "one call of the entry per input group"
    got = got.cpu().to(torch.int64) % SIZE
    differ = (got != want).any(-1).any(-1).numpy()
    print(f"1x16 g{g} {OUT} x 32 beam {beam}: {int(differ.sum())} rows differ from float64, {int(near.sum())} rows have a near tie, "
          f"{int((differ & ~near).sum())} differ without one")
    assert not (differ & ~near).any(), f"{int((differ & ~near).sum())} rows without a near tie differ from the float64 torch route"
    assert differ.mean() <= DIFFER_CAP
    XTX, ref = c["XTX"].double(), c["reference"].double()
    before = float(tuning.calibrated_error(_dequantize_weight(c["prev"], book4.double(), scales4.double()), ref, XTX))
    after = float(tuning.calibrated_error(_dequantize_weight(got, book4.double(), scales4.double()), ref, XTX))
    print(f"calibrated error {before:.6g} -> {after:.6g}")
    assert after <= before


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
def test_fixture_case_a_on_the_kernel_route(hk, monkeypatch, dtype):
    import aqlm.tuning as tuning

    c = golden("a", torch.float32)
    for name in ("books", "scales", "target"):
        assert torch.equal(c[name].to(dtype).float(), c[name]), f"the fixture's {name} are exact in {dtype}"
    calls = []
    real = hk.code_search_1x16_xtx_step
    monkeypatch.setattr(hk, "code_search_1x16_xtx_step", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    got = tuning.find_optimal_codes_calibrated(c["XTX"].to(DEV), c["target"].to(dtype).to(DEV), c["books"].to(dtype).to(DEV), stored(c["prev"]).to(DEV),
                                               c["scales"].to(dtype).to(DEV), beam_size=c["beam"], group_order=c["group_order"])
    assert len(calls) == 8
    differ = ((got.cpu().to(torch.int64) % SIZE) != c["expected"]).any(-1).any(-1)
    assert not bool(differ.any()), f"{int(differ.sum())} rows differ from the reference's codes"


def test_update_codes_calibrated_on_a_gpu_layer_rebuilds_the_derived_copies(hk):
    import aqlm.tuning as tuning
    from aqlm import QuantizedLinear
    from aqlm_amd.utils import _dequantize_weight

    g, fin, out = 8, 64, OUT
    c = layer(g, torch.float16, fin, out)
    m = QuantizedLinear(fin, out, g, 1, 1, 16, bias=False, device=DEV, dtype=torch.float16)
    with torch.no_grad():
        m.codes.copy_(stored(c["prev"]))
        m.codebooks.copy_(c["book"].reshape(1, SIZE, 1, g))
        m.scales.copy_(c["scales"].reshape(-1, 1, 1, 1))
        x = torch.randn((3, fin), generator=torch.Generator().manual_seed(3)).half().to(DEV)
        m(x)  # derived copies exist before the update
        XTX, ref = c["XTX"].to(DEV), c["reference"].to(DEV)
        before, version, holder = float(tuning.calibrated_error(m, ref, XTX)), m.codes._version, m.codes
        changed = int(tuning.update_codes_calibrated_(m, ref, XTX, beam_size=4))
        assert m.codes is holder and m.codes._version > version and changed > 0
        assert changed == int((m.codes.cpu() != stored(c["prev"])).any(-1).sum())
        dense = _dequantize_weight(m.codes.to(torch.int64) % SIZE, m.codebooks.float(), m.scales.float())
        y, want = m(x).float(), F.linear(x.float(), dense)
        assert float((y - want).abs().max()) <= 2e-3 * float(want.abs().max()) + 1e-3
        assert float(tuning.calibrated_error(m, ref, XTX)) <= before


def test_routing_counts_the_launches(hk, monkeypatch):
    import aqlm.tuning as tuning

    c = golden("a", torch.float32)
    calls = []
    real = hk.code_search_1x16_xtx_step
    monkeypatch.setattr(hk, "code_search_1x16_xtx_step", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    args = lambda target: (c["XTX"].to(DEV), target.to(DEV), c["books"].half().to(DEV), stored(c["prev"]).to(DEV), c["scales"].half().to(DEV))  # noqa: E731
    tuning.find_optimal_codes_calibrated(*args(c["target"]), beam_size=4, dim_order=[0])
    assert len(calls) == 64 // 8, "in / g calls of the entry; a dim_order of one codebook is accepted"
    del calls[:]
    tuning.find_optimal_codes_calibrated(*args(c["target"]), beam_size=9)
    tuning.find_optimal_codes_calibrated(*args(c["target"].double()), beam_size=1)
    monkeypatch.setattr(tuning, "CODE_SEARCH_KERNEL", False)
    tuning.find_optimal_codes_calibrated(*args(c["target"]), beam_size=1)
    assert not calls, "beam 9, a float64 target and CODE_SEARCH_KERNEL = False keep the torch route"
