"""The routed packed launch (aqlm_hip_gemv_1x16_routed_packed) where its table entries DIFFER, on the MI355X.  The kernel is
parameterised per entry by what the repack decided for that expert's codes -- ``waves``, ``steps``, ``x_copies`` and either the
live codebook or, for a relabelled buffer, the permuted codebook image inside the packed buffer --, the block size is the largest
wave count of the table and the body idles the waves beyond an entry's own.  tests/test_moe_packed_gpu.py draws uniform codes, so
every entry of its tables packs alike and nothing is relabelled.  Here: Zipf and row-correlated codes (tests/moe_experts.py),
labels dealt out or kept, tables that mix wave counts, step counts (up to 104: four mask words) and both codebook kinds, the
slice-first instantiation, a bias per expert, ragged and tiny shapes, 1 / 3 / 60 experts, top_k up to 8, strided x, per-pair
magnitudes and non-finite rows; then ``prepack_experts(relabel=True)`` at module level: report, forward, staleness, hipGraph.

Every case checks, with bounds restated from existing contracts:
  (a) each (pair, segment) row is bit-identical to ``hk.code1x16_matmat_packed`` at batch 1 of that expert on that row;
  (b) a subset of rows meets the fp64 oracle within ``check_close`` of tests/test_hip_parity.py (what the single-layer kernel's
      skewed-histogram tests use);
  (c) the accumulator cells are all zero after every launch;
  (d) pairs whose id lies outside [0, E) give zero rows;
  (e) every ``PackedCodes.desc`` (relabelled, waves, steps) equals what the numpy model of the format predicts (g8; the model is
      g8 only) -- a case that does not reach its path fails;
and the table read back from the device carries, per entry, the descriptor's waves / steps and a codebook pointer that lies
inside the packed buffer exactly when the buffer is relabelled.  Block level: mean |y - ref| / mean |ref| < 2e-3 (fp16) /
1.6e-2 (bf16) as in tests/test_moe_gpu.py."""
import pytest
import torch

from tests import moe_experts as mx
from tests.test_hip_parity import check_close
from tests.test_moe_gpu import E as MODULE_E
from tests.test_moe_gpu import _module, _route, _w64
from tests.test_moe_packed_gpu import _cells_at_rest

pytestmark = pytest.mark.gpu

DTYPES = [torch.float16, torch.bfloat16]


def _oracle64(layer, xr):
    """fp64: W x (+ bias) of one row, W dequantised in fp64 on the device."""
    y = _w64(layer) @ xr.double()
    if layer[3] is not None:
        y = y + layer[3].double()
    return y.cpu().numpy()


def _launch(x, ids, table, tail, E, S, fout, fin, g, per_pair):
    return torch.ops.aqlm.code1x16_moe_matmat_packed(x, ids, table, [E, S, fout, fin, g, ids.shape[1]] + tail, per_pair)


def _check_descs(packed, plans, recipes, what):
    """(e): the device's decision is the model's, per layer; where there is no model (g16) at least: labels kept are kept."""
    for e, per in enumerate(packed):
        for s, (pk, _, _, _) in enumerate(per):
            d = pk.desc
            assert not d.variable_geometry, f"{what} expert {e} seg {s}: variable geometry in a uniform-only repack"
            if plans[e][s] is not None:
                got = (bool(d.relabelled), int(d.waves), int(d.steps))
                assert got == plans[e][s], f"{what} expert {e} seg {s}: repack decided {got}, the model {plans[e][s]}"
            if not recipes[e][s].relabel:
                assert not d.relabelled, f"{what} expert {e} seg {s}: relabelled although relabel=False"


def _check_table(table, tail, packed, g, what):
    """The device table, read back: waves / steps of every entry are its descriptor's, the codebook pointer is the image inside
    the packed buffer for a relabelled entry and the live tensor otherwise; max_waves of the tail is the largest wave count."""
    from aqlm_amd import _native

    words = _native.ROUTED_PACKED_ENTRY_WORDS
    flat = [seg for per in packed for seg in per]
    tab = table.cpu().view(len(flat), words)
    off = {name: getattr(_native.RoutedPackedEntry, name).offset for name in ("codebook", "bias", "waves", "steps")}
    raw = tab.numpy().view("uint8").reshape(len(flat), words * 8)
    for i, (pk, cb, _, bias) in enumerate(flat):
        cbp = int(raw[i, off["codebook"]:off["codebook"] + 8].view("uint64")[0])
        waves, steps = (int(raw[i, off[n]:off[n] + 4].view("int32")[0]) for n in ("waves", "steps"))
        assert (waves, steps) == (int(pk.desc.waves), int(pk.desc.steps)), (what, i)
        assert int(raw[i, off["bias"]:off["bias"] + 8].view("uint64")[0]) == (0 if bias is None else bias.data_ptr()), (what, i)
        lo, hi = pk.data_ptr(), pk.data_ptr() + pk.buf.numel()
        if pk.desc.relabelled:
            assert lo < cbp and cbp + 65536 * g * 2 <= hi, f"{what} entry {i}: a relabelled entry's codebook must be the image in its buffer"
        else:
            assert cbp == cb.data_ptr(), f"{what} entry {i}: an entry with the checkpoint's labels reads the live codebook"
    assert tail[1] == max(int(pk.desc.waves) for pk, _, _, _ in flat), (what, tail)


def _check_launch(y, x, ids, layers, packed, per_pair, dtype, what, oracle_pairs, bits_stride=1):
    """(a) - (d) of one launch.  ``oracle_pairs``: the pairs checked against fp64; ``bits_stride``: every n-th pair (and the oracle
    pairs) is compared with the single-layer kernel."""
    from aqlm_amd.inference_kernels import hip_kernel as hk

    E, S, k = len(packed), len(packed[0]), ids.shape[1]
    assert tuple(y.shape) == (ids.numel(), S, packed[0][0][0].out_features)
    assert _cells_at_rest(), f"{what}: cells not zero after the launch"
    seen = 0
    for p, e in enumerate(ids.long().cpu().view(-1).tolist()):
        if not 0 <= e < E:
            assert torch.count_nonzero(y[p]) == 0, f"{what} pair {p} id {e}: rows of a pair without an expert must be zero"
            continue
        if p % bits_stride and p not in oracle_pairs:
            continue
        xr = x[p if per_pair else p // k]
        for s in range(S):
            pk, cb, sc, bias = packed[e][s]
            tag = f"{what} pair {p} expert {e} seg {s}"
            ref = hk.code1x16_matmat_packed(xr.view(1, -1), pk, cb, sc, bias)
            assert torch.equal(y[p, s].view(1, -1), ref), f"{tag}: not bit-identical to aqlm_hip_gemv_1x16_packed at batch 1"
            if p in oracle_pairs:
                check_close(y[p, s].float().cpu().numpy(), _oracle64(layers[e][s], xr), dtype, tag)
                seen += 1
    return seen


def _ids(T, k, E, gen, dev, dtype=torch.int64):
    return mx.router_ids(T, k, E, gen, dev, dtype)


def _with_hostile(ids, E):
    """Every third id replaced by one outside [0, E): -1, E, 2^40 (int64) ..."""
    bad = [-1, E, E + 7, -(2 ** 31)] + ([2 ** 40, -(2 ** 40)] if ids.dtype == torch.int64 else [2 ** 31 - 1])
    out = ids.clone()
    flat = out.view(-1)
    sel = torch.arange(flat.numel(), device=ids.device)[1::3]
    flat[sel] = torch.tensor(bad, dtype=ids.dtype, device=ids.device)[torch.arange(sel.numel(), device=ids.device) % len(bad)]
    return out


def _table(recipes, seed, S, fin, fout, g, dtype, dev, what, bias=False):
    from aqlm_amd.inference_kernels import hip_kernel as hk

    per = recipes if isinstance(recipes[0], list) else [[r] * S for r in recipes]
    layers, packed, plans = mx.build_experts(per, seed, S, fin, fout, g, dtype, dev, bias=bias)
    _check_descs(packed, plans, per, what)
    assert hk.routed_packed_supported([p[0] for row in packed for p in row]), what
    table, tail = hk.routed_packed_table(packed, dev)
    _check_table(table, tail, packed, g, what)
    return layers, packed, table, tail


def _x(rows, fin, gen, dev, dtype):
    return torch.randn((rows, fin), generator=gen, device=dev).to(dtype)


# ---------------------------------------------------------------------------------------------------------------------------
# all entries relabelled / all labels kept
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("g", [8, 16])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", mx.SMALL_SHAPES, ids=[s[0] for s in mx.SMALL_SHAPES])
@pytest.mark.parametrize("relabel", [True, False], ids=["relabelled", "kept"])
def test_zipf_experts_with_labels_dealt_out_or_kept(relabel, shape, dtype, g):
    """Zipf 0.8 / 1.2 experts, labels sorted by use or shuffled.  ``relabel=True``: every entry reads the codebook image of its
    own buffer (asserted from the descriptor and from the table).  ``relabel=False``: the same experts with the checkpoint's labels
    -- long streams (14 waves x 5 steps for Zipf 1.2 sorted) next to short ones in one table."""
    name, S, fin, fout, per_pair = shape
    dev = torch.device("cuda:0")
    what = f"zipf {'relabelled' if relabel else 'kept'} {name} g{g} {dtype}"
    recipes = mx.zipf_table(relabel)
    layers, packed, table, tail = _table(recipes, mx.SEED_SMALL, S, fin, fout, g, dtype, dev, what)
    E = len(recipes)
    for e, per in enumerate(packed):
        for pk, _, _, _ in per:
            # g8: every entry, as the model says.  g16 has no model: the device's word -- 32 slices of 2048 entries; shuffled
            # labels already spread a Zipf law evenly enough over them that the repack may keep them, labels sorted by use never do
            if g == 8 or not relabel or recipes[e].b:
                assert bool(pk.desc.relabelled) == relabel, f"{what} expert {e}"
    if relabel:  # (the table check above holds every relabelled entry's codebook pointer inside its own packed buffer)
        assert sum(bool(pk.desc.relabelled) for per in packed for pk, _, _, _ in per) >= (E * S if g == 8 else E * S // 2), what
    gen = torch.Generator(device=dev).manual_seed(41)
    for T, k in [(1, 1), (1, 2), (5, 2), (16, 4)]:
        rnd = _ids(T, k, E, gen, dev)
        for rname, ids in (("router", rnd), ("one_expert", torch.full((T, k), 2, dtype=torch.int32, device=dev)),
                           ("hostile", _with_hostile(rnd, E))):
            x = _x(T * k if per_pair else T, fin, gen, dev, dtype)
            y = _launch(x, ids, table, tail, E, S, fout, fin, g, per_pair)
            _check_launch(y, x, ids, layers, packed, per_pair, dtype, f"{what} T{T} k{k} {rname}", oracle_pairs=range(4))


# ---------------------------------------------------------------------------------------------------------------------------
# one table, entries of every kind
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_mixed_table_of_wave_counts_steps_and_codebook_kinds(dtype):
    """uniform | Zipf 1.2 kept | Zipf 1.2 relabelled | row-block relabelled | row-block kept | Zipf 0.8 relabelled, the second
    segment of every expert three recipes on: wave counts 5 .. 14, steps 1 .. 5, both codebook kinds in one launch whose block
    size is the largest wave count.  Routings put several pairs on the entry with the fewest waves and on the one with the most."""
    dev, g, S, fin, fout = torch.device("cuda:0"), 8, 2, 1024, 2048
    what = f"mixed {dtype}"
    recipes = mx.segment_recipes(mx.MIXED, S)
    layers, packed, table, tail = _table(recipes, mx.SEED_MIXED, S, fin, fout, g, dtype, dev, what)
    E = len(recipes)
    descs = [[pk.desc for pk, _, _, _ in per] for per in packed]
    waves = [int(d.waves) for per in descs for d in per]
    assert len(set(waves)) >= 3 and tail[1] == max(waves) and min(waves) < tail[1], (waves, tail)
    assert any(d.relabelled for per in descs for d in per) and not all(d.relabelled for per in descs for d in per)
    assert any(int(per[0].waves) != int(per[1].waves) for per in descs), "no expert whose two segments differ in waves"
    small = min(range(E), key=lambda e: min(int(d.waves) for d in descs[e]))
    large = max(range(E), key=lambda e: min(int(d.waves) for d in descs[e]))
    assert int(descs[small][0].waves) < int(descs[large][0].waves) == tail[1]
    gen = torch.Generator(device=dev).manual_seed(42)
    both = _ids(16, 2, E, gen, dev)
    both[:6, 0], both[:6, 1] = small, large  # six pairs each on the fewest-waves and the most-waves expert, the rest as routed
    routings = {"small_and_large": both, "hostile": _with_hostile(both, E).to(torch.int32), "router_T32": _ids(32, 2, E, gen, dev),
                "all_on_large": torch.full((32, 2), large, dtype=torch.int64, device=dev),
                "all_on_small": torch.full((7, 1), small, dtype=torch.int64, device=dev), "k4": _ids(9, 4, E, gen, dev)}
    for rname, ids in routings.items():
        x = _x(ids.shape[0], fin, gen, dev, dtype)
        y = _launch(x, ids, table, tail, E, S, fout, fin, g, False)
        _check_launch(y, x, ids, layers, packed, False, dtype, f"{what} {rname}", oracle_pairs=range(6))


# ---------------------------------------------------------------------------------------------------------------------------
# full size
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", mx.FULL_SHAPES, ids=[s[0] for s in mx.FULL_SHAPES])
def test_full_size_table_with_four_mask_words(shape):
    """Mixtral's projections (4096 -> 14336 twice, 14336 -> 4096): uniform experts, Zipf 1.2 sorted with the labels kept (16 waves
    x 104 steps by the model: four mask words per lane column), and relabelled experts (16 x 23, 14 x 9) in one table."""
    name, S, fin, fout, per_pair = shape
    dev, g, dtype = torch.device("cuda:0"), 8, torch.float16
    what = f"full {name}"
    recipes = mx.segment_recipes(mx.FULL_MIX, S)
    layers, packed, table, tail = _table(recipes, mx.SEED_FULL, S, fin, fout, g, dtype, dev, what)
    E = len(recipes)
    descs = [pk.desc for per in packed for pk, _, _, _ in per]
    assert max(int(d.steps) for d in descs) > 96, "no entry with more than three mask words"
    assert min(int(d.steps) for d in descs) <= 32 and any(d.relabelled for d in descs) and not all(d.relabelled for d in descs)
    gen = torch.Generator(device=dev).manual_seed(43)
    ids = _ids(32, 2, E, gen, dev)  # 64 pairs
    flat = ids.view(-1).tolist()
    one_per_recipe = [flat.index(e) for e in range(E)]
    x = _x(64 if per_pair else 32, fin, gen, dev, dtype)
    y = _launch(x, ids, table, tail, E, S, fout, fin, g, per_pair)
    assert _check_launch(y, x, ids, layers, packed, per_pair, dtype, f"{what} 64 pairs", one_per_recipe, bits_stride=9) == E * S
    ids = _with_hostile(_ids(3, 2, E, gen, dev), E)
    x = _x(6 if per_pair else 3, fin, gen, dev, dtype)
    y = _launch(x, ids, table, tail, E, S, fout, fin, g, per_pair)
    _check_launch(y, x, ids, layers, packed, per_pair, dtype, f"{what} 6 pairs, hostile ids", oracle_pairs=())


# ---------------------------------------------------------------------------------------------------------------------------
# slice-first instantiation (g8)
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_slice_first_instantiation_on_a_tall_layer(dtype):
    """256 -> 57344: 3584 rows per row group, whose tables no longer fit next to the full x window, so the launch takes
    gemv_1x16_packed_routed_kernel<..., 0u> (asserted from the geometry tail, not assumed).  Three experts, one relabelled."""
    from aqlm_amd.inference_kernels import hip_kernel as hk

    dev, g, S = torch.device("cuda:0"), 8, 1
    fin, fout = mx.SLICE_FIRST_SHAPE
    what = f"slice-first {dtype}"
    layers, packed, table, tail = _table(mx.SLICE_FIRST, mx.SEED_SLICE_FIRST, S, fin, fout, g, dtype, dev, what)
    assert tail[2] == 1, f"{fin} -> {fout} is not slice-first for the routed packed launch: {tail}"
    assert any(pk.desc.relabelled for (pk, _, _, _), in packed) and not all(pk.desc.relabelled for (pk, _, _, _), in packed)
    assert 0 < tail[3] <= 160 * 1024 and tail[3] == hk._lib.aqlm_hip_gemv_1x16_routed_packed_lds_bytes(fout, fin, g)
    E = len(packed)
    gen = torch.Generator(device=dev).manual_seed(44)
    for rname, ids, per_pair in (("router", _ids(4, 2, E, gen, dev), False), ("pair_rows", _ids(3, 3, E, gen, dev), True),
                                 ("hostile", _with_hostile(_ids(4, 2, E, gen, dev), E), False)):
        x = _x(ids.numel() if per_pair else ids.shape[0], fin, gen, dev, dtype)
        y = _launch(x, ids, table, tail, E, S, fout, fin, g, per_pair)
        _check_launch(y, x, ids, layers, packed, per_pair, dtype, f"{what} {rname}", oracle_pairs=range(3))


# ---------------------------------------------------------------------------------------------------------------------------
# bias, ragged row groups, fewer rows than row groups, 65 input groups
# ---------------------------------------------------------------------------------------------------------------------------
RAGGED = [("out1000", 2, 1024, 1000, False), ("out37", 1, 520, 37, True), ("in520", 2, 520, 1000, False)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", RAGGED, ids=[s[0] for s in RAGGED])
def test_bias_and_ragged_shapes(shape, dtype):
    """A bias per expert and projection (the entry's ``bias`` pointer, null in every other MoE test); out_features = 1000: the
    last row group is short; 37: fewer rows than row groups (empty groups, and the zero rows of orphan pairs written with
    ``nrows = min(RG, M - row0)``); in_features = 520: 65 input groups, which the routed launch on the canonical codes declines."""
    from aqlm_amd.inference_kernels import hip_kernel as hk

    name, S, fin, fout, per_pair = shape
    dev, g = torch.device("cuda:0"), 8
    what = f"{name} {dtype}"
    recipes = mx.segment_recipes(mx.MIXED, S)[:4]
    layers, packed, table, tail = _table(recipes, 35, S, fin, fout, g, dtype, dev, what, bias=True)
    E = len(recipes)
    assert all(seg[3] is not None for per in packed for seg in per)
    gen = torch.Generator(device=dev).manual_seed(45)
    if fin == 520:
        ids = _ids(2, 2, E, gen, dev)
        with pytest.raises((NotImplementedError, ValueError)):
            torch.ops.aqlm.code1x16_moe_matmat(_x(2, fin, gen, dev, dtype), ids, hk.routed_table(layers, dev), [E, S, fout, fin, g, 2], False)
    for T, k in [(1, 1), (3, 2), (16, 4)]:
        rnd = _ids(T, k, E, gen, dev)
        for rname, ids in (("router", rnd), ("hostile", _with_hostile(rnd, E))):
            x = _x(T * k if per_pair else T, fin, gen, dev, dtype)
            y = _launch(x, ids, table, tail, E, S, fout, fin, g, per_pair)
            _check_launch(y, x, ids, layers, packed, per_pair, dtype, f"{what} T{T} k{k} {rname}", oracle_pairs=range(4))
    # x = 0: the bias alone, bit for bit
    ids = _ids(2, 2, E, gen, dev)
    y = _launch(torch.zeros((4 if per_pair else 2, fin), dtype=dtype, device=dev), ids, table, tail, E, S, fout, fin, g, per_pair)
    for p, e in enumerate(ids.view(-1).tolist()):
        for s in range(S):
            assert torch.equal(y[p, s], packed[e][s][3]), (what, p, e, s)
    assert _cells_at_rest()


# ---------------------------------------------------------------------------------------------------------------------------
# expert count, top_k, id type
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ids_dtype", [torch.int64, torch.int32])
@pytest.mark.parametrize("E", [1, 3, 60])
def test_expert_count_and_top_k(E, ids_dtype):
    """1, 3 and 60 experts (the ids E - 1 and E both present: the last expert and the first orphan), top_k 1 / 2 / 4 / 8 up to
    exactly 64 pairs, int64 ids on fp16 experts and int32 ids on bf16 experts.  Beyond one round of the recipes the experts keep
    their labels: the model's label deal takes about a second per layer in numpy, its other decisions are checked for all 120."""
    dev, g, S, fin, fout = torch.device("cuda:0"), 8, 2, 1024, 512
    dtype = torch.float16 if ids_dtype == torch.int64 else torch.bfloat16
    what = f"E{E} {ids_dtype}"
    recipes = [[mx.MIXED[(e + 3 * s) % len(mx.MIXED)] for s in range(S)] for e in range(E)]
    if E > 6:
        recipes = recipes[:6] + [[r._replace(relabel=False) if r.kind != "uniform" else r for r in per] for per in recipes[6:]]
    layers, packed, table, tail = _table(recipes, 36, S, fin, fout, g, dtype, dev, what)
    gen = torch.Generator(device=dev).manual_seed(46)
    for k in (1, 2, 4, 8):
        for T in (64 // k, 3):
            ids = _ids(T, k, E, gen, dev, ids_dtype)
            flat = ids.view(-1)
            flat[0] = E - 1
            if flat.numel() > 1:
                flat[1] = E
            if flat.numel() > 2:
                flat[2] = -1
            x = _x(T, fin, gen, dev, dtype)
            y = _launch(x, ids, table, tail, E, S, fout, fin, g, False)
            _check_launch(y, x, ids, layers, packed, False, dtype, f"{what} T{T} k{k}", oracle_pairs=(0, 3, 4), bits_stride=1 if T == 3 else 3)


# ---------------------------------------------------------------------------------------------------------------------------
# strided x
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", mx.SMALL_SHAPES, ids=[s[0] for s in mx.SMALL_SHAPES])
def test_x_rows_taken_from_a_wider_tensor(shape, dtype):
    """Token rows and pair rows as a column slice of a wider tensor: the row stride exceeds in_features (16-byte aligned rows are
    launched as they are, not copied)."""
    name, S, fin, fout, per_pair = shape
    dev, g = torch.device("cuda:0"), 8
    what = f"strided {name} {dtype}"
    recipes = [mx.uniform(), mx.zipf(1.2, True, False), mx.rowblock(0.9, True)]
    layers, packed, table, tail = _table(recipes, 37, S, fin, fout, g, dtype, dev, what)
    E = len(recipes)
    gen = torch.Generator(device=dev).manual_seed(47)
    for T, k in [(1, 2), (6, 2), (16, 4)]:
        ids = _with_hostile(_ids(T, k, E, gen, dev), E)
        rows = T * k if per_pair else T
        x = mx.strided_rows(rows, fin, gen, dev, dtype)
        y = _launch(x, ids, table, tail, E, S, fout, fin, g, per_pair)
        _check_launch(y, x, ids, layers, packed, per_pair, dtype, f"{what} T{T} k{k}", oracle_pairs=range(3))
        assert torch.equal(y, _launch(x.contiguous(), ids, table, tail, E, S, fout, fin, g, per_pair)), what


# ---------------------------------------------------------------------------------------------------------------------------
# magnitudes and non-finite rows
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_per_pair_magnitudes_and_non_finite_rows_in_one_launch(dtype):
    """The fixed-point unit of the fused finalize comes from max |x| of each pass: three pairs of ONE expert with x rows scaled by
    2^-10, 1 and 2^6 each meet the oracle on their own scale.  Then a NaN and a +Inf in two pairs of an expert that also serves
    clean pairs: NaN rows / non-finite rows for those two, every other pair bit-identical to the clean launch, cells at rest
    (non-finite values are ordinary data to these kernels; the single-layer kernel is held to the same in test_hip_parity.py)."""
    dev, g, S, fin, fout = torch.device("cuda:0"), 8, 2, 1024, 2048
    what = f"magnitudes {dtype}"
    recipes = [mx.zipf(1.2, True, True), mx.uniform(), mx.zipf(1.2, True, False)]
    layers, packed, table, tail = _table(recipes, 38, S, fin, fout, g, dtype, dev, what)
    E = len(recipes)
    gen = torch.Generator(device=dev).manual_seed(48)
    for e in range(E):
        ids = torch.tensor([[e], [e], [e], [(e + 1) % E], [(e + 2) % E]], device=dev)
        x = _x(5, fin, gen, dev, dtype)
        x[0] *= 2.0 ** -10
        x[2] *= 2.0 ** 6
        y = _launch(x, ids, table, tail, E, S, fout, fin, g, False)
        assert _check_launch(y, x, ids, layers, packed, False, dtype, f"{what} expert {e}", oracle_pairs=range(5)) == 5 * S
    for e in range(E):
        ids = torch.tensor([[e], [e], [e], [(e + 1) % E], [e], [(e + 2) % E]], device=dev)
        x = _x(6, fin, gen, dev, dtype)
        clean = _launch(x, ids, table, tail, E, S, fout, fin, g, False)
        xn = x.clone()
        xn[1, 17] = float("nan")
        xn[2, 1000] = float("inf")
        yn = _launch(xn, ids, table, tail, E, S, fout, fin, g, False)
        assert _cells_at_rest(), f"{what} expert {e}: cells not zero after non-finite rows"
        assert torch.isnan(yn[1]).all(), f"{what} expert {e}: the NaN pair's rows must be NaN"
        assert not torch.isfinite(yn[2]).any(), f"{what} expert {e}: the Inf pair's rows must be non-finite"
        keep = [0, 3, 4, 5]
        assert torch.equal(yn[keep], clean[keep]), f"{what} expert {e}: a non-finite pair changed another pair's bits"
        assert torch.equal(_launch(x, ids, table, tail, E, S, fout, fin, g, False), clean)
        assert _cells_at_rest()


# ---------------------------------------------------------------------------------------------------------------------------
# prepack_experts(relabel=True) at module level
# ---------------------------------------------------------------------------------------------------------------------------
def _skewed_module(dtype, dev, seed=0):
    """``_module(1024, 2048)`` of tests/test_moe_gpu.py whose experts carry Zipf / row-correlated codes (same seed: same weights)."""
    cfg, q, _ = _module(1024, 2048, dtype, dev, seed=seed)
    with torch.no_grad():
        for e in range(MODULE_E):
            for j, name in enumerate(("w1", "w3", "w2")):
                lin = getattr(q.expert(e), name)
                recipe, seed_codes = mx.module_layer(e, j)
                cu = mx.recipe_codes(recipe, lin.codes.shape[0], lin.codes.shape[1], seed_codes)
                lin.codes.copy_(torch.from_numpy(cu.astype("uint16").view("int16").reshape(tuple(lin.codes.shape))))
    return cfg, q


def _relabelled_module(monkeypatch, dtype, dev, seed=0):
    import aqlm_amd.moe as moe

    cfg, q = _skewed_module(dtype, dev, seed)
    monkeypatch.setattr(moe, "ROUTED_PACKED_MAX_PAIRS", 64)
    rep = moe.prepack_experts(q, min_codes=1, relabel=True)
    assert rep["blocks"] == 1 and rep["layers_packed"] == 3 * MODULE_E and rep["layers_skipped"] == 0, rep
    assert rep["blocks_served"] == 1 and rep["blocks_fallback"] == 0 and rep["packed_bytes"] > 0, rep
    for lin in q._expert_layers():
        d = lin._packed_codes.desc
        assert d.relabelled and not d.variable_geometry, "a skewed expert layer kept its labels under relabel=True"
    return cfg, q


def _block_tol(dtype):
    return 2e-3 if dtype == torch.float16 else 1.6e-2


@pytest.mark.parametrize("dtype", DTYPES)
def test_block_forward_after_prepack_experts_with_relabelling(monkeypatch, dtype):
    """tests/test_moe_packed_gpu.py::test_block_forward_after_prepack_experts on relabelled skewed experts: the report, the
    forward within the block tolerance of the unprepacked twin, both projection launches bit for bit against the per-expert loop
    on the prepacked layers."""
    from aqlm_amd.inference_kernels import hip_kernel as hk

    dev = torch.device("cuda:0")
    _, plain = _skewed_module(dtype, dev)
    _, q = _relabelled_module(monkeypatch, dtype, dev)
    gen = torch.Generator(device=dev).manual_seed(3)
    real = torch.ops.aqlm.code1x16_moe_matmat_packed
    for T in (1, 2, 4, 16, 32):
        x = _x(T, 1024, gen, dev, dtype)
        ids, w = _route(T, 2, gen, dev)
        with torch.no_grad():
            tables = q._routed_packed_tables_for(x, ids)
            assert tables is not None, T
            y, y_plain = q(x, ids, w).double(), plain(x, ids, w).double()
            rel = ((y - y_plain).abs().mean() / y_plain.abs().mean()).item()
            assert rel < _block_tol(dtype), (T, rel)
            (tab13, tail13), (tab2, tail2) = tables
            gu = real(x, ids, tab13, [MODULE_E, 2, 2048, 1024, 8, 2] + tail13, False)
            h = q.act_fn(gu[:, 0]) * gu[:, 1]
            y2 = real(h, ids, tab2, [MODULE_E, 1, 1024, 2048, 8, 2] + tail2, True)
            for p, e in enumerate(ids.view(-1).cpu().tolist()):
                ex = q.expert(e)
                for s, lin in enumerate((ex.w1, ex.w3)):
                    ref = hk.code1x16_matmat_packed(x[p // 2].view(1, -1), lin._packed_codes, lin.codebooks, lin.scales, None)
                    assert torch.equal(gu[p, s].view(1, -1), ref), (T, p, e, s)
                ref = hk.code1x16_matmat_packed(h[p].view(1, -1), ex.w2._packed_codes, ex.w2.codebooks, ex.w2.scales, None)
                assert torch.equal(y2[p, 0].view(1, -1), ref), (T, p, e)
    assert _cells_at_rest()


def test_kept_labels_on_skewed_experts_fall_back_and_say_so(monkeypatch):
    """``prepack_experts()`` as it ships (``relabel=False``) on the same skewed experts: the repack declines the layers whose
    streams, with the checkpoint's labels, exceed the capacity it is given (Zipf 1.2 with sorted labels: 14 waves x 5 steps where
    balanced streams take 6 x 1), the report says so, and the block keeps the routed launch on the canonical codes, bit for bit."""
    import warnings

    import aqlm_amd.moe as moe

    dev, dtype = torch.device("cuda:0"), torch.float16
    _, plain = _skewed_module(dtype, dev, seed=9)
    _, q = _skewed_module(dtype, dev, seed=9)
    monkeypatch.setattr(moe, "ROUTED_PACKED_MAX_PAIRS", 64)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)  # "cannot take the prepacked matvec", once per shape
        rep = moe.prepack_experts(q, min_codes=1)
    assert rep["layers_skipped"] > 0 and rep["layers_packed"] + rep["layers_skipped"] == 3 * MODULE_E, rep
    assert (rep["blocks"], rep["blocks_served"], rep["blocks_fallback"]) == (1, 0, 1), rep
    assert all(lin._packed_codes is None or not lin._packed_codes.desc.relabelled for lin in q._expert_layers())
    gen = torch.Generator(device=dev).manual_seed(10)
    for T in (1, 4, 32):
        x = _x(T, 1024, gen, dev, dtype)
        ids, w = _route(T, 2, gen, dev)
        with torch.no_grad():
            assert q._routed_packed_tables_for(x, ids) is None and q.takes_routed_path(x, ids)
            assert torch.equal(q(x, ids, w), plain(x, ids, w)), T


def test_a_rewritten_codebook_behind_a_codebook_image(monkeypatch):
    """Staleness as the ``prepack_experts`` docstring states it for ``relabel=True`` (the kernels read a derived codebook image):
    a versioned in-place write and a ``.data`` write followed by ``invalidate_derived_state()`` are served correctly by the very
    next forward; a ``.data`` write alone at the latest after one full round of the periodic check
    (``inference.DERIVED_CHECK_EVERY`` eager forwards).  Correct: within the block tolerance of a never-prepacked twin given the
    same write; a doubled codebook moves the output by more than 1e-2."""
    import aqlm_amd.inference as inf

    dev, dtype = torch.device("cuda:0"), torch.float16
    every = 3 * MODULE_E  # one layer per eager forward
    monkeypatch.setattr(inf, "DERIVED_CHECK_EVERY", every)
    _, q = _relabelled_module(monkeypatch, dtype, dev, seed=7)
    _, fresh = _skewed_module(dtype, dev, seed=7)
    gen = torch.Generator(device=dev).manual_seed(8)
    x = _x(2, 1024, gen, dev, dtype)
    ids = torch.tensor([[0, 3], [3, 5]], device=dev)
    w = torch.full((2, 2), 0.5, device=dev)

    def agree(what):
        with torch.no_grad():
            assert q._routed_packed_tables_for(x, ids) is not None, what
            y, ref = q(x, ids, w).double(), fresh(x, ids, w).double()
        rel = ((y - ref).abs().mean() / ref.abs().mean()).item()
        assert rel < 2e-3, (what, rel)
        return y

    def moved(a, b):
        return ((a - b).abs().mean() / b.abs().mean()).item()

    y0 = agree("before")
    with torch.no_grad():
        for blk in (q, fresh):
            blk.expert(0).w2.codebooks.mul_(2)  # versioned: image and table are rebuilt by the next forward
    table_before = q._packed_tables
    y1 = agree("codebook written in place")
    assert q._packed_tables is not table_before and q.expert(0).w2._packed_codes.desc.relabelled
    assert moved(y1, y0) > 1e-2, "the doubled codebook should change the output"
    for blk in (q, fresh):
        blk.expert(3).w1.codebooks.data.mul_(2)  # neither identity nor version changes ...
    q.expert(3).w1.invalidate_derived_state()  # ... said by hand
    y2 = agree("codebook written through .data, then invalidate_derived_state()")
    assert moved(y2, y1) > 1e-2, "the doubled codebook should change the output"
    assert q.expert(3).w1._packed_codes.desc.relabelled
    for blk in (q, fresh):
        blk.expert(5).w3.codebooks.data.mul_(2)  # ... and not said at all: the periodic check finds it
    with torch.no_grad():
        for _ in range(every):
            q(x, ids, w)
    y3 = agree("codebook written through .data, one round of the periodic check later")
    assert moved(y3, y2) > 1e-2, "the doubled codebook should change the output"
    assert _cells_at_rest()


def test_relabelled_block_decode_step_replays_from_a_graph(monkeypatch):
    """A T = 4 decode step of a MixtralSparseMoeBlock on relabelled skewed experts, captured once and replayed on three inputs that
    route differently: every replay equals eager bit for bit, the cells are at rest."""
    from transformers.models.mixtral.modeling_mixtral import MixtralSparseMoeBlock

    dev, T = torch.device("cuda:0"), 4
    cfg, q = _relabelled_module(monkeypatch, torch.float16, dev, seed=5)
    block = MixtralSparseMoeBlock(cfg).to(dev, torch.float16).eval()
    with torch.no_grad():
        block.gate.weight.normal_(0, 0.5)
    block.experts = q
    taken = []
    real = q._forward_routed_packed
    monkeypatch.setattr(q, "_forward_routed_packed", lambda *a: (taken.append(1), real(*a))[1])
    gen = torch.Generator(device=dev).manual_seed(6)
    inputs = [torch.randn((1, T, 1024), generator=gen, device=dev).half() for _ in range(3)]
    static = inputs[0].clone()
    with torch.no_grad():
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(2):
                block(static)
        torch.cuda.current_stream().wait_stream(s)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = block(static)
        assert len(taken) == 3, "the captured step did not take the routed packed launches"
        routes = set()
        for x in inputs:
            static.copy_(x)
            graph.replay()
            eager = block(x)
            torch.cuda.synchronize()
            assert torch.equal(out, eager)
            routes.add(tuple(block.gate(x.view(-1, 1024))[2].view(-1).tolist()))
    assert len(routes) == 3, "the three inputs should route differently"
    assert _cells_at_rest()
