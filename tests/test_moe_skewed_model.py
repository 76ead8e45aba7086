"""The inputs of tests/test_moe_packed_skewed_gpu.py really are the hard ones (CPU, numpy model of the packed format): what the
repack must decide for every recipe / shape those tests use at g8 -- relabelled or not, NW, T -- and the properties they rely on.
A later change of seeds, recipes or shapes that turns the tables back into the uniform case (every entry alike, nothing
relabelled, one mask word) fails here, without a GPU."""
from tests import moe_experts as mx


def _flat(plans):
    return [p for per in plans for p in per]


def test_zipf_tables_are_relabelled_when_allowed_and_long_when_not():
    for name, S, fin, fout, _ in mx.SMALL_SHAPES:
        dealt = _flat(mx.table_plans(mx.zipf_table(True), mx.SEED_SMALL, S, fin, fout))
        kept = _flat(mx.table_plans(mx.zipf_table(False), mx.SEED_SMALL, S, fin, fout))
        assert all(relabelled for relabelled, _, _ in dealt), (name, dealt)
        assert not any(relabelled for relabelled, _, _ in kept), (name, kept)
        assert len({(nw, t) for _, nw, t in dealt}) >= 2, (name, dealt)  # the entries of one table differ
        # labels as the checkpoint has them: long streams (more waves, several steps), and no two recipes alike
        assert max(nw for _, nw, _ in kept) > max(nw for _, nw, _ in dealt), (name, kept, dealt)
        assert max(t for _, _, t in kept) >= 5 and len({(nw, t) for _, nw, t in kept}) >= 3, (name, kept)
        assert sum(nw * t for _, nw, t in kept) > sum(nw * t for _, nw, t in dealt), (name, kept, dealt)


def test_mixed_table_mixes_wave_counts_steps_and_codebook_kinds():
    plans = mx.table_plans(mx.segment_recipes(mx.MIXED, 2), mx.SEED_MIXED, 2, 1024, 2048)
    flat = _flat(plans)
    assert len({nw for _, nw, _ in flat}) >= 3, flat
    assert len({t for _, _, t in flat}) >= 3, flat
    assert any(relabelled for relabelled, _, _ in flat) and not all(relabelled for relabelled, _, _ in flat), flat
    assert any(per[0][1:] != per[1][1:] for per in plans), "no expert whose two segments differ in waves x steps"
    assert min(nw for _, nw, _ in flat) < max(nw for _, nw, _ in flat)  # the launch idles waves of some entry


def test_slice_first_table_holds_both_codebook_kinds():
    fin, fout = mx.SLICE_FIRST_SHAPE
    flat = _flat(mx.table_plans(mx.SLICE_FIRST, mx.SEED_SLICE_FIRST, 1, fin, fout))
    assert any(relabelled for relabelled, _, _ in flat) and not all(relabelled for relabelled, _, _ in flat), flat


def test_full_size_zipf_with_kept_labels_needs_more_than_one_mask_word():
    """One full-size layer (the w1 | w3 shape; tens of seconds for the whole table in numpy): Zipf 1.2 with sorted labels kept as
    they are is the `steps > 32` case of the full-size GPU test (104 steps: four mask words)."""
    name, S, fin, fout, _ = mx.FULL_SHAPES[0]
    e = mx.FULL_MIX.index(mx.zipf(1.2, True, False))
    relabelled, nw, t = mx.predicted_plan(mx.FULL_MIX[e], fout, fin // 8, mx.code_seed(mx.SEED_FULL, e, 0))
    assert not relabelled and t > 32 and nw == 16, (relabelled, nw, t)
    assert mx.segment_recipes(mx.FULL_MIX, S)[e][0] == mx.FULL_MIX[e]  # the layer checked here is a layer of the GPU test's table


def test_module_experts_are_relabelled_in_both_projection_shapes():
    """The experts of the ``prepack_experts(relabel=True)`` tests: one round of the recipes in the hidden -> intermediate shape
    (w1) and in the intermediate -> hidden shape (w2); the device asserts ``desc.relabelled`` for all 24 layers."""
    for e in range(len(mx.MODULE_RECIPES)):
        for j, (fin, fout) in ((0, (1024, 2048)), (2, (2048, 1024))):
            recipe, seed = mx.module_layer(e, j)
            relabelled, nw, t = mx.predicted_plan(recipe, fout, fin // 8, seed)
            assert relabelled, (e, j, recipe, nw, t)
