"""Expert tables for the MoE tests that leave the track of ``tests/test_moe_gpu.py::_experts`` (8 experts, uniform codes, no
bias): any number of experts, a code recipe per (expert, segment) -- uniform, Zipf, row-correlated --, labels kept or dealt out by
the repack, an optional bias per layer.  Test infrastructure only.

The routed packed launch is parameterised per table entry by what the repack decided for that expert's codes (``waves``,
``steps``, live codebook or the permuted image inside the packed buffer), so the tables built here come with the decision the
numpy model of the format (``tests/packed_model.py``, g8) predicts for every layer: relabelled or not, NW, T.  The CPU test
``tests/test_moe_skewed_model.py`` holds the recipes to the properties the GPU tests rely on; the GPU tests hold the device to
the prediction."""
from collections import namedtuple

import numpy as np

from tests import packed_model as pm

Recipe = namedtuple("Recipe", "kind a b relabel")  # kind: uniform | zipf (a = alpha, b = labels sorted by use) | rowblock (a = p)


def uniform(relabel=True):
    return Recipe("uniform", 0.0, False, bool(relabel))


def zipf(alpha, sorted_labels, relabel):
    return Recipe("zipf", float(alpha), bool(sorted_labels), bool(relabel))


def rowblock(p, relabel):
    return Recipe("rowblock", float(p), False, bool(relabel))


# the tables of tests/test_moe_packed_skewed_gpu.py (g8 predictions are checked on the CPU in tests/test_moe_skewed_model.py)
SMALL_SHAPES = [("w13", 2, 1024, 2048, False), ("w2", 1, 2048, 1024, True)]  # name, segments, in, out, x rows per pair
FULL_SHAPES = [("w13", 2, 4096, 14336, False), ("w2", 1, 14336, 4096, True)]
ZIPF4 = [(0.8, True), (0.8, False), (1.2, True), (1.2, False)]
MIXED = [uniform(), zipf(1.2, True, False), zipf(1.2, True, True), rowblock(0.9, True), rowblock(0.9, False), zipf(0.8, True, True)]
FULL_MIX = [uniform(), zipf(1.2, True, False), zipf(1.2, True, True), zipf(0.8, True, True)]
SLICE_FIRST_SHAPE = (256, 57344)  # in -> out: a row group's tables no longer fit next to the full x window
SLICE_FIRST = [uniform(), zipf(1.2, True, True), zipf(0.8, False, False)]
SEED_SMALL, SEED_MIXED, SEED_FULL, SEED_SLICE_FIRST = 31, 32, 33, 34


# the experts of the module-level tests (prepack_experts(relabel=True)): every layer skewed
MODULE_RECIPES = [zipf(0.8, True, True), zipf(1.2, True, True), rowblock(0.9, True), zipf(1.2, False, True)]
SEED_MODULE = 50


def module_layer(e, j):
    """-> (recipe, code seed) of projection j (w1, w3, w2) of expert e of the module-level tests."""
    return MODULE_RECIPES[(e + j) % len(MODULE_RECIPES)], code_seed(SEED_MODULE + j, e, 0)


def zipf_table(relabel):
    return [zipf(a, s, relabel) for a, s in ZIPF4]


def segment_recipes(recipes, S):
    """A recipe per expert -> a recipe per (expert, segment): segment s of expert e takes recipe (e + 3 s) of the list, so the two
    projections of one expert differ wherever the list is not constant."""
    return [[recipes[(e + 3 * s) % len(recipes)] for s in range(S)] for e in range(len(recipes))]


def code_seed(seed, e, s):
    return seed * 1000 + 2 * e + s


def recipe_codes(recipe, fout, in_groups, seed):
    """-> unsigned codes [fout, in_groups] (int64 in [0, 65536)) of one layer."""
    if recipe.kind == "uniform":
        return np.random.default_rng(seed).integers(0, 65536, size=(fout, in_groups)).astype(np.int64)
    if recipe.kind == "zipf":
        return pm.zipf_codes(fout, in_groups, recipe.a, recipe.b, seed)
    if recipe.kind == "rowblock":
        return pm.rowblock_codes(fout, in_groups, recipe.a, seed)
    raise ValueError(recipe.kind)


def model_plan(codes_unsigned, relabel):
    """What ``prepack_1x16(..., relabel=relabel, uniform_only=True)`` must decide for g8 codes, by the numpy model of the format:
    (relabelled, NW, T)."""
    new = pm.plan_labels(codes_unsigned) if relabel else None
    c = codes_unsigned if new is None else new[codes_unsigned]
    _, a = pm.lane_steps(c)
    longest = int(a[:, -1].max())
    nw = pm.choose_waves(longest)
    return new is not None, nw, (longest + 64 * nw - 1) // (64 * nw)


_PLANS = {}


def predicted_plan(recipe, fout, in_groups, seed, codes_unsigned=None):
    """``model_plan`` of the recipe's codes, remembered per (recipe, shape, seed): the fp16 and bf16 cases of a test share it."""
    key = (recipe, fout, in_groups, seed)
    if key not in _PLANS:
        cu = recipe_codes(recipe, fout, in_groups, seed) if codes_unsigned is None else codes_unsigned
        _PLANS[key] = model_plan(cu, recipe.relabel)
    return _PLANS[key]


def table_plans(recipes, seed, S, fin, fout):
    """The model's plan of every layer of the g8 table ``build_experts`` builds from the same arguments: plans[e][s]."""
    per = recipes if isinstance(recipes[0], list) else [[r] * S for r in recipes]
    return [[predicted_plan(per[e][s], fout, fin // 8, code_seed(seed, e, s)) for s in range(S)] for e in range(len(per))]


ROOMY_EXTRA_BYTES = 256 * 16 * 128 * 1024  # 256 streams x 16 waves x 128 steps (the format's limits) x 1 KiB per step


def pack_layer(codes, g, codebooks, relabel):
    """``hk.prepack_1x16(codes, g, codebooks=codebooks, relabel=relabel, uniform_only=True)``; where that declines the layer, the
    same repack with more room.  ``prepack_1x16`` hands aqlm_hip_prepack_1x16_ex the capacity aqlm_hip_prepack_1x16_bytes asks for,
    which holds streams up to 1.5 x the balanced length: skewed codes whose labels are KEPT (14 waves x 5 steps where balanced
    streams take 6 x 1; 16 x 104 at Mixtral's size) do not fit, and the library leaves such a layer to the direct kernel.  The C
    entry takes any capacity of at least that size, and the buffers it then builds are valid buffers of the format which every
    launch must serve: they are how the long-stream paths (several steps, more than one mask word) are reached here."""
    import ctypes
    import warnings

    import torch

    from aqlm_amd import _native
    from aqlm_amd.inference_kernels import hip_kernel as hk

    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)  # "cannot take the prepacked matvec": expected for kept labels, see above
        pk = hk.prepack_1x16(codes, g, codebooks=codebooks, relabel=relabel, uniform_only=True)
    if pk is not None:
        return pk
    out_features, in_features = codes.shape[0], codes.shape[1] * g
    cap = hk._lib.aqlm_hip_prepack_1x16_bytes(out_features, in_features, g)
    if cap == 0:
        return None
    codes = codes.contiguous()
    scratch = torch.empty((cap + ROOMY_EXTRA_BYTES,), dtype=torch.uint8, device=codes.device)
    desc = _native.PackedDesc()
    flags = (0 if relabel else _native.PREPACK_NO_RELABEL) | _native.PREPACK_UNIFORM_ONLY
    with torch.cuda.device(codes.device):
        rc = hk._lib.aqlm_hip_prepack_1x16_ex(codes.data_ptr(), out_features, in_features, g, scratch.data_ptr(), scratch.numel(),
                                              ctypes.byref(desc), flags, hk._stream_ptr(codes.device))
    if rc == _native.E_UNSUPPORTED:
        return None
    _native.check(rc, "aqlm prepack_1x16 (roomy)")
    pk = hk.PackedCodes(scratch[: int(desc.used_bytes)].clone(), desc)
    pk.set_codebook_range(codebooks)
    return pk


def build_experts(recipes, seed, S, fin, fout, g, dtype, dev, bias=False):
    """``recipes``: one Recipe per expert, or a list of S recipes per expert.  -> (layers, packed, plans):
    ``layers[e][s] = (codes, codebooks, scales, bias or None)`` as ``tests/test_moe_gpu.py::_experts`` builds them,
    ``packed[e][s] = (PackedCodes, codebooks, scales, bias or None)`` with the buffer of ``hk.prepack_1x16(codes, g,
    codebooks=cb, relabel=recipe.relabel, uniform_only=True)`` (``pack_layer``), ``plans[e][s]`` the model's (relabelled, NW, T) at g8, None at
    g16 (the numpy model is g8 only)."""
    import torch

    from aqlm_amd.inference_kernels import hip_kernel as hk

    per = recipes if isinstance(recipes[0], list) else [[r] * S for r in recipes]
    gen = torch.Generator(device=dev).manual_seed(seed)
    layers, packed, plans = [], [], []
    for e, row in enumerate(per):
        assert len(row) == S
        lrow, prow, mrow = [], [], []
        for s, recipe in enumerate(row):
            cs = code_seed(seed, e, s)
            cu = recipe_codes(recipe, fout, fin // g, cs)
            codes = torch.from_numpy(cu.astype(np.uint16).view(np.int16).reshape(fout, fin // g, 1)).to(dev)
            cb = torch.randn((1, 65536, 1, g), generator=gen, device=dev).to(dtype)
            sc = (torch.rand((fout, 1, 1, 1), generator=gen, device=dev) * 0.5 + 0.25).to(dtype)
            b = (torch.randn((fout,), generator=gen, device=dev) * 0.5).to(dtype) if bias else None
            pk = pack_layer(codes, g, cb, recipe.relabel)
            assert pk is not None, f"expert {e} segment {s} ({recipe}) fell off the packed path"
            lrow.append((codes, cb, sc, b))
            prow.append((pk, cb, sc, b))
            mrow.append(predicted_plan(recipe, fout, fin // g, cs, cu) if g == 8 else None)
        layers.append(lrow)
        packed.append(prow)
        plans.append(mrow)
    return layers, packed, plans


def plain_experts(num_experts, seed, S, fin, fout, g, dtype, dev, bias=False):
    """``tests/test_moe_gpu.py::_experts`` (uniform codes, canonical layout only) for any number of experts and with an optional
    bias per layer: ``layers[e][s] = (codes, codebooks, scales, bias or None)``."""
    import torch

    gen = torch.Generator(device=dev).manual_seed(seed)
    layers = []
    for _ in range(num_experts):
        per = []
        for _ in range(S):
            codes = torch.randint(-32768, 32768, (fout, fin // g, 1), generator=gen, device=dev, dtype=torch.int32).to(torch.int16)
            cb = torch.randn((1, 65536, 1, g), generator=gen, device=dev).to(dtype)
            sc = (torch.rand((fout, 1, 1, 1), generator=gen, device=dev) * 0.5 + 0.25).to(dtype)
            b = (torch.randn((fout,), generator=gen, device=dev) * 0.5).to(dtype) if bias else None
            per.append((codes, cb, sc, b))
        layers.append(per)
    return layers


def router_ids(T, k, num_experts, gen, dev, dtype=None):
    """[T, k] ids as a router gives them: distinct experts per token where there are enough, any expert otherwise."""
    import torch

    if k <= num_experts:
        ids = torch.topk(torch.rand((T, num_experts), generator=gen, device=dev), k, dim=-1).indices
    else:
        ids = torch.randint(0, num_experts, (T, k), generator=gen, device=dev)
    return ids if dtype is None else ids.to(dtype)


def strided_rows(rows, fin, gen, dev, dtype):
    """[rows, fin] taken as a column slice of a wider tensor: row stride fin + 24, rows 16-byte aligned, not contiguous."""
    import torch

    x = torch.randn((rows, fin + 24), generator=gen, device=dev).to(dtype)[:, 8:8 + fin]
    assert x.stride(0) == fin + 24 and x.data_ptr() % 16 == 0 and (rows == 1 or not x.is_contiguous())
    return x
