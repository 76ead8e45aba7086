#!/usr/bin/env python
"""Development-time tool: write tests/golden/code_update_golden.npz, the inputs and expected codes that
tests/test_code_search_host.py holds the torch route of ``aqlm.tuning.find_optimal_codes`` to.

    python tools/gen_code_update_golden.py /path/to/the/reference/checkout

The expected codes come from the reference's own ``beam_search_optimal_codes`` (``src/beam_search_l2.py`` of that checkout) on the
CPU.  Only data goes into the fixture.  The inputs lie on a dyadic grid -- codebook and target values are multiples of 2^-6 with
|k| < 256 (codebooks: |k| < 128, stored as int8), scales are powers of two -- so that every fp32 sum of the search is exact and
the expected codes do not depend on the BLAS of the machine that runs the test.  A seed is discarded when
  * float64 finds an exact tie between candidates of any decision (every top-k of the run, taken with one more candidate, must
    be strictly ascending; for one codebook the best two scores of every group must differ),
  * the fp32 run and the float64 run of the reference disagree anywhere,
  * a trust-ratio threshold lies within 1e-4 (relative) of a cumulative norm, or admits all or only one of the selected changes,
  * a case changes no code or every code.
No test imports this file and it never runs where the reference is absent.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

GRID = 2.0 ** -6
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# name -> (layer, options); layers below
CASES = {
    "a": ("L1", dict(beam_size=1)),
    "b": ("L1", dict(beam_size=1, max_update_fraction=0.1)),
    "c": ("L1", dict(beam_size=1, max_update_fraction=0.1, trust_ratio="auto")),
    "d": ("L2", dict(beam_size=1)),
    "e": ("L2", dict(beam_size=4)),
    "f": ("L3", dict(beam_size=2, dim_order=[2, 0, 3, 1])),
    "g": ("L4", dict(beam_size=2, max_update_fraction=0.5)),
}
# name -> (out_features, in_features, num_codebooks, nbits, out_group_size, in_group_size)
LAYERS = {"L1": (64, 256, 1, 16, 1, 8), "L2": (64, 256, 2, 8, 1, 8), "L3": (32, 256, 4, 8, 1, 16), "L4": (32, 128, 2, 8, 2, 8)}


class _Order:
    """random.Random stand-in whose shuffle installs a given order."""

    def __init__(self, order):
        self.order = list(order)

    def shuffle(self, values):
        values[:] = self.order


def make_layer(shape, seed):
    out_features, in_features, K, nbits, ogs, g = shape
    rng = np.random.default_rng(seed)
    size, og, ig = 2 ** nbits, out_features // ogs, in_features // g
    books = np.clip(np.rint(rng.normal(0, 40, size=(K, size, ogs, g))), -127, 127).astype(np.int8)
    prev = rng.integers(0, size, size=(og, ig, K))
    scale_exp = rng.integers(-1, 2, size=(og,)).astype(np.int8)
    near = rng.integers(0, size, size=(og, ig, K))  # the target sits near other codes than the previous ones for half the groups
    near = np.where(rng.random((og, ig, 1)) < 0.5, prev, near)
    unscaled = sum(books[c].astype(np.int64)[near[..., c]] for c in range(K))  # [og, ig, ogs, g]
    unscaled = unscaled + np.rint(rng.normal(0, 12, size=unscaled.shape)).astype(np.int64)
    half = (scale_exp == -1)[:, None, None, None]
    unscaled = np.where(half, 2 * np.rint(unscaled / 2).astype(np.int64), unscaled)  # times 1/2 stays on the grid
    limit = np.where(scale_exp[:, None, None, None] == 1, 127, np.where(half, 510, 255))
    unscaled = np.clip(unscaled, -limit, limit)
    target = unscaled * (2.0 ** scale_exp.astype(np.float64))[:, None, None, None]
    assert np.all(target == np.rint(target)) and np.abs(target).max() < 256
    target = target.transpose(0, 2, 1, 3).reshape(out_features, in_features).astype(np.int16)
    return {"codebook_k": books, "prev_codes": prev.astype(np.uint16 if nbits == 16 else np.uint8), "scale_exp": scale_exp,
            "reference_k": target}


def tensors(layer, dtype):
    books = torch.from_numpy(layer["codebook_k"].astype(np.float64) * GRID).to(dtype)
    target = torch.from_numpy(layer["reference_k"].astype(np.float64) * GRID).to(dtype)
    scales = torch.from_numpy(2.0 ** layer["scale_exp"].astype(np.float64)).to(dtype).reshape(-1, 1, 1, 1)
    prev = torch.from_numpy(layer["prev_codes"].astype(np.int64))
    return target, books, prev, scales


class Audit:
    """Wraps torch.topk and torch.searchsorted while the reference runs in float64."""

    def __init__(self):
        self.ok, self.cumulative, self.threshold = True, None, None

    def __enter__(self):
        self._topk, self._search = torch.topk, torch.searchsorted

        def topk(input, k, *args, **kwargs):
            kwargs.pop("sorted", None)
            if input.shape[-1] > k:
                wide = self._topk(input, k + 1, *args, sorted=True, **kwargs).values
                if not bool((wide[..., 1:] != wide[..., :-1]).all()):
                    self.ok = False
            return self._topk(input, k, *args, sorted=True, **kwargs)

        def searchsorted(sequence, value, **kwargs):
            self.cumulative, self.threshold = sequence.clone(), float(value)
            return self._search(sequence, value, **kwargs)

        torch.topk, torch.searchsorted = topk, searchsorted
        return self

    def __exit__(self, *exc):
        torch.topk, torch.searchsorted = self._topk, self._search


def run(search, layer, options, dtype):
    target, books, prev, scales = tensors(layer, dtype)
    opts = dict(options)
    order = opts.pop("dim_order", None)
    return search(target, books, prev, scales, dim_rng=None if order is None else _Order(order), **opts)


def one_codebook_is_tie_free(layer):
    target, books, _, scales = tensors(layer, torch.float64)
    K, size, ogs, g = books.shape
    og = scales.shape[0]
    r = (target.reshape(og, ogs, -1, g).permute(0, 2, 1, 3) / scales).flatten(2, 3).flatten(0, 1)
    flat = books[0].flatten(-2, -1)
    scores = flat.square().sum(-1)[None] - 2 * r @ flat.T
    best = scores.topk(2, largest=False).values
    return bool((best[:, 0] != best[:, 1]).all())


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("reference", help="path of the reference checkout (the directory that holds src/beam_search_l2.py)")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "code_update_golden.npz"))
    ap.add_argument("--seed", type=int, default=0, help="first seed tried for every layer")
    args = ap.parse_args()
    os.environ["AQ_USE_JIT"] = "0"  # plain Python functions: the audit wraps torch.topk
    sys.path.insert(0, os.path.abspath(args.reference))
    from src.beam_search_l2 import beam_search_optimal_codes as search

    arrays, meta = {}, {"grid": GRID, "layers": {}, "cases": {}}
    for name, shape in LAYERS.items():
        mine = {c: o for c, (l, o) in CASES.items() if l == name}
        seed = args.seed
        while True:
            layer = make_layer(shape, seed)
            expected, resolved = {}, {}
            good = shape[2] > 1 or one_codebook_is_tie_free(layer)
            for case, options in mine.items():
                if not good:
                    break
                options = dict(options)
                if options.get("trust_ratio") == "auto":
                    with Audit() as probe:  # every selected change admitted: the cumulative norms of all of them
                        run(search, layer, dict(options, trust_ratio=1e9), torch.float64)
                    middle = len(probe.cumulative) // 2
                    w_norm = probe.threshold / 1e9
                    options["trust_ratio"] = float((probe.cumulative[middle] + probe.cumulative[middle + 1]) / 2 / w_norm)
                with Audit() as audit:
                    wide = run(search, layer, options, torch.float64)
                narrow = run(search, layer, options, torch.float32)
                good = audit.ok and bool((wide == narrow).all())
                if good and audit.cumulative is not None:
                    gap = float(((audit.cumulative - audit.threshold).abs() / audit.threshold).min())
                    admitted = 1 + int((audit.cumulative < audit.threshold).sum())
                    good = gap > 1e-4 and 1 < admitted < len(audit.cumulative)
                    options["admitted"] = admitted
                prev = torch.from_numpy(layer["prev_codes"].astype(np.int64))
                share = float((narrow != prev).any(-1).float().mean())
                good = good and 0 < share < 1
                options["changed_share"] = share
                expected[case], resolved[case] = narrow, options
            if good:
                break
            seed += 1
        meta["layers"][name] = {"shape": list(shape), "seed": seed}
        for key, value in layer.items():
            arrays[f"{name}_{key}"] = value
        for case in mine:
            arrays[f"{case}_expected"] = expected[case].numpy().astype(layer["prev_codes"].dtype)
            meta["cases"][case] = {"layer": name, "options": resolved[case]}
            print(case, name, "seed", seed, resolved[case])
    arrays["meta"] = np.array(json.dumps(meta))
    np.savez_compressed(args.out, **arrays)
    print(args.out, os.path.getsize(args.out), "bytes")


if __name__ == "__main__":
    main()
