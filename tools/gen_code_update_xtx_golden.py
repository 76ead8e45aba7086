#!/usr/bin/env python
"""Development-time tool: write tests/golden/code_update_xtx_golden.npz, the inputs and expected codes that
tests/test_code_search_xtx_host.py holds ``aqlm.tuning.find_optimal_codes_calibrated`` to.

    python tools/gen_code_update_xtx_golden.py /path/to/the/reference/checkout

The expected codes come from the reference's own ``beam_search_optimal_codes`` (``src/beam_search_xtx.py`` of that checkout, imported
with AQ_USE_JIT=0) on the CPU.  Only data goes into the fixture, integer-coded (``load`` below is how a reader turns it into tensors;
the test has the same few lines):
  * codebooks: multiples of 2^-6 stored as int8 (the 65536 entries of a 1x16 codebook are the sums hi[s >> 8] + lo[s & 255] of two
    stored tables); scales: powers of two stored as exponents;
  * the target: the scaled sum of the codewords ``near_codes`` plus ``noise_k`` * 2^-6 -- stored as ``near_shift`` = (near_codes - prev_codes) mod the
    codebook size and that int8 noise;
  * XTX = X^T X + 16 I of a small integer calibration matrix X [samples, in], stored as X (int8); every entry of XTX is an integer that
    float32 holds exactly, and the test forms it as float32 values;
  * the expected codes and ``meta``.
A seed is discarded when
  * the float32 run and the float64 run of the reference disagree anywhere,
  * some top-k of the float64 run, taken with one more candidate over all beams x codes of the step, is not strictly ascending or
    has a gap below 2^-18 times the step's largest |score|, on any output group,
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
NEAR = 2.0 ** -18
SAMPLES = 48
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# name -> (out_features, in_features, num_codebooks, nbits, out_group_size, in_group_size)
LAYERS = {"A": (32, 64, 1, 16, 1, 8), "B": (64, 128, 2, 8, 1, 8), "C": (32, 128, 4, 8, 1, 16), "D": (32, 64, 2, 8, 2, 8),
          "E": (32, 256, 8, 8, 1, 32)}
# name -> (layer, beam_size, shuffled)
CASES = {"a": ("A", 1, False), "b1": ("B", 1, False), "b4": ("B", 4, False), "c": ("C", 2, True), "d": ("D", 2, False), "e": ("E", 4, False)}


class _Orders:
    """random.Random stand-in whose shuffle installs the next of the given orders."""

    def __init__(self, orders):
        self.orders = [list(o) for o in orders]

    def shuffle(self, values):
        values[:] = self.orders.pop(0)


def make_layer(shape, seed):
    out_features, in_features, K, nbits, ogs, g = shape
    rng = np.random.default_rng(seed)
    size, og, ig = 2 ** nbits, out_features // ogs, in_features // g
    spread = 1.5 if K >= 8 else 4 if K * size * ogs * g > 4096 else 30  # (the larger tables are most of the file: fewer distinct values there)
    arrays = {}
    if nbits == 16:
        for half in ("hi", "lo"):
            arrays[f"codebook_{half}_k"] = np.clip(np.rint(rng.normal(0, spread, size=(256, ogs, g))), -100, 100).astype(np.int8)
    else:
        arrays["codebook_k"] = np.clip(np.rint(rng.normal(0, spread, size=(K, size, ogs, g))), -100, 100).astype(np.int8)
    prev = rng.integers(0, size, size=(og, ig, K))
    near = rng.integers(0, size, size=(og, ig, K))  # the target sits near other codes than the previous ones for three groups in ten
    near = np.where(rng.random((og, ig, 1)) < 0.7, prev, near)
    dt = np.uint16 if nbits == 16 else np.uint8
    arrays["prev_codes"], arrays["near_shift"] = prev.astype(dt), ((near - prev) % size).astype(dt)
    arrays["noise_k"] = np.clip(np.rint(rng.normal(0, 1.0 if K >= 8 else 1.5, size=(out_features, in_features))), -8, 8).astype(np.int8)
    arrays["scale_exp"] = rng.integers(-1, 2, size=(og,)).astype(np.int8)
    X = np.clip(np.rint(rng.normal(0, 1.0 if K >= 8 else 1.5 if K >= 4 else 3.0, size=(SAMPLES, in_features))), -9, 9)
    arrays["x_k"] = np.clip(X + np.roll(X, 1, axis=1), -18, 18).astype(np.int8)  # neighbouring features correlate
    return arrays


def load(layer, shape, dtype):
    """(XTX, target, codebooks, prev_codes, scales) as tensors of ``dtype`` from the stored arrays of one layer."""
    out_features, in_features, K, nbits, ogs, g = shape
    if nbits == 16:
        books = (layer["codebook_hi_k"][:, None].astype(np.float64) + layer["codebook_lo_k"][None, :].astype(np.float64)).reshape(1, 65536, ogs, g)
    else:
        books = layer["codebook_k"].astype(np.float64)
    books = books * GRID
    near = (layer["prev_codes"].astype(np.int64) + layer["near_shift"].astype(np.int64)) % books.shape[1]
    unscaled = sum(books[c][near[..., c]] for c in range(K))  # [og, ig, ogs, g]
    unscaled = unscaled.transpose(0, 2, 1, 3).reshape(out_features, in_features) + layer["noise_k"].astype(np.float64) * GRID
    factors = 2.0 ** layer["scale_exp"].astype(np.float64)
    target = unscaled * np.repeat(factors, ogs)[:, None]
    x = layer["x_k"].astype(np.float64)
    XTX = (x.T @ x + 16 * np.eye(in_features)).astype(np.float32)  # integers below 2^24: exact
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dtype)  # noqa: E731
    return t(XTX), t(target), t(books), torch.from_numpy(layer["prev_codes"].astype(np.int64)), t(factors).reshape(-1, 1, 1, 1)


class Audit:
    """Wraps torch.topk (the reference's per-beam selection) and Tensor.topk (its selection over the beams) while the reference runs
    in float64: whether every step's best beam_size + 1 scores over all beams x codes are strictly ascending with gaps of at least
    NEAR times the step's largest |score|, on every output group."""

    def __init__(self):
        self.ok, self.pending, self.largest = True, [], None

    def __enter__(self):
        self._topk, self._method = torch.topk, torch.Tensor.topk
        audit = self

        def topk(input, k, dim=0, largest=False, sorted=False):
            assert dim == 0 and not largest
            audit.pending.append(audit._topk(input, min(k + 1, input.shape[0]), dim=0, largest=False, sorted=True).values)
            peak = input.abs().max(0).values
            audit.largest = peak if audit.largest is None else torch.maximum(audit.largest, peak)
            return audit._topk(input, k, dim=0, largest=False, sorted=True)

        def method(self, k, dim=0, largest=False, sorted=True):
            if audit.pending:
                wide = audit._topk(torch.cat(audit.pending, 0), k + 1, dim=0, largest=False, sorted=True).values
                audit.ok = audit.ok and bool(((wide[1:] - wide[:-1]) > NEAR * audit.largest[None]).all())
                audit.pending, audit.largest = [], None
            return audit._method(self, k, dim=dim, largest=largest, sorted=True)

        torch.topk, torch.Tensor.topk = topk, method
        return self

    def __exit__(self, *exc):
        torch.topk, torch.Tensor.topk = self._topk, self._method


def orders_for(shape, shuffled, seed):
    K, ng = shape[2], shape[1] // shape[5]
    if not shuffled:
        return None, None
    rng = np.random.default_rng(1000 + seed)
    return [int(j) for j in rng.permutation(ng)], [[int(c) for c in rng.permutation(K)] for _ in range(ng)]


def run(search, layer, shape, beam, group_order, dim_orders, dtype):
    XTX, target, books, prev, scales = load(layer, shape, dtype)
    rng = None if group_order is None else _Orders([group_order] + dim_orders)
    return search(XTX=XTX, reference_weight=target, codebooks=books, prev_codes=prev, scales=scales, beam_size=beam, dim_rng=rng, verbose=False)


_SEARCH = None


def try_seed(job):
    """(seed, layer arrays, {case: (codes, info)}) when the seed passes every condition for every case of the layer, else None."""
    global _SEARCH
    name, seed = job
    if _SEARCH is None:
        torch.set_num_threads(1)
        from src.beam_search_xtx import beam_search_optimal_codes

        _SEARCH = beam_search_optimal_codes
    shape = LAYERS[name]
    layer = make_layer(shape, seed)
    results = {}
    for case, (owner, beam, shuffled) in CASES.items():
        if owner != name:
            continue
        group_order, dim_orders = orders_for(shape, shuffled, seed)
        with Audit() as audit:
            wide = run(_SEARCH, layer, shape, beam, group_order, dim_orders, torch.float64)
        if not audit.ok:
            return None
        narrow = run(_SEARCH, layer, shape, beam, group_order, dim_orders, torch.float32)
        prev = torch.from_numpy(layer["prev_codes"].astype(np.int64))
        share = float((narrow != prev).any(-1).float().mean())
        if not (bool((wide == narrow).all()) and 0 < share < 1):
            return None
        results[case] = (narrow, {"layer": name, "beam_size": beam, "group_order": group_order, "dim_order": dim_orders, "changed_share": share})
    return seed, layer, results


def main():
    import multiprocessing

    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("reference", help="path of the reference checkout (the directory that holds src/beam_search_xtx.py)")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "code_update_xtx_golden.npz"))
    ap.add_argument("--seed", type=int, default=0, help="first seed tried for every layer")
    ap.add_argument("--tries", type=int, default=4000, help="seeds tried per layer before giving up")
    ap.add_argument("--jobs", type=int, default=max(1, (os.cpu_count() or 2) - 1))
    args = ap.parse_args()
    os.environ["AQ_USE_JIT"] = "0"  # plain Python functions: the audit wraps torch.topk
    sys.path.insert(0, os.path.abspath(args.reference))

    arrays, meta = {}, {"grid": GRID, "near": NEAR, "layers": {}, "cases": {}}
    for name, shape in LAYERS.items():
        with multiprocessing.Pool(args.jobs) as pool:  # seeds in order: the smallest passing seed wins, whatever the job count
            found = next((r for r in pool.imap(try_seed, ((name, s) for s in range(args.seed, args.seed + args.tries))) if r), None)
        if found is None:
            raise SystemExit(f"layer {name}: no seed in {args.tries} passes the conditions")
        seed, layer, results = found
        meta["layers"][name] = {"shape": list(shape), "seed": seed}
        for key, value in layer.items():
            arrays[f"{name}_{key}"] = value
        for case, (codes, info) in results.items():
            arrays[f"{case}_expected"] = codes.numpy().astype(layer["prev_codes"].dtype)
            meta["cases"][case] = info
            print(case, name, "seed", seed, {k: v for k, v in info.items() if k not in ("group_order", "dim_order")}, flush=True)
    arrays["meta"] = np.array(json.dumps(meta))
    np.savez_compressed(args.out, **arrays)
    print(args.out, os.path.getsize(args.out), "bytes")


if __name__ == "__main__":
    main()
