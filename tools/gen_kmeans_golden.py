#!/usr/bin/env python
"""Development-time tool: write tests/golden/kmeans_golden.npz, the inputs and expected results that tests/test_kmeans_host.py holds
the torch route of ``aqlm.tuning.fit_kmeans`` / ``find_nearest_cluster`` / ``init_aq_kmeans`` to.

    python tools/gen_kmeans_golden.py /path/to/the/reference/checkout

The expected centroids, codes and iteration counts come from the reference's own ``fit_kmeans``, ``find_nearest_cluster``
(``src/kmeans.py`` of that checkout) and ``init_aq_kmeans`` (``src/aq.py``) on the CPU, run as plain Python (``AQ_USE_JIT=0``).  Only
data goes into the fixture: the inputs, the seed and the rows ``torch.randperm`` drew from it for the initial centroids, and per case
the centroids, the codes, the assignment the last update was made with and the number of Lloyd iterations run.  A seed is discarded
when
  * at any iteration, or at the final assignment, some point's float64 margin between its best and its second-best centroid falls
    below 1e-4 of the score scale ``|x|^2 + max_c |C_c|^2``,
  * the fp32 run and the float64 run of the reference disagree on any code or on the iteration count,
so that the expected codes do not depend on the BLAS of the machine that runs the test.  No test imports this file and it never runs
where the reference is absent.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MARGIN = 1e-4
# name -> (points, dim, k, fit_kmeans options)
FITS = {"a": (512, 8, 32, dict(max_iter=7)), "b": (384, 16, 16, dict(max_iter=1000))}
# name -> (out_features, in_features, num_codebooks, out_group_size, in_group_size, codebook_size, max_iter)
LAYERS = {"c": (32, 64, 2, 1, 8, 16, 50)}


class Watch:
    """Counts the Lloyd iterations of the reference and checks the float64 margins of every assignment it makes: the reference
    updates its centroids through ``clone().index_reduce_(0, indices, data, "mean", include_self=False)``, once per iteration."""

    def __init__(self):
        self.iterations, self.smallest, self.last_indices = 0, float("inf"), None
        self.original = torch.Tensor.index_reduce_

    def margin(self, data, centroids):
        x, c = data.double(), centroids.double()
        scores = c.square().sum(-1)[None] - 2 * x @ c.T
        best = torch.topk(scores, 2, dim=-1, largest=False).values
        scale = x.square().sum(-1) + c.square().sum(-1).max()
        return float(((best[:, 1] - best[:, 0]) / scale).min())

    def __enter__(self):
        watch = self

        def index_reduce_(tensor, dim, index, source, reduce, **kw):
            watch.iterations += 1
            watch.smallest = min(watch.smallest, watch.margin(source, tensor))
            watch.last_indices = index.clone()
            return watch.original(tensor, dim, index, source, reduce, **kw)

        torch.Tensor.index_reduce_ = index_reduce_
        return self

    def __exit__(self, *exc):
        torch.Tensor.index_reduce_ = self.original


def run_fit(km, data, k, seed, options):
    torch.manual_seed(seed)
    with Watch() as watch:
        centroids, codes, _ = km.fit_kmeans(data, k, **options)
    smallest = min(watch.smallest, watch.margin(data, centroids))
    again, _ = km.find_nearest_cluster(data, centroids)
    assert torch.equal(again, codes)
    return centroids, codes, watch.iterations, watch.last_indices, smallest


def fit_case(km, shape, seed):
    n, d, k, options = shape
    data = torch.from_numpy(np.random.default_rng(seed).normal(size=(n, d)).astype(np.float32))
    torch.manual_seed(seed)
    rows = torch.randperm(n)[:k]
    c32, i32, it32, u32, m32 = run_fit(km, data, k, seed, options)
    c64, i64, it64, u64, m64 = run_fit(km, data.double(), k, seed, options)
    if min(m32, m64) < MARGIN or it32 != it64 or not torch.equal(i32, i64) or not torch.equal(u32, u64):
        return None
    return {"data": data.numpy(), "rows": rows.numpy(), "centroids": c32.numpy(), "codes": i32.numpy().astype(np.int32),
            "update_codes": u32.numpy().astype(np.int32)}, {"seed": seed, "k": k, "iterations": it32, "options": options,
                                                            "smallest_margin": min(m32, m64)}


def layer_case(aq, shape, seed):
    out_features, in_features, K, ogs, g, size, max_iter = shape
    weight = torch.from_numpy(np.random.default_rng(seed).normal(size=(out_features, in_features)).astype(np.float32))
    n = (out_features // ogs) * (in_features // g)
    torch.manual_seed(seed)
    rows = torch.stack([torch.randperm(n)[:size] for _ in range(K)])
    results = []
    for dtype in (torch.float32, torch.float64):
        torch.manual_seed(seed)
        with Watch() as watch:
            codes, books = aq.init_aq_kmeans(weight.to(dtype), num_codebooks=K, out_group_size=ogs, in_group_size=g, codebook_size=size,
                                             max_iter=max_iter)
        # the final assignment of every codebook, against the residue it was made on
        residue = weight.to(dtype).reshape(out_features // ogs, ogs, in_features // g, g).swapaxes(1, 2).reshape(n, ogs * g).clone()
        smallest = watch.smallest
        for c in range(K):
            smallest = min(smallest, watch.margin(residue, books[c].flatten(1)))
            residue -= books[c].flatten(1)[codes[..., c].flatten()]
        results.append((codes, books, watch.iterations, smallest))
    (c32, b32, it32, m32), (c64, _, it64, m64) = results
    if min(m32, m64) < MARGIN or it32 != it64 or not torch.equal(c32, c64):
        return None
    return {"weight": weight.numpy(), "rows": rows.numpy(), "codebooks": b32.numpy(), "codes": c32.numpy().astype(np.int32)}, {
        "seed": seed, "shape": [out_features, in_features, K, ogs, g, size], "max_iter": max_iter, "iterations": it32,
        "smallest_margin": min(m32, m64)}


def main():
    parser = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    parser.add_argument("reference", help="a checkout of the reference implementation (the directory that holds src/)")
    parser.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "kmeans_golden.npz"))
    args = parser.parse_args()
    os.environ["AQ_USE_JIT"] = "0"
    sys.path.insert(0, os.path.abspath(args.reference))
    import src.aq as aq
    import src.kmeans as km

    arrays, meta = {}, {"margin": MARGIN, "cases": {}}
    for name, make, module, shapes in (("fit", fit_case, km, FITS), ("layer", layer_case, aq, LAYERS)):
        for case, shape in shapes.items():
            for seed in range(1, 200):
                found = make(module, shape, seed)
                if found is not None:
                    break
            else:
                raise SystemExit(f"case {case}: no seed passed the margin and agreement checks")
            for key, value in found[0].items():
                arrays[f"{case}_{key}"] = value
            meta["cases"][case] = dict(found[1], kind=name)
            print(case, found[1])
    np.savez_compressed(args.out, meta=json.dumps(meta), **arrays)
    print("wrote", args.out, os.path.getsize(args.out), "bytes")


if __name__ == "__main__":
    main()
