#!/usr/bin/env python
"""Residual k-means initialisation on the MI355X (aqlm_amd/tuning.py): the fused Lloyd kernels (aqlm_hip_kmeans_assign,
aqlm_hip_kmeans_update) against the torch route, which is the reference's formulation -- chunked
``addmm(bmm norms, data, C^T, beta=-0.5).argmax(1)`` that writes and re-reads every score in fp32, then ``index_reduce_(mean)``.

Per shape (a 4096 x 4096 Gaussian weight divided by its row norms, as 1x16 g8, 1x16 g16 and 2x8 g8):
  step_*   ONE Lloyd iteration (assignment, sums, update) from centroids drawn from the data, on either route;
  assign_us / assign_nosums_us   the kernel entry alone with and without its sums: the difference prices the integer adds
           (``add_gb_per_s`` = points * d * 8 bytes over that difference, where it exceeds the spreads);
  full_*   a whole ``init_aq_kmeans`` at ``--full-iters`` Lloyd iterations per codebook (100: the reference's recipes), the final
           assignment and the residue included, on either route, the relative error ``||W - W_q||^2 / ||W||^2`` each reached and the
           Lloyd iterations each ran (the convergence check at every tenth iteration may stop a fit early).
The two routes alternate within one process, --iters calls per round (the full init: one) after warm-up calls of each, --repeats
rounds: median of the rounds' medians and the spread (max - min) over the rounds (``*_spread_us``), device events around every call.
``residual_init``: the errors tests/test_kmeans_gpu.py compares on its 64 x 128 weight (kernel route at seed 0, torch route over
five seeds).

    python tools/kmeans_benchmark.py [--shapes 1x16g8,1x16g16,2x8g8] [--iters 5] [--repeats 5] [--full-iters 100] [--merge] [--out FILE]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = {"1x16g8": (1, 65536, 8), "1x16g16": (1, 65536, 16), "2x8g8": (2, 256, 8)}  # (codebooks, entries, g)
FEATURES = 4096


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def rounds_alternating(fns, iters, repeats, warmup=2):
    """[(median of the rounds' medians, spread over the rounds)] per fn in microseconds; the calls of the fns alternate"""
    for _ in range(warmup):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    meds = [[] for _ in fns]
    for _ in range(repeats):
        times = [[] for _ in fns]
        for _ in range(iters):
            for i, fn in enumerate(fns):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn()
                b.record()
                b.synchronize()
                times[i].append(a.elapsed_time(b) * 1e3)
        for i, t in enumerate(times):
            meds[i].append(median(t))
    return [(round(median(m), 1), round(max(m) - min(m), 1)) for m in meds]


def residual_init(tuning):
    """The figures of tests/test_kmeans_gpu.py::test_init_aq_kmeans_on_the_kernel_route."""
    from aqlm_amd.utils import _dequantize_weight

    weight = torch.randn((64, 128), generator=torch.Generator().manual_seed(5)).cuda()
    out = {}
    for scheme, (K, size, options) in {"2x8": (2, 256, {"max_iter": 10}), "1x16": (1, 65536, {"max_iter": 3, "max_points_per_centroid": 1})}.items():
        def run(seed, switch):
            tuning.KMEANS_KERNEL = switch
            try:
                codes, books = tuning.init_aq_kmeans(weight, num_codebooks=K, out_group_size=1, in_group_size=8, codebook_size=size,
                                                     generator=torch.Generator().manual_seed(seed), **options)
            finally:
                tuning.KMEANS_KERNEL = True
            return float((weight - _dequantize_weight(codes, books, None)).square().sum() / weight.square().sum())

        errors = [run(seed, False) for seed in range(5)]
        out[scheme] = {"kernel_route_error_seed0": run(0, True), "torch_route_errors": errors, "torch_route_mean": sum(errors) / 5,
                       "torch_route_spread": max(errors) - min(errors)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--full-iters", type=int, default=100)
    ap.add_argument("--skip-full", action="store_true", help="time the single iteration only")
    ap.add_argument("--merge", action="store_true", help="keep the rows of other shapes already in the output file")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    shapes = [s.strip() for s in args.shapes.split(",") if s.strip()]
    if any(s not in SHAPES for s in shapes):
        raise SystemExit(f"kmeans_benchmark: --shapes takes a comma list of {sorted(SHAPES)}")
    if not torch.cuda.is_available():
        raise SystemExit("kmeans_benchmark: no GPU (a timing taken anywhere else says nothing about the MI355X)")

    import aqlm.tuning as tuning
    from aqlm_amd.inference_kernels import hip_kernel
    from aqlm_amd.utils import _dequantize_weight

    dev = torch.device("cuda")
    rows = []
    for shape in shapes:
        K, size, g = SHAPES[shape]
        gen = torch.Generator().manual_seed(FEATURES + size + g)
        weight = torch.randn((FEATURES, FEATURES), generator=gen).to(dev)
        weight = weight / weight.norm(dim=-1, keepdim=True)
        data = weight.reshape(-1, g).contiguous()
        n = data.shape[0]
        absmax = float(data.abs().max())
        start = data[torch.randperm(n, generator=gen)[:size].to(dev)].contiguous()
        from_kernel = tuning._kmeans_step(data, start, absmax, True)
        from_torch = tuning._kmeans_step(data, start, absmax, False)
        (step_k, step_k_spread), (step_t, step_t_spread), (assign, assign_spread), (alone, alone_spread) = rounds_alternating(
            [lambda: tuning._kmeans_step(data, start, absmax, True), lambda: tuning._kmeans_step(data, start, absmax, False),
             lambda: hip_kernel.kmeans_assign(data, start, absmax), lambda: hip_kernel.kmeans_assign(data, start, absmax, with_sums=False)],
            args.iters, args.repeats)
        adds = assign - alone
        row = {"weight": [FEATURES, FEATURES], "shape": shape, "points": n, "centroids": size, "dim": g,
               "step_kernel_us": step_k, "step_kernel_spread_us": step_k_spread, "step_torch_us": step_t, "step_torch_spread_us": step_t_spread,
               "step_ratio": round(step_k / step_t, 4), "assign_us": assign, "assign_spread_us": assign_spread, "assign_nosums_us": alone,
               "assign_nosums_spread_us": alone_spread, "scores_per_ns": round(n * size / (alone * 1e3), 1),
               "add_path": "lds" if size * g * 8 <= 65536 else "direct",
               "add_gb_per_s": round(n * g * 8 / (adds * 1e3), 1) if adds > assign_spread + alone_spread else None,
               "centroid_max_abs_diff_after_one_step": float((from_kernel - from_torch).abs().max())}
        if not args.skip_full:
            errors, steps = {}, {}
            step = tuning._kmeans_step

            def full(switch):
                tuning.KMEANS_KERNEL = switch
                ran = []
                tuning._kmeans_step = lambda *a: (ran.append(1), step(*a))[1]
                try:
                    codes, books = tuning.init_aq_kmeans(weight, num_codebooks=K, out_group_size=1, in_group_size=g, codebook_size=size,
                                                         max_iter=args.full_iters, generator=torch.Generator().manual_seed(1))
                finally:
                    tuning.KMEANS_KERNEL = True
                    tuning._kmeans_step = step
                errors[switch] = (weight - _dequantize_weight(codes, books, None)).square().sum() / weight.square().sum()
                steps[switch] = len(ran)  # Lloyd iterations run over all codebooks (the convergence check may stop a fit early)

            (full_k, full_k_spread), (full_t, full_t_spread) = rounds_alternating([lambda: full(True), lambda: full(False)], 1, args.repeats, warmup=1)
            row.update({"full_iters": args.full_iters, "full_kernel_us": full_k, "full_kernel_spread_us": full_k_spread, "full_torch_us": full_t,
                        "full_torch_spread_us": full_t_spread, "full_ratio": round(full_k / full_t, 4),
                        "full_kernel_error": float(errors[True]), "full_torch_error": float(errors[False]),
                        "full_kernel_lloyd_iterations": steps[True], "full_torch_lloyd_iterations": steps[False]})
        rows.append(row)
        print(json.dumps(row), flush=True)
        del weight, data, start, from_kernel, from_torch
        torch.cuda.empty_cache()
    out = args.out or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "kmeans.json")
    result = {"tool": "tools/kmeans_benchmark.py", "device": torch.cuda.get_device_name(0), "iters": args.iters, "repeats": args.repeats,
              "rows": rows, "residual_init": residual_init(tuning)}
    if args.merge and os.path.exists(out):
        result["rows"] = [r for r in json.load(open(out))["rows"] if r["shape"] not in shapes] + rows
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", out)


if __name__ == "__main__":
    main()
