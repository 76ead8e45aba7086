#!/usr/bin/env python
"""Updating the codes of 1x16 layers on the MI355X (the V step of PV-tuning, aqlm_amd/tuning.py): the fused nearest-codeword search
kernel (aqlm_hip_code_search_1x16) against the torch route, which is the reference's formulation -- chunked
``addmm(|C|^2, r, C^T, alpha=-2).argmin(-1)`` that writes and re-reads every score in fp32.

Per layer (fp16 codebook and scales, fp32 target = the dequantised weight of random codes + 0.3 sigma noise on the unscaled
weights, so that about half the groups change code) and ``max_update_fraction`` (1.0, 0.01), one call of
``aqlm.tuning.find_optimal_codes`` -- selection by top-k, the search, the non-finite guard:
  kernel_us   with ``CODE_SEARCH_KERNEL = True``;
  torch_us    with ``CODE_SEARCH_KERNEL = False``;
the two routes alternate within one process, --iters calls per round after two warm-up calls of each, --repeats rounds: median of the
rounds' medians and the spread (max - min) over the rounds (``*_spread_us``), device events around every call.  ``ratio`` = kernel
/ torch.  ``search_us``: the two launches of the kernel entry on their own (the same groups), and ``scores_per_ns`` = groups *
65536 over that time.  ``codes_differ``: groups on which the two routes' results differ (fp32 evaluation against the kernel's
split operands: near-ties only).

    python tools/code_update_benchmark.py [--iters 5] [--repeats 5] [--out FILE]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

LAYERS = [(4096, 4096, 8), (4096, 14336, 8), (4096, 4096, 16)]  # (in, out, g)
FRACTIONS = [1.0, 0.01]
ENTRIES = 65536


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("code_update_benchmark: no GPU (a timing taken anywhere else says nothing about the MI355X)")

    import aqlm.tuning as tuning
    from aqlm_amd.inference_kernels import hip_kernel

    dev = torch.device("cuda")
    rows = []
    for fin, fout, g in LAYERS:
        gen = torch.Generator().manual_seed(fin + fout + g)
        books = torch.randn((1, ENTRIES, 1, g), generator=gen).half().to(dev)
        unsigned = torch.randint(0, ENTRIES, (fout, fin // g), generator=gen).to(dev)
        scales = (torch.rand((fout, 1, 1, 1), generator=gen) + 0.5).half().to(dev)
        noise = torch.randn((fout, fin // g, g), generator=gen).to(dev)
        target = ((books[0, :, 0][unsigned].float() + 0.3 * noise) * scales.float().reshape(-1, 1, 1)).reshape(fout, fin).contiguous()
        prev = torch.where(unsigned >= ENTRIES // 2, unsigned - ENTRIES, unsigned).to(torch.int16)[..., None]
        del noise
        for fraction in FRACTIONS:
            def call(switch, fraction=fraction):
                tuning.CODE_SEARCH_KERNEL = switch
                try:
                    return tuning.find_optimal_codes(target, books, prev, scales, max_update_fraction=fraction)
                finally:
                    tuning.CODE_SEARCH_KERNEL = True

            groups = fout * fin // g
            count = groups if fraction == 1.0 else -(-groups // 100)
            ids = None if fraction == 1.0 else torch.randperm(groups, device=dev)[:count]
            out = torch.empty((count,), dtype=torch.int16, device=dev)
            from_kernel, from_torch = call(True), call(False)
            (kernel, kernel_spread), (torch_us, torch_spread), (search, search_spread) = rounds_alternating(
                [lambda: call(True), lambda: call(False),
                 lambda: hip_kernel.code_search_1x16(target, scales.reshape(-1), books, g, group_ids=ids, codes_out=out)],
                args.iters, args.repeats)
            row = {"in_features": fin, "out_features": fout, "scheme": f"1x16g{g}", "dtype": "fp16", "max_update_fraction": fraction,
                   "groups_searched": count, "kernel_us": kernel, "kernel_spread_us": kernel_spread, "torch_us": torch_us,
                   "torch_spread_us": torch_spread, "ratio": round(kernel / torch_us, 4), "search_us": search,
                   "search_spread_us": search_spread, "scores_per_ns": round(count * ENTRIES / (search * 1e3), 1),
                   "codes_changed": int((from_kernel != prev).sum()), "codes_differ": int((from_kernel != from_torch).sum())}
            rows.append(row)
            print(json.dumps(row), flush=True)
    result = {"tool": "tools/code_update_benchmark.py", "device": torch.cuda.get_device_name(0), "iters": args.iters,
              "repeats": args.repeats, "rows": rows}
    out = args.out or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "code_update.json")
    with open(out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", out)


if __name__ == "__main__":
    main()
