#!/usr/bin/env python
"""The input gradient of the dense K x 8 layers on the MI355X: the fused transposed MFMA GEMM (aqlm_hip_gemm_kx8_transposed, W built
tile by tile in LDS) against the route it replaces, dequantise + ``torch.matmul`` (``hip_kernel.USE_FUSED_KX8_TRANSPOSED = False``).

Per scheme (2x8 g8, 1x8 g8, 8x8 g32), shape (4096 x 4096, 4096 -> 14336, 14336 -> 4096; fp16, uniform random codes) and row count
(16, 64, 256, 1024, 4096), the closure of ``get_backward_pass_kernel`` under both settings:
  fused_us / dequant_us      one eager call end to end, device events around it -- NOT kernel time: the host's launches and the
                             allocator are inside (two launches and the allocation of W on the dequantise side); the two routes alternate within one process, --iters calls per
                             round, --repeats rounds: median of the rounds' medians, ``*_spread_us`` = max - min over the rounds;
  fused_peak_mb / dequant_peak_mb   the allocator's peak during one call above what was allocated before it (grad_input included);
  rel_diff                   |fused - dequant| / |dequant| of the two results (they differ in the order of the fp32 sums only);
  splits_bound               the most slices the entry may have chosen (its workspace bound over the bytes of one slice).
``thresholds``: per scheme the smallest measured row count from which, at every shape and every larger row count, the fused call is no
slower than the other route by more than the larger of the two spreads -- what ``hip_kernel.FUSED_KX8_TRANSPOSED_MIN_ROWS`` is set
from; null = nowhere.

    python tools/kx8_transposed_benchmark.py [--iters 20] [--repeats 3] [--out profiles/kx8_transposed.json]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SCHEMES = {"2x8g8": (2, 8), "1x8g8": (1, 8), "8x8g32": (8, 32)}
SHAPES = [(4096, 4096), (4096, 14336), (14336, 4096)]  # (in, out)
ROWS = [16, 64, 256, 1024, 4096]


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def rounds_alternating(fns, iters, repeats, warmup=3):
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


def peak_mb(fn):
    fn()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1)


def thresholds(rows):
    """scheme -> smallest row count from which the fused call holds at every shape and every larger measured row count"""
    out = {}
    for scheme in SCHEMES:
        ok = {n: all(r["fused_us"] <= r["dequant_us"] + max(r["fused_spread_us"], r["dequant_spread_us"])
                     for r in rows if r["scheme"] == scheme and r["rows"] == n) for n in ROWS}
        out[scheme] = next((n for i, n in enumerate(ROWS) if all(ok[m] for m in ROWS[i:])), None)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join("profiles", "kx8_transposed.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark needs the MI355X"
    dev = torch.device("cuda:0")

    from aqlm_amd import _native
    from aqlm_amd.inference_kernels import get_backward_pass_kernel
    from aqlm_amd.inference_kernels import hip_kernel as hk

    results = {"device": torch.cuda.get_device_name(0), "iters": args.iters, "repeats": args.repeats, "rows": []}
    hk.FUSED_KX8_TRANSPOSED_MIN_ROWS = 1  # the flag alone decides the route here
    for scheme, (K, g) in SCHEMES.items():
        for fin, fout in SHAPES:
            gen = torch.Generator(device=dev).manual_seed(fin + fout + K)
            codes = torch.randint(-128, 128, (fout, fin // g, K), generator=gen, device=dev, dtype=torch.int32).to(torch.int8)
            books = (torch.randn((K, 256, 1, g), generator=gen, device=dev) * 0.05).half()
            scales = (torch.rand((fout, 1, 1, 1), generator=gen, device=dev) * 0.2 + 0.05).half()
            backward = get_backward_pass_kernel(books, True)
            for rows in ROWS:
                gy = (torch.randn((rows, fout), generator=gen, device=dev) * 0.1).half()

                def route(fused):
                    def run():
                        hk.USE_FUSED_KX8_TRANSPOSED = fused
                        return backward(gy, codes, books, scales, None)
                    return run

                fused, dequant = route(True), route(False)
                assert hk.codekx8_matmat_transposed(gy, codes, books, scales) is not None, "the fused launch declined the call"
                a, b = fused().float(), dequant().float()
                row = {"scheme": scheme, "in": fin, "out": fout, "rows": rows,
                       "rel_diff": float((a - b).norm() / b.norm().clamp_min(1e-30)),
                       "splits_bound": int(_native.lib.aqlm_hip_gemm_kx8_transposed_workspace_bytes(rows, fout, fin, 0)) // (rows * fin * 4) or 1,
                       "fused_peak_mb": peak_mb(fused), "dequant_peak_mb": peak_mb(dequant)}
                del a, b
                for name, (t, spread) in zip(("fused", "dequant"), rounds_alternating([fused, dequant], args.iters, args.repeats)):
                    row[f"{name}_us"], row[f"{name}_spread_us"] = t, spread
                row["ratio"] = round(row["fused_us"] / row["dequant_us"], 3)
                results["rows"].append(row)
                print(json.dumps(row), flush=True)
            del codes, books, scales
            torch.cuda.empty_cache()
    hk.USE_FUSED_KX8_TRANSPOSED = True
    results["thresholds"] = thresholds(results["rows"])
    print(json.dumps({"thresholds": results["thresholds"]}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(results, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
