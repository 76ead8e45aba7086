#!/usr/bin/env python
"""The input gradient of the dense 1x16 layers on the MI355X: the fused transposed MFMA GEMM (aqlm_hip_gemm_1x16_transposed, codebook
vectors gathered per row tile, W built in LDS) against the route it replaces, dequantise + ``torch.matmul``
(``hip_kernel.USE_FUSED_1X16_TRANSPOSED = False``).  The protocol is that of tools/kx8_transposed_benchmark.py.

Per group size (8, 16), shape (4096 x 4096, 4096 -> 14336, 14336 -> 4096; fp16, uniform random codes) and row count
(16, 64, 256, 1024, 4096), the closure of ``get_backward_pass_kernel`` under both settings:
  fused_us / dequant_us      one eager call end to end, device events around it -- NOT kernel time: the host's launches and the
                             allocator are inside (two launches and the allocation of W on the dequantise side); the two routes
                             alternate within one process, --iters calls per round, --repeats rounds: median of the rounds' medians,
                             ``*_spread_us`` = max - min over the rounds;
  fused_peak_mb / dequant_peak_mb   the allocator's peak during one call above what was allocated before it (grad_input included);
  rel_diff                   |fused - dequant| / |dequant| of the two results (they differ in the order of the fp32 sums only);
  splits                     the slices the entry chooses (its workspace over the bytes of one slice).
``windows``: per group size the largest contiguous run of measured row counts at which, at every shape, the fused call is no slower
than the other route by more than the cell's spread (the larger of the two routes') -- [first, last] is what
``hip_kernel.FUSED_1X16_TRANSPOSED_ROWS`` is set from; null = no such run (of equally long runs the one at fewer rows).

    python tools/x16_transposed_benchmark.py [--iters 20] [--repeats 3] [--out profiles/x16_transposed.json]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.kx8_transposed_benchmark import peak_mb, rounds_alternating  # noqa: E402

GROUPS = [8, 16]
SHAPES = [(4096, 4096), (4096, 14336), (14336, 4096)]  # (in, out)
ROWS = [16, 64, 256, 1024, 4096]


def windows(rows):
    """group size -> [first, last] of the longest contiguous run of row counts that hold at every shape, or None"""
    out = {}
    for g in GROUPS:
        ok = [all(r["fused_us"] <= r["dequant_us"] + max(r["fused_spread_us"], r["dequant_spread_us"])
                  for r in rows if r["g"] == g and r["rows"] == n) for n in ROWS]
        best, start = None, None
        for i, good in enumerate(ok + [False]):
            if good and start is None:
                start = i
            if not good and start is not None:
                if best is None or i - start > best[1] - best[0] + 1:
                    best = (start, i - 1)
                start = None
        out[f"g{g}"] = None if best is None else [ROWS[best[0]], ROWS[best[1]]]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join("profiles", "x16_transposed.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark needs the MI355X"
    dev = torch.device("cuda:0")

    from aqlm_amd import _native
    from aqlm_amd.inference_kernels import get_backward_pass_kernel
    from aqlm_amd.inference_kernels import hip_kernel as hk

    results = {"device": torch.cuda.get_device_name(0), "iters": args.iters, "repeats": args.repeats, "rows": []}
    hk.FUSED_1X16_TRANSPOSED_ROWS = (1, 1 << 30)  # the flag alone decides the route here
    for g in GROUPS:
        for fin, fout in SHAPES:
            gen = torch.Generator(device=dev).manual_seed(fin + fout + g)
            codes = torch.randint(-32768, 32768, (fout, fin // g, 1), generator=gen, device=dev, dtype=torch.int32).to(torch.int16)
            books = (torch.randn((1, 65536, 1, g), generator=gen, device=dev) * 0.05).half()
            scales = (torch.rand((fout, 1, 1, 1), generator=gen, device=dev) * 0.2 + 0.05).half()
            backward = get_backward_pass_kernel(books, True)
            for rows in ROWS:
                gy = (torch.randn((rows, fout), generator=gen, device=dev) * 0.1).half()

                def route(fused):
                    def run():
                        hk.USE_FUSED_1X16_TRANSPOSED = fused
                        return backward(gy, codes, books, scales, None)
                    return run

                fused, dequant = route(True), route(False)
                assert hk.code1x16_matmat_transposed(gy, codes, books, scales) is not None, "the fused launch declined the call"
                a, b = fused().float(), dequant().float()
                row = {"g": g, "in": fin, "out": fout, "rows": rows,
                       "rel_diff": float((a - b).norm() / b.norm().clamp_min(1e-30)),
                       "splits": int(_native.lib.aqlm_hip_gemm_1x16_transposed_workspace_bytes(rows, fout, fin, 0)) // (rows * fin * 4) or 1,
                       "fused_peak_mb": peak_mb(fused), "dequant_peak_mb": peak_mb(dequant)}
                del a, b
                for name, (t, spread) in zip(("fused", "dequant"), rounds_alternating([fused, dequant], args.iters, args.repeats)):
                    row[f"{name}_us"], row[f"{name}_spread_us"] = t, spread
                row["ratio"] = round(row["fused_us"] / row["dequant_us"], 3)
                results["rows"].append(row)
                print(json.dumps(row), flush=True)
            del codes, books, scales
            torch.cuda.empty_cache()
    hk.USE_FUSED_1X16_TRANSPOSED = True
    results["windows"] = windows(results["rows"])
    print(json.dumps({"windows": results["windows"]}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(results, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
