#!/usr/bin/env python
"""The K x 9..16-bit g 8 layers (2x16, 2x12, 4x16) on the MI355X: the direct matvec (aqlm_hip_gemv_kx16) and the fused
dequantise-to-MFMA kernel (aqlm_hip_gemm_kx16_rows) against the generic routes they replace.  The protocol is that of
tools/x16_transposed_benchmark.py.

Per scheme, shape (4096 x 4096, 4096 -> 14336, 14336 -> 4096; fp16, uniform random codes) and row count (1, 4, 6, 7, 16, 64, 256, 1024):
  new_us / old_us      one eager call end to end, device events around it -- NOT kernel time: the host's launches and the allocator are
                       inside; new = ``codekx16_matmat`` with the matvec switched on up to 6 rows, ``codekx16_matmat_rows`` above;
                       old = ``ops.generic_matmat`` up to 6 rows, ``ops.generic_matmat_dequant`` (dequantise + library GEMM) above.
                       The routes alternate within one process, --iters calls per round, --repeats rounds: median of the rounds'
                       medians, ``*_spread_us`` = max - min over the rounds;
  dense_us             ``F.linear`` on a dense fp16 weight of the shape, in the same alternation: for the record only;
  rel_diff             |new - old| / |old| of the two results.
``decode``: per scheme, whether the matvec wins beyond the spread (new + the larger spread < old) at 1 row on all three shapes --
what ``hip_kernel.USE_KX16_GEMV`` is set from.  ``fused_max_rows``: the largest measured row count n >= 7 such that the fused kernel
wins beyond the spread at every measured row count 7 .. n, on every shape and scheme -- ``hip_kernel.FUSED_KX16_MAX_ROWS``; 0 = nowhere.

    python tools/kx16_benchmark.py [--iters 20] [--repeats 3] [--out profiles/kx16.json]
"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.kx8_transposed_benchmark import rounds_alternating  # noqa: E402

SCHEMES = [(2, 16), (2, 12), (4, 16)]
SHAPES = [(4096, 4096), (4096, 14336), (14336, 4096)]  # (in, out)
ROWS = [1, 4, 6, 7, 16, 64, 256, 1024]
GEMV_MAX_ROWS = 6


def wins(r):
    return r["new_us"] + max(r["new_spread_us"], r["old_spread_us"]) < r["old_us"]


def decide(rows):
    decode = {f"{K}x{nbits}": all(wins(r) for r in rows if (r["K"], r["nbits"], r["rows"]) == (K, nbits, 1)) for K, nbits in SCHEMES}
    fused = 0
    for n in (m for m in ROWS if m > GEMV_MAX_ROWS):
        if not all(wins(r) for r in rows if r["rows"] == n):
            break
        fused = n
    return decode, fused


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join("profiles", "kx16.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark needs the MI355X"
    dev = torch.device("cuda:0")

    from aqlm_amd.inference_kernels import hip_kernel as hk

    ops = torch.ops.aqlm
    results = {"device": torch.cuda.get_device_name(0), "iters": args.iters, "repeats": args.repeats, "rows": []}
    hk.USE_KX16_GEMV = True
    for K, nbits in SCHEMES:
        for fin, fout in SHAPES:
            gen = torch.Generator(device=dev).manual_seed(fin + fout + 100 * K + nbits)
            codes = torch.randint(-32768, 32768, (fout, fin // 8, K), generator=gen, device=dev, dtype=torch.int32).to(torch.int16)
            books = (torch.randn((K, 1 << nbits, 1, 8), generator=gen, device=dev) * 0.05).half()
            scales = (torch.rand((fout, 1, 1, 1), generator=gen, device=dev) * 0.2 + 0.05).half()
            dense = (torch.randn((fout, fin), generator=gen, device=dev) * 0.05).half()
            for rows in ROWS:
                x = (torch.randn((rows, fin), generator=gen, device=dev) * 0.1).half()
                if rows <= GEMV_MAX_ROWS:
                    new = lambda: hk.codekx16_matmat(x, codes, books, scales, None)  # noqa: E731
                    old = lambda: ops.generic_matmat(x, codes, books, scales, None)  # noqa: E731
                else:
                    new = lambda: hk.codekx16_matmat_rows(x, codes, books, scales, None)  # noqa: E731
                    old = lambda: ops.generic_matmat_dequant(x, codes, books, scales, None)  # noqa: E731
                a, b = new(), old()
                assert a is not None, "the fused launch declined the call"
                row = {"K": K, "nbits": nbits, "in": fin, "out": fout, "rows": rows,
                       "rel_diff": float((a.float() - b.float()).norm() / b.float().norm().clamp_min(1e-30))}
                del a, b
                timed = rounds_alternating([new, old, lambda: F.linear(x, dense)], args.iters, args.repeats)
                for name, (t, spread) in zip(("new", "old", "dense"), timed):
                    row[f"{name}_us"], row[f"{name}_spread_us"] = t, spread
                row["ratio"] = round(row["new_us"] / row["old_us"], 3)
                results["rows"].append(row)
                print(json.dumps(row), flush=True)
            del codes, books, scales, dense
            torch.cuda.empty_cache()
    results["decode"], results["fused_max_rows"] = decide(results["rows"])
    print(json.dumps({"decode": results["decode"], "fused_max_rows": results["fused_max_rows"]}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(results, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
