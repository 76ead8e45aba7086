#!/usr/bin/env python
"""Time the calibrated code update (``aqlm.tuning.find_optimal_codes_calibrated``) on the GPU: the kernel route (one
aqlm_hip_code_search_kx8_xtx launch per input group; with ``--scheme 1x16`` one aqlm_hip_code_search_1x16_xtx call per input group)
against the torch route for the same call, alternating in one process.

    python tools/code_update_xtx_benchmark.py [--out profiles/code_update_xtx.json] [--rounds 3] [--shapes 4096x4096,4096x14336]
    python tools/code_update_xtx_benchmark.py --scheme 1x16 [--out profiles/code_update_xtx_1x16.json] [--shapes 4096x4096] [--beams 1,4,8]

Per cell (shape, scheme, beam_size): the median over ``--rounds`` rounds after one warm-up call per route, timed with device events,
and the spread (max - min) / median of each route; ``step_us``: the median of 20 launches of the step entry alone (a later group:
beam_size positions); ``outside_share``: the share of the kernel route's call spent outside the launches (1 - groups * step / call);
``rows_differ``: output rows on which the two routes' codes disagree.  Inputs: seeded Gaussian codebooks, a target of planted
codewords plus noise, XTX = X^T X / n of a correlated X."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SCHEMES = ((2, 8), (1, 8), (8, 32))
BEAMS = (1, 4, 8, 16)
SCHEMES_1X16 = ((1, 8),)  # one codebook of 65536 entries, g 8
BEAMS_1X16 = (1, 4, 8)


def timed(fn):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    out = fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) * 1e3, out


def make(out, fin, K, g, dev, size=256):
    gen = torch.Generator(device="cpu").manual_seed(out + fin + 100 * K + g)
    books = torch.randn((K, size, 1, g), generator=gen).half()
    ng = fin // g
    planted = torch.randint(0, size, (out, ng, K), generator=gen)
    prev = planted.clone()
    moved = torch.rand((out, ng), generator=gen) < 0.5
    prev[moved] = torch.randint(0, size, (int(moved.sum()), K), generator=gen)
    scales = (torch.rand((out, 1, 1, 1), generator=gen) + 0.5).half()
    books, planted, prev, scales = books.to(dev), planted.to(dev), prev.to(dev), scales.to(dev)
    from aqlm_amd.utils import _dequantize_weight

    target = _dequantize_weight(planted, books.float(), scales.float()) + 0.35 * torch.randn((out, fin), device=dev)
    X = torch.randn((2 * fin, fin), device=dev)
    X = X + 0.6 * X.roll(1, 1)
    XTX = (X.T @ X / X.shape[0]).contiguous()
    stored = torch.where(prev >= size // 2, prev - size, prev).to(torch.int8 if size == 256 else torch.int16)
    return XTX, target, books, stored, scales


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--scheme", choices=("kx8", "1x16"), default="kx8")
    ap.add_argument("--out", default=None, help="default: profiles/code_update_xtx.json, or profiles/code_update_xtx_1x16.json")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--shapes", default=None, help="in x out, comma separated (default 4096x4096,4096x14336; 1x16: 4096x4096)")
    ap.add_argument("--beams", default=None, help="comma separated (default 1,4,8,16; 1x16: 1,4,8)")
    args = ap.parse_args()
    wide = args.scheme == "1x16"
    size = 65536 if wide else 256
    args.out = args.out or os.path.join(ROOT, "profiles", "code_update_xtx_1x16.json" if wide else "code_update_xtx.json")
    args.shapes = args.shapes or ("4096x4096" if wide else "4096x4096,4096x14336")
    beams = tuple(int(b) for b in args.beams.split(",")) if args.beams else (BEAMS_1X16 if wide else BEAMS)
    import aqlm.tuning as tuning
    from aqlm_amd.inference_kernels import hip_kernel as hk

    dev = torch.device("cuda")
    rows = []
    for shape in args.shapes.split(","):
        fin, out = (int(v) for v in shape.split("x"))
        for K, g in (SCHEMES_1X16 if wide else SCHEMES):
            XTX, target, books, stored, scales = make(out, fin, K, g, dev, size)
            ng = fin // g
            for beam in beams:
                call = lambda: tuning.find_optimal_codes_calibrated(XTX, target, books, stored, scales, beam_size=beam)  # noqa: E731
                times, results = {True: [], False: []}, {}
                for r in range(args.rounds + 1):
                    for switch in (True, False):
                        tuning.CODE_SEARCH_KERNEL = switch
                        try:
                            us, codes = timed(call)
                        finally:
                            tuning.CODE_SEARCH_KERNEL = True
                        results[switch] = codes
                        if r:
                            times[switch].append(us)
                t = torch.randn((beam, out, g), device=dev)
                loss = torch.rand((beam, out), device=dev)
                codes_in = stored[None, :, 0, :].expand(beam, out, K).contiguous()
                H = XTX[:g, :g].contiguous()
                q = torch.rand((K, size), device=dev)
                flat = books.reshape(K, size, g).contiguous()
                if wide:
                    q = ((flat.float() @ H) * flat.float()).sum(-1).contiguous()  # C H C^T: the filter of this entry reads the scores
                    step = lambda: hk.code_search_1x16_xtx_step(t, loss, codes_in, H, q[0], flat, scales.reshape(-1), beam)  # noqa: E731
                else:
                    step = lambda: hk.code_search_kx8_xtx_step(t, loss, codes_in, H, q, flat, scales.reshape(-1), beam)  # noqa: E731
                step()
                step_us = statistics.median(timed(step)[0] for _ in range(20))
                kernel_us, torch_us = statistics.median(times[True]), statistics.median(times[False])
                row = {"in": fin, "out": out, "scheme": f"1x16g{g}" if wide else f"{K}x8g{g}", "beam_size": beam, "kernel_us": kernel_us, "torch_us": torch_us,
                       "ratio": kernel_us / torch_us, "kernel_spread": (max(times[True]) - min(times[True])) / kernel_us,
                       "torch_spread": (max(times[False]) - min(times[False])) / torch_us, "step_us": step_us,
                       "outside_share": 1 - ng * step_us / kernel_us,
                       "rows_differ": int((results[True] != results[False]).any(-1).any(-1).sum()), "rows": out, "rounds": args.rounds}
                print(json.dumps(row), flush=True)
                rows.append(row)
                with open(args.out, "w") as f:
                    json.dump({"device": torch.cuda.get_device_name(0), "cells": rows}, f, indent=1)
            del XTX, target
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
