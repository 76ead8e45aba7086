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

``--scheme`` (a comma list of K x 8 schemes: 2x8g8, 1x8g8, 4x8g16, 8x8g32) times the K x 8 layers instead: the fused beam search
kernel (aqlm_hip_code_search_kx8) against the torch route for the same call -- per step a [groups, beams, 256] fp32 score tensor in
chunks and ``torch.topk`` over it -- for every ``--beam`` (a comma list, default 1,4,8,16; 8x8g32 stops at 8), on 4096 -> 4096 and
4096 -> 14336 (fp16 codebooks and scales, fp32 target = planted codewords + 0.35 sigma noise, previous codes = the planted ones with
one code of every second group drawn anew: about half the groups change).  Same columns; ``search_us`` is the one launch of the
kernel entry, ``scores_per_ns`` = groups * K * beams-after-the-first-step * 256 over that time, ``codes_differ`` counts groups on
which the routes differ (fp32 evaluation in another order: near-ties only).  Written to profiles/code_update_kx8.json; ``--merge``
keeps the rows of other (scheme, beam) cells already in that file.

    python tools/code_update_benchmark.py --scheme 2x8g8,1x8g8 --beam 1,4,8,16 [--merge]
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


KX8_LAYERS = [(4096, 4096), (4096, 14336)]  # (in, out)
KX8_SCHEMES = {"2x8g8": (2, 8), "1x8g8": (1, 8), "4x8g16": (4, 16), "8x8g32": (8, 32)}
KX8_MAX_BEAM = {"8x8g32": 8}


def main_kx8(args):
    import aqlm.tuning as tuning
    from aqlm_amd.inference_kernels import hip_kernel

    dev = torch.device("cuda")
    schemes = [s.strip() for s in args.scheme.split(",")]
    beams = [int(b) for b in args.beam.split(",")]
    rows = []
    for scheme in schemes:
        K, g = KX8_SCHEMES[scheme]
        for fin, fout in KX8_LAYERS:
            gen = torch.Generator().manual_seed(fin + fout + 100 * K + g)
            groups = fout * fin // g
            books = torch.randn((K, 256, 1, g), generator=gen).half().to(dev)
            planted = torch.randint(0, 256, (groups, K), generator=gen).to(dev)
            scales = (torch.rand((fout, 1, 1, 1), generator=gen) + 0.5).half().to(dev)
            r = 0.35 * torch.randn((groups, g), generator=gen).to(dev)
            for c in range(K):
                r += books[c, :, 0][planted[:, c]].float()
            target = (r.reshape(fout, fin // g, g) * scales.float().reshape(-1, 1, 1)).reshape(fout, fin).contiguous()
            del r
            moved = (torch.rand((groups,), generator=gen) < 0.5).to(dev)
            which = torch.randint(0, K, (groups,), generator=gen).to(dev)
            fresh = torch.randint(0, 256, (groups,), generator=gen).to(dev)
            unsigned = planted.clone()
            unsigned[torch.arange(groups, device=dev), which] = torch.where(moved, fresh, planted[torch.arange(groups, device=dev), which])
            prev = torch.where(unsigned >= 128, unsigned - 256, unsigned).to(torch.int8).reshape(fout, fin // g, K)
            del planted, moved, which, fresh, unsigned
            for beam in beams:
                if beam > KX8_MAX_BEAM.get(scheme, 16):
                    continue
                for fraction in FRACTIONS:
                    def call(switch, fraction=fraction, beam=beam):
                        tuning.CODE_SEARCH_KERNEL = switch
                        try:
                            return tuning.find_optimal_codes(target, books, prev, scales, beam_size=beam, max_update_fraction=fraction)
                        finally:
                            tuning.CODE_SEARCH_KERNEL = True

                    count = groups if fraction == 1.0 else -(-groups // 100)
                    ids = None if fraction == 1.0 else torch.randperm(groups, device=dev)[:count]
                    out = torch.empty((count, K), dtype=torch.int8, device=dev)
                    from_kernel, from_torch = call(True), call(False)
                    (kernel, kernel_spread), (torch_us, torch_spread), (search, search_spread) = rounds_alternating(
                        [lambda: call(True), lambda: call(False),
                         lambda: hip_kernel.code_search_kx8(target, scales.reshape(-1), books, prev.reshape(-1, K), g, beam, group_ids=ids,
                                                            codes_out=out)],
                        args.iters, args.repeats, warmup=1)
                    scored = count * 256 * (1 + (K - 1) * beam)
                    row = {"in_features": fin, "out_features": fout, "scheme": scheme, "beam_size": beam, "dtype": "fp16",
                           "max_update_fraction": fraction, "groups_searched": count, "kernel_us": kernel, "kernel_spread_us": kernel_spread,
                           "torch_us": torch_us, "torch_spread_us": torch_spread, "ratio": round(kernel / torch_us, 4), "search_us": search,
                           "search_spread_us": search_spread, "scores_per_ns": round(scored / (search * 1e3), 2),
                           "groups_changed": int((from_kernel != prev).any(-1).sum()),
                           "groups_differ": int((from_kernel != from_torch).any(-1).sum())}
                    rows.append(row)
                    print(json.dumps(row), flush=True)
    out = args.out or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "code_update_kx8.json")
    if args.merge and os.path.exists(out):
        cells = {(r["scheme"], r["beam_size"]) for r in rows}
        rows = [r for r in json.load(open(out))["rows"] if (r["scheme"], r["beam_size"]) not in cells] + rows
    result = {"tool": "tools/code_update_benchmark.py --scheme", "device": torch.cuda.get_device_name(0), "iters": args.iters,
              "repeats": args.repeats, "rows": rows}
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--scheme", default=None, help="a comma list of K x 8 schemes (2x8g8, 1x8g8, 4x8g16, 8x8g32): time those instead of 1x16")
    ap.add_argument("--beam", default="1,4,8,16", help="with --scheme: a comma list of beam sizes")
    ap.add_argument("--merge", action="store_true", help="with --scheme: keep the rows of other cells already in the output file")
    args = ap.parse_args()
    if args.scheme is not None and any(s.strip() not in KX8_SCHEMES for s in args.scheme.split(",")):
        raise SystemExit(f"code_update_benchmark: --scheme takes a comma list of {sorted(KX8_SCHEMES)}")
    if not torch.cuda.is_available():
        raise SystemExit("code_update_benchmark: no GPU (a timing taken anywhere else says nothing about the MI355X)")
    if args.scheme is not None:
        return main_kx8(args)

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
