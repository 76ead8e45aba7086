#!/usr/bin/env python
"""Training codebooks and scales on the MI355X: the gradient kernels (aqlm_amd/tuning.py) against the reference's definition under
autograd, with the frozen layer as the floor.  ``--scheme 1x16g8`` (default): the indexed kernels aqlm_hip_codebook_grad_1x16 /
aqlm_hip_scales_grad_1x16 at 4096 x 4096, 4096 -> 14336, 14336 -> 4096.  ``--scheme 2x8g8`` (4096 x 4096, 4096 -> 11008, 11008 ->
4096) and ``--scheme 8x8g32`` (4096 x 4096): the fixed-point LDS kernels aqlm_hip_codebook_grad_kx8 / aqlm_hip_scales_grad_kx8; their
rows go to profiles/codebook_grad_kx8.json (one file for the K x 8 schemes: a run replaces the rows of its own scheme).

Per shape (fp16, uniform random codes) and row count (512, 2048, 8192), one training
step = forward + backward with a gradient for the input, the codebook and the scales:
  hip      the HIP route (forward kernel of the frozen layer; grad_input, dW GEMM, the two gradient launches);
  torch    the torch route (``tuning.CODEBOOK_GRAD_KERNEL = False``): F.linear(x, _dequantize_weight(...)) under autograd;
  frozen   the frozen layer: grad_input only -- what the step costs without any parameter gradient.
Each route eager (``*_eager_us``) and captured in a hipGraph and replayed (``*_graph_us``); the three routes alternate within one
process, --iters steps per round, --repeats rounds: median of the rounds' medians and the spread (max - min) over the rounds, device
events around every step.  ``*_peak_mb``: the peak of the allocator during one eager step above what was allocated before it.
``dw_gemm_us``, ``codebook_grad_us``, ``scales_grad_us``: the three pieces of the HIP route's backward on their own, alternating
(dW then still sits in the Infinity Cache, as it does in a step: it was just written).  ``index_build_us`` / ``index_mb``: the
one-off inverted index of the layer (torch ops) and what it holds.  ``ratio`` = hip / torch of the eager step.
K x 8 rows have no index; they add ``maxima_us`` / ``accumulate_us`` / ``finish_us``, the three launches of the codebook gradient
on their own (device time per kernel from torch.profiler over --iters calls; ``kernel_times_error`` when the profiler is not
usable), and ``lds_add_per_ns`` = positions * g * K 64-bit LDS adds / the accumulate launch's time.

    python tools/codebook_grad_benchmark.py [--scheme 1x16g8|2x8g8|8x8g32] [--iters 10] [--repeats 3] [--out FILE]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [(4096, 4096), (4096, 14336), (14336, 4096)]  # (in, out)
# scheme -> (num_codebooks, nbits, g, shapes, default output)
SCHEMES = {"1x16g8": (1, 16, 8, SHAPES, "codebook_grad.json"),
           "2x8g8": (2, 8, 8, [(4096, 4096), (4096, 11008), (11008, 4096)], "codebook_grad_kx8.json"),
           "8x8g32": (8, 8, 32, [(4096, 4096)], "codebook_grad_kx8.json")}
ROWS = [512, 2048, 8192]


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


def captured(fn):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fn()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    return g


def kernel_times(fn, iters, names):
    """Mean device time in microseconds of the kernels whose name holds one of ``names``, over ``iters`` calls of fn."""
    from torch.profiler import ProfilerActivity, profile

    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(iters):
            fn()
        torch.cuda.synchronize()
    total, count = {n: 0.0 for n in names}, {n: 0 for n in names}
    for ev in prof.events():
        for n in names:
            if n in ev.name:
                total[n] += float(getattr(ev, "device_time", 0.0) or getattr(ev, "cuda_time", 0.0))
                count[n] += 1
    missing = [n for n in names if count[n] == 0]
    if missing:
        raise RuntimeError(f"no kernel events for {missing}")
    return {n: round(total[n] / count[n], 1) for n in names}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scheme", choices=sorted(SCHEMES), default="1x16g8")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    K, nbits, G, shapes, out_name = SCHEMES[args.scheme]
    kx8 = nbits == 8
    if args.out is None:
        args.out = os.path.join("profiles", out_name)
    assert torch.cuda.is_available(), "this benchmark needs the MI355X"
    dev = torch.device("cuda:0")

    import aqlm
    import aqlm.tuning as tuning
    from aqlm_amd.inference import _TrainableMatmul1x16, _TrainableMatmulKx8
    from aqlm_amd.inference_kernels import hip_kernel as hk

    results = {"device": torch.cuda.get_device_name(0), "iters": args.iters, "repeats": args.repeats, "chunk": hk.CODEBOOK_GRAD_CHUNK,
               "rows": []}
    if kx8:
        del results["chunk"]
    for fin, fout in shapes:
        gen = torch.Generator(device=dev).manual_seed(fin + fout)

        def layer(trainable):
            m = aqlm.QuantizedLinear(fin, fout, G, 1, K, nbits, bias=False, device=dev, dtype=torch.float16)
            g2 = torch.Generator(device=dev).manual_seed(fin * 3 + fout)
            lo = -(2 ** (nbits - 1))
            with torch.no_grad():
                m.codes.copy_(torch.randint(lo, -lo, m.codes.shape, generator=g2, device=dev, dtype=torch.int32).to(m.codes.dtype))
                m.codebooks.copy_(torch.randn(m.codebooks.shape, generator=g2, device=dev) * 0.05)
                m.scales.copy_(torch.rand(m.scales.shape, generator=g2, device=dev) * 0.2 + 0.05)
            if trainable:
                tuning.make_trainable(torch.nn.ModuleDict({"l": m}))
            return m

        train, frozen = layer(True), layer(False)
        index = None
        if not kx8:
            hk.build_codebook_grad_index(train.codes, 8)  # warm-up of the sort
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            index = hk.build_codebook_grad_index(train.codes, 8)
            b.record()
            b.synchronize()
            index_us, index_mb = a.elapsed_time(b) * 1e3, index.nbytes() / 2 ** 20
        tuning.prepare(torch.nn.ModuleDict({"l": train}))
        for rows in ROWS:
            x = (torch.randn((rows, fin), generator=gen, device=dev) * 0.5).half().requires_grad_(True)
            gy = (torch.randn((rows, fout), generator=gen, device=dev) * 0.1).half()

            def step(m, switch):
                def run():
                    tuning.CODEBOOK_GRAD_KERNEL = switch
                    for p in (m.codebooks, m.scales, x):
                        p.grad = None
                    m(x).backward(gy)
                return run

            fns = {"hip": step(train, True), "torch": step(train, False), "frozen": step(frozen, True)}
            if kx8:
                row = {"scheme": args.scheme, "in": fin, "out": fout, "rows": rows}
            else:
                row = {"in": fin, "out": fout, "rows": rows, "index_build_us": round(index_us, 1), "index_mb": round(index_mb, 2)}
            tuning.CODEBOOK_GRAD_KERNEL = True
            assert type(train(x).grad_fn).__name__ == (_TrainableMatmulKx8 if kx8 else _TrainableMatmul1x16).__name__ + "Backward"
            # the two routes agree (fp16 storage: the torch route rounds dW, the scaled dW and its scatter-add to fp16)
            fns["hip"]()
            g_hip = train.codebooks.grad.float().clone()
            fns["torch"]()
            g_torch = train.codebooks.grad.float().clone()
            row["codebook_grad_rel_diff_hip_vs_torch"] = float((g_hip - g_torch).norm() / g_torch.norm().clamp_min(1e-30))
            for name, fn in fns.items():
                fn()
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats()
                base = torch.cuda.memory_allocated()
                fn()
                torch.cuda.synchronize()
                row[f"{name}_peak_mb"] = round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1)
            for (name, _), (t, spread) in zip(fns.items(), rounds_alternating(list(fns.values()), args.iters, args.repeats)):
                row[f"{name}_eager_us"], row[f"{name}_eager_spread_us"] = t, spread
            graphs = {}
            for name, fn in fns.items():
                try:
                    fn()
                    graphs[name] = captured(fn)
                except Exception as e:  # a route that cannot be captured is reported, not hidden
                    row[f"{name}_graph_error"] = f"{type(e).__name__}: {e}"[:200]
                    torch.cuda.synchronize()
            if graphs:
                timed = rounds_alternating([g.replay for g in graphs.values()], args.iters, args.repeats)
                for name, (t, spread) in zip(graphs, timed):
                    row[f"{name}_graph_us"], row[f"{name}_graph_spread_us"] = t, spread
            del graphs
            tuning.CODEBOOK_GRAD_KERNEL = True
            gy2, x2 = gy.reshape(-1, fout), x.detach().reshape(-1, fin)
            dw = torch.mm(gy2.t(), x2)
            if kx8:
                parts = [lambda: torch.mm(gy2.t(), x2), lambda: hk.codebook_grad_kx8(dw, train.scales, train.codes, G, out_dtype=torch.float16),
                         lambda: hk.scales_grad_kx8(dw, train.codes, train.codebooks, out_dtype=torch.float16)]
                try:
                    for name, t in kernel_times(parts[1], args.iters, ("maxima", "accumulate", "finish")).items():
                        row[f"{name}_us"] = t
                    row["lds_add_per_ns"] = round(fout * fin * K / (row["accumulate_us"] * 1e3), 2)
                except Exception as e:  # reported, not hidden
                    row["kernel_times_error"] = f"{type(e).__name__}: {e}"[:200]
            else:
                parts = [lambda: torch.mm(gy2.t(), x2), lambda: hk.codebook_grad_1x16(dw, train.scales, index, out_dtype=torch.float16),
                         lambda: hk.scales_grad_1x16(dw, train.codes, train.codebooks, out_dtype=torch.float16)]
            for name, (t, spread) in zip(("dw_gemm", "codebook_grad", "scales_grad"), rounds_alternating(parts, args.iters, args.repeats)):
                row[f"{name}_us"], row[f"{name}_spread_us"] = t, spread
            row["ratio"] = round(row["hip_eager_us"] / row["torch_eager_us"], 3)
            results["rows"].append(row)
            print(json.dumps(row), flush=True)
            del dw, x, gy
        del train, frozen, index
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    if kx8 and os.path.exists(args.out):  # one file for the K x 8 schemes: the other schemes' rows stay
        with open(args.out) as f:
            kept = [r for r in json.load(f).get("rows", []) if r.get("scheme") != args.scheme]
        results["rows"] = kept + results["rows"]
    with open(args.out, "w") as f:
        json.dump(results, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
