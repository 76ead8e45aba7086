#!/usr/bin/env python
"""Training codebooks and scales of 1x16 g8 layers on the MI355X: the indexed gradient kernels (aqlm_hip_codebook_grad_1x16,
aqlm_hip_scales_grad_1x16; aqlm_amd/tuning.py) against the reference's definition under autograd, with the frozen layer as the floor.

Per shape (4096 x 4096, 4096 -> 14336, 14336 -> 4096; fp16, uniform random codes) and row count (512, 2048, 8192), one training
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

    python tools/codebook_grad_benchmark.py [--iters 10] [--repeats 3] [--out profiles/codebook_grad.json]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [(4096, 4096), (4096, 14336), (14336, 4096)]  # (in, out)
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join("profiles", "codebook_grad.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark needs the MI355X"
    dev = torch.device("cuda:0")

    import aqlm
    import aqlm.tuning as tuning
    from aqlm_amd.inference import _TrainableMatmul1x16
    from aqlm_amd.inference_kernels import hip_kernel as hk

    results = {"device": torch.cuda.get_device_name(0), "iters": args.iters, "repeats": args.repeats, "chunk": hk.CODEBOOK_GRAD_CHUNK,
               "rows": []}
    for fin, fout in SHAPES:
        gen = torch.Generator(device=dev).manual_seed(fin + fout)

        def layer(trainable):
            m = aqlm.QuantizedLinear(fin, fout, 8, 1, 1, 16, bias=False, device=dev, dtype=torch.float16)
            g2 = torch.Generator(device=dev).manual_seed(fin * 3 + fout)
            with torch.no_grad():
                m.codes.copy_(torch.randint(-32768, 32768, m.codes.shape, generator=g2, device=dev, dtype=torch.int32).to(torch.int16))
                m.codebooks.copy_(torch.randn(m.codebooks.shape, generator=g2, device=dev) * 0.05)
                m.scales.copy_(torch.rand(m.scales.shape, generator=g2, device=dev) * 0.2 + 0.05)
            if trainable:
                tuning.make_trainable(torch.nn.ModuleDict({"l": m}))
            return m

        train, frozen = layer(True), layer(False)
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
            row = {"in": fin, "out": fout, "rows": rows, "index_build_us": round(index_us, 1), "index_mb": round(index_mb, 2)}
            tuning.CODEBOOK_GRAD_KERNEL = True
            assert type(train(x).grad_fn).__name__ == _TrainableMatmul1x16.__name__ + "Backward"
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
    with open(args.out, "w") as f:
        json.dump(results, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
