#!/usr/bin/env python
"""One Mixtral-8x7B-shaped MoE expert block (hidden 4096, intermediate 14336, 8 experts, top-2, 1x16 g8, random codes, fp16) at
T in {1, 2, 4, 8, 16} tokens:
  (a) routed  -- QuantizedMixtralExperts.forward on the routed launches (aqlm_hip_gemv_1x16_routed), eager;
  (b) graph   -- the same forward captured in a hipGraph and replayed;
  (c) loop    -- a per-expert loop on the existing ops through each expert's QuantizedLinear.forward (prepacked experts for
                 T <= 6 rows per expert, as a dense-MLP model would run them; the expert ids go to the host);
  (d) dense   -- transformers' MixtralExperts in fp16, eager.
Median wall time per call over --iters calls (CUDA events), in microseconds.  Writes --out (default profiles/moe_block.json).

--grouped: the expert-grouped launches (aqlm_hip_moe_bucket + aqlm_hip_gemm_1x16_grouped) against the module's own per-expert loop
(QuantizedMixtralExperts._forward_loop, the route of more than 64 pairs before them) and, up to 64 pairs, the routed launches, at
T up to 512; eager calls of the old and the new route alternate within one process (one pair of device events each).  Adds
grouped_graph_us (captured and replayed) and one forward + backward row at the largest T for the grouped path and the
differentiable loop.  Writes --out (default profiles/moe_grouped.json).

--only packed: the routed PACKED launches on a block prepacked with aqlm_amd.moe.prepack_experts (routed_packed_eager_us,
routed_packed_graph_us) next to today's routes measured in the same call -- the captured direct-routed block (routed_graph_us, on a
second, not prepacked block of the same weights) and the eager per-expert loop (loop_eager_us) -- their calls alternating, --repeats
times over.  The route is forced for every T (ROUTED_PACKED_MAX_PAIRS is what this run measures): the largest pair count up to which
the captured prepacked block beat both other routes by more than the spread of the direct-routed figure goes into the output as
"routed_packed_max_pairs", beside ESTIMATE["packed_t1_us"].  Writes --out (default profiles/moe_block_packed.json).

--backward: forward + backward of the block (x and top_k_weights requiring grad, a random grad-output) at T in {8, 32, 128, 512}:
the device backward (one transposed grouped launch per projection group, aqlm_hip_gemm_1x16_grouped_transposed) eager and captured
with the forward in one hipGraph, against the per-expert loop backward (aqlm_amd.moe.GROUPED_BACKWARD = False, eager: the behaviour
before that launch existed).  The three alternate within one process over --repeats rounds of --iters steps, each step on the next
of three input sets that route differently; median of the rounds' medians and the spread (max - min) over the rounds.  Also the
peak-memory delta of one step (torch.cuda.max_memory_allocated over the memory allocated before it).  Writes --out (default
profiles/moe_grouped_backward.json).

    python tools/moe_benchmark.py [--only graph] [--tokens 1,2,4,8,16]
    python tools/moe_benchmark.py --only packed [--tokens 1,2,4,8,16,32] [--repeats 3]
    python tools/moe_benchmark.py --grouped [--tokens 1,2,4,8,16,32,40,64,128,256,512]
    python tools/moe_benchmark.py --backward [--tokens 8,32,128,512] [--iters 30] [--repeats 3]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

H, I, E, K = 4096, 14336, 8, 2
# the direct 1x16 kernel gathers about 1 M codes per 3.8 us across the chip
ESTIMATE = {"routed_t1_kernel_us": 2 * 3 * (I * H / 8) / 1e6 * 3.8, "packed_t1_us": 75.0, "dense_t1_us": 140.0,
            "basis": "DESIGN.md 4.1: 3.8 us per million codes (direct kernel), 2 experts x 3 layers x 7.3 M codes; packed per-expert "
                     "matvecs at 1.2 TB/s; dense reads 704 MB"}


def build(dev, dense_too):
    from transformers import MixtralConfig
    from transformers.models.mixtral.modeling_mixtral import MixtralExperts

    from aqlm_amd.moe import QuantizedMixtralExperts

    cfg = MixtralConfig(hidden_size=H, intermediate_size=I, num_local_experts=E, num_experts_per_tok=K)
    q = QuantizedMixtralExperts(cfg, dict(in_group_size=8, out_group_size=1, num_codebooks=1, nbits_per_codebook=16), device=dev,
                                dtype=torch.float16)
    gen = torch.Generator(device=dev).manual_seed(0)
    with torch.no_grad():
        for e in range(E):
            for s in ("w1", "w3", "w2"):
                lin = getattr(q.expert(e), s)
                lin.codes.copy_(torch.randint(-32768, 32768, lin.codes.shape, generator=gen, device=dev, dtype=torch.int32))
                lin.codebooks.copy_(torch.randn(lin.codebooks.shape, generator=gen, device=dev) * 0.05)
                lin.scales.copy_(torch.rand(lin.scales.shape, generator=gen, device=dev) * 0.2 + 0.05)
    dense = None
    if dense_too:
        dense = MixtralExperts(cfg).to(dev, torch.float16)
        with torch.no_grad():
            dense.gate_up_proj.normal_(0, 0.02)
            dense.down_proj.normal_(0, 0.02)
    return q, dense


def loop_forward(q, x, ids, w):
    """(c): tokens grouped per expert on the host, each expert's QuantizedLinears called through their own forward."""
    out = torch.zeros(x.shape, dtype=torch.float32, device=x.device)
    for e in torch.unique(ids).tolist():
        tok, pos = torch.where(ids == e)
        ex = q.expert(e)
        xe = x[tok]
        h = q.act_fn(ex.w1(xe)) * ex.w3(xe)
        out.index_add_(0, tok, ex.w2(h).float() * w[tok, pos, None])
    return out.to(x.dtype)


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) * 1e3)
    times.sort()
    return round(times[len(times) // 2], 2)


def timed_alternating(fns, iters, warmup):
    """median per call of each of `fns`, their calls interleaved (a, b, a, b, ...) so that clocks and caches drift alike"""
    for _ in range(warmup):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    times = [[] for _ in fns]
    for _ in range(iters):
        for i, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            times[i].append(a.elapsed_time(b) * 1e3)
    return [round(sorted(t)[len(t) // 2], 2) for t in times]


def captured(fn):
    fn()
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fn()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    return g


def grouped_main(args):
    dev = torch.device("cuda:0")
    q, _ = build(dev, False)
    gen = torch.Generator(device=dev).manual_seed(1)
    tokens = [int(t) for t in args.tokens.split(",")]
    rows = []
    for T in tokens:
        x = torch.randn((T, H), generator=gen, device=dev).half()
        logits = torch.randn((T, E), generator=gen, device=dev)
        w, ids = torch.topk(torch.softmax(logits, -1), K, dim=-1)
        w = w / w.sum(-1, keepdim=True)
        row = {"tokens": T, "pairs": T * K, "experts_hit": len(set(ids.view(-1).tolist()))}
        with torch.no_grad():
            fns = [lambda: q._forward_grouped(x, ids, w), lambda: q._forward_loop(x, ids, w)]
            names = ["grouped_eager_us", "loop_eager_us"]
            if T * K <= 64:
                fns.append(lambda: q._forward_routed(x, ids, w))
                names.append("routed_eager_us")
            row.update(zip(names, timed_alternating(fns, args.iters, args.warmup)))
            g = captured(lambda: q._forward_grouped(x, ids, w))
            row["grouped_graph_us"] = timed(g.replay, args.iters, args.warmup)
            del g
        rows.append(row)
        print(json.dumps(row), flush=True)
    T = tokens[-1]
    x0 = torch.randn((T, H), generator=gen, device=dev).half()
    logits = torch.randn((T, E), generator=gen, device=dev)
    w0, ids = torch.topk(torch.softmax(logits, -1), K, dim=-1)
    x, w = x0.clone().requires_grad_(), w0.clone().requires_grad_()
    bwd = {"tokens": T, "what": "forward + backward of (y * 1).sum(), x and top_k_weights requiring grad"}

    def step(fwd):
        x.grad = w.grad = None
        fwd(x, ids, w).float().sum().backward()

    bwd["grouped_fwd_bwd_us"], bwd["loop_fwd_bwd_us"] = timed_alternating([lambda: step(q._forward_grouped), lambda: step(q._forward_loop)],
                                                                          max(3, args.iters // 5), 2)
    print(json.dumps(bwd), flush=True)
    result = {"block": {"hidden": H, "intermediate": I, "experts": E, "top_k": K, "scheme": "1x16g8", "dtype": "float16"},
              "device": torch.cuda.get_device_name(dev), "iters": args.iters, "rows": rows, "forward_backward": bwd}
    out = args.out or os.path.join("profiles", "moe_grouped.json")
    os.makedirs(os.path.dirname(out) or ".", exist_ok=True)
    with open(out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))


def backward_main(args):
    import aqlm_amd.moe as moe

    dev = torch.device("cuda:0")
    q, _ = build(dev, False)
    gen = torch.Generator(device=dev).manual_seed(1)
    SETS = 3
    rows = []
    for T in [int(t) for t in args.tokens.split(",")]:
        sets = []
        for _ in range(SETS):
            x = torch.randn((T, H), generator=gen, device=dev).half().requires_grad_()
            w, ids = torch.topk(torch.softmax(torch.randn((T, E), generator=gen, device=dev), -1), K, dim=-1)
            w = (w / w.sum(-1, keepdim=True)).requires_grad_()
            sets.append((x, ids, w, torch.randn((T, H), generator=gen, device=dev).half()))
        turn = [0, 0]

        def eager(route, slot):
            x, ids, w, gy = sets[turn[slot] % SETS]
            turn[slot] += 1
            moe.GROUPED_BACKWARD = route
            try:
                x.grad = w.grad = None
                q(x, ids, w).backward(gy)
            finally:
                moe.GROUPED_BACKWARD = True

        # the captured step: static inputs, refreshed from the next set before every replay (the copies are inside the timed window:
        # four small device copies, which a training loop pays as well)
        sx, sids, sw, sgy = (t.detach().clone() for t in sets[0])
        sx.requires_grad_()
        sw.requires_grad_()

        def static_step():
            sx.grad = sw.grad = None
            q(sx, sids, sw).backward(sgy)

        graph = captured(static_step)
        gturn = [0]

        def replay():
            x, ids, w, gy = sets[gturn[0] % SETS]
            gturn[0] += 1
            with torch.no_grad():
                sx.copy_(x)
                sids.copy_(ids)
                sw.copy_(w)
                sgy.copy_(gy)
            graph.replay()

        fns = [lambda: eager(True, 0), replay, lambda: eager(False, 1)]
        names = ["device_eager_us", "device_graph_us", "loop_eager_us"]
        runs = [timed_alternating(fns, args.iters, args.warmup) for _ in range(args.repeats)]
        row = {"tokens": T, "pairs": T * K, "experts_hit": [len(set(s[1].view(-1).tolist())) for s in sets]}
        for i, name in enumerate(names):
            vals = sorted(r[i] for r in runs)
            row[name] = vals[len(vals) // 2]
            row[name.replace("_us", "_spread_us")] = round(vals[-1] - vals[0], 2)
        for name, route in (("device_peak_delta_mb", True), ("loop_peak_delta_mb", False)):
            torch.cuda.synchronize()
            for s in sets:
                s[0].grad = s[2].grad = None
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            eager(route, 0)
            torch.cuda.synchronize()
            row[name] = round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1)
        x = sets[0][0]  # the two routes on the same step: the gradients differ in their last bits only
        turn[0] = turn[1] = 0
        eager(True, 0)
        a = x.grad.float().clone()
        eager(False, 1)
        row["x_grad_rel_diff_device_vs_loop"] = float(((a - x.grad.float()).abs().mean() / x.grad.float().abs().mean()).item())
        del graph
        rows.append(row)
        print(json.dumps(row), flush=True)
    result = {"block": {"hidden": H, "intermediate": I, "experts": E, "top_k": K, "scheme": "1x16g8", "dtype": "float16"},
              "device": torch.cuda.get_device_name(dev), "iters": args.iters, "repeats": args.repeats, "warmup": args.warmup,
              "what": "forward + backward of one experts block, x and top_k_weights requiring grad; median over the repeats of the "
                      "median step time (device events), spread = max - min over the repeats; three input sets in rotation",
              "rows": rows,
              "command": f"python tools/moe_benchmark.py --backward --tokens {args.tokens} --iters {args.iters} --repeats {args.repeats}"}
    out = args.out or os.path.join("profiles", "moe_grouped_backward.json")
    os.makedirs(os.path.dirname(out) or ".", exist_ok=True)
    with open(out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))


def packed_main(args):
    import aqlm_amd.moe as moe

    dev = torch.device("cuda:0")
    q, _ = build(dev, False)
    qp, _ = build(dev, False)  # same seed: the same weights, prepacked
    report = moe.prepack_experts(qp)
    moe.ROUTED_PACKED_MAX_PAIRS = moe.MAX_ROUTED_PAIRS  # measure the route at every T; the constant is this run's result
    gen = torch.Generator(device=dev).manual_seed(1)
    names = ["routed_graph_us", "routed_packed_graph_us", "loop_eager_us", "routed_packed_eager_us"]
    rows = []
    with torch.no_grad():
        for T in [int(t) for t in args.tokens.split(",")]:
            x = torch.randn((T, H), generator=gen, device=dev).half()
            logits = torch.randn((T, E), generator=gen, device=dev)
            w, ids = torch.topk(torch.softmax(logits, -1), K, dim=-1)
            w = w / w.sum(-1, keepdim=True)
            assert qp._routed_packed_tables_for(x, ids) is not None, "the prepacked block does not take the routed packed launches"
            g_direct, g_packed = captured(lambda: q(x, ids, w)), captured(lambda: qp(x, ids, w))
            fns = [g_direct.replay, g_packed.replay, lambda: loop_forward(q, x, ids, w), lambda: qp(x, ids, w)]
            runs = [timed_alternating(fns, args.iters, args.warmup) for _ in range(args.repeats)]
            row = {"tokens": T, "pairs": T * K, "experts_hit": len(set(ids.view(-1).tolist()))}
            for i, name in enumerate(names):
                vals = sorted(r[i] for r in runs)
                row[name] = vals[len(vals) // 2]
                row[name.replace("_us", "_runs_us")] = [r[i] for r in runs]
            row["routed_graph_spread_us"] = round(max(r[0] for r in runs) - min(r[0] for r in runs), 2)
            row["packed_wins"] = bool(max(r[1] for r in runs) < min(r[0] for r in runs) - row["routed_graph_spread_us"]
                                      and max(r[1] for r in runs) < min(r[2] for r in runs))
            del g_direct, g_packed
            rows.append(row)
            print(json.dumps(row), flush=True)
    best = 0
    for row in rows:  # the largest pair count UP TO which the prepacked block wins
        if not row["packed_wins"]:
            break
        best = row["pairs"]
    result = {"block": {"hidden": H, "intermediate": I, "experts": E, "top_k": K, "scheme": "1x16g8", "dtype": "float16"},
              "device": torch.cuda.get_device_name(dev), "iters": args.iters, "repeats": args.repeats, "estimate": ESTIMATE,
              "prepack_experts": report, "rows": rows, "routed_packed_max_pairs": best,
              "rule": "packed_wins: every repeat of routed_packed_graph_us below the smallest routed_graph_us minus its spread over "
                      "the repeats, and below every loop_eager_us; routed_packed_max_pairs: the largest pairs up to which all rows win",
              "command": f"python tools/moe_benchmark.py --only packed --tokens {args.tokens} --iters {args.iters} --repeats {args.repeats}"}
    out = args.out or os.path.join("profiles", "moe_block_packed.json")
    os.makedirs(os.path.dirname(out) or ".", exist_ok=True)
    with open(out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tokens", default=None)
    ap.add_argument("--grouped", action="store_true")
    ap.add_argument("--backward", action="store_true")
    ap.add_argument("--only", choices=["routed", "graph", "loop", "dense", "packed"], default=None)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.backward:
        args.tokens = args.tokens or "8,32,128,512"
        return backward_main(args)
    if args.grouped:
        args.tokens = args.tokens or "1,2,4,8,16,32,40,64,128,256,512"
        return grouped_main(args)
    if args.only == "packed":
        args.tokens = args.tokens or "1,2,4,8,16,32"
        return packed_main(args)
    args.tokens = args.tokens or "1,2,4,8,16"
    args.out = args.out or os.path.join("profiles", "moe_block.json")
    dev = torch.device("cuda:0")
    modes = [args.only] if args.only else ["routed", "graph", "loop", "dense"]
    q, dense = build(dev, "dense" in modes)
    rows = []
    gen = torch.Generator(device=dev).manual_seed(1)
    with torch.no_grad():
        for T in [int(t) for t in args.tokens.split(",")]:
            x = torch.randn((T, H), generator=gen, device=dev).half()
            logits = torch.randn((T, E), generator=gen, device=dev)
            w, ids = torch.topk(torch.softmax(logits, -1), K, dim=-1)
            w = w / w.sum(-1, keepdim=True)
            row = {"tokens": T, "experts_hit": len(set(ids.view(-1).tolist()))}
            if "routed" in modes:
                row["routed_eager_us"] = timed(lambda: q(x, ids, w), args.iters, args.warmup)
            if "graph" in modes:
                q(x, ids, w)
                torch.cuda.synchronize()
                s = torch.cuda.Stream()
                s.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(s):
                    q(x, ids, w)
                torch.cuda.current_stream().wait_stream(s)
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):
                    q(x, ids, w)
                row["routed_graph_us"] = timed(g.replay, args.iters, args.warmup)
                del g
            if "loop" in modes:
                row["loop_eager_us"] = timed(lambda: loop_forward(q, x, ids, w), args.iters, args.warmup)
            if "dense" in modes:
                row["dense_fp16_eager_us"] = timed(lambda: dense(x, ids, w), args.iters, args.warmup)
            rows.append(row)
            print(json.dumps(row), flush=True)
    result = {"block": {"hidden": H, "intermediate": I, "experts": E, "top_k": K, "scheme": "1x16g8", "dtype": "float16"},
              "device": torch.cuda.get_device_name(dev), "estimate": ESTIMATE, "rows": rows}
    if not args.only:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
