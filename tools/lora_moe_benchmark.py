#!/usr/bin/env python
"""LoRA adapters on the routed experts of one Mixtral-8x7B-shaped block (8 experts, hidden 4096, intermediate 14336, top_k 2;
1x16 g8, random codes, fp16; prepacked with ``aqlm_amd.moe.prepack_experts``), rank 16 on w1 / w2 / w3 of all experts, at
T = 1 / 2 / 4 / 8 / 16 / 32 / 64 / 128 tokens (2 .. 256 pairs), with one adapter for every token and with 4 adapters mixed per
token.  Three routes, each captured in a hipGraph and replayed (the protocol of tools/lora_benchmark.py):
  (a) base  -- the block without adapters (``bank.select(None)``: the bare block's launches; up to 64 pairs the routed packed
               launches, beyond them the expert-grouped GEMM);
  (b) torch -- ``aqlm_amd.lora``'s torch path on top of the same base launches (``ROUTED_BGMV_MAX_PAIRS = 0``): PEFT's formula per
               (adapter, expert), masked by adapter id and expert id;
  (c) hip   -- the two launches of aqlm_hip_lora_bgmv_routed per projection group, in place on the base launches' outputs.
The replays of the three alternate within one process; every replay first copies the next of three input sets into the static
input (inside the timed window, the same for all three); device events; median over --repeats rounds of the median of --iters
replays, spread = max - min over the rounds.  The routing is that of tools/moe_benchmark.py --only packed (same generator, same
order), so ``base_graph_us`` can be held against ``routed_packed_graph_us`` of profiles/moe_block_packed.json up to T = 32 (there
without the input copy).  ``routed_bgmv_max_pairs`` in the output is the largest pair count up to which (c) beat (b) in both
adapter mixes at every measured count -- every round of (c) below the smallest round of (b) minus (b)'s spread -- and is what
``aqlm_amd.lora.ROUTED_BGMV_MAX_PAIRS`` is set to (0 when it wins nowhere).  Writes --out (default profiles/lora_moe.json).

    python tools/lora_moe_benchmark.py [--tokens 1,2,4,8,16,32,64,128] [--iters 30] [--repeats 3]

``--prefill`` measures the prefill route instead, on the same block and with the same protocol: T = 256 / 512 / 1024 / 2048 / 4096
tokens (512 .. 8192 pairs, the grouped base launches under capture), three adapter mixes (one adapter; 4 adapters as 4 contiguous
sequences; 4 adapters interleaved per token), (b) with ``ROUTED_SGMV_MAX_PAIRS = 0`` against (c) the two launches of
aqlm_hip_lora_sgmv_routed per projection group plus the 16-pair bucket launch.  ``routed_sgmv_max_pairs`` in the output is the
largest pair count up to which (c) beat (b) at that count and every smaller one in all three mixes, the launch's own limit when it
won at every measured count, and is what ``aqlm_amd.lora.ROUTED_SGMV_MAX_PAIRS`` is set to.  As data only, ``eager_rows`` holds
eager calls at 1024 / 2048 / 4096 pairs: the per-expert loop with ``on_rows`` (what an eager call of that size runs) against the
grouped base launches with the new route (``moe.GROUPED_EAGER_MAX_PAIRS`` raised for the measurement).  Writes --out (default
profiles/lora_moe_prefill.json).

    python tools/lora_moe_benchmark.py --prefill [--tokens 256,512,1024,2048,4096] [--iters 20] [--repeats 3]

``--train`` measures a TRAINING step -- forward + backward, hidden_states requiring grad, adapter ``ad0`` trainable, the other
three frozen, a fixed grad-output -- on the same block at T = 8 / 256 / 1024 / 4096 tokens (16 .. 8192 pairs) in the three mixes of
``--prefill``, plus one skewed routing at 2048 pairs (three tokens in four on experts 0 and 1): (a) the bare block's step
(``bank.select(None)``), (b) the torch path of the same commit (``ROUTED_TRAIN_MAX_PAIRS = 0``), (c) the device route
(aqlm_hip_lora_sgmv_routed under autograd, its backward on the transposed table plus aqlm_hip_lora_grad_routed).  Each both eager
(host clock around a step that ends in a device synchronise) and captured in a hipGraph and replayed (device events); median
over --repeats rounds of the median of --iters steps, spread = max - min over the rounds; the peak-memory delta of one eager step
(``torch.cuda.max_memory_allocated`` over the memory allocated before it).  ``routed_train_max_pairs`` in the output is the
largest pair count up to which (c) beat (b), eager AND captured, at that count and every smaller one in every mix, the launch's
own limit when it won at every measured count, and is what ``aqlm_amd.lora.ROUTED_TRAIN_MAX_PAIRS`` is set to.  Writes --out
(default profiles/lora_moe_train.json).

    python tools/lora_moe_benchmark.py --train [--tokens 8,256,1024,4096] [--iters 20] [--repeats 3]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from lora_benchmark import captured, timed_alternating  # noqa: E402
from moe_benchmark import E, H, I, K, build  # noqa: E402

RANK, ADAPTERS, SETS = 16, 4, 3


class Holder(torch.nn.Module):
    def __init__(self, experts):
        super().__init__()
        self.experts = experts


def adapter(seed):
    gen = torch.Generator().manual_seed(seed)
    state = {}
    for e in range(E):
        for w, (fin, fout) in (("w1", (H, I)), ("w3", (H, I)), ("w2", (I, H))):
            state[f"base_model.model.experts.{e}.{w}.lora_A.weight"] = (torch.randn((RANK, fin), generator=gen) / fin ** 0.5).half()
            state[f"base_model.model.experts.{e}.{w}.lora_B.weight"] = (torch.randn((fout, RANK), generator=gen) * 0.02).half()
    return state, {"peft_type": "LORA", "r": RANK, "lora_alpha": 2 * RANK, "bias": "none", "target_modules": ["w1", "w2", "w3"]}


PREFILL_TOKENS = "256,512,1024,2048,4096"
EAGER_PAIRS = (1024, 2048, 4096)


def timed_eager(fns, iters, warmup):
    """median per call of each of the eager `fns`, interleaved; a host clock around work that ends in a device synchronise (the
    per-expert loop syncs with the host, so device events alone would miss its waits)"""
    import time

    for _ in range(warmup):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    times = [[] for _ in fns]
    for _ in range(iters):
        for i, fn in enumerate(fns):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times[i].append((time.perf_counter() - t0) * 1e6)
    return [round(sorted(t)[len(t) // 2], 2) for t in times]


def prefill(args):
    """--prefill: base / torch path / routed sgmv at prefill pair counts, three adapter mixes; writes profiles/lora_moe_prefill.json."""
    import aqlm_amd.lora as lora
    import aqlm_amd.moe as moe
    from aqlm_amd import _native

    dev = torch.device("cuda:0")
    q, _ = build(dev, False)
    report = moe.prepack_experts(q)
    holder = Holder(q)
    bank = lora.attach_adapters(holder, {f"ad{i}": adapter(100 + i) for i in range(ADAPTERS)})
    block = holder.experts
    gen = torch.Generator(device=dev).manual_seed(1)
    names = ["base_graph_us", "torch_graph_us", "hip_graph_us"]
    token_counts = [int(t) for t in args.tokens.split(",")]
    limit = _native.MAX_LORA_SGMV_ROUTED_PAIRS
    table, eager_rows = [], []
    with torch.no_grad():
        for T in token_counts:
            if T % ADAPTERS:
                raise SystemExit(f"--prefill: {T} tokens do not split into {ADAPTERS} sequences")
            sets = [torch.randn((T, H), generator=gen, device=dev).half() for _ in range(SETS)]
            logits = torch.randn((T, E), generator=gen, device=dev)
            w, idx = torch.topk(torch.softmax(logits, -1), K, dim=-1)
            w = w / w.sum(-1, keepdim=True)
            seq_ids = torch.arange(ADAPTERS, device=dev, dtype=torch.int64)
            tok_ids = (torch.arange(T, device=dev) % ADAPTERS).to(torch.int64)
            mixes = (("one adapter", "ad0"), (f"{ADAPTERS} adapters, contiguous sequences", seq_ids),
                     (f"{ADAPTERS} adapters interleaved per token", tok_ids))
            for mix, selection in mixes:
                static = sets[0].clone()
                graphs, outs = [], []
                for which, max_pairs in ((None, 0), (selection, 0), (selection, limit)):
                    bank.select(which)
                    lora.ROUTED_SGMV_MAX_PAIRS = max_pairs  # the route is decided when the call is captured
                    g, out = captured(lambda: block(static, idx, w))
                    graphs.append(g)
                    outs.append(out)
                turn = [0] * len(graphs)

                def replay(i):
                    static.copy_(sets[turn[i] % SETS])
                    turn[i] += 1
                    graphs[i].replay()

                fns = [lambda i=i: replay(i) for i in range(len(graphs))]
                runs = [timed_alternating(fns, args.iters, args.warmup) for _ in range(args.repeats)]
                row = {"tokens": T, "pairs": T * K, "adapters": mix}
                for i, name in enumerate(names):
                    vals = sorted(r[i] for r in runs)
                    row[name] = vals[len(vals) // 2]
                    row[name.replace("_us", "_runs_us")] = [r[i] for r in runs]
                    row[name.replace("_us", "_spread_us")] = round(vals[-1] - vals[0], 2)
                row["hip_wins"] = bool(max(r[2] for r in runs) < min(r[1] for r in runs) - row["torch_graph_spread_us"])
                static.copy_(sets[0])
                for g in graphs:
                    g.replay()
                torch.cuda.synchronize()
                row["rel_diff_hip_vs_torch"] = float(((outs[2].float() - outs[1].float()).abs().mean()
                                                      / outs[1].float().abs().mean()).item())
                row["rel_size_of_the_adapter_term"] = float(((outs[1].float() - outs[0].float()).abs().mean()
                                                             / outs[0].float().abs().mean()).item())
                del graphs, outs
                table.append(row)
                print(json.dumps(row), flush=True)
                if T * K in EAGER_PAIRS:  # data only: what an eager call of this size runs against the grouped base + new route
                    bank.select(selection)
                    x0 = sets[0]
                    keep = moe.GROUPED_EAGER_MAX_PAIRS

                    def loop():
                        moe.GROUPED_EAGER_MAX_PAIRS = keep
                        return block(x0, idx, w)

                    def grouped():
                        moe.GROUPED_EAGER_MAX_PAIRS = moe.MAX_GROUPED_PAIRS
                        try:
                            return block(x0, idx, w)
                        finally:
                            moe.GROUPED_EAGER_MAX_PAIRS = keep

                    lora.ROUTED_SGMV_MAX_PAIRS = limit
                    assert not q.takes_grouped_path(x0, idx), "an eager call of this size was expected to run the per-expert loop"
                    eruns = [timed_eager([loop, grouped], max(args.iters // 2, 3), 2) for _ in range(args.repeats)]
                    erow = {"tokens": T, "pairs": T * K, "adapters": mix}
                    for i, name in enumerate(("eager_loop_on_rows_us", "eager_grouped_sgmv_us")):
                        vals = sorted(r[i] for r in eruns)
                        erow[name] = vals[len(vals) // 2]
                        erow[name.replace("_us", "_runs_us")] = [r[i] for r in eruns]
                    erow["rel_diff"] = float(((grouped().float() - loop().float()).abs().mean() / loop().float().abs().mean()).item())
                    eager_rows.append(erow)
                    print(json.dumps(erow), flush=True)
    best, all_won = 0, True
    for T in token_counts:  # the largest pair count UP TO which the new route wins in all three mixes
        if not all(r["hip_wins"] for r in table if r["tokens"] == T):
            all_won = False
            break
        best = T * K
    result = {"block": {"hidden": H, "intermediate": I, "experts": E, "top_k": K, "scheme": "1x16g8", "dtype": "float16",
                        "rank": RANK, "adapters": ADAPTERS, "projections": ["w1", "w3", "w2"]},
              "device": torch.cuda.get_device_name(dev), "iters": args.iters, "repeats": args.repeats, "warmup": args.warmup,
              "prepack_experts": report,
              "what": "one block forward captured in a hipGraph and replayed, the copy of the next of three input sets included; "
                      "median over the repeats of the median replay (device events), spread = max - min over the repeats; "
                      "eager_rows (data only): eager calls, host clock around a call that ends in a device synchronise, the "
                      "per-expert loop + on_rows against the grouped base launches + aqlm_hip_lora_sgmv_routed",
              "rows": table, "eager_rows": eager_rows, "hip_won_at_every_count": all_won, "largest_count_won_up_to": best,
              "routed_sgmv_max_pairs": limit if all_won else best,
              "rule": "hip_wins: every repeat of hip_graph_us below the smallest torch_graph_us minus its spread over the repeats; "
                      "routed_sgmv_max_pairs: the largest pair count up to which all three adapter mixes win at that count and "
                      "every smaller one; the launch's own limit when it won at every measured count; 0 when it never won",
              "command": f"python tools/lora_moe_benchmark.py --prefill --tokens {args.tokens} --iters {args.iters} "
                         f"--repeats {args.repeats}"}
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps({k: v for k, v in result.items() if k not in ("rows", "eager_rows")}))


TRAIN_TOKENS = "8,256,1024,4096"
SKEWED_TOKENS = 1024


def train(args):
    """--train: forward + backward of base / torch path / device route, eager and captured; writes profiles/lora_moe_train.json."""
    import aqlm_amd.lora as lora
    import aqlm_amd.moe as moe
    from aqlm_amd import _native

    dev = torch.device("cuda:0")
    q, _ = build(dev, False)
    report = moe.prepack_experts(q)
    holder = Holder(q)
    bank = lora.attach_adapters(holder, {f"ad{i}": adapter(100 + i) for i in range(ADAPTERS)})
    block = holder.experts
    trained = [p for store in (block.lora_A, block.lora_B) for p in store["ad0"].parameters()]
    for p in trained:
        p.requires_grad_(True)
    gen = torch.Generator(device=dev).manual_seed(1)
    limit = _native.MAX_LORA_SGMV_ROUTED_PAIRS
    routes = (("base", None, 0), ("torch", "selection", 0), ("hip", "selection", limit))
    token_counts = [int(t) for t in args.tokens.split(",")]
    cases = [(T, False) for T in token_counts] + ([(SKEWED_TOKENS, True)] if SKEWED_TOKENS in token_counts else [])
    table = []
    for T, skewed in cases:
        if T % ADAPTERS:
            raise SystemExit(f"--train: {T} tokens do not split into {ADAPTERS} sequences")
        x = torch.randn((T, H), generator=gen, device=dev).half().requires_grad_()
        logits = torch.randn((T, E), generator=gen, device=dev)
        if skewed:
            logits[torch.arange(T, device=dev) % 4 != 3, :2] += 20.0
        w, idx = torch.topk(torch.softmax(logits, -1), K, dim=-1)
        w = w / w.sum(-1, keepdim=True)
        r = torch.randn((T, H), generator=gen, device=dev)
        seq_ids = torch.arange(ADAPTERS, device=dev, dtype=torch.int64)
        tok_ids = (torch.arange(T, device=dev) % ADAPTERS).to(torch.int64)
        mixes = (("one adapter", "ad0"), (f"{ADAPTERS} adapters, contiguous sequences", seq_ids),
                 (f"{ADAPTERS} adapters interleaved per token", tok_ids))
        for mix, selection in (mixes[2:] if skewed else mixes):

            def step():
                x.grad = None
                for p in trained:
                    p.grad = None
                (block(x, idx, w).float() * r).sum().backward()

            def eager(which, max_pairs):
                bank.select(selection if which else None)
                lora.ROUTED_TRAIN_MAX_PAIRS = max_pairs
                step()

            graphs, grads, peaks = [], [], []
            for name, which, max_pairs in routes:
                bank.select(selection if which else None)
                lora.ROUTED_TRAIN_MAX_PAIRS = max_pairs  # the route is decided when the step is captured
                step()
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats()
                before = torch.cuda.memory_allocated()
                step()
                torch.cuda.synchronize()
                peaks.append(round((torch.cuda.max_memory_allocated() - before) / 2 ** 20, 1))
                g, _ = captured(step)
                graphs.append(g)
                g.replay()
                torch.cuda.synchronize()
                grads.append([x.grad.float().clone()] + [p.grad.float().clone() for p in trained if p.grad is not None])
            fns_graph = [g.replay for g in graphs]
            fns_eager = [lambda which=which, max_pairs=max_pairs: eager(which, max_pairs) for _, which, max_pairs in routes]
            runs_g = [timed_alternating(fns_graph, args.iters, args.warmup) for _ in range(args.repeats)]
            runs_e = [timed_eager(fns_eager, args.iters, 2) for _ in range(args.repeats)]
            row = {"tokens": T, "pairs": T * K, "adapters": mix, "routing": "skewed" if skewed else "router-like",
                   "pairs_per_expert": torch.bincount(idx.reshape(-1), minlength=E).tolist()}
            for kind, runs in (("graph", runs_g), ("eager", runs_e)):
                for i, (name, _, _) in enumerate(routes):
                    vals = sorted(rr[i] for rr in runs)
                    row[f"{name}_{kind}_us"] = vals[len(vals) // 2]
                    row[f"{name}_{kind}_runs_us"] = [rr[i] for rr in runs]
                    row[f"{name}_{kind}_spread_us"] = round(vals[-1] - vals[0], 2)
                row[f"hip_wins_{kind}"] = bool(max(rr[2] for rr in runs) < min(rr[1] for rr in runs) - row[f"torch_{kind}_spread_us"])
            row["hip_wins"] = row["hip_wins_graph"] and row["hip_wins_eager"]
            for (name, _, _), peak in zip(routes, peaks):
                row[f"{name}_peak_delta_mb"] = peak
            rel = lambda a, b: float(((a - b).abs().mean() / b.abs().mean()).item())  # noqa: E731
            row["rel_diff_x_grad_hip_vs_torch"] = rel(grads[2][0], grads[1][0])
            row["rel_diff_weight_grads_hip_vs_torch"] = max(rel(a, b) for a, b in zip(grads[2][1:], grads[1][1:]) if float(b.abs().max()))
            del graphs, grads
            table.append(row)
            print(json.dumps(row), flush=True)
    best, all_won = 0, True
    for T in token_counts:  # the largest pair count UP TO which the device route wins in every mix
        if not all(row["hip_wins"] for row in table if row["tokens"] == T):
            all_won = False
            break
        best = T * K
    result = {"block": {"hidden": H, "intermediate": I, "experts": E, "top_k": K, "scheme": "1x16g8", "dtype": "float16",
                        "rank": RANK, "adapters": ADAPTERS, "trained": ["ad0"], "projections": ["w1", "w3", "w2"]},
              "device": torch.cuda.get_device_name(dev), "iters": args.iters, "repeats": args.repeats, "warmup": args.warmup,
              "prepack_experts": report,
              "what": "one training step of the block (forward + backward, hidden_states and adapter ad0 requiring grad): *_graph_us "
                      "captured in a hipGraph and replayed (device events), *_eager_us eager (host clock, ends in a device "
                      "synchronise); median over the repeats of the median step, spread = max - min over the repeats; "
                      "*_peak_delta_mb: torch.cuda.max_memory_allocated of one eager step over the memory allocated before it",
              "rows": table, "hip_won_at_every_count": all_won, "largest_count_won_up_to": best,
              "routed_train_max_pairs": limit if all_won else best,
              "rule": "hip_wins_{graph,eager}: every repeat of hip below the smallest torch minus its spread over the repeats; "
                      "hip_wins: both; routed_train_max_pairs: the largest pair count up to which every mix wins at that count and "
                      "every smaller one; the launch's own limit when it won at every measured count; 0 when it never won",
              "command": f"python tools/lora_moe_benchmark.py --train --tokens {args.tokens} --iters {args.iters} "
                         f"--repeats {args.repeats}"}
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps({k: v for k, v in result.items() if k != "rows"}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--train", action="store_true",
                    help=f"measure a training step (forward + backward) at {TRAIN_TOKENS} tokens, the device route against the torch "
                         "path; writes profiles/lora_moe_train.json")
    ap.add_argument("--prefill", action="store_true",
                    help=f"measure the prefill route (aqlm_hip_lora_sgmv_routed) at {PREFILL_TOKENS} tokens against the torch path; "
                         "writes profiles/lora_moe_prefill.json")
    ap.add_argument("--tokens", default=None, help="default 1,2,4,8,16,32,64,128; with --prefill " + PREFILL_TOKENS)
    ap.add_argument("--iters", type=int, default=None, help="default 30; with --prefill 20")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None, help="default profiles/lora_moe.json; with --prefill profiles/lora_moe_prefill.json")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/lora_moe_benchmark.py measures on the GPU; none found")
    if args.train:
        args.tokens = args.tokens or TRAIN_TOKENS
        args.iters = args.iters or 20
        args.out = args.out or os.path.join("profiles", "lora_moe_train.json")
        return train(args)
    if args.prefill:
        args.tokens = args.tokens or PREFILL_TOKENS
        args.iters = args.iters or 20
        args.out = args.out or os.path.join("profiles", "lora_moe_prefill.json")
        return prefill(args)
    args.tokens = args.tokens or "1,2,4,8,16,32,64,128"
    args.iters = args.iters or 30
    args.out = args.out or os.path.join("profiles", "lora_moe.json")

    import aqlm_amd.lora as lora
    import aqlm_amd.moe as moe
    from aqlm_amd import _native

    dev = torch.device("cuda:0")
    q, _ = build(dev, False)
    report = moe.prepack_experts(q)
    holder = Holder(q)
    bank = lora.attach_adapters(holder, {f"ad{i}": adapter(100 + i) for i in range(ADAPTERS)})
    block = holder.experts
    gen = torch.Generator(device=dev).manual_seed(1)    # the inputs and routing of tools/moe_benchmark.py --only packed
    gen2 = torch.Generator(device=dev).manual_seed(2)   # the two other input sets
    names = ["base_graph_us", "torch_graph_us", "hip_graph_us"]
    token_counts = [int(t) for t in args.tokens.split(",")]
    table = []
    with torch.no_grad():
        for T in token_counts:
            x = torch.randn((T, H), generator=gen, device=dev).half()
            logits = torch.randn((T, E), generator=gen, device=dev)
            w, idx = torch.topk(torch.softmax(logits, -1), K, dim=-1)
            w = w / w.sum(-1, keepdim=True)
            sets = [x] + [torch.randn((T, H), generator=gen2, device=dev).half() for _ in range(SETS - 1)]
            ids = (torch.arange(T, device=dev) % ADAPTERS).to(torch.int64)
            base_route = ("routed packed" if q._prepack is not None and q.takes_routed_path(x, idx)
                          and q._routed_packed_tables_for(x, idx) is not None else
                          "routed" if q.takes_routed_path(x, idx) else "grouped" if q.takes_grouped_path(x, idx) else "loop")
            for mix, selection in (("one adapter", "ad0"), (f"{ADAPTERS} adapters mixed per token", ids)):
                static = sets[0].clone()
                graphs, outs = [], []
                for which, max_pairs in ((None, 0), (selection, 0), (selection, _native.MAX_LORA_ROWS)):
                    bank.select(which)
                    lora.ROUTED_BGMV_MAX_PAIRS = max_pairs  # the route is decided when the call is captured
                    g, out = captured(lambda: block(static, idx, w))
                    graphs.append(g)
                    outs.append(out)
                turn = [0] * len(graphs)

                def replay(i):
                    static.copy_(sets[turn[i] % SETS])
                    turn[i] += 1
                    graphs[i].replay()

                fns = [lambda i=i: replay(i) for i in range(len(graphs))]
                runs = [timed_alternating(fns, args.iters, args.warmup) for _ in range(args.repeats)]
                row = {"tokens": T, "pairs": T * K, "adapters": mix, "base_route": base_route,
                       "experts_hit": len(set(idx.view(-1).tolist()))}
                for i, name in enumerate(names):
                    vals = sorted(r[i] for r in runs)
                    row[name] = vals[len(vals) // 2]
                    row[name.replace("_us", "_runs_us")] = [r[i] for r in runs]
                    row[name.replace("_us", "_spread_us")] = round(vals[-1] - vals[0], 2)
                row["hip_wins"] = bool(max(r[2] for r in runs) < min(r[1] for r in runs) - row["torch_graph_spread_us"])
                static.copy_(sets[0])
                for g in graphs:
                    g.replay()
                torch.cuda.synchronize()
                row["rel_diff_hip_vs_torch"] = float(((outs[2].float() - outs[1].float()).abs().mean()
                                                      / outs[1].float().abs().mean()).item())
                row["rel_size_of_the_adapter_term"] = float(((outs[1].float() - outs[0].float()).abs().mean()
                                                             / outs[0].float().abs().mean()).item())
                del graphs, outs
                table.append(row)
                print(json.dumps(row), flush=True)
    best = 0
    for T in token_counts:  # the largest pair count UP TO which the HIP route wins
        if not all(r["hip_wins"] for r in table if r["tokens"] == T):
            break
        best = T * K
    result = {"block": {"hidden": H, "intermediate": I, "experts": E, "top_k": K, "scheme": "1x16g8", "dtype": "float16",
                        "rank": RANK, "adapters": ADAPTERS, "projections": ["w1", "w3", "w2"]},
              "device": torch.cuda.get_device_name(dev), "iters": args.iters, "repeats": args.repeats, "warmup": args.warmup,
              "prepack_experts": report,
              "what": "one block forward captured in a hipGraph and replayed, the copy of the next of three input sets included; "
                      "median over the repeats of the median replay (device events), spread = max - min over the repeats",
              "rows": table, "routed_bgmv_max_pairs": best,
              "rule": "hip_wins: every repeat of hip_graph_us below the smallest torch_graph_us minus its spread over the repeats; "
                      "routed_bgmv_max_pairs: the largest pair count up to which both adapter mixes win at every measured count",
              "command": f"python tools/lora_moe_benchmark.py --tokens {args.tokens} --iters {args.iters} --repeats {args.repeats}"}
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps({k: v for k, v in result.items() if k != "rows"}))


if __name__ == "__main__":
    main()
