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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tokens", default="1,2,4,8,16,32,64,128")
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join("profiles", "lora_moe.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/lora_moe_benchmark.py measures on the GPU; none found")

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
