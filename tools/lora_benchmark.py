#!/usr/bin/env python
"""LoRA adapters on a Llama-3-8B-shaped decoder block of prepacked 1x16 g8 layers (hidden 4096, 8 KV heads of 128, intermediate
14336; random codes, fp16), rank 16 on all seven projections, at 1 / 2 / 4 / 8 / 16 / 32 / 64 rows, with one adapter for every row
and with 4 adapters mixed over the rows.  Three routes, each captured in a hipGraph and replayed:
  (a) base   -- the block without adapters (``bank.select(None)``);
  (b) plain  -- the adapters as plain torch ops on top of the unchanged base layers: PEFT's formula ``y + (x @ A^T) @ B^T * scaling``
                per layer, what a user of this package wrote before the batched launch existed (4 adapters: the same per adapter,
                masked by ``ids == a`` -- a loop over the adapters, so it stays capturable);
  (c) bgmv   -- the two launches of aqlm_hip_lora_bgmv per layer (``aqlm_amd.lora`` with the route forced on).
The replays of the three alternate within one process; every replay first copies the next of three input sets into the static
input (inside the timed window, the same for all three); device events; median over --repeats rounds of the median of --iters
replays, spread = max - min over the rounds.  ``bgmv_max_rows`` in the output is the largest row count up to which (c) beat (b) in
both adapter mixes -- every round of (c) below the smallest round of (b) minus (b)'s spread -- and is what
``aqlm_amd.lora.BGMV_MAX_ROWS`` is set to.  Writes --out (default profiles/lora_bgmv.json).

    python tools/lora_benchmark.py [--rows 1,2,4,8,16,32,64] [--iters 50] [--repeats 3]

``--prefill`` measures the row counts above the BGMV route instead -- 96 / 128 / 256 / 512 / 1024 / 2048 / 4096 rows, the same
block, the same protocol -- with three adapter mixes: one adapter by name; 4 adapters as 4 contiguous sequences (per-sequence ids
of a [4, rows / 4, H] input); 4 adapters interleaved row by row (every 16-row tile holds all four: the worst case for the passes
of the segmented kernel).  Routes: (a) base, (b) torch -- ``aqlm_amd.lora``'s torch path, what these row counts ran before the
segmented launch existed (both row limits 0), (c) sgmv -- the two launches of aqlm_hip_lora_sgmv per layer.  ``sgmv_max_rows`` is
the largest row count up to which (c) beat (b) in all three mixes by the rule above, and is what ``aqlm_amd.lora.SGMV_MAX_ROWS`` is
set to (AQLM_HIP_MAX_LORA_SGMV_ROWS when it won at every count, 0 when it lost at the first).  ``sgmv_op_us`` times the two
launches alone, captured, per distinct projection shape.  Writes --out (default profiles/lora_sgmv.json).

    python tools/lora_benchmark.py --prefill [--rows 96,128,256,512,1024,2048,4096] [--iters 50] [--repeats 3]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

H, KV, I, RANK, ADAPTERS, SETS = 4096, 1024, 14336, 16, 4, 3
SHAPES = {"q_proj": (H, H), "k_proj": (H, KV), "v_proj": (H, KV), "o_proj": (H, H), "gate_proj": (H, I), "up_proj": (H, I),
          "down_proj": (I, H)}


class Block(torch.nn.Module):
    """The seven projections in a decoder block's data flow (attention and norms left out: they are the same in every route)."""

    def __init__(self, dev):
        super().__init__()
        from aqlm_amd import QuantizedLinear

        gen = torch.Generator(device=dev).manual_seed(0)
        for name, (fin, fout) in SHAPES.items():
            lin = QuantizedLinear(fin, fout, 8, 1, 1, 16, bias=False, device=dev, dtype=torch.float16)
            with torch.no_grad():
                lin.codes.copy_(torch.randint(-32768, 32768, lin.codes.shape, generator=gen, device=dev, dtype=torch.int32))
                lin.codebooks.copy_(torch.randn(lin.codebooks.shape, generator=gen, device=dev) * 0.05)
                lin.scales.copy_(torch.rand(lin.scales.shape, generator=gen, device=dev) * 0.2 + 0.05)
            setattr(self, name, lin)

    def forward(self, h):
        q, k, v = self.q_proj(h), self.k_proj(h), self.v_proj(h)
        h2 = self.o_proj(q)
        return self.down_proj(self.gate_proj(h2) * self.up_proj(h2)), k, v


def adapter(seed):
    gen = torch.Generator().manual_seed(seed)
    state = {}
    for name, (fin, fout) in SHAPES.items():
        state[f"base_model.model.{name}.lora_A.weight"] = (torch.randn((RANK, fin), generator=gen) / fin ** 0.5).half()
        state[f"base_model.model.{name}.lora_B.weight"] = (torch.randn((fout, RANK), generator=gen) * 0.02).half()
    return state, {"peft_type": "LORA", "r": RANK, "lora_alpha": 2 * RANK, "bias": "none", "target_modules": sorted(SHAPES)}


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
        out = fn()
    return g, out


def timed_alternating(fns, iters, warmup):
    """median per call of each of `fns`, their calls interleaved (a, b, c, a, b, c, ...) so that clocks and caches drift alike"""
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


PREFILL_ROWS = "96,128,256,512,1024,2048,4096"


def prefill(args):
    """--prefill: base / torch path / sgmv at prefill row counts, three adapter mixes; writes profiles/lora_sgmv.json."""
    import aqlm_amd.lora as lora
    from aqlm_amd import _native
    from aqlm_amd.inference_kernels import hip_kernel

    dev = torch.device("cuda:0")
    block = Block(dev)
    with torch.no_grad():
        block(torch.zeros((1, H), dtype=torch.float16, device=dev))
    prepacked = sum(getattr(block, n)._packed_codes is not None for n in SHAPES)
    bank = lora.attach_adapters(block, {f"ad{i}": adapter(100 + i) for i in range(ADAPTERS)})
    gen = torch.Generator(device=dev).manual_seed(1)
    names = ["base_graph_us", "torch_graph_us", "sgmv_graph_us"]
    row_counts = [int(r) for r in args.rows.split(",")]
    table = []
    with torch.no_grad():
        for rows in row_counts:
            if rows % ADAPTERS:
                raise SystemExit(f"--prefill: {rows} rows do not split into {ADAPTERS} sequences")
            sets = [torch.randn((rows, H), generator=gen, device=dev).half() for _ in range(SETS)]
            seq_ids = torch.arange(ADAPTERS, device=dev, dtype=torch.int64)
            row_ids = (torch.arange(rows, device=dev) % ADAPTERS).to(torch.int64)
            mixes = (("one adapter", "ad0", (rows, H)), (f"{ADAPTERS} adapters, contiguous sequences", seq_ids, (ADAPTERS, rows // ADAPTERS, H)),
                     (f"{ADAPTERS} adapters interleaved by row", row_ids, (rows, H)))
            for mix, selection, shape in mixes:
                static = sets[0].clone()
                graphs, outs = [], []
                for which, bgmv_rows, sgmv_rows in ((None, 0, 0), (selection, 0, 0), (selection, 0, _native.MAX_LORA_SGMV_ROWS)):
                    bank.select(which)
                    lora.BGMV_MAX_ROWS, lora.SGMV_MAX_ROWS = bgmv_rows, sgmv_rows  # the route is decided when the call is captured
                    g, out = captured(lambda: block(static.view(shape)))
                    graphs.append(g)
                    outs.append(out[0].view(rows, -1))
                turn = [0] * len(graphs)

                def replay(i):
                    static.copy_(sets[turn[i] % SETS])
                    turn[i] += 1
                    graphs[i].replay()

                fns = [lambda i=i: replay(i) for i in range(len(graphs))]
                runs = [timed_alternating(fns, args.iters, args.warmup) for _ in range(args.repeats)]
                row = {"rows": rows, "adapters": mix}
                for i, name in enumerate(names):
                    vals = sorted(r[i] for r in runs)
                    row[name] = vals[len(vals) // 2]
                    row[name.replace("_us", "_runs_us")] = [r[i] for r in runs]
                    row[name.replace("_us", "_spread_us")] = round(vals[-1] - vals[0], 2)
                row["sgmv_wins"] = bool(max(r[2] for r in runs) < min(r[1] for r in runs) - row["torch_graph_spread_us"])
                static.copy_(sets[0])
                graphs[1].replay()
                graphs[2].replay()
                torch.cuda.synchronize()
                row["rel_diff_sgmv_vs_torch"] = float(((outs[2].float() - outs[1].float()).abs().mean()
                                                       / outs[1].float().abs().mean()).item())
                row["rel_size_of_the_adapter_term"] = float(((outs[1].float() - outs[0].float()).abs().mean()
                                                             / outs[0].float().abs().mean()).item())
                del graphs, outs
                # the two launches alone, captured, on one projection of every distinct shape
                ops = {}
                for name in ("q_proj", "k_proj", "gate_proj", "down_proj"):
                    layer = getattr(block, name)
                    fin, fout = SHAPES[name]
                    xin = torch.randn((rows, fin), generator=gen, device=dev).half()
                    yio = torch.zeros((rows, fout), dtype=torch.float16, device=dev)
                    tbl, ranks = layer._device_table(dev)
                    if isinstance(selection, str):
                        words = tbl.shape[0] // len(ranks)
                        call = lambda: hip_kernel.lora_sgmv_(yio, xin, None, tbl[:words], [1, ranks[0], fout, fin])  # noqa: E731
                    else:
                        per_row = selection if selection is row_ids else seq_ids.repeat_interleave(rows // ADAPTERS)
                        call = lambda: hip_kernel.lora_sgmv_(yio, xin, per_row, tbl, [len(ranks), max(ranks), fout, fin])  # noqa: E731
                    g, _ = captured(call)
                    ops[f"{fin}->{fout}"] = timed_alternating([g.replay], args.iters, args.warmup)[0]
                    del g
                row["sgmv_op_us"] = ops
                table.append(row)
                print(json.dumps(row), flush=True)
    best, all_won = 0, True
    for rows in row_counts:  # the largest row count UP TO which the segmented launches win
        if not all(r["sgmv_wins"] for r in table if r["rows"] == rows):
            all_won = False
            break
        best = rows
    result = {"block": {"hidden": H, "kv": KV, "intermediate": I, "scheme": "1x16g8", "dtype": "float16", "projections": list(SHAPES),
                        "prepacked_layers": prepacked, "rank": RANK, "adapters": ADAPTERS},
              "device": torch.cuda.get_device_name(dev), "iters": args.iters, "repeats": args.repeats, "warmup": args.warmup,
              "what": "one block forward captured in a hipGraph and replayed, the copy of the next of three input sets included; "
                      "median over the repeats of the median replay (device events), spread = max - min over the repeats; "
                      "sgmv_op_us: the two launches of aqlm_hip_lora_sgmv alone on one projection, captured, median replay",
              "rows": table, "sgmv_max_rows": best, "sgmv_won_at_every_count": all_won,
              "rule": "sgmv_wins: every repeat of sgmv_graph_us below the smallest torch_graph_us minus its spread over the repeats; "
                      "sgmv_max_rows: the largest row count up to which all three adapter mixes win",
              "command": f"python tools/lora_benchmark.py --prefill --rows {args.rows} --iters {args.iters} --repeats {args.repeats}"}
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps({k: v for k, v in result.items() if k != "rows"}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--prefill", action="store_true",
                    help=f"measure the segmented route at prefill row counts ({PREFILL_ROWS}) against the torch path; writes "
                         "profiles/lora_sgmv.json")
    ap.add_argument("--rows", default=None, help="default 1,2,4,8,16,32,64; with --prefill " + PREFILL_ROWS)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None, help="default profiles/lora_bgmv.json; with --prefill profiles/lora_sgmv.json")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/lora_benchmark.py measures on the GPU; none found")
    if args.rows is None:
        args.rows = PREFILL_ROWS if args.prefill else "1,2,4,8,16,32,64"
    if args.out is None:
        args.out = os.path.join("profiles", "lora_sgmv.json" if args.prefill else "lora_bgmv.json")
    if args.prefill:
        return prefill(args)

    import aqlm_amd.lora as lora
    from aqlm_amd import _native

    dev = torch.device("cuda:0")
    block = Block(dev)
    with torch.no_grad():
        block(torch.zeros((1, H), dtype=torch.float16, device=dev))
    prepacked = sum(getattr(block, n)._packed_codes is not None for n in SHAPES)
    bank = lora.attach_adapters(block, {f"ad{i}": adapter(100 + i) for i in range(ADAPTERS)})
    gen = torch.Generator(device=dev).manual_seed(1)
    names = ["base_graph_us", "plain_graph_us", "bgmv_graph_us"]
    table = []
    with torch.no_grad():
        for rows in [int(r) for r in args.rows.split(",")]:
            sets = [torch.randn((rows, H), generator=gen, device=dev).half() for _ in range(SETS)]
            ids = (torch.arange(rows, device=dev) % ADAPTERS).to(torch.int64)
            for mix, selection in (("one adapter", "ad0"), (f"{ADAPTERS} adapters mixed", ids)):
                static = sets[0].clone()
                graphs, outs = [], []
                for which, max_rows in ((None, 0), (selection, 0), (selection, _native.MAX_LORA_ROWS)):
                    bank.select(which)
                    lora.BGMV_MAX_ROWS = max_rows  # the route is decided when the call is captured
                    g, out = captured(lambda: block(static))
                    graphs.append(g)
                    outs.append(out[0])
                turn = [0] * len(graphs)

                def replay(i):
                    static.copy_(sets[turn[i] % SETS])
                    turn[i] += 1
                    graphs[i].replay()

                fns = [lambda i=i: replay(i) for i in range(len(graphs))]
                runs = [timed_alternating(fns, args.iters, args.warmup) for _ in range(args.repeats)]
                row = {"rows": rows, "adapters": mix}
                for i, name in enumerate(names):
                    vals = sorted(r[i] for r in runs)
                    row[name] = vals[len(vals) // 2]
                    row[name.replace("_us", "_runs_us")] = [r[i] for r in runs]
                    row[name.replace("_us", "_spread_us")] = round(vals[-1] - vals[0], 2)
                row["bgmv_wins"] = bool(max(r[2] for r in runs) < min(r[1] for r in runs) - row["plain_graph_spread_us"])
                # the two adapter routes on the same input: they differ by the roundings the plain ops add
                static.copy_(sets[0])
                graphs[1].replay()
                graphs[2].replay()
                torch.cuda.synchronize()
                row["rel_diff_bgmv_vs_plain"] = float(((outs[2].float() - outs[1].float()).abs().mean()
                                                       / outs[1].float().abs().mean()).item())
                row["rel_size_of_the_adapter_term"] = float(((outs[1].float() - outs[0].float()).abs().mean()
                                                             / outs[0].float().abs().mean()).item())
                del graphs, outs
                table.append(row)
                print(json.dumps(row), flush=True)
    best = 0
    for rows in [int(r) for r in args.rows.split(",")]:  # the largest row count UP TO which the batched launches win
        if not all(r["bgmv_wins"] for r in table if r["rows"] == rows):
            break
        best = rows
    result = {"block": {"hidden": H, "kv": KV, "intermediate": I, "scheme": "1x16g8", "dtype": "float16", "projections": list(SHAPES),
                        "prepacked_layers": prepacked, "rank": RANK, "adapters": ADAPTERS},
              "device": torch.cuda.get_device_name(dev), "iters": args.iters, "repeats": args.repeats, "warmup": args.warmup,
              "what": "one block forward captured in a hipGraph and replayed, the copy of the next of three input sets included; "
                      "median over the repeats of the median replay (device events), spread = max - min over the repeats",
              "rows": table, "bgmv_max_rows": best,
              "rule": "bgmv_wins: every repeat of bgmv_graph_us below the smallest plain_graph_us minus its spread over the repeats; "
                      "bgmv_max_rows: the largest row count up to which both adapter mixes win",
              "command": f"python tools/lora_benchmark.py --rows {args.rows} --iters {args.iters} --repeats {args.repeats}"}
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps({k: v for k, v in result.items() if k != "rows"}))


if __name__ == "__main__":
    main()
