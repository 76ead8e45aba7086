#!/usr/bin/env python
"""W straight from packed 1x16 codes (aqlm_hip_dequant_1x16_packed) against the route it replaces, on the MI355X.

Kernels, per shape (4096 x 4096, 4096 -> 14336, 14336 -> 4096, 8192 -> 28672 at g8 and 4096 x 4096 at g16; fp16, uniform random codes):
  dequant_canonical_us  aqlm_hip_dequant_1x16 on the canonical int16 codes (what a layer that keeps both copies runs);
  unpack_dequant_us     aqlm_hip_unpack_1x16 + aqlm_hip_dequant_1x16: the route of a dropped layer before this kernel existed;
  packed_dequant_us     the new kernel as it is launched by default;
  packed_dequant_by_xcd_us / packed_dequant_stream_major_us   the new kernel with either grid order forced (`packed_dequant_by_xcd`
                        = 2 / 0: the slices of one row group co-resident on an XCD, or the unpack kernel's stream-major grid).
Each case is captured in a hipGraph that walks N copies of the layer (own packed buffer, codes and W each; N chosen so that one
replay touches more than the 256 MB Infinity Cache, so every launch starts cold) and replayed; the cases alternate within one
process, --iters replays per round, --repeats rounds: median of the rounds' medians per launch and the spread (max - min) over the
rounds.  `ratio` = packed_dequant_us / unpack_dequant_us.

Module level (4096 x 4096 and 4096 -> 14336, strictly dropped layers, eager calls, device events, alternating): a 512-row forward and a
512-row forward + backward on the former route (unpack, then the large-batch op / its autograd function on the unpacked codes) and
through QuantizedLinear as it is now.

Memory: `memory_report(model)["code_bits_per_weight"]` of a stack of Llama-3-8B-shaped decoder layers (--stack-layers of them: q / o
4096 x 4096, k / v 4096 -> 1024, gate / up 4096 -> 14336, down 14336 -> 4096; the figure is a ratio and does not depend on the depth)
after one 512-row call and three single-row calls per layer: default `prepack_model()`, `single_copy=True`, and the state the default
converged to before the packed dequant existed (the 512-row call restored every layer's codes for good: both copies).

    python tools/packed_dequant_benchmark.py [--iters 20] [--repeats 3] [--out profiles/packed_dequant.json]
"""
import argparse
import ctypes
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [(8, 4096, 4096), (8, 4096, 14336), (8, 14336, 4096), (8, 8192, 28672), (16, 4096, 4096)]
CACHE_BYTES = 256 << 20


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


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


def rounds_alternating(fns, iters, repeats, warmup=3):
    """[(median of the rounds' medians, spread over the rounds)] per fn; the calls of the fns alternate"""
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
    return [(median(m), max(m) - min(m)) for m in meds]


def kernel_rows(args, dev):
    from aqlm_amd import _native
    from aqlm_amd.inference_kernels import hip_kernel as hk

    lib = _native.lib
    rows = []
    for g, fin, fout in SHAPES:
        gen = torch.Generator(device=dev).manual_seed(fin + fout + g)
        codes = torch.randint(-32768, 32768, (fout, fin // g, 1), generator=gen, device=dev, dtype=torch.int32).to(torch.int16)
        cb = (torch.randn((1, 65536, 1, g), generator=gen, device=dev) * 0.05).half()
        scales = (torch.rand((fout, 1, 1, 1), generator=gen, device=dev) * 0.2 + 0.05).half()
        packed = hk.prepack_1x16(codes, g, codebooks=cb)
        assert packed is not None
        w_bytes = fout * fin * 2
        n = max(2, min(8, -(-CACHE_BYTES * 5 // 4 // (packed.numel() + w_bytes))))
        layers = []
        for _ in range(n):
            pk = hk.PackedCodes(packed.buf.clone(), packed.desc)
            layers.append((pk, codes.clone(), torch.empty_like(codes), torch.empty((fout, fin), dtype=torch.float16, device=dev)))
        ref = hk.code1x16_dequant(codes, cb, scales)
        assert torch.equal(hk.dequant_1x16_packed(packed, cb, scales), ref), "the new kernel disagrees with the old route"
        stream = lambda: torch.cuda.current_stream().cuda_stream  # noqa: E731

        def canonical():
            for pk, c, _, W in layers:
                assert lib.aqlm_hip_dequant_1x16(c.data_ptr(), cb.data_ptr(), scales.data_ptr(), W.data_ptr(), fout, fin, g, _native.F16, stream()) == 0

        def unpack_dequant():
            for pk, _, c, W in layers:
                assert lib.aqlm_hip_unpack_1x16(ctypes.byref(pk.desc), pk.data_ptr(), c.data_ptr(), stream()) == 0
                assert lib.aqlm_hip_dequant_1x16(c.data_ptr(), cb.data_ptr(), scales.data_ptr(), W.data_ptr(), fout, fin, g, _native.F16, stream()) == 0

        def from_packed():
            for pk, _, _, W in layers:
                assert lib.aqlm_hip_dequant_1x16_packed(ctypes.byref(pk.desc), pk.data_ptr(), cb.data_ptr(), scales.data_ptr(), W.data_ptr(),
                                                        _native.F16, stream()) == 0

        graphs = [captured(canonical), captured(unpack_dequant)]
        old = _native.get_tuning("packed_dequant_by_xcd")
        try:
            for knob in (1, 2, 0):
                _native.set_tuning("packed_dequant_by_xcd", knob)
                graphs.append(captured(from_packed))
        finally:
            _native.set_tuning("packed_dequant_by_xcd", old)
        res = rounds_alternating([gr.replay for gr in graphs], args.iters, args.repeats)
        assert torch.equal(layers[-1][3], ref)
        names = ["dequant_canonical", "unpack_dequant", "packed_dequant", "packed_dequant_by_xcd", "packed_dequant_stream_major"]
        row = {"g": g, "in_features": fin, "out_features": fout, "layers_per_replay": n, "packed_bytes": packed.numel(),
               "waves": int(packed.desc.waves), "steps": int(packed.desc.steps)}
        for name, (med, spread) in zip(names, res):
            row[name + "_us"] = round(med / n, 2)
            row[name + "_spread_us"] = round(spread / n, 2)
        row["ratio"] = round(row["packed_dequant_us"] / row["unpack_dequant_us"], 3)
        row["ratio_by_xcd"] = round(row["packed_dequant_by_xcd_us"] / row["unpack_dequant_us"], 3)
        row["ratio_stream_major"] = round(row["packed_dequant_stream_major_us"] / row["unpack_dequant_us"], 3)
        print(json.dumps(row), flush=True)
        rows.append(row)
        del layers, graphs
        torch.cuda.empty_cache()
    return rows


def _layer(fin, fout, dev, seed):
    from aqlm import QuantizedLinear

    m = QuantizedLinear(fin, fout, 8, 1, 1, 16, bias=False, device=dev, dtype=torch.float16)
    gen = torch.Generator(device=dev).manual_seed(seed)
    with torch.no_grad():
        m.codes.copy_(torch.randint(-32768, 32768, m.codes.shape, generator=gen, device=dev, dtype=torch.int32))
        m.codebooks.copy_(torch.randn(m.codebooks.shape, generator=gen, device=dev) * 0.05)
        m.scales.copy_(torch.rand(m.scales.shape, generator=gen, device=dev) * 0.2 + 0.05)
    return m


def module_rows(args, dev):
    from aqlm.checkpoint import prepack_model
    from aqlm_amd.inference_kernels import hip_kernel as hk

    rows = []
    for fin, fout in [(4096, 4096), (4096, 14336)]:
        m = _layer(fin, fout, dev, fin + fout)
        prepack_model(torch.nn.ModuleDict({"l": m}), drop_canonical=True)
        assert m._codes_dropped
        x = torch.randn(512, fin, device=dev, dtype=torch.float16)
        gy = torch.randn(512, fout, device=dev, dtype=torch.float16)
        xg = x.clone().requires_grad_(True)

        def old_forward():
            with torch.no_grad():
                return hk.code1x16_matmat_dequant(x, hk.unpack_1x16(m._packed_codes), m.codebooks, m.scales, m.bias)

        def new_forward():
            with torch.no_grad():
                return m(x)

        def old_step():
            xg.grad = None
            m.gemm_op.apply(xg, hk.unpack_1x16(m._packed_codes), m.codebooks, m.scales, m.bias).backward(gy)

        def new_step():
            xg.grad = None
            m(xg).backward(gy)

        assert torch.equal(old_forward(), new_forward())
        old_step()
        g_old = xg.grad.clone()
        new_step()
        assert torch.equal(xg.grad, g_old) and m._codes_dropped
        res = rounds_alternating([old_forward, new_forward, old_step, new_step], args.iters, args.repeats)
        row = {"in_features": fin, "out_features": fout, "rows": 512}
        for name, (med, spread) in zip(["forward_unpack_route", "forward_packed_route", "forward_backward_unpack_route",
                                        "forward_backward_packed_route"], res):
            row[name + "_us"] = round(med, 1)
            row[name + "_spread_us"] = round(spread, 1)
        print(json.dumps(row), flush=True)
        rows.append(row)
    return rows


def memory_rows(args, dev):
    from aqlm.checkpoint import memory_report, prepack_model

    def stack():
        mods, seed = [], 0
        for _ in range(args.stack_layers):
            for fin, fout in [(4096, 4096), (4096, 1024), (4096, 1024), (4096, 4096), (4096, 14336), (4096, 14336), (14336, 4096)]:
                seed += 1
                mods.append(_layer(fin, fout, dev, seed))
        return torch.nn.ModuleList(mods)

    def use(model):
        with torch.no_grad():
            for m in model:
                m(torch.randn(512, m.in_features, device=dev, dtype=torch.float16))
                for _ in range(3):
                    m(torch.randn(1, m.in_features, device=dev, dtype=torch.float16))
        torch.cuda.synchronize()
        rep = memory_report(model)
        return {"code_bits_per_weight": round(rep["code_bits_per_weight"], 3), "codes_dropped_layers": rep["codes_dropped_layers"]}

    out = {"stack_layers": args.stack_layers}
    model = stack()
    prepack_model(model)
    out["default"] = use(model)
    del model
    torch.cuda.empty_cache()
    model = stack()
    prepack_model(model, single_copy=True)
    out["single_copy"] = use(model)
    del model
    torch.cuda.empty_cache()
    model = stack()
    prepack_model(model, drop_canonical=False)
    out["default_before_packed_dequant"] = use(model)
    out["default_before_packed_dequant"]["note"] = ("both copies: the state every layer was left in once a 512-row call had restored its "
                                                    "codes for good")
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--stack-layers", type=int, default=2)
    ap.add_argument("--only", choices=["kernels", "modules", "memory"], default=None)
    ap.add_argument("--out", default=os.path.join("profiles", "packed_dequant.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    dev = torch.device("cuda:0")
    result = {"device": torch.cuda.get_device_name(0), "dtype": "float16", "iters": args.iters, "repeats": args.repeats,
              "method": "device events; kernels: hipGraph replay over layers_per_replay rotating copies (> 256 MB per replay), per-launch "
                        "figure = replay / copies; cases alternate in one process; median of the rounds' medians, spread = max - min over rounds"}
    if args.only in (None, "kernels"):
        result["kernels"] = kernel_rows(args, dev)
    if args.only in (None, "modules"):
        result["modules"] = module_rows(args, dev)
    if args.only in (None, "memory"):
        result["memory"] = memory_rows(args, dev)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
