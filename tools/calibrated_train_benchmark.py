#!/usr/bin/env python
"""Calibrated training of codebooks and scales on the MI355X (aqlm_amd/tuning.py, ``calibrated_loss_and_grads``): the kernel route
(aqlm_hip_calib_delta, one library GEMM, aqlm_hip_calib_rows, aqlm_hip_calib_codebook_grad_1x16 / _kx8) against the torch route, which is
autograd through ``_dequantize_weight`` and the reference's ``_compute_mse``.

Per shape (a 4096 x 4096 Gaussian weight, ``XTX = X^T X / n`` of 8192 Gaussian rows with per-feature scales, as 1x16 g8, 1x16 g16, 2x8 g8
and 8x8 g32; fp32 masters, random codes):
  step_*     ONE ``calibrated_loss_and_grads`` on either route (the 1x16 index built beforehand);
  delta_us / gemm_us / rows_us / codebook_grad_us   the four parts of the kernel route alone, and ``gemm_share`` = gemm / their sum;
  quantize_* ONE ``quantize_layer_`` of an fp16 layer at ``relative_mse_tolerance = 0.01`` (``--max-epochs`` caps it), split into the
             k-means initialisation, the searches and the rest (the training steps), with the epochs it ran and the errors.
The two routes alternate within one process, --iters calls per round after warm-up calls of each, --repeats rounds: median of the
rounds' medians and the spread (max - min) over the rounds (``*_spread_us``), device events around every call (the protocol of
tools/kmeans_benchmark.py).

    python tools/calibrated_train_benchmark.py [--shapes 1x16g8,1x16g16,2x8g8,8x8g32] [--iters 5] [--repeats 5] [--max-epochs 50]
                                               [--skip-quantize] [--merge] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.kmeans_benchmark import rounds_alternating  # noqa: E402

SHAPES = {"1x16g8": (1, 16, 8), "1x16g16": (1, 16, 16), "2x8g8": (2, 8, 8), "8x8g32": (8, 8, 32)}  # (codebooks, bits, g)
FEATURES = 4096


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--max-epochs", type=int, default=50)
    ap.add_argument("--steps-per-epoch", type=int, default=100)
    ap.add_argument("--skip-quantize", action="store_true", help="time the single step only")
    ap.add_argument("--merge", action="store_true", help="keep the rows of other shapes already in the output file")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    shapes = [s.strip() for s in args.shapes.split(",") if s.strip()]
    if any(s not in SHAPES for s in shapes):
        raise SystemExit(f"calibrated_train_benchmark: --shapes takes a comma list of {sorted(SHAPES)}")
    if not torch.cuda.is_available():
        raise SystemExit("calibrated_train_benchmark: no GPU (a timing taken anywhere else says nothing about the MI355X)")

    import aqlm.tuning as tuning
    from aqlm import QuantizedLinear
    from aqlm_amd.inference_kernels import hip_kernel

    dev = torch.device("cuda")
    rows = []
    for shape in shapes:
        K, nbits, g = SHAPES[shape]
        gen = torch.Generator().manual_seed(FEATURES + 100 * K + nbits + g)
        weight = (torch.randn((FEATURES, FEATURES), generator=gen) * 0.02).to(dev)
        x = (torch.randn((2 * FEATURES, FEATURES), generator=gen) * (0.5 + torch.rand((1, FEATURES), generator=gen))).to(dev)
        xtx = x.T @ x / x.shape[0]
        xtx = (0.5 * (xtx + xtx.T)).contiguous()
        del x
        size = 2 ** nbits
        unsigned = torch.randint(0, size, (FEATURES, FEATURES // g, K), generator=gen)
        codes = torch.where(unsigned >= size // 2, unsigned - size, unsigned).to(torch.int16 if nbits == 16 else torch.int8).to(dev)
        books = (torch.randn((K, size, 1, g), generator=gen) * 0.02 / K ** 0.5).to(dev)
        scales = (torch.rand((FEATURES, 1, 1, 1), generator=gen) + 0.5).to(dev)
        index = hip_kernel.build_codebook_grad_index(codes, g) if nbits == 16 else None

        def step(switch):
            tuning.CALIBRATED_GRAD_KERNEL = switch
            try:
                return tuning.calibrated_loss_and_grads(codes, books, scales, weight, xtx, index=index)
            finally:
                tuning.CALIBRATED_GRAD_KERNEL = True

        assert tuning._calibrated_grad_route(codes, books, scales, weight, xtx), "the kernel route declined the benchmark's own shape"
        from_kernel, from_torch = step(True), step(False)
        agreement = [float((a.double() - b.double()).abs().max() / b.double().abs().max()) for a, b in zip(from_kernel, from_torch)]
        delta = hip_kernel.calib_delta(codes, books, scales, weight)
        product = torch.mm(delta, xtx)
        if nbits == 16:
            grad = lambda: hip_kernel.calib_codebook_grad_1x16(product, scales, index)  # noqa: E731
        else:
            grad = lambda: hip_kernel.calib_codebook_grad_kx8(product, scales, codes, g)  # noqa: E731
        timed = rounds_alternating(
            [lambda: step(True), lambda: step(False), lambda: hip_kernel.calib_delta(codes, books, scales, weight, out=delta),
             lambda: torch.mm(delta, xtx, out=product), lambda: hip_kernel.calib_rows(product, delta, codes, books), grad],
            args.iters, args.repeats)
        (step_k, step_k_spread), (step_t, step_t_spread), (t_delta, _), (t_gemm, _), (t_rows, _), (t_grad, _) = timed
        parts = t_delta + t_gemm + t_rows + t_grad
        row = {"weight": [FEATURES, FEATURES], "shape": shape, "step_kernel_us": step_k, "step_kernel_spread_us": step_k_spread,
               "step_torch_us": step_t, "step_torch_spread_us": step_t_spread, "step_ratio": round(step_k / step_t, 4),
               "delta_us": t_delta, "gemm_us": t_gemm, "rows_us": t_rows, "codebook_grad_us": t_grad, "gemm_share": round(t_gemm / parts, 4),
               "gemm_tflops": round(2 * FEATURES ** 3 / (t_gemm * 1e6), 1),
               "kernel_vs_torch_route_rel_inf": dict(zip(("loss", "d_codebooks", "d_scales"), agreement))}
        del delta, product, from_kernel, from_torch
        if not args.skip_quantize:
            layer = QuantizedLinear(FEATURES, FEATURES, g, 1, K, nbits, bias=False, device=dev, dtype=torch.float16)
            spent = {"init": 0.0, "search": 0.0}
            originals = {"init": tuning.init_layer_kmeans_, "search": tuning.update_codes_calibrated_}

            def clocked(what):
                def run(*a, **kw):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    result = originals[what](*a, **kw)
                    torch.cuda.synchronize()
                    spent[what] += time.perf_counter() - t0
                    return result
                return run

            tuning.init_layer_kmeans_, tuning.update_codes_calibrated_ = clocked("init"), clocked("search")
            try:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                report = tuning.quantize_layer_(layer, weight, xtx, relative_mse_tolerance=0.01, max_epochs=args.max_epochs,
                                                steps_per_epoch=args.steps_per_epoch, generator=torch.Generator(device=dev).manual_seed(1), seed=1)
                torch.cuda.synchronize()
                total = time.perf_counter() - t0
            finally:
                tuning.init_layer_kmeans_, tuning.update_codes_calibrated_ = originals["init"], originals["search"]
            row.update({"quantize_s": round(total, 3), "quantize_init_s": round(spent["init"], 3), "quantize_search_s": round(spent["search"], 3),
                        "quantize_training_s": round(total - spent["init"] - spent["search"], 3), "quantize_epochs": report["epochs"],
                        "quantize_stopped_early": report["stopped_early"], "quantize_steps_per_epoch": args.steps_per_epoch,
                        "quantize_routes": report["routes"], "quantize_initial_error": report["initial_error"],
                        "quantize_error": report["error"], "quantize_losses": [round(v, 8) for v in report["losses"]]})
            del layer
        print(json.dumps(row), flush=True)
        rows.append(row)
        torch.cuda.empty_cache()

    out = args.out or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "calibrated_train.json")
    if args.merge and os.path.exists(out):
        kept = [r for r in json.load(open(out))["rows"] if r["shape"] not in shapes]
        rows = kept + rows
    doc = {"tool": "tools/calibrated_train_benchmark.py", "device": torch.cuda.get_device_name(0), "torch": torch.__version__,
           "iters": args.iters, "repeats": args.repeats, "rows": rows}
    with open(out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(f"wrote {out}")


if __name__ == "__main__":
    main()
