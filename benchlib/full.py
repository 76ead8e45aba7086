"""`bench.py --full`: everything the benchmark reports besides its headline figure, run after the timed region of the same process --
the roofline object of the timed step, its outputs against the generic HIP kernel and the CPU oracle, `cpu_baseline`, `sharded_70b`,
the budgeted `detail` breakdown and `gpu_reference_baseline`.  A plain run does none of it."""
import json
import os
import time

from .emit import ExtrasWatchdog
from .layers import CEILING_BOTH, CEILING_GATHER, CEILING_LAUNCH, HBM_PEAK_GBPS, ROOT


def roofline(step, ev_ms, steps, packed):
    """Roofline of the dominant kernel (1x16 gemv): HIP events on the launch stream over the timed region.  HBM traffic needs the PMC
    counters, i.e. a rocprofv3 run of this very command: it cannot be measured from inside; the value is read from the committed
    summary of that run (tools/gpu/final_evidence.sh -> profiles/pmc_traffic.json) and labelled as such."""
    launches = steps * step.n
    avg_launch_us = ev_ms * 1e3 / launches
    bytes_per_launch = step.bytes / step.n
    achieved = bytes_per_launch / avg_launch_us * 1e-3  # GB/s
    traffic, traffic_source = None, None
    try:
        pm = json.load(open(os.path.join(ROOT, "profiles", "pmc_traffic.json")))
        traffic = pm.get("gemv_1x16_hbm_bytes_per_launch")
        traffic_source = "profiles/pmc_traffic.json: " + pm.get("how", "rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE over bench.py")
    except Exception:  # noqa: BLE001
        pass
    return {"bound": "hbm", "achieved": achieved, "peak": HBM_PEAK_GBPS, "unit": "GB/s", "frac": achieved / HBM_PEAK_GBPS,
            "traffic": traffic, "traffic_source": traffic_source,
            "kernel": ("aqlm::gemv_1x16_packed_kernel<F16,1,3,65520,4> (prepacked codes, finalize inside the kernel; both shapes)"
                       if packed else "aqlm::gemv_kernel<F16,1x16,g8,NB=1>"),
            "avg_launch_us": avg_launch_us, "algorithmic_bytes_per_launch": bytes_per_launch, "launches_timed": launches,
            # what bounds this metric for a one-launch-per-layer operator: the 1.45 us launch boundary
            # (43 % for the mix), two LDS gathers per code (32 %), both at once (22.5 %)
            "ceiling": {"launch_bound_frac": CEILING_LAUNCH, "lds_gather_bound_frac": CEILING_GATHER, "both_frac": CEILING_BOTH,
                        "boundary_us": 1.45, "what": "fraction of the 8 TB/s roofline a one-launch-per-layer 1x16 matvec can reach on the headline mix"},
            "frac_of_ceiling": achieved / HBM_PEAK_GBPS / min(CEILING_LAUNCH, CEILING_GATHER),
            "frac_of_ceiling_both": achieved / HBM_PEAK_GBPS / CEILING_BOTH,
            "note": "one launch = one matvec = one kernel; duration = HIP-event time of the timed region / matvecs; achieved uses "
                    "ALGORITHMIC bytes (2 B per code) even where the prepacked path reads ~4.8 B per code; rocprofv3 durations: profiles/"}


def run(args, result, lib, dev, rank, world, layers, nblocks, side_file, t_process):
    """Fill `result` with the extras.  Returns False when the watchdog fired (it is emitting the line and ending the process)."""
    # the step's outputs against the CPU ORACLE (oracle/aqlm_oracle.c, the restated reference path -- checker only, rank 0) on one
    # layer of each shape, and against the generic HIP kernel (a different code path) on every rank
    from aqlm_amd.inference_kernels import hip_kernel as hk

    from . import cpu as CPU

    parity, parity_oracle = {}, {}
    for L in (layers[0], layers[1]):
        ref = hk.generic_matmat(L.x[:1], L.codes, L.codebooks, L.scales.reshape(-1, 1, 1, 1), None).float()
        got = L.y[:1].float()
        parity[f"{L.fin}x{L.fout}"] = float((got - ref).abs().mean() / ref.abs().mean())
        if rank == 0:
            parity_oracle[f"{L.fin}x{L.fout}"] = CPU.oracle_parity(L, got)
    result["parity_mean_rel_vs_generic_kernel"] = parity
    result["parity_mean_rel_vs_cpu_oracle"] = parity_oracle
    assert all(v < 1e-3 for v in parity.values()), f"bench outputs are off: {parity}"
    assert all(v < 1e-3 for v in parity_oracle.values()), f"bench outputs differ from the CPU oracle: {parity_oracle}"

    # ---- everything below must never cost the headline line: a watchdog emits what there is and ends the process if the extras
    # are not done within their budget
    extras = ExtrasWatchdog(result, rank, float(os.environ.get("AQLM_BENCH_EXTRAS_TIMEOUT_S", "480")), side_file)
    try:
        if rank == 0 and not args.no_cpu:  # the CPU leg first: `cpu_baseline` must not depend on the budgeted extras
            extras.section = "cpu_baseline"
            try:  # (guarded on its own: rank 0 must reach the collectives of `sharded_70b` like every other rank)
                result["cpu_baseline"] = CPU.cpu_baseline(float(os.environ.get("AQLM_BENCH_CPU_SAMPLE_S", "12")))
            except Exception as e:  # noqa: BLE001
                result["cpu_baseline_error"] = f"{type(e).__name__}: {e}"
        if not args.no_detail:
            from . import detail as DT
            from . import sharded as SH

            extras.section = "sharded_70b"
            try:
                result["sharded_70b"] = SH.sharded_70b(lib, dev, rank, world, args.steps)
            except Exception as e:  # noqa: BLE001 - an extra never costs the headline line
                result["sharded_70b"] = {"error": f"{type(e).__name__}: {e}"}
            result["detail"] = {}  # filled in place: a timed-out run still reports what it had
            budget = 0.0 if args.full_detail else float(os.environ.get("AQLM_BENCH_DETAIL_BUDGET_S", "42"))
            ctx = DT.Ctx(lib, dev, rank, world, max(4, args.steps // 5), layers, nblocks, result["value"])
            DT.run_detail(ctx, result["detail"], t_process, budget, args.full_detail, extras)
        if rank == 0 and not args.no_cpu:
            extras.section = "gpu_reference_baseline"
            result["gpu_reference_baseline"] = CPU.gpu_reference_baseline()
    except Exception as e:  # noqa: BLE001 - whatever an extra does (an import error included), the line goes out
        import traceback

        result["extras_error"] = {"section": extras.section, "error": f"{type(e).__name__}: {e}", "traceback": traceback.format_exc()[-1500:]}
    result["bench_wall_s"] = round(time.perf_counter() - t_process, 1)
    return extras.finish()
