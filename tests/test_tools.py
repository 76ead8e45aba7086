"""CPU smoke tests of the measurement tools (so that they do not rot between GPU runs)."""
import csv
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_decode_benchmark_loop_runs_on_cpu():
    out = subprocess.check_output([sys.executable, os.path.join(ROOT, "tools", "decode_benchmark.py"), "--model", "tiny",
                                   "--dense-only", "--device", "cpu", "--tokens", "4", "--prompt", "4"], cwd=ROOT, timeout=600)
    res = json.loads(out.decode().strip().splitlines()[-1])
    assert res["model"] == "tiny" and res["dense_fp16_eager"]["tokens_per_s"] > 0
    assert len(res["dense_fp16_eager"]["first_tokens"]) == 4


def test_make_pmc_traffic_applies_the_gfx950_correction(tmp_path):
    cols = ["Correlation_Id", "Dispatch_Id", "Agent_Id", "Queue_Id", "Process_Id", "Thread_Id", "Grid_Size", "Kernel_Id",
            "Kernel_Name", "Workgroup_Size", "LDS_Block_Size", "Scratch_Size", "VGPR_Count", "Accum_VGPR_Count", "SGPR_Count",
            "Counter_Name", "Counter_Value", "Start_Timestamp", "End_Timestamp"]
    main = "void aqlm::gemv_1x16_packed_kernel<aqlm::F16, 1, 4, 65520u>(aqlm::PackedGemvParams)"
    fin = "void aqlm::gemv_1x16_packed_finalize<aqlm::F16>(aqlm::PackedFinalizeParams)"
    rows = {"pmc_fetch": [(main, "FETCH_SIZE", 1000.0), (main, "FETCH_SIZE", 3000.0), (fin, "FETCH_SIZE", 10.0),
                          (fin, "FETCH_SIZE", 10.0), ("aqlm::pk_count_kernel(...)", "FETCH_SIZE", 9e9)],
            "pmc_write": [(main, "WRITE_SIZE", 100.0), (main, "WRITE_SIZE", 100.0), (fin, "WRITE_SIZE", 4.0), (fin, "WRITE_SIZE", 4.0)]}
    for d, rs in rows.items():
        os.makedirs(tmp_path / d)
        with open(tmp_path / d / "bench_counter_collection.csv", "w", newline="") as f:
            w = csv.writer(f)
            w.writerow(cols)
            for name, counter, val in rs:
                w.writerow([1, 1, "Agent 2", 1, 1, 1, 1, 1, name, 1024, 0, 0, 98, 0, 48, counter, val, 0, 1])
    out = subprocess.check_output([sys.executable, os.path.join(ROOT, "tools", "make_pmc_traffic.py"), str(tmp_path)], cwd=ROOT)
    t = json.loads(out)
    k = t["per_kernel"][main]
    assert k["FETCH_SIZE_KB"] == 2000.0 and k["hbm_bytes"] == 2 * 2000.0 * 1024 + 100.0 * 1024 and k["launches"] == 2
    assert not any("pk_" in name for name in t["per_kernel"])
    per_matvec = (2 * k["hbm_bytes"] + 2 * (2 * 10.0 * 1024 + 4.0 * 1024)) / 2     # main + finalize per matvec
    assert abs(t["gemv_1x16_hbm_bytes_per_launch"] - per_matvec) < 1e-6


def test_arrangement_bound_orders_and_bound_are_consistent():
    """tools/arrangement_bound.py: the restated greedy deal beats the ascending order, a short annealing run does not make it
    worse, every order is a permutation inside the rows' pools, and nothing beats the degree bound."""
    import numpy as np
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import arrangement_bound as ab
    finally:
        sys.path.pop(0)
    c, x, row = ab.make_wave(3, 512, np.random.default_rng(7))
    gc, gx = ab.greedy(c, x, row)
    ac, ax = ab.anneal(gc, gx, row, 20000)
    base, g, a, lb = ab.cost(c, x).sum(), ab.cost(gc, gx).sum(), ab.cost(ac, ax).sum(), ab.degree_bound(c, x).sum()
    assert lb <= a <= g + 0.05 and g < 0.8 * base and lb >= 2.0, (base, g, a, lb)
    for r in np.unique(row):  # the entries of a row stay in the row (as multisets of (codebook slot, x slot) pairs)
        sel = row == r
        want = sorted(zip(c[sel].ravel().tolist(), x[sel].ravel().tolist()))
        assert sorted(zip(gc[sel].ravel().tolist(), gx[sel].ravel().tolist())) == want
        assert sorted(zip(ac[sel].ravel().tolist(), ax[sel].ravel().tolist())) == want


def test_bench_self_launches_under_torch_distributed_run():
    """`python bench.py --gpus 2` (no WORLD_SIZE in the environment) must re-execute itself under torch.distributed.run with one
    rank per GPU; AQLM_BENCH_LAUNCH_PROBE=1 stops each rank after the rendezvous and one gloo collective, so the launcher path is
    covered without a GPU."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env["AQLM_BENCH_LAUNCH_PROBE"] = "1"
    out = subprocess.check_output([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "1"],
                                  cwd=ROOT, env=env, timeout=300, stderr=subprocess.DEVNULL)
    lines = out.decode().splitlines()
    assert len(lines) == 1, lines  # ONE line on stdout for the whole job: rank 1 prints nothing, stray prints go to stderr
    assert json.loads(lines[-1]) == {"launch_probe": True, "world": 2, "sum_of_ranks_plus_1": 3.0}


def test_bench_launcher_command_is_the_drivers_form():
    sys.path.insert(0, ROOT)
    import bench

    cmd = bench.launcher_command(8, ["--gpus", "8", "--steps", "5"], port=29555)
    assert cmd[1:4] == ["-m", "torch.distributed.run", "--nnodes=1"] and "--nproc-per-node=8" in cmd
    assert cmd[cmd.index("--master-addr") + 1] == "127.0.0.1" and cmd[cmd.index("--master-port") + 1] == "29555"
    assert cmd[-4:] == ["--gpus", "8", "--steps", "5"] and cmd[-5].endswith("bench.py")
    # a mismatch between --gpus and the launcher's world size is reported, not asserted
    env = dict(os.environ, WORLD_SIZE="3", RANK="0", LOCAL_RANK="0")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2"], cwd=ROOT, env=env, capture_output=True, timeout=300)
    assert p.returncode != 0 and b"WORLD_SIZE=3" in p.stderr


def test_bench_extras_watchdog_prints_the_line_and_ends_the_process():
    """bench.py's extras (detail, sharded figures with captured collectives, CPU / reference legs) run after the timed region; if
    they hang -- a collective that cannot be captured on 8 GPUs was never exercised before the driver's scaling tier -- the one
    JSON line must still come out: rank 0 prints what it has, every rank exits 0."""
    code = ("import sys, time; sys.path.insert(0, %r); import bench\n"
            "res = {'metric': 'm', 'value': 1.5, 'detail': {'a': 1}}\n"
            "w = bench.ExtrasWatchdog(res, int(sys.argv[1]), 0.3)\n"
            "w.section = 'sharded_70b'\n"
            "time.sleep(60)\n"
            "print('not reached')\n") % ROOT
    p0 = subprocess.run([sys.executable, "-c", code, "0"], cwd=ROOT, capture_output=True, timeout=120)
    assert p0.returncode == 0 and b"not reached" not in p0.stdout
    line = json.loads([l for l in p0.stdout.decode().splitlines() if l.startswith("{")][-1])
    assert line["value"] == 1.5 and line["detail"] == {"a": 1} and line["extras_timed_out"] == {"after_s": 0.3, "section": "sharded_70b"}
    p1 = subprocess.run([sys.executable, "-c", code, "1"], cwd=ROOT, capture_output=True, timeout=120)
    assert p1.returncode == 0 and p1.stdout.strip() == b""
    # finished in time: nothing is printed by the watchdog, finish() says go on
    code2 = ("import sys, time; sys.path.insert(0, %r); import bench\n"
             "w = bench.ExtrasWatchdog({'value': 2}, 0, 0.5)\n"
             "assert w.finish()\n"
             "time.sleep(1.0)\n"
             "print('done')\n") % ROOT
    p2 = subprocess.run([sys.executable, "-c", code2], cwd=ROOT, capture_output=True, timeout=120)
    assert p2.returncode == 0 and p2.stdout.strip() == b"done"


def test_bench_result_line_is_the_last_and_only_thing_on_stdout(tmp_path):
    """Round 5 lost its driver record to librccl's banner: a C-level printf sits in the stdio buffer of fd 1 and is flushed at
    process exit, AFTER Python's print of the JSON line.  bench.py now points fd 1 at stderr for the life of the process and
    writes the line to the saved descriptor, once (benchlib/emit.py).  The probe runs that very path with a pending C
    printf, Python chatter and an atexit print (exit handlers run) in the way; the driver's parse -- json.loads of the last stdout line, which must
    carry `roofline` and `cpu_baseline` -- has to succeed, and nothing else may be on stdout."""
    side = tmp_path / "bench_result.json"
    env = dict(os.environ, AQLM_BENCH_EMIT_PROBE="1", AQLM_BENCH_RESULT_FILE=str(side))
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")], cwd=ROOT, env=env, capture_output=True, timeout=300)
    assert p.returncode == 0, p.stderr.decode()
    lines = p.stdout.decode().splitlines()
    parsed = json.loads(lines[-1])
    assert "roofline" in parsed and "cpu_baseline" in parsed and parsed["value"] == 1.0
    assert len(lines) == 1, lines
    assert b"pretend banner" in p.stderr and b"python chatter" in p.stderr  # the chatter is not lost, it is on stderr
    # the process ends normally, so its exit handlers run (profilers write their files there): what they print lands on stderr
    assert b"atexit chatter" in p.stderr and b"atexit chatter" not in p.stdout
    assert json.loads(side.read_text()) == parsed                            # the same document next to it


def test_bench_headline_path_stays_readable():
    """the headline path of bench.py (arguments, workload, timed region, output dump, emission) stays under 300 lines;
    the roofline and the untimed extras of --full live in benchlib/."""
    n = sum(1 for _ in open(os.path.join(ROOT, "bench.py")))
    assert n < 300, n
    src = open(os.path.join(ROOT, "bench.py")).read()
    assert "emit_final(result, rank" in src and "StdoutGuard.install()" in src and "print(json.dumps" not in src


@pytest.mark.gpu
def test_bench_plain_run_dumps_the_last_steps_outputs(tmp_path):
    """A plain run prints the headline and nothing that belongs to --full; --dump-outputs writes the 64 layer outputs of the last
    timed step as float32, and they are what the seeded layers compute (layer 0 against the generic HIP kernel, a different path)."""
    import numpy as np
    import torch

    out = tmp_path / "outputs"
    env = dict(os.environ, AQLM_BENCH_RESULT_FILE=str(tmp_path / "bench_result.json"))
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--dump-outputs", str(out)], cwd=ROOT, env=env, capture_output=True, timeout=600)
    assert p.returncode == 0, p.stderr.decode()[-3000:]
    lines = p.stdout.decode().splitlines()
    assert len(lines) == 1, lines
    d = json.loads(lines[0])
    assert d["steps"] == 3 and d["ms_per_step"] > 0 and d["unit"] == "GB/s" and d["higher_is_better"] is True and d["dtype"] == "f16"
    assert d["value"] > 0 and not {"roofline", "detail", "sharded_70b", "gpu_reference_baseline", "parity_mean_rel_vs_cpu_oracle"} & set(d)
    files = sorted(os.listdir(out))
    assert len(files) == 64 and files[0] == "layer00_4096x4096.npy" and files[1] == "layer01_4096x11008.npy"
    assert sum(os.path.getsize(out / f) for f in files) < 64 << 20
    y0 = np.load(out / files[0])
    assert y0.dtype == np.float32 and y0.shape == (1, 4096)

    sys.path.insert(0, ROOT)
    from aqlm_amd.inference_kernels import hip_kernel as hk
    from benchlib.layers import Layer

    L = Layer(4096, 4096, 1, 16, 8, 0, torch.device("cuda:0"))  # bench.py's layer 0 (seed = 2 * block)
    ref = hk.generic_matmat(L.x[:1], L.codes, L.codebooks, L.scales.reshape(-1, 1, 1, 1), None).float().cpu().numpy()
    assert float(np.abs(y0 - ref).mean() / np.abs(ref).mean()) < 1e-3


def test_bench_detail_sections_respect_the_time_budget(monkeypatch):
    """benchlib.detail.run_detail: sections run in priority order, one is only STARTED while the process is younger than the budget
    (a --full run stays near a minute; `--full-detail` = budget 0 runs all), an exception in a section is recorded and does not
    stop the others, and what did not run is listed."""
    import time

    sys.path.insert(0, ROOT)
    from benchlib import detail as DT

    ran = []

    def quick(name, secs=0.0, fail=False):
        def fn(c, d):
            ran.append(name)
            time.sleep(secs)
            if fail:
                raise RuntimeError("boom")
            d[name] = True
        return fn

    monkeypatch.setattr(DT, "SECTIONS", [("a", quick("a", 0.3)), ("b", quick("b", fail=True)), ("c", quick("c", 0.3)), ("d", quick("d"))])
    det = {}
    t0 = time.perf_counter()
    DT.run_detail(None, det, t0, 0.5, False)
    assert ran == ["a", "b", "c"] and det["skipped"] == ["d"] and "skipped_note" in det
    assert det["a"] and det["c"] and det["b_error"].startswith("RuntimeError") and set(det["section_seconds"]) == {"a", "b", "c"}
    ran.clear()
    det = {}
    DT.run_detail(None, det, t0 - 100.0, 0.0, True)          # no budget: everything runs however old the process is
    assert ran == ["a", "b", "c", "d"] and det["skipped"] == []
