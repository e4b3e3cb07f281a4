"""Step time of the captured training step with a linear mean function against the same engine with the zero mean, SAL x 2 on
the Power shape (N = 8611, D = 4, M = 100, S = 32): engine.ElboEngine, one step per graph replay.  The two engines are timed in
ALTERNATING blocks in one process on one device (HIP events around each block; the warm-up / steps convention of bench.py, which
this script does not touch), so that clock and thermal drift hit both alike.  `--trace` additionally runs the mean engine for a
few eager steps in a fresh child process under `rocprofv3 --kernel-trace --stats` and reports the mean times of k_mean_fwd,
k_mean_bwd and k_mean_bwd_fin.  Prints one JSON line; not a bench.py workload, and no threshold is attached to its numbers.

What differs between the two steps: the mean's program has a per-row block, so its row kernel runs 16 rows per wave where the
zero-mean step runs 10; Adam is a launch of its own instead of riding in the backward launches; and the two mean kernels (three
launches) are added.

    python tools/bench_mean.py --steps 500 --warmup 50 --blocks 5 --trace > profiles/mean_step.txt
"""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import torch                                    # noqa: E402

from oracle import tgp_oracle as orc            # noqa: E402

DEV = "cuda:0"
KERNELS = ("k_mean_fwd", "k_mean_bwd_fin", "k_mean_bwd")


def engine(prob, with_mean):
    from tgp.pytorch_amd.engine import ElboEngine
    D = prob["X"].shape[1]
    gen = torch.Generator().manual_seed(9)
    mean = ("linear", 0.3 * torch.randn(D, generator=gen, dtype=torch.float64), torch.zeros(1, dtype=torch.float64)) if with_mean else None
    return ElboEngine(prob["X"], prob["Y"], prob["params"], prob["N_total"], flow_blocks=prob["program"], S=prob["xs"].numel(),
                      lr=0.01, device=DEV, mean=mean)


def block(eng, steps):
    """microseconds per step over `steps` single-step graph replays"""
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(steps):
        eng.replay()
    t1.record()
    torch.cuda.synchronize()
    return 1e3 * t0.elapsed_time(t1) / steps


def kernel_trace(steps):
    """{kernel: mean microseconds} of the mean kernels from a child process under rocprofv3 (the program goes after `--`)."""
    out = {}
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "mean", "--", sys.executable,
               os.path.abspath(__file__), "--eager-steps", str(steps)]
        subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, timeout=600)
        for path in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
            with open(path) as fh:
                for row in csv.DictReader(fh):
                    name = row.get("Name", "")
                    for key in KERNELS:
                        if key in name:
                            out[key] = {"calls": int(row["Calls"]), "mean_us": float(row["AverageNs"]) / 1e3}
                            break
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=500, help="steps per timed block")
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--blocks", type=int, default=5, help="alternating timed blocks per engine")
    ap.add_argument("--trace", action="store_true", help="add the kernel-trace times of the mean kernels (child process)")
    ap.add_argument("--eager-steps", type=int, default=0, help="(the traced child) run this many eager steps of the mean engine")
    args = ap.parse_args(argv)
    prob = orc.synthetic_problem(8611, 4, 100, seed=0, flow="sal2", S=32)
    if args.eager_steps:
        eng = engine(prob, True)
        for _ in range(args.eager_steps):
            eng.step()
        torch.cuda.synchronize()
        eng.check_status()
        return
    engines = {"linear_mean": engine(prob, True), "zero_mean": engine(prob, False)}
    for eng in engines.values():
        eng.capture(unroll=1)
        for _ in range(args.warmup):
            eng.replay()
    torch.cuda.synchronize()
    times = {k: [] for k in engines}
    for _ in range(args.blocks):
        for k, eng in engines.items():
            times[k].append(block(eng, args.steps))
    res = {"workload": "captured_step_power_sal2", "steps": args.steps, "warmup": args.warmup, "blocks": args.blocks,
           "device": torch.cuda.get_device_name(0)}
    for k, ts in times.items():
        engines[k].check_status()
        res[k + "_us_per_step_median"] = sorted(ts)[len(ts) // 2]
        res[k + "_us_per_step_blocks"] = ts
        res[k + "_elbo"] = engines[k].scalars()[0]
    res["mean_minus_zero_us"] = res["linear_mean_us_per_step_median"] - res["zero_mean_us_per_step_median"]
    if args.trace:
        res["kernel_trace"] = kernel_trace(20)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
