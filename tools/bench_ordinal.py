"""Step time of the eager ordinal training step (ops.elbo_step, lik = LIK_ORDINAL, K = 5 with the default edges, SAL x 1) on the
Power shape (N = 8611, D = 4, M = 100, S = 32) against the eager LIK_BERNOULLI step on the same chain, kernel and rows.  Both take
the general-M path at every M, so the two steps differ in the likelihood kernel alone (k_ell_quad<EllOrdinal> against
k_ell_quad<EllBern>).  The steps are timed in ALTERNATING blocks in one process on one device (HIP events around each block; the
warm-up / steps convention of bench.py, which this script does not touch).  `--trace` additionally runs a few steps of each
likelihood in a fresh child process under `rocprofv3 --kernel-trace --stats` and reports the mean times of the two k_ell_quad
instantiations.  Prints one JSON line; not a bench.py workload, and no threshold is attached to its numbers.

    python tools/bench_ordinal.py --steps 200 --warmup 20 --blocks 5 --trace > profiles/ordinal_step.txt
"""
import argparse
import csv
import glob
import json
import math
import os
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import torch                                    # noqa: E402

from oracle import tgp_oracle as orc            # noqa: E402

DEV = "cuda:0"
KERNELS = {"EllOrdinal": "k_ell_quad_ordinal", "EllBern": "k_ell_quad_bern"}
NUM_CLASSES = 5
NOISE_VAR = 0.3


def problem():
    """The Power-shape problem with targets of five ordered classes (the classes of a smooth latent under noise of variance
    NOISE_VAR, cut at the default edges) and, for the Bernoulli step, the labels `class >= 2` of the same rows."""
    prob = orc.synthetic_problem(8611, 4, 100, seed=0, flow="sal1", S=32)
    p = prob["params"]
    p["raw_outputscale"] = orc.inv_softplus(0.8).reshape(1)
    p["m"] = 0.5 * p["m"]
    p["log_var_noise"] = torch.tensor([math.log(NOISE_VAR)], dtype=torch.float64)
    g = torch.Generator().manual_seed(100)
    w = torch.randn(4, generator=g, dtype=torch.float64)
    prob["edges"] = torch.tensor([j - NUM_CLASSES / 2.0 for j in range(1, NUM_CLASSES)], dtype=torch.float64)
    z = 1.5 * torch.sin(prob["X"] @ w) + math.sqrt(NOISE_VAR) * torch.randn(8611, generator=g, dtype=torch.float64)
    prob["classes"] = (z.reshape(-1, 1) > prob["edges"].reshape(1, -1)).sum(1).to(torch.float64).reshape(-1, 1)
    prob["labels"] = (prob["classes"] >= 2).to(torch.float64)
    return prob


def stepper(prob, lik):
    """A closure running one eager step of `lik` ("ordinal" / "bernoulli") with everything resident on the device."""
    from tgp.pytorch_amd import lib as L
    from tgp.pytorch_amd import ops
    p = {k: v.to(DEV) for k, v in prob["params"].items()}
    X = prob["X"].to(DEV)
    Y = (prob["classes"] if lik == "ordinal" else prob["labels"]).to(DEV)
    edges = prob["edges"].to(DEV)
    flow = ops.FlowSpec(prob["program"], p["theta"].numel(), 0, DEV)

    def step():
        return ops.elbo_step(X, Y, p["Z"], p["raw_lengthscale"], p["raw_outputscale"], p["m"], p["Lam"], p["log_var_noise"],
                             prob["N_total"], flow=flow, theta=p["theta"], S=32,
                             lik=L.LIK_ORDINAL if lik == "ordinal" else L.LIK_BERNOULLI, df=edges if lik == "ordinal" else None)
    return step


def block(step, steps):
    """microseconds per step over `steps` eager steps"""
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(steps):
        step()
    t1.record()
    torch.cuda.synchronize()
    return 1e3 * t0.elapsed_time(t1) / steps


def kernel_trace(steps):
    """{instantiation: calls, mean microseconds} of k_ell_quad from a child process under rocprofv3 (the program goes after `--`)."""
    out = {}
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "ordinal", "--", sys.executable,
               os.path.abspath(__file__), "--eager-steps", str(steps)]
        subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, timeout=600)
        for path in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
            with open(path) as fh:
                for row in csv.DictReader(fh):
                    name = row.get("Name", "")
                    for key, label in KERNELS.items():
                        if "k_ell_quad" in name and key in name:      # (every (lanes per row, nodes in flight) instantiation)
                            acc = out.setdefault(label, {"calls": 0, "total_us": 0.0})
                            acc["calls"] += int(row["Calls"])
                            acc["total_us"] += int(row["Calls"]) * float(row["AverageNs"]) / 1e3
    for acc in out.values():
        acc["mean_us"] = acc.pop("total_us") / acc["calls"]
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200, help="steps per timed block")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--blocks", type=int, default=5, help="alternating timed blocks per step")
    ap.add_argument("--trace", action="store_true", help="add the kernel-trace times of k_ell_quad<EllOrdinal / EllBern> (child process)")
    ap.add_argument("--eager-steps", type=int, default=0, help="(the traced child) run this many steps of each likelihood")
    args = ap.parse_args(argv)
    prob = problem()
    steppers = {"ordinal": stepper(prob, "ordinal"), "bernoulli": stepper(prob, "bernoulli")}
    if args.eager_steps:
        for key, step in steppers.items():
            for _ in range(args.eager_steps):
                out, _, status, _ = step()
            torch.cuda.synchronize()
            assert int(status[0]) == 0 and bool(torch.isfinite(out[0]))
        return
    last = {}
    for k, step in steppers.items():
        for _ in range(args.warmup):
            last[k] = step()
    torch.cuda.synchronize()
    times = {k: [] for k in steppers}
    for _ in range(args.blocks):
        for k, step in steppers.items():
            times[k].append(block(step, args.steps))
    res = {"workload": "eager_step_power_sal1", "num_classes": NUM_CLASSES, "steps": args.steps, "warmup": args.warmup,
           "blocks": args.blocks, "device": torch.cuda.get_device_name(0)}
    for k, ts in times.items():
        out, _, status, _ = last[k]
        assert int(status[0]) == 0 and int(status[1]) == 0
        res[k + "_us_per_step_median"] = sorted(ts)[len(ts) // 2]
        res[k + "_us_per_step_blocks"] = ts
        res[k + "_elbo"] = float(out[0])
    res["ordinal_over_bernoulli"] = res["ordinal_us_per_step_median"] / res["bernoulli_us_per_step_median"]
    if args.trace:
        tr = kernel_trace(10)
        res["kernel_trace"] = tr
        if len(tr) == 2:
            res["k_ell_quad_ordinal_over_bern"] = tr["k_ell_quad_ordinal"]["mean_us"] / tr["k_ell_quad_bern"]["mean_us"]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
