"""Step time of the eager negative-binomial training step (ops.elbo_step, lik = LIK_NEGBIN, SAL x 1, r = 2) on the Power shape
(N = 8611, D = 4, M = 100, S = 32) against the eager Poisson step on the same chain, the same counts and the same covariance
function (RBF).  Both likelihoods take the general-M path at every M, so the two steps differ in the likelihood kernel alone
(k_ell_quad<EllNegBin> against k_ell_quad<EllPois>).  The steps are timed in ALTERNATING blocks in one process on one device (HIP
events around each block; the warm-up / steps convention of bench.py, which this script does not touch); the median of the
blocks is reported.  `--trace` additionally runs a few steps of each likelihood in a fresh child process under
`rocprofv3 --kernel-trace --stats` and reports the mean per-call times of the two k_ell_quad instantiations.  Prints one JSON
line; not a bench.py workload, and no threshold is attached to its numbers.

    python tools/bench_negbin.py --steps 200 --warmup 20 --blocks 5 --trace > profiles/negbin_step.txt
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
DISPERSION = 2.0
KERNELS = {"EllNegBin": "k_ell_quad_negbin", "EllPois": "k_ell_quad_pois"}


def problem():
    """The Power-shape problem with over-dispersed count targets (a Gamma-Poisson mixture of r = 2) and a q(u) that keeps the
    log-mean small."""
    prob = orc.synthetic_problem(8611, 4, 100, seed=0, flow="sal1", S=32)
    p = prob["params"]
    p["raw_outputscale"] = orc.inv_softplus(0.3).reshape(1)
    p["m"] = 0.3 * p["m"]
    g = torch.Generator().manual_seed(100)
    w = torch.randn(4, generator=g, dtype=torch.float64)
    mean = torch.exp(0.5 + 0.8 * torch.sin(prob["X"] @ w))
    mix = torch._standard_gamma(torch.full_like(mean, DISPERSION), generator=g) / DISPERSION
    prob["counts"] = torch.poisson(mean * mix, generator=g).reshape(-1, 1)
    return prob


def stepper(prob, lik):
    """A closure running one eager step of `lik` ("negbin" / "poisson") with everything resident on the device."""
    from tgp.pytorch_amd import lib as L
    from tgp.pytorch_amd import ops
    p = {k: v.to(DEV) for k, v in prob["params"].items()}
    X, Y = prob["X"].to(DEV), prob["counts"].to(DEV)
    flow = ops.FlowSpec(prob["program"], p["theta"].numel(), 0, DEV)
    # the noise slot: log r for the negative binomial; read by no Poisson kernel
    lvn = torch.tensor([math.log(DISPERSION)], dtype=torch.float64, device=DEV)

    def step():
        return ops.elbo_step(X, Y, p["Z"], p["raw_lengthscale"], p["raw_outputscale"], p["m"], p["Lam"], lvn, prob["N_total"],
                             flow=flow, theta=p["theta"], S=32, kernel="scale_rbf",
                             lik=L.LIK_NEGBIN if lik == "negbin" else L.LIK_POISSON)
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
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "negbin", "--", sys.executable,
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
    ap.add_argument("--trace", action="store_true", help="add the kernel-trace times of k_ell_quad<EllNegBin / EllPois> (child process)")
    ap.add_argument("--eager-steps", type=int, default=0, help="(the traced child) run this many steps of each likelihood")
    args = ap.parse_args(argv)
    prob = problem()
    steppers = {"negbin": stepper(prob, "negbin"), "poisson": stepper(prob, "poisson")}
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
    res = {"workload": "eager_step_power_sal1_counts", "dispersion": DISPERSION, "steps": args.steps, "warmup": args.warmup,
           "blocks": args.blocks, "device": torch.cuda.get_device_name(0)}
    for k, ts in times.items():
        out, g, status, _ = last[k]
        assert int(status[0]) == 0 and int(status[1]) == 0
        res[k + "_us_per_step_median"] = sorted(ts)[len(ts) // 2]
        res[k + "_us_per_step_blocks"] = ts
        res[k + "_elbo"] = float(out[0])
        res[k + "_g_lvn"] = float(g["lvn"].reshape(-1)[0])
    res["negbin_over_poisson"] = res["negbin_us_per_step_median"] / res["poisson_us_per_step_median"]
    if args.trace:
        tr = kernel_trace(10)
        res["kernel_trace"] = tr
        if len(tr) == 2:
            res["k_ell_quad_negbin_over_pois"] = tr["k_ell_quad_negbin"]["mean_us"] / tr["k_ell_quad_pois"]["mean_us"]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
