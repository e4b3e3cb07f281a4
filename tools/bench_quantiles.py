"""Time of the exact 95 % band + median (model.predictive_quantiles, Q = 3) against the path the coverage metric took before it:
sample_from_predictive_distribution(S = 100) + the device-to-host copy of the (Dy, S, N, 1) draws + numpy.quantile.  Shapes:
the Power test split (N = 957) and the Power training split (N = 8611), D = 4, M = 100, SAL x 2 and tanh 3 x 2, S = 50 and
100 quadrature nodes.  The two paths are timed in ALTERNATING blocks in one process on one device (HIP events around each
block, the host work of the sampled path included because the block ends in a synchronise after it; the warm-up / calls
convention of bench.py, which this script does not touch).  `--trace` additionally runs the exact path in a fresh child
process under `rocprofv3 --kernel-trace --stats` and reports the mean time of k_pred_quantile.  Prints one JSON line per
configuration; not a bench.py workload, and no threshold is attached to its numbers.

    python tools/bench_quantiles.py --calls 50 --warmup 5 --blocks 5 --trace > profiles/quantiles.txt
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

import numpy                                    # noqa: E402
import torch                                    # noqa: E402

from oracle import tgp_oracle as orc            # noqa: E402

DEV = "cuda:0"
PROBS = [0.025, 0.5, 0.975]
CONFIGS = [(N, flow, S) for N in (957, 8611) for flow in ("sal2", "tanh3x2") for S in (50, 100)]


def build(N, flow, S):
    from tgp.pytorch_amd import config as cg
    from tgp.pytorch_amd.flow import compile_flow, instance_flow
    from tgp.pytorch_amd.flows import SAL, StepTanhL
    from tgp.pytorch_amd.kernels import instance_kernel
    from tgp.pytorch_amd.likelihoods import GaussianNonLinearMean
    from tgp.pytorch_amd.models import sparse_MF_SP
    cg.set_maximum_precission()
    cg.device = DEV
    prob = orc.synthetic_problem(N, 4, 100, seed=0, flow=flow, S=S, perturb=flow != "sal2")
    p = prob["params"]
    K = instance_kernel("scale_rbf", ard_num_dim=4, num_multioutput=1, kernel_is_shared=False,
                        init_params={"length_scale": 2.0, "kernel_scale": 2.0, "noisy_variance": 1e-6})
    lik = GaussianNonLinearMean(1, 0.05, False, quadrature_points=S)
    specs = SAL(2) if flow == "sal2" else instance_flow(StepTanhL(3, 2, add_f0=True))
    model = sparse_MF_SP(["zero", K], prob["X"], p["Z"].clone(), N, lik, 1, True, False, False, False, False, [specs], "single", 0.0)
    with torch.no_grad():
        model.Z.data = p["Z"].reshape(1, 100, 4).clone()
        model.q_U.variational_mean.data = p["m"].reshape(1, 100).clone()
        model.q_U.chol_variational_covar.data = p["Lam"].reshape(1, 100, 100).clone()
        for prm, val in zip(compile_flow(model.G_matrix[0])[1], p["theta"]):
            prm.data = val.clone().reshape(())
    model = model.to(DEV)
    model.set_is_training(False)
    return model, prob["X"].to(DEV)


def exact(model, X):
    return model.predictive_quantiles(X, PROBS)


def sampled(model, X):
    samples, _, _ = model.sample_from_predictive_distribution(X, S=100)
    return numpy.quantile(samples.to("cpu").numpy(), PROBS, axis=1)


def block(fn, model, X, calls):
    """milliseconds per call over `calls` calls"""
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(calls):
        fn(model, X)
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / calls


def kernel_trace(config, calls):
    """[{kernel, calls, mean_us}] of k_pred_quantile at one configuration, from a child process under rocprofv3 (the program
    goes after `--`)."""
    out = []
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "quant", "--", sys.executable,
               os.path.abspath(__file__), "--only", "exact", "--config", "%d,%s,%d" % config, "--calls", str(calls), "--warmup", "2",
               "--blocks", "1"]
        subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, timeout=600)
        for path in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
            with open(path) as fh:
                for row in csv.DictReader(fh):
                    if "k_pred_quantile" in row.get("Name", ""):
                        out.append({"kernel": row["Name"], "calls": int(row["Calls"]), "mean_us": float(row["AverageNs"]) / 1e3})
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50, help="calls per timed block")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--blocks", type=int, default=5, help="alternating timed blocks per path")
    ap.add_argument("--only", choices=["both", "exact"], default="both")
    ap.add_argument("--config", default=None, help="N,flow,S: this configuration only (the trace's child process)")
    ap.add_argument("--trace", action="store_true", help="add the kernel-trace time of k_pred_quantile at N = 8611, S = 100 "
                                                         "(one child process per flow)")
    args = ap.parse_args(argv)
    configs = CONFIGS
    if args.config is not None:
        n, flow, s = args.config.split(",")
        configs = [(int(n), flow, int(s))]
    if not torch.cuda.is_available():
        raise SystemExit("bench_quantiles.py needs the GPU: nothing is measured without one")
    paths = {"exact": exact} if args.only == "exact" else {"exact": exact, "sampled": sampled}
    for N, flow, S in configs:
        model, X = build(N, flow, S)
        for fn in paths.values():
            for _ in range(args.warmup):
                fn(model, X)
        torch.cuda.synchronize()
        times = {k: [] for k in paths}
        for _ in range(args.blocks):
            for k, fn in paths.items():
                times[k].append(block(fn, model, X, args.calls))
        res = {"workload": "quantiles_power", "N": N, "flow": flow, "S": S, "Q": len(PROBS), "calls": args.calls,
               "warmup": args.warmup, "blocks": args.blocks}
        for k, ts in times.items():
            res[k + "_ms_per_call_median"] = sorted(ts)[len(ts) // 2]
            res[k + "_ms_per_call_blocks"] = ts
        if "sampled" in times:
            res["sampled_over_exact"] = res["sampled_ms_per_call_median"] / res["exact_ms_per_call_median"]
        print(json.dumps(res), flush=True)
    if args.trace:
        for cfg in ((8611, "sal2", 100), (8611, "tanh3x2", 100)):
            print(json.dumps({"kernel_trace": kernel_trace(cfg, 20), "N": cfg[0], "flow": cfg[1], "S": cfg[2], "Q": len(PROBS)}),
                  flush=True)


if __name__ == "__main__":
    main()
