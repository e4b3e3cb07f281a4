"""Step time of the eager Beta training step (ops.elbo_step, lik = LIK_BETA, SAL x 1, precision 10) on the Power shape
(N = 8611, D = 4, M = 100, S = 32) against the eager Gamma step on the same chain, rows and covariance function (RBF).  Both
likelihoods take the general-M path at every M, so the two steps differ in the likelihood kernel alone (k_ell_quad<EllBeta>
against k_ell_quad<EllGamma>).  The steps are timed in ALTERNATING blocks in one process on one device (HIP events around each
block; the warm-up / steps convention of bench.py, which this script does not touch); the median of the blocks is reported.
`--trace` additionally runs a few steps of the Beta, the Gamma and the negative-binomial likelihood -- the other policy with two
lgamma-class calls per node -- in a fresh child process under `rocprofv3 --kernel-trace --stats` and reports the mean per-call
times of the three k_ell_quad instantiations.  `--quantiles` times model.predictive_quantiles (Q = 3: the exact 2.5 %, 50 % and
97.5 % quantiles of the mixture of Betas) against 100 predictive draws per row + numpy.quantile, the sampled recipe, at N = 957
and N = 8611 rows of a TGP with M = 100.  Prints one JSON line; not a bench.py workload, and no threshold is attached to its
numbers.

    python tools/bench_beta.py --steps 200 --warmup 20 --blocks 5 --trace --quantiles > profiles/beta_step.txt
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
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import numpy                                    # noqa: E402
import torch                                    # noqa: E402

from oracle import tgp_oracle as orc            # noqa: E402

DEV = "cuda:0"
PRECISION, SHAPE = 10.0, 3.0
KERNELS = {"EllBeta": "k_ell_quad_beta", "EllGamma": "k_ell_quad_gamma", "EllNegBin": "k_ell_quad_negbin"}


def problem():
    """The Power-shape problem with proportions (Beta noise of precision 10 around a smooth mean), positive targets and counts
    of a smooth mean for the Gamma and the negative-binomial step, and a q(u) that keeps the flow's value small."""
    prob = orc.synthetic_problem(8611, 4, 100, seed=0, flow="sal1", S=32)
    p = prob["params"]
    p["raw_outputscale"] = orc.inv_softplus(0.3).reshape(1)
    p["m"] = 0.3 * p["m"]
    g = torch.Generator().manual_seed(100)
    w = torch.randn(4, generator=g, dtype=torch.float64)
    eta = 0.8 * torch.sin(prob["X"] @ w)
    mu = torch.sigmoid(0.3 + eta)
    a = torch._standard_gamma(mu * PRECISION, generator=g)
    b = torch._standard_gamma((1.0 - mu) * PRECISION, generator=g)
    prob["beta"] = (a / (a + b)).clamp(1e-6, 1.0 - 1e-6).reshape(-1, 1)
    mean = torch.exp(0.5 + eta)
    prob["gamma"] = (mean * torch._standard_gamma(torch.full_like(mean, SHAPE), generator=g) / SHAPE).reshape(-1, 1)
    prob["negbin"] = torch.poisson(mean, generator=g).reshape(-1, 1)
    return prob


def stepper(prob, lik):
    """A closure running one eager step of `lik` ("beta" / "gamma" / "negbin") with everything resident on the device."""
    from tgp.pytorch_amd import lib as L
    from tgp.pytorch_amd import ops
    p = {k: v.to(DEV) for k, v in prob["params"].items()}
    X, Y = prob["X"].to(DEV), prob[lik].to(DEV)
    flow = ops.FlowSpec(prob["program"], p["theta"].numel(), 0, DEV)
    # the noise slot: log phi, log a, log r
    lvn = torch.tensor([math.log({"beta": PRECISION, "gamma": SHAPE, "negbin": SHAPE}[lik])], dtype=torch.float64, device=DEV)
    lik_id = {"beta": L.LIK_BETA, "gamma": L.LIK_GAMMA, "negbin": L.LIK_NEGBIN}[lik]

    def step():
        return ops.elbo_step(X, Y, p["Z"], p["raw_lengthscale"], p["raw_outputscale"], p["m"], p["Lam"], lvn, prob["N_total"],
                             flow=flow, theta=p["theta"], S=32, lik=lik_id)
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
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "beta", "--", sys.executable,
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


def quantile_times(prob, reps=7):
    """{N: {exact_ms, sampled_ms}}: model.predictive_quantiles(X, [0.025, 0.5, 0.975]) against 100 predictive draws per row +
    numpy.quantile on the host, each the median of `reps` calls after one warm-up call, on a TGP (SAL x 1, M = 100)."""
    from tgp.pytorch_amd import config as cg
    from tgp.pytorch_amd import flows as G
    from tgp.pytorch_amd.kernels import instance_kernel
    from tgp.pytorch_amd.likelihoods import Beta
    from tgp.pytorch_amd.models import sparse_MF_SP
    cg.set_maximum_precission()
    cg.device = DEV
    X, p = prob["X"], prob["params"]
    K = instance_kernel("scale_rbf", ard_num_dim=4, num_multioutput=1, kernel_is_shared=False,
                        init_params={"length_scale": 2.0, "kernel_scale": 0.3, "noisy_variance": 1e-6})
    model = sparse_MF_SP(["zero", K], X, p["Z"].clone(), X.shape[0], Beta(precision_init=PRECISION), 1, True, False, False, False,
                         False, [G.SAL(1)], "single", 0.0,
                         init_params={"variational_distribution": {"variance_scale": 1e-5, "mean_scale": 0.0}}).to(DEV)
    with torch.no_grad():
        model.q_U.variational_mean.data = p["m"].reshape(1, -1).to(DEV)
        model.q_U.chol_variational_covar.data = p["Lam"].reshape(1, 100, 100).to(DEV)
    model.set_is_training(False)
    out = {}
    for N in (957, 8611):
        Xd = X[:N].to(DEV)

        def exact():
            return model.predictive_quantiles(Xd, [0.025, 0.5, 0.975]).cpu()

        def sampled():
            s, _, _ = model.sample_from_predictive_distribution(Xd, S=100)
            return numpy.quantile(s.to("cpu").numpy(), [0.025, 0.5, 0.975], axis=1)

        res = {}
        for name, fn in (("exact_ms", exact), ("sampled_ms", sampled)):
            fn()
            ts = []
            for _ in range(reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                ts.append(1e3 * (time.perf_counter() - t0))
            res[name] = sorted(ts)[len(ts) // 2]
        out[str(N)] = res
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200, help="steps per timed block")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--blocks", type=int, default=5, help="alternating timed blocks per step")
    ap.add_argument("--trace", action="store_true",
                    help="add the kernel-trace times of k_ell_quad<EllBeta / EllGamma / EllNegBin> (child process)")
    ap.add_argument("--quantiles", action="store_true", help="add the times of the exact quantiles against the sampled recipe")
    ap.add_argument("--eager-steps", type=int, default=0, help="(the traced child) run this many steps of each likelihood")
    args = ap.parse_args(argv)
    prob = problem()
    if args.eager_steps:
        for key in ("beta", "gamma", "negbin"):
            step = stepper(prob, key)
            for _ in range(args.eager_steps):
                out, _, status, _ = step()
            torch.cuda.synchronize()
            assert int(status[0]) == 0 and bool(torch.isfinite(out[0]))
        return
    steppers = {"beta": stepper(prob, "beta"), "gamma": stepper(prob, "gamma")}
    last = {}
    for k, step in steppers.items():
        for _ in range(args.warmup):
            last[k] = step()
    torch.cuda.synchronize()
    times = {k: [] for k in steppers}
    for _ in range(args.blocks):
        for k, step in steppers.items():
            times[k].append(block(step, args.steps))
    res = {"workload": "eager_step_power_sal1", "precision": PRECISION, "shape": SHAPE, "steps": args.steps, "warmup": args.warmup,
           "blocks": args.blocks, "device": torch.cuda.get_device_name(0)}
    for k, ts in times.items():
        out, _, status, _ = last[k]
        assert int(status[0]) == 0 and int(status[1]) == 0
        res[k + "_us_per_step_median"] = sorted(ts)[len(ts) // 2]
        res[k + "_us_per_step_blocks"] = ts
        res[k + "_elbo"] = float(out[0])
    res["beta_over_gamma"] = res["beta_us_per_step_median"] / res["gamma_us_per_step_median"]
    if args.trace:
        tr = kernel_trace(10)
        res["kernel_trace"] = tr
        if len(tr) == 3:
            res["k_ell_quad_beta_over_negbin"] = tr["k_ell_quad_beta"]["mean_us"] / tr["k_ell_quad_negbin"]["mean_us"]
            res["k_ell_quad_beta_over_gamma"] = tr["k_ell_quad_beta"]["mean_us"] / tr["k_ell_quad_gamma"]["mean_us"]
    if args.quantiles:
        res["predictive_quantiles_q3"] = quantile_times(prob)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
