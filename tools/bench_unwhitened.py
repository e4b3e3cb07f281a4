"""Step time of the eager unwhitened training step (is_whiten=False) against the eager whitened step, SAL x 2 on the Power shape
(N = 8611, D = 4, M = 100): ELBO -> (-ELBO).backward() -> torch.optim.Adam.step() on the drop-in model classes, the loop
Trainer_SP runs when no step engine applies.  The two models are timed in ALTERNATING blocks in one process on one device
(HIP events around each block; the warm-up / steps convention of bench.py, which this script does not touch), so that clock
and thermal drift hit both alike.  `--trace` additionally runs the unwhitened loop for a few steps in a fresh child process
under `rocprofv3 --kernel-trace --stats` and reports the mean times of k_unwhiten and k_kmm_bwd.  Prints one JSON line; not a
bench.py workload, and no threshold is attached to its numbers.

    python tools/bench_unwhitened.py --steps 200 --warmup 20 --blocks 5 --trace > profiles/unwhitened_step.txt
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


def build(prob, is_whiten):
    from tgp.pytorch_amd import config as cg
    from tgp.pytorch_amd.flow import compile_flow
    from tgp.pytorch_amd.flows import SAL
    from tgp.pytorch_amd.kernels import instance_kernel
    from tgp.pytorch_amd.likelihoods import GaussianNonLinearMean
    from tgp.pytorch_amd.models import sparse_MF_SP
    cg.set_maximum_precission()
    cg.device = DEV
    p = prob["params"]
    N, D = prob["X"].shape
    M = p["m"].numel()
    K = instance_kernel("scale_rbf", ard_num_dim=D, num_multioutput=1, kernel_is_shared=False,
                        init_params={"length_scale": 2.0, "kernel_scale": 2.0, "noisy_variance": 1e-6})
    lik = GaussianNonLinearMean(1, 0.05, False, quadrature_points=prob["xs"].numel())
    model = sparse_MF_SP(["zero", K], prob["X"], p["Z"].clone(), N, lik, 1, is_whiten, False, False, False, False, [SAL(2)],
                         "single", 0.0)
    with torch.no_grad():
        model.Z.data = p["Z"].reshape(1, M, D).clone()
        model.q_U.variational_mean.data = p["m"].reshape(1, M).clone()
        # (+ 0.5 I: a q(u) factor whose covariance is well away from singular in either parameterisation)
        model.q_U.chol_variational_covar.data = (p["Lam"] + 0.5 * torch.eye(M, dtype=torch.float64)).reshape(1, M, M).clone()
        model.covariance_function.raw_outputscale.data = p["raw_outputscale"].reshape(1).clone()
        model.covariance_function.base_kernel.raw_lengthscale.data = p["raw_lengthscale"].reshape(1, 1, D).clone()
        model.likelihood.log_var_noise.data = p["log_var_noise"].reshape(1, 1).clone()
        for prm, val in zip(compile_flow(model.G_matrix[0])[1], p["theta"]):
            prm.data = val.clone().reshape(())
    model = model.to(DEV)
    model.set_is_training(True)
    return model


class Loop:
    def __init__(self, prob, is_whiten):
        self.model = build(prob, is_whiten)
        self.opt = torch.optim.Adam(self.model.parameters(), lr=0.01)
        self.X, self.Y = prob["X"].to(DEV), prob["Y"].to(DEV)
        self.elbo = None

    def step(self):
        elbo, _, _ = self.model.ELBO(self.X, self.Y)
        self.opt.zero_grad()
        (-elbo).backward()
        self.opt.step()
        self.elbo = elbo.detach()

    def block(self, steps):
        """milliseconds per step over `steps` steps"""
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(steps):
            self.step()
        t1.record()
        torch.cuda.synchronize()
        return t0.elapsed_time(t1) / steps


def kernel_trace(steps):
    """{kernel name prefix: mean microseconds} from a child process under rocprofv3 (the program goes after `--`)."""
    out = {}
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "unwh", "--", sys.executable, os.path.abspath(__file__),
               "--only", "unwhitened", "--steps", str(steps), "--warmup", "2", "--blocks", "1"]
        subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, timeout=600)
        for path in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
            with open(path) as fh:
                for row in csv.DictReader(fh):
                    name = row.get("Name", "")
                    for key in ("k_unwhiten", "k_kmm_bwd_fin", "k_kmm_bwd"):
                        if key in name:
                            out.setdefault(key, []).append((name, int(row["Calls"]), float(row["AverageNs"]) / 1e3))
                            break
    return {k: [{"kernel": n, "calls": c, "mean_us": u} for n, c, u in v] for k, v in out.items()}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200, help="steps per timed block")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--blocks", type=int, default=5, help="alternating timed blocks per model")
    ap.add_argument("--only", choices=["both", "unwhitened"], default="both")
    ap.add_argument("--trace", action="store_true", help="add the kernel-trace times of k_unwhiten / k_kmm_bwd (child process)")
    args = ap.parse_args(argv)
    prob = orc.synthetic_problem(8611, 4, 100, seed=0, flow="sal2", S=32)
    loops = {"unwhitened": Loop(prob, False)}
    if args.only == "both":
        loops["whitened"] = Loop(prob, True)
    for lp in loops.values():
        for _ in range(args.warmup):
            lp.step()
    torch.cuda.synchronize()
    times = {k: [] for k in loops}
    for _ in range(args.blocks):
        for k, lp in loops.items():
            times[k].append(lp.block(args.steps))
    res = {"workload": "eager_step_power_sal2", "steps": args.steps, "warmup": args.warmup, "blocks": args.blocks}
    for k, ts in times.items():
        ts = sorted(ts)
        res[k + "_ms_per_step_median"] = ts[len(ts) // 2]
        res[k + "_ms_per_step_blocks"] = times[k]
        res[k + "_elbo"] = float(loops[k].elbo)
    if "whitened" in times:
        res["unwhitened_over_whitened"] = res["unwhitened_ms_per_step_median"] / res["whitened_ms_per_step_median"]
    if args.trace:
        res["kernel_trace"] = kernel_trace(20)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
