"""Step time of the eager training step (ops.elbo_step, SAL x 2) on the Power shape (N = 8611, D = 4, M = 100, S = 32) for the
covariance functions 'scale_rbf', 'scale_matern32', 'scale_matern52' and 'scale_rq' (alpha = 2).  The RBF step of this shape takes
the fused row kernels; the other three take the general-M path, where they differ in the covariance element function alone
(cov_value / cov_gweight of csrc/tgp_dev.hpp).  The steps are timed in ALTERNATING blocks in one process on one device (HIP events
around each block; the warm-up / steps convention of bench.py, which this script does not touch).  Prints one JSON line; not a
bench.py workload, and no threshold is attached to its numbers.

    python tools/bench_kernels.py --steps 200 --warmup 20 --blocks 5 >> profiles/kernel_family.txt
"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import torch                                    # noqa: E402

from oracle import tgp_oracle as orc            # noqa: E402

DEV = "cuda:0"
KINDS = {"rbf": ("scale_rbf", None), "matern32": ("scale_matern32", None), "matern52": ("scale_matern52", None),
         "rq": ("scale_rq", 2.0)}


def stepper(prob, kernel, alpha):
    """A closure running one eager step with `kernel`, everything resident on the device."""
    from tgp.pytorch_amd import ops
    p = {k: v.to(DEV) for k, v in prob["params"].items()}
    X, Y = prob["X"].to(DEV), prob["Y"].to(DEV)
    flow = ops.FlowSpec(prob["program"], p["theta"].numel(), 0, DEV)
    ro = p["raw_outputscale"] if alpha is None else ops.rq_scale(p["raw_outputscale"], alpha)

    def step():
        return ops.elbo_step(X, Y, p["Z"], p["raw_lengthscale"], ro, p["m"], p["Lam"], p["log_var_noise"], prob["N_total"],
                             flow=flow, theta=p["theta"], S=32, kernel=kernel)
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


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200, help="steps per timed block")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--blocks", type=int, default=5, help="alternating timed blocks per kernel")
    args = ap.parse_args(argv)
    prob = orc.synthetic_problem(8611, 4, 100, seed=0, flow="sal2", S=32)
    steppers = {k: stepper(prob, name, alpha) for k, (name, alpha) in KINDS.items()}
    last = {}
    for k, step in steppers.items():
        for _ in range(args.warmup):
            last[k] = step()
    torch.cuda.synchronize()
    times = {k: [] for k in steppers}
    for _ in range(args.blocks):
        for k, step in steppers.items():
            times[k].append(block(step, args.steps))
    res = {"workload": "eager_step_power_sal2", "steps": args.steps, "warmup": args.warmup, "blocks": args.blocks,
           "device": torch.cuda.get_device_name(0)}
    for k, ts in times.items():
        out, _, status, _ = last[k]
        assert int(status[0]) == 0 and int(status[1]) == 0 and bool(torch.isfinite(out[0]))
        res[k + "_us_per_step_median"] = sorted(ts)[len(ts) // 2]
        res[k + "_us_per_step_blocks"] = ts
        res[k + "_elbo"] = float(out[0])
    for k in ("matern52", "rq"):
        res[k + "_over_matern32"] = res[k + "_us_per_step_median"] / res["matern32_us_per_step_median"]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
