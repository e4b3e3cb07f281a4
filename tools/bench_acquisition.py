"""Measurements of the acquisition functions (tgp_predict_acquisition_f64).  Not a bench.py workload, no threshold:

  acquisition  ops.predict_acquisition with partials against the same formula from torch ops on the same device with the S x N
               node table materialised (tests/acquisition_model.py: the oracle's flow, its slope by autograd, the three branches
               of log h), for "ei", "log_ei" and "pi", at N = 957 and N = 8611, SAL x 2 and tanh 3 x 2, S = 32.
  suggest      one utils.suggest_candidates call, 64 starts x 50 steps, D = 4, M = 100 (SAL x 2, S = 32), kind "log_ei": per step
               one ops.qf_moments, one ops.qf_input_grad and one ops.predict_acquisition with the fused chain rule -- what
               model.acquisition launches, here on the ops themselves.
  ALTERNATING blocks in one process, HIP events around work that ends in a synchronise, medians of 5 with the block spread.

    python tools/bench_acquisition.py > profiles/acquisition.txt
"""
import argparse
import json
import math
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import numpy as np                              # noqa: E402
import torch                                    # noqa: E402

from bench_input_grad import alternate, problem  # noqa: E402

DEV = "cuda:0"
F64 = torch.float64
JITTER = 1e-6


def flows():
    from oracle import tgp_oracle as orc
    return (("sal2", orc.sal_program(2)), ("tanh3x2", orc.steptanh_program(3, 2, np.random.default_rng(0))))


def bench_acquisition(blocks, N, S=32):
    import acquisition_model as AM
    from oracle import tgp_oracle as orc
    from tgp.pytorch_amd import ops
    g = torch.Generator().manual_seed(1)
    mu = torch.randn(N, dtype=F64, generator=g).to(DEV)
    v = (0.05 + torch.rand(N, dtype=F64, generator=g)).to(DEV)
    lvn = torch.full((1,), math.log(0.05), dtype=F64, device=DEV)
    xs, ws = orc.hermgauss(S)
    xs, wn = xs.to(DEV), (ws / math.sqrt(math.pi)).to(DEV)
    best = 0.5
    out = []
    for name, (program, theta) in flows():
        spec, th = ops.FlowSpec(program, theta.numel(), 0, DEV), theta.to(DEV)
        for kind in AM.KINDS:
            fns = {"hip": lambda: ops.predict_acquisition(mu, v, lvn, kind, best, spec, th, S, want_partials=True),
                   "torch": lambda: AM.acquisition(mu, v, lvn, kind, best, 1.0, xs, wn, program, th, want_partials=True)}
            (a, b), (c, d) = fns["hip"](), fns["torch"]()
            rel = lambda x, y: float((x - y).abs().max() / y.abs().max())
            res = alternate(fns, {"hip": 50, "torch": 10}, blocks, 3)
            out.append({"flow": name, "kind": kind, "N": N, "S": S, "value_rel_diff_to_torch": rel(a, c),
                        "partials_rel_diff_to_torch": rel(b, d), "hip_over_torch": res["hip"]["median_ms"] / res["torch"]["median_ms"],
                        "ms": res})
    return out


class OpsModel:
    """model.acquisition on the ops themselves: q(f) moments, their Jacobians, the acquisition launch with the fused chain."""

    def __init__(self, params, spec, theta, lvn, S):
        self.params, self.spec, self.theta, self.lvn, self.S = params, spec, theta, lvn, S

    def acquisition(self, X, kind="log_ei", best=None, maximize=True, beta=2.0, return_grad=False):
        from tgp.pytorch_amd import ops
        mu, v = ops.qf_moments(X, *self.params, jitter=JITTER, check=False)
        jac = ops.qf_input_grad(X, *self.params, jitter=JITTER, check=False) if return_grad else None
        return ops.predict_acquisition(mu, v, self.lvn, kind, best, self.spec, self.theta, self.S, maximize=maximize, jac=jac)


def bench_suggest(blocks, D=4, M=100, S=32, starts=64, steps=50):
    from tgp.pytorch_amd import ops, utils
    _, Z, rl, ro, m, Lam = problem(8611, D, M)
    program, theta = flows()[0][1]
    model = OpsModel((Z, rl, ro, m, Lam), ops.FlowSpec(program, theta.numel(), 0, DEV), theta.to(DEV),
                     torch.full((1,), math.log(0.05), dtype=F64, device=DEV), S)
    bounds = torch.tensor([[-2.0] * D, [2.0] * D], dtype=F64, device=DEV)

    def run():
        return utils.suggest_candidates(model, bounds, kind="log_ei", best=1.0, num_starts=starts, steps=steps,
                                        generator=torch.Generator().manual_seed(0))
    x, val, finals = run()
    res = alternate({"suggest": run}, {"suggest": 1}, blocks, 1)
    return {"D": D, "M": M, "S": S, "starts": starts, "steps": steps, "value": float(val),
            "ms_per_step": res["suggest"]["median_ms"] / (steps + 1), "ms": res}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=5, help="alternating timed blocks per candidate")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        sys.exit("bench_acquisition.py measures on a HIP device: none found")
    print(json.dumps({"acquisition": bench_acquisition(args.blocks, 957) + bench_acquisition(args.blocks, 8611),
                      "suggest": bench_suggest(args.blocks)}))


if __name__ == "__main__":
    main()
