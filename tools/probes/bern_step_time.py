"""ms per training step (ops.elbo_step, ELBO + every gradient) of a Bernoulli TGP at the heart / banknote shapes (M = 100),
next to a Gaussian TGP step of the same shape -- on the fused path (RBF) and on the general-M path (forced by the
Matern-3/2 kernel, the only switch the ABI has besides M).  HIP events around `--steps` back-to-back calls after a warm-up.

    python tools/probes/bern_step_time.py [--steps 200]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from oracle import tgp_oracle as orc          # noqa: E402  (parameter recipe only)
from tgp.pytorch_amd import lib as L          # noqa: E402
from tgp.pytorch_amd import ops               # noqa: E402

SHAPES = {"heart": (269, 12), "banknote": (1235, 4)}


def program(name):
    """heart: SAL_InvBCL x 1 (SAL, affine, inverse Box-Cox, affine); banknote: BCL_AL x 5 (Box-Cox, affine, arcsinh, affine)"""
    if name == "heart":
        return [(1, 0, 0, 0), (0, 0, 2, 0), (5, 0, 4, 0), (0, 0, 5, 0)], 7
    prog, off = [], 0
    for _ in range(5):
        prog += [(4, 0, off, 0), (0, 0, off + 1, 0), (3, 0, off + 3, 0), (0, 0, off + 7, 0)]
        off += 9
    return prog, off


def time_step(name, lik, kernel, steps, S=100):
    N, D = SHAPES[name]
    dev = torch.device("cuda:0")
    prob = orc.synthetic_problem(N, D, 100, seed=3, flow=None, S=S)
    p = {k: v.to(dev) for k, v in prob["params"].items()}
    prog, P = program(name)
    theta = torch.zeros(P, dtype=torch.float64, device=dev)
    for kind, _, off, _ in prog:                      # near-identity values for every kind
        if kind == 0:
            theta[off] = 1.0
        elif kind in (4, 5):
            theta[off] = 1.0
        elif kind == 3:
            theta[off + 1] = 1.0
            theta[off + 3] = 1.0
        elif kind == 1:
            theta[off + 1] = 1.0
    Y = prob["Y"].to(dev)
    if lik == L.LIK_BERNOULLI:
        Y = (Y > 0).to(torch.float64)
    flow = ops.FlowSpec(prog, P, 0, dev)
    args = (prob["X"].to(dev), Y, p["Z"], p["raw_lengthscale"], p["raw_outputscale"], p["m"], p["Lam"],
            p["log_var_noise"], float(N))
    kw = dict(flow=flow, theta=theta, S=S, kernel=kernel, lik=lik)
    for _ in range(10):
        ops.elbo_step(*args, **kw)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        out, _, status, _ = ops.elbo_step(*args, **kw)
    e1.record()
    torch.cuda.synchronize()
    assert int(status[0]) == 0 and bool(torch.isfinite(out).all())
    return e0.elapsed_time(e1) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    a = ap.parse_args()
    for name in SHAPES:
        b = time_step(name, L.LIK_BERNOULLI, "scale_rbf", a.steps)
        gf = time_step(name, L.LIK_FLOW, "scale_rbf", a.steps)
        gm = time_step(name, L.LIK_FLOW, "scale_matern32", a.steps)
        print("%-9s N=%5d M=100 S=100  bernoulli (general path) %.3f ms  gaussian fused %.3f ms  gaussian general "
              "(matern32) %.3f ms" % (name, SHAPES[name][0], b, gf, gm))


if __name__ == "__main__":
    main()
