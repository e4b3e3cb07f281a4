"""Step time of the composed multi-class training step and the kernel time of its likelihood launch.  Not a bench.py
workload.  Shape: N = 8611, D = 4, M = 100, C = 4, S = 32, SAL x 2 per class, counter-based draws.

    python tools/bench_multiclass.py --steps 200 --warmup 20              # one JSON line: ms per composed step (HIP events)
    python tools/bench_multiclass.py --kernels --steps 50                 # the two likelihood launches alone, for a kernel trace:
    rocprofv3 --kernel-trace --stats -d OUT -- python tools/bench_multiclass.py --kernels --steps 50

`--kernels` launches k_ell_softmax (S * C = 128 flow evaluations per row) and the stand-alone k_ell_quad at the same N with
S = 128 nodes (the same number of flow evaluations per row), `--steps` times each.
"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import torch                                    # noqa: E402

from tgp.pytorch_amd import config as cg        # noqa: E402
from tgp.pytorch_amd import ops                 # noqa: E402
from tgp.pytorch_amd.flows import SAL           # noqa: E402
from tgp.pytorch_amd.kernels import instance_kernel             # noqa: E402
from tgp.pytorch_amd.likelihoods import MulticlassCategorical   # noqa: E402
from tgp.pytorch_amd.models import sparse_MF_SP                 # noqa: E402
from tgp.pytorch_amd.synthetic import synthetic_problem         # noqa: E402

N, D, M, C, S = 8611, 4, 100, 4, 32


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--kernels", action="store_true")
    args = ap.parse_args(argv)
    cg.set_maximum_precission()
    dev = "cuda:0"
    prob = synthetic_problem(N, D, M, seed=0, flow="sal2", S=32)
    X = prob["X"].to(dev)
    Y = torch.randint(0, C, (N, 1), generator=torch.Generator().manual_seed(0)).to(torch.float64).to(dev)
    if args.kernels:
        g = torch.Generator().manual_seed(1)
        mu = torch.randn(C, N, generator=g, dtype=torch.float64).to(dev)
        v = (0.1 + torch.rand(C, N, generator=g, dtype=torch.float64)).to(dev)
        flow = ops.FlowSpec(prob["program"], prob["params"]["theta"].numel(), 0, None)
        theta1 = prob["params"]["theta"].to(dev)
        spec, theta = ops.SoftmaxSpec([flow] * C), theta1.repeat(C)
        lvn = torch.zeros(1, dtype=torch.float64, device=dev)
        for _ in range(args.steps):
            ops.ell_softmax(Y, mu, v, spec, theta, S, seed=1)
            ops.ell_flow(Y.reshape(-1), mu[0].contiguous(), v[0].contiguous(), lvn, flow, theta1, S * C)
        torch.cuda.synchronize()
        print(json.dumps({"workload": "multiclass_kernels", "launch_pairs": args.steps}))
        return
    K = instance_kernel("scale_rbf", ard_num_dim=D, num_multioutput=C, kernel_is_shared=False,
                        init_params={"length_scale": 2.0, "kernel_scale": 2.0})
    lik = MulticlassCategorical(C)
    lik.SMC = S
    model = sparse_MF_SP(["zero", K], prob["X"], prob["params"]["Z"], float(N), lik, C, True, False, False, False, False,
                         [SAL(2)] * C, "single", 0.0).to(dev)
    opt = torch.optim.Adam(model.parameters(), lr=0.01)

    def step():
        elbo, _, _ = model.ELBO(X, Y)
        opt.zero_grad()
        (-elbo).backward()
        opt.step()
        return elbo
    for _ in range(args.warmup):
        step()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(args.steps):
        elbo = step()
    t1.record()
    torch.cuda.synchronize()
    ms = t0.elapsed_time(t1) / args.steps
    print(json.dumps({"workload": "multiclass_composed_step", "N": N, "D": D, "M": M, "C": C, "S": S, "ms_per_step": ms,
                      "steps": args.steps, "warmup": args.warmup, "elbo": float(elbo),
                      "finite": bool(torch.isfinite(elbo.detach()).all())}))


if __name__ == "__main__":
    main()
