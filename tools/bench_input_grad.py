"""Measurements of the input gradients of q(f) (tgp_qf_input_grad_f64) and of the predictive moments
(tgp_predict_moment_grads_f64).  Not a bench.py workload, no threshold:

  qf        ops.qf_input_grad against the same two Jacobians from torch ops on the same device -- autograd through a materialised
            K_XZ (expanded squared distances, so that N = 250 000 fits) and the triangular solves, one backward for mu and one
            for v -- and against ops.qf_moments alone (what the gradient costs over the forward), at the Power shape (N = 8611,
            D = 4, M = 100), at N = 957 and at N = 250 000, D = 8, M = 1000.  Jitter 1e-6 on both routes.  The torch route's
            solves are products with L^-1 of K_ZZ from ops.cholesky: torch.linalg.solve_triangular ended in
            HIPBLAS_STATUS_ALLOC_FAILED (hipblasDtrsm) at these shapes with the torch build the numbers were taken with.
  partials  ops.predict_moment_grads against ops.predict at the Power shape, SAL x 2 and tanh 3 x 2, S = 32.
  ALTERNATING blocks in one process, HIP events around work that ends in a synchronise, medians of 5 with the block spread.
  --once    two calls of ops.qf_input_grad per shape after nothing else: the process to put under a kernel trace.

    python tools/bench_input_grad.py > profiles/input_grad.txt
"""
import argparse
import json
import math
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import numpy as np                              # noqa: E402
import torch                                    # noqa: E402
from torch.nn.functional import softplus        # noqa: E402

DEV = "cuda:0"
F64 = torch.float64
SHAPES = ((8611, 4, 100), (957, 4, 100), (250000, 8, 1000))
JITTER = 1e-6


def timed(fn, reps):
    """milliseconds per call over `reps` calls (HIP events; the last call's work has finished when the second event has)"""
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / reps


def alternate(fns, reps, blocks, warmup):
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(blocks):
        for k, fn in fns.items():
            times[k].append(timed(fn, reps[k]))
    return {k: {"median_ms": sorted(v)[len(v) // 2], "min_ms": min(v), "max_ms": max(v), "reps_per_block": reps[k]}
            for k, v in times.items()}


def problem(N, D, M, seed=0):
    g = torch.Generator().manual_seed(seed)
    X = torch.randn(N, D, dtype=F64, generator=g)
    Z = X[torch.randperm(N, generator=g)[:M]].clone()          # rows of X, as the greedy initialiser leaves them
    isp = math.log(math.expm1(2.0))
    rl, ro = torch.full((D,), isp, dtype=F64), torch.full((1,), isp, dtype=F64)
    m = 0.5 * torch.randn(M, dtype=F64, generator=g)
    Lam = math.sqrt(1e-5) * torch.eye(M, dtype=F64) + 0.05 * torch.tril(torch.randn(M, M, dtype=F64, generator=g))
    return tuple(t.to(DEV) for t in (X, Z, rl, ro, m, Lam))


def torch_input_grad(X, Z, rl, ro, m, Lam):
    """(dmu, dv) from torch ops: K_XZ materialised, the triangular solve as a product with L^-1, and autograd back to X (RBF)."""
    from tgp.pytorch_amd import ops
    Xg = X.detach().requires_grad_(True)
    ils, s2 = 1.0 / softplus(rl), softplus(ro).reshape(())
    Zs, Xs = Z * ils, Xg * ils
    M = Z.shape[0]
    eye = torch.eye(M, dtype=F64, device=X.device)
    Kzz = s2 * torch.exp(-0.5 * torch.cdist(Zs, Zs).pow(2)) + JITTER * eye
    _, Linv, _ = ops.cholesky(Kzz, want_inverse=True)         # (the M x M factor from the library on both routes; see the docstring)
    d2 = ((Zs * Zs).sum(1, keepdim=True) + (Xs * Xs).sum(1).reshape(1, -1) - 2.0 * Zs @ Xs.t()).clamp_min(0.0)   # (M, N), contiguous
    A = Linv @ (s2 * torch.exp(-0.5 * d2))
    Lq = torch.tril(Lam)
    mu = A.t() @ m
    v = s2 + (A * ((Lq @ Lq.t() - eye) @ A)).sum(0)
    dmu, = torch.autograd.grad(mu.sum(), Xg, retain_graph=True)
    dv, = torch.autograd.grad(v.sum(), Xg)
    return dmu, dv


def bench_qf(N, D, M, blocks):
    from tgp.pytorch_amd import ops
    X, Z, rl, ro, m, Lam = problem(N, D, M)
    fns = {"hip": lambda: ops.qf_input_grad(X, Z, rl, ro, m, Lam, jitter=JITTER, check=False),
           "torch": lambda: torch_input_grad(X, Z, rl, ro, m, Lam),
           "qf_moments": lambda: ops.qf_moments(X, Z, rl, ro, m, Lam, jitter=JITTER, check=False)}
    small = N * M < 10 ** 7
    reps = {"hip": 20 if small else 2, "torch": 10 if small else 1, "qf_moments": 20 if small else 2}
    (a, b), (c, d) = fns["hip"](), fns["torch"]()
    rel = lambda x, y: float((x - y).abs().max() / y.abs().max())
    res = alternate(fns, reps, blocks, 2 if small else 1)
    return {"N": N, "D": D, "M": M, "dmu_rel_diff_to_torch": rel(a, c), "dv_rel_diff_to_torch": rel(b, d),
            "hip_over_torch": res["hip"]["median_ms"] / res["torch"]["median_ms"],
            "hip_over_qf_moments": res["hip"]["median_ms"] / res["qf_moments"]["median_ms"], "ms": res}


def bench_partials(blocks, N=8611, S=32):
    from oracle import tgp_oracle as orc
    from tgp.pytorch_amd import ops
    g = torch.Generator().manual_seed(1)
    mu = torch.randn(N, dtype=F64, generator=g).to(DEV)
    v = (0.05 + torch.rand(N, dtype=F64, generator=g)).to(DEV)
    lvn = torch.full((1,), math.log(0.05), dtype=F64, device=DEV)
    out = []
    for name, (program, theta) in (("sal2", orc.sal_program(2)), ("tanh3x2", orc.steptanh_program(3, 2, np.random.default_rng(0)))):
        spec, th = ops.FlowSpec(program, theta.numel(), 0, DEV), theta.to(DEV)
        fns = {"moment_grads": lambda: ops.predict_moment_grads(mu, v, lvn, spec, th, S),
               "predict": lambda: ops.predict(mu, v, lvn, spec, th, S)}
        res = alternate(fns, {"moment_grads": 50, "predict": 50}, blocks, 3)
        out.append({"flow": name, "N": N, "S": S, "grads_over_predict": res["moment_grads"]["median_ms"] / res["predict"]["median_ms"],
                    "ms": res})
    return out


def once():
    from tgp.pytorch_amd import ops
    for N, D, M in SHAPES:
        args = problem(N, D, M)
        for _ in range(2):
            ops.qf_input_grad(*args, jitter=JITTER, check=False)
        torch.cuda.synchronize()
    print(json.dumps({"once": "2 calls per shape", "shapes": SHAPES}))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=5, help="alternating timed blocks per candidate")
    ap.add_argument("--once", action="store_true", help="two calls per shape and nothing else (for a kernel trace)")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        sys.exit("bench_input_grad.py measures on a HIP device: none found")
    if args.once:
        return once()
    print(json.dumps({"qf": [bench_qf(*s, args.blocks) for s in SHAPES], "partials": bench_partials(args.blocks)}))


if __name__ == "__main__":
    main()
