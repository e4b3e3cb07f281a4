"""Measurements of the posterior derivative: the slope variance under q(f) (tgp_qf_input_grad_var_f64) and the input gradients of
pathwise draws (tgp_pathwise_grad_f64).  Not a bench.py workload, no threshold:

  dvar   ops.qf_input_grad_var against the same formula from torch ops on the same device with J (rows, M, D) materialised
         (k_g(0) / l_d^2 + sum_m A_d C_d per input, A_d = L^-1 J_d^T as a product with L^-1 of K_ZZ from ops.cholesky, in passes
         of 16 384 rows so that N = 250 000 fits), and ops.qf_input_grad alongside: the cost read as "so many mean gradients".
         N = 957 and 8611 at D = 4, M = 100; N = 250 000, D = 8, M = 1000.  Jitter 1e-6 on both routes.
  grad   ops.pathwise_grad against torch ops with the features' derivatives Phi'_X (rows, 2 R2) and J materialised, one product
         per input, and ops.pathwise_eval alongside: "so many evaluations".  S = 100, R2 = 1024 at the M = 100 shapes,
         S = 64, R2 = 2048 at M = 1000.
  ALTERNATING blocks in one process, HIP events around work that ends in a synchronise, medians of 5 with the block spread.

    python tools/bench_derivative.py > profiles/derivative.txt
"""
import argparse
import json
import math
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import torch                                    # noqa: E402
from torch.nn.functional import softplus        # noqa: E402

DEV = "cuda:0"
F64 = torch.float64
SHAPES = ((957, 4, 100, 100, 1024), (8611, 4, 100, 100, 1024), (250000, 8, 1000, 64, 2048))      # N, D, M, S, R2
JITTER = 1e-6
PASS = 16384


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


def problem(N, D, M, S, R2, seed=0):
    g = torch.Generator().manual_seed(seed)
    X = torch.randn(N, D, dtype=F64, generator=g)
    Z = X[torch.randperm(N, generator=g)[:M]].clone()          # rows of X, as the greedy initialiser leaves them
    isp = math.log(math.expm1(2.0))
    rl, ro = torch.full((D,), isp, dtype=F64), torch.full((1,), isp, dtype=F64)
    m = 0.5 * torch.randn(M, dtype=F64, generator=g)
    Lam = math.sqrt(1e-5) * torch.eye(M, dtype=F64) + 0.05 * torch.tril(torch.randn(M, M, dtype=F64, generator=g))
    omega = torch.randn(R2, D, dtype=F64, generator=g)
    W, eps = torch.randn(S, 2 * R2, dtype=F64, generator=g), torch.randn(S, M, dtype=F64, generator=g)
    return tuple(t.to(DEV) for t in (X, Z, rl, ro, m, Lam, omega, W, eps))


def jacobian(Xs, Zs, ils, s2):
    """J (rows, M, D) of the RBF kernel from the scaled rows."""
    diff = Xs.unsqueeze(1) - Zs.unsqueeze(0)
    return -(s2 * torch.exp(-0.5 * (diff * diff).sum(-1))).unsqueeze(-1) * diff * ils


def torch_dvar(X, Z, rl, ro, Lam):
    from tgp.pytorch_amd import ops
    ils, s2 = 1.0 / softplus(rl), softplus(ro).reshape(())
    Zs = Z * ils
    M = Z.shape[0]
    eye = torch.eye(M, dtype=F64, device=X.device)
    Kzz = s2 * torch.exp(-0.5 * torch.cdist(Zs, Zs).pow(2)) + JITTER * eye
    _, Linv, _ = ops.cholesky(Kzz, want_inverse=True)         # (the M x M factor from the library on both routes)
    Lq = torch.tril(Lam)
    Wm = Lq @ Lq.t() - eye
    out = torch.empty_like(X)
    for r0 in range(0, X.shape[0], PASS):
        J = jacobian(X[r0:r0 + PASS] * ils, Zs, ils, s2)
        for d in range(X.shape[1]):
            A = Linv @ J[:, :, d].t()
            out[r0:r0 + PASS, d] = s2 * ils[d] * ils[d] + (A * (Wm @ A)).sum(0)
    return out


def torch_grad(X, Z, rl, ro, omega, coef):
    ils, s2 = 1.0 / softplus(rl), softplus(ro).reshape(())
    Zs, wd = Z * ils, omega * ils
    R2 = omega.shape[0]
    out = torch.empty(coef.shape[1], X.shape[0], X.shape[1], dtype=F64, device=X.device)
    for r0 in range(0, X.shape[0], PASS):
        Xs = X[r0:r0 + PASS] * ils
        a = Xs @ omega.t()
        ns, cs = -torch.sin(a), torch.cos(a)
        J = jacobian(Xs, Zs, ils, s2)
        for d in range(X.shape[1]):
            dphi = torch.cat([ns * wd[:, d], cs * wd[:, d], J[:, :, d]], 1)          # Phi'_X and J_d side by side: (rows, 2 R2 + M)
            out[:, r0:r0 + PASS, d] = (dphi @ coef).t()
    return out


def bench(N, D, M, S, R2, blocks):
    from tgp.pytorch_amd import ops
    X, Z, rl, ro, m, Lam, omega, W, eps = problem(N, D, M, S, R2)
    coef = ops.pathwise_coeff(Z, rl, ro, m, Lam, omega, W, eps, jitter=JITTER, check=False)
    rel = lambda x, y: float((x - y).abs().max() / y.abs().max())          # noqa: E731
    small = N * M < 10 ** 7
    fns = {"dvar_hip": lambda: ops.qf_input_grad_var(X, Z, rl, ro, m, Lam, jitter=JITTER, check=False),
           "dvar_torch": lambda: torch_dvar(X, Z, rl, ro, Lam),
           "qf_input_grad": lambda: ops.qf_input_grad(X, Z, rl, ro, m, Lam, jitter=JITTER, check=False),
           "grad_hip": lambda: ops.pathwise_grad(X, Z, rl, ro, omega, coef),
           "grad_torch": lambda: torch_grad(X, Z, rl, ro, omega, coef),
           "pathwise_eval": lambda: ops.pathwise_eval(X, Z, rl, ro, omega, coef)}
    reps = {k: (10 if small else 1) for k in fns}
    diffs = {"dvar_rel_diff_to_torch": rel(fns["dvar_hip"](), fns["dvar_torch"]()),
             "grad_rel_diff_to_torch": rel(fns["grad_hip"](), fns["grad_torch"]())}
    res = alternate(fns, reps, blocks, 2 if small else 1)
    md = lambda k: res[k]["median_ms"]                                      # noqa: E731
    out = {"N": N, "D": D, "M": M, "S": S, "R2": R2}
    out.update(diffs)
    out.update({"dvar_hip_over_torch": md("dvar_hip") / md("dvar_torch"), "dvar_hip_over_qf_input_grad": md("dvar_hip") / md("qf_input_grad"),
                "grad_hip_over_torch": md("grad_hip") / md("grad_torch"), "grad_hip_over_pathwise_eval": md("grad_hip") / md("pathwise_eval"),
                "ms": res})
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=5, help="alternating timed blocks per candidate")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        sys.exit("bench_derivative.py measures on a HIP device: none found")
    print(json.dumps({"derivative": [bench(*s, args.blocks) for s in SHAPES]}))


if __name__ == "__main__":
    main()
