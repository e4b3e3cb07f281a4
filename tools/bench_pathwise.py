"""Measurements of pathwise posterior function draws (tgp_pathwise_coeff_f64 + tgp_pathwise_eval_f64).  Not a bench.py workload,
no threshold:

  shapes     Power test split (N = 957, D = 4, M = 100, R2 = 1024, S = 100), Power training split (N = 8611, same), a large shard
             (N = 250000, D = 8, M = 1000, R2 = 2048, S = 64): coeff + eval, against (a) the same formula from torch ops with Phi_X
             (N x 2 R2) materialised, and at N = 957 and N = 4096 against (b) the existing joint route ops.qf_cov +
             ops.qf_joint_sample_safe with S = 100.  ALTERNATING blocks in one process, HIP events around work that ends in a
             synchronise, medians with the block spread.  K_ZZ gets a jitter of 1e-6 in every route.
  --once     one coeff + eval per shape after one warm-up call, nothing else: the process to put under a kernel trace or a
             counter run.  Rates of the row kernel from its traced time: 2 N (2 R2 + M) S flop on the matrix cores,
             N R2 sincos calls, 8 S N bytes stored.

    python tools/bench_pathwise.py
    rocprofv3 --kernel-trace --stats ... -- python tools/bench_pathwise.py --once       (and --pmc ... in runs of their own)

profiles/pathwise.txt holds the timings of the first, the k_pw_* lines of the trace and the counter sums, and the reading.
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
JIT = 1e-6
SHAPES = ((957, 4, 100, 1024, 100), (8611, 4, 100, 1024, 100), (250000, 8, 1000, 2048, 64))
JOINT_N = (957, 4096)


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


def inputs(N, D, M, R2, S, seed=0):
    """Seeded standard-normal rows, Z the first M of them, length-scales 1 (D = 4) or 2 (D = 8), q(u) of order one."""
    from tgp.pytorch_amd.pathwise import spectral_frequencies
    g = torch.Generator().manual_seed(seed)
    X = torch.randn(max(N, M), D, dtype=F64, generator=g)
    isp = math.log(math.expm1(1.0 if D <= 4 else 2.0))
    q = dict(X=X[:N], Z=X[:M].clone(), raw_ls=torch.full((D,), isp, dtype=F64), raw_os=torch.full((1,), 0.6, dtype=F64),
             m=torch.randn(M, dtype=F64, generator=g),
             Lam=torch.tril(0.3 * torch.randn(M, M, dtype=F64, generator=g) / math.sqrt(M)) + 0.7 * torch.eye(M, dtype=F64),
             omega=spectral_frequencies("scale_rbf", R2, D, g), W=torch.randn(S, 2 * R2, dtype=F64, generator=g),
             eps=torch.randn(S, M, dtype=F64, generator=g))
    return {k: v.to(DEV).contiguous() for k, v in q.items()}


def torch_route(q):
    """The same formula from torch ops (RBF), Phi_X and K_XZ materialised."""
    ils = 1.0 / softplus(q["raw_ls"])
    s2 = softplus(q["raw_os"]).reshape(())
    R2 = q["omega"].shape[0]
    amp = torch.sqrt(s2 / R2)

    def feats(A):
        a = (A * ils) @ q["omega"].T
        return amp * torch.cat([torch.cos(a), torch.sin(a)], 1)

    def kern(A, B):
        return s2 * torch.exp(-0.5 * torch.cdist(A * ils, B * ils).pow(2))
    M = q["Z"].shape[0]
    L = torch.linalg.cholesky(kern(q["Z"], q["Z"]) + JIT * torch.eye(M, dtype=F64, device=DEV))
    v = q["m"].reshape(-1, 1) + torch.tril(q["Lam"]) @ q["eps"].T - torch.linalg.solve_triangular(L, feats(q["Z"]) @ q["W"].T,
                                                                                                 upper=False)
    nu = torch.linalg.solve_triangular(L.T, v, upper=True)
    return (feats(q["X"]) @ q["W"].T + kern(q["X"], q["Z"]) @ nu).T


def hip_route(q):
    from tgp.pytorch_amd import ops
    coef = ops.pathwise_coeff(q["Z"], q["raw_ls"], q["raw_os"], q["m"], q["Lam"], q["omega"], q["W"], q["eps"], jitter=JIT, check=False)
    return ops.pathwise_eval(q["X"], q["Z"], q["raw_ls"], q["raw_os"], q["omega"], coef)


def hip_parts(q):
    from tgp.pytorch_amd import ops
    coef = ops.pathwise_coeff(q["Z"], q["raw_ls"], q["raw_os"], q["m"], q["Lam"], q["omega"], q["W"], q["eps"], jitter=JIT, check=False)
    return {"coeff": lambda: ops.pathwise_coeff(q["Z"], q["raw_ls"], q["raw_os"], q["m"], q["Lam"], q["omega"], q["W"], q["eps"],
                                                jitter=JIT, check=False),
            "eval": lambda: ops.pathwise_eval(q["X"], q["Z"], q["raw_ls"], q["raw_os"], q["omega"], coef)}


def joint_route(q, S):
    from tgp.pytorch_amd import ops
    N = q["X"].shape[0]
    e = torch.randn(S, N, dtype=F64, device=DEV, generator=torch.Generator(DEV).manual_seed(1))

    def run():
        mu, Sigma = ops.qf_cov(q["X"], q["Z"], q["raw_ls"], q["raw_os"], q["m"], q["Lam"], jitter=JIT, check=False)
        return ops.qf_joint_sample_safe(mu, Sigma, e, jitter=JIT)
    return run


def bench_shape(N, D, M, R2, S, blocks):
    q = inputs(N, D, M, R2, S)
    small = N <= 10000
    fns = {"hip": lambda: hip_route(q), "torch_materialised": lambda: torch_route(q)}
    fns.update({"hip_" + k: f for k, f in hip_parts(q).items()})
    reps = {k: (10 if small else 1) for k in fns}
    F1, F2 = fns["hip"](), fns["torch_materialised"]()
    diff = float((F1 - F2).abs().max() / F2.abs().max())
    del F1, F2
    res = alternate(fns, reps, blocks, 2 if small else 1)
    k = 2 * R2 + M
    return {"N": N, "D": D, "M": M, "R2": R2, "S": S, "rel_diff_to_torch": diff, "phi_x_bytes": N * 2 * R2 * 8,
            "row_kernel_mfma_flop": 2 * N * k * S, "row_kernel_sincos": N * R2, "row_kernel_store_bytes": 8 * S * N,
            "hip_over_torch": res["hip"]["median_ms"] / res["torch_materialised"]["median_ms"], "times": res}


def bench_joint(N, blocks):
    D, M, R2, S = 4, 100, 1024, 100
    q = inputs(N, D, M, R2, S)
    import warnings
    from tgp.pytorch_amd import ops
    fns = {"pathwise": lambda: hip_route(q), "qf_cov_joint_sample": joint_route(q, S)}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", ops.NumericalWarning)
        res = alternate(fns, {"pathwise": 5, "qf_cov_joint_sample": 2}, blocks, 1)
    return {"N": N, "D": D, "M": M, "R2": R2, "S": S, "pathwise_over_joint": res["pathwise"]["median_ms"] /
            res["qf_cov_joint_sample"]["median_ms"], "times": res}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--once", action="store_true")
    ap.add_argument("--shapes", default="0,1,2")
    args = ap.parse_args(argv)
    from tgp.pytorch_amd import config as cg
    cg.set_maximum_precission()
    cg.device = DEV
    which = [SHAPES[int(i)] for i in args.shapes.split(",") if i != ""]
    if args.once:
        for shp in which:
            q = inputs(*shp)
            hip_route(q)
            torch.cuda.synchronize()
            hip_route(q)
            torch.cuda.synchronize()
            print(json.dumps({"once": shp}))
        return
    print(json.dumps({"tool": "tools/bench_pathwise.py", "device": torch.cuda.get_device_name(0), "blocks": args.blocks, "jitter": JIT}))
    for shp in which:
        print(json.dumps({"shape": bench_shape(*shp, args.blocks)}))
        sys.stdout.flush()
    for N in JOINT_N:
        print(json.dumps({"joint": bench_joint(N, args.blocks)}))
        sys.stdout.flush()


if __name__ == "__main__":
    main()
