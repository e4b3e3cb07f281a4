"""Measurements of the closed-form optimal q(u) and the collapsed training step.  Not a bench.py workload, no threshold:

  optimal_qu   tgp_optimal_qu_f64 (K_ZX generated on chip) against the materialised route -- ops.knm, the N x M matrix in HBM,
               ops.gemm for K_ZX K_XZ, torch.linalg for the M x M chain -- at N = 8611, D = 4, M = 100 and N = 10000, D = 8, M = 1000
  step         the captured collapsed engine step (optimal q(u) -> the unchanged step -> Adam on the hyper-parameters) against the
               captured Adam SVGP step (the svgp_power workload's step: its code is the parent's), same shape
  convergence  synthetic_power, M = 100: the ELBO 15 000 Adam epochs of SVGP reach, and the collapsed steps / wall time until
               the collapsed bound passes it
The pairs are timed in ALTERNATING blocks in one process on one device, HIP events around each block, medians over the blocks.

    python tools/bench_collapsed.py > profiles/collapsed_step.txt
"""
import argparse
import json
import math
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import torch                                    # noqa: E402

DEV = "cuda:0"
F64 = torch.float64


def timed(fn, reps):
    """milliseconds per call over `reps` calls (HIP events)"""
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
            times[k].append(timed(fn, reps))
    return {k: {"median_ms": sorted(v)[len(v) // 2], "blocks_ms": v} for k, v in times.items()}


def problem(N, D, M, seed=0):
    from tgp.pytorch_amd.synthetic import synthetic_problem
    prob = synthetic_problem(N, D, M, seed=seed, flow=None)
    p = prob["params"]
    return prob["X"].to(DEV), prob["Y"].reshape(-1).to(DEV), {k: v.to(DEV) for k, v in p.items()}, float(prob["N_total"])


def bench_optimal_qu(N, D, M, reps, blocks, warmup):
    from tgp.pytorch_amd import ops
    X, Y, p, N_total = problem(N, D, M)
    Z, rl, ro, lvn = p["Z"], p["raw_lengthscale"].reshape(-1), p["raw_outputscale"].reshape(-1), p["log_var_noise"].reshape(-1)
    out = (torch.empty(M, dtype=F64, device=DEV), torch.empty(M, M, dtype=F64, device=DEV))
    MP, NP = (M + 127) // 128 * 128, (N + 127) // 128 * 128
    Kp = torch.zeros(NP, MP, dtype=F64, device=DEV)
    Cp = torch.zeros(MP, MP, dtype=F64, device=DEV)
    eye = torch.eye(M, dtype=F64, device=DEV)
    how = {"product": "ops.gemm"}

    def fused():
        return ops.optimal_qu(X, Y, Z, rl, ro, lvn, N_total, out=out, check=False)

    def materialised():
        K = ops.knm(X, Z, rl, ro)                                 # (N, M) in HBM
        if how["product"] == "ops.gemm":
            Kp[:N, :M].copy_(K)
            C = ops.gemm(Kp, Kp, trans_a=True, C=Cp)[:M, :M]
        else:
            C = K.T @ K
        b = K.T @ Y
        Lk = torch.linalg.cholesky(ops.kmm(Z, rl, ro))
        Li = torch.linalg.solve_triangular(Lk, eye, upper=False)
        s = (N_total / N) * torch.exp(-lvn[0])
        B = eye + s * (Li @ C @ Li.T)
        Lpi = torch.linalg.solve_triangular(torch.linalg.cholesky(B.flip(0, 1)), eye, upper=False)
        Lam = Lpi.T.flip(0, 1)
        return s * (Lam @ (Lam.T @ (Li @ b))), Lam
    try:
        materialised()
    except Exception as e:                       # (the padded product is an operator of its own: say what stood in for it)
        how["product"] = "torch.matmul (ops.gemm refused: %s)" % str(e)[:80]
    (m1, L1), (m2, L2) = fused(), materialised()
    agree = float(((m1 - m2).abs().max() / m2.abs().max()).cpu())
    res = alternate({"fused": fused, "materialised": materialised}, reps, blocks, warmup)
    return {"N": N, "D": D, "M": M, "fused_ms": res["fused"]["median_ms"], "materialised_ms": res["materialised"]["median_ms"],
            "fused_over_materialised": res["fused"]["median_ms"] / res["materialised"]["median_ms"], "blocks": res,
            "materialised_product": how["product"], "m_rel_diff": agree}


def engines(X, Y, params, N_total, lr=0.01):
    from tgp.pytorch_amd.engine import ElboEngine
    adam = ElboEngine(X, Y, {k: v.clone() for k, v in params.items()}, N_total, device=DEV, lr=lr)
    coll = ElboEngine(X, Y, {k: v.clone() for k, v in params.items()}, N_total, device=DEV, lr=lr, collapsed=True)
    adam.capture()
    coll.capture()
    return adam, coll


def bench_step(reps, blocks, warmup):
    X, Y, p, N_total = problem(8611, 4, 100)
    adam, coll = engines(X, Y, p, N_total)
    res = alternate({"adam_svgp": lambda: adam.replay_many(reps), "collapsed": lambda: coll.replay_many(reps)}, 1, blocks, max(warmup // reps, 1))
    adam.check_status()
    coll.check_status()
    a, c = res["adam_svgp"]["median_ms"] / reps * 1e3, res["collapsed"]["median_ms"] / reps * 1e3
    return {"shape": "N=8611 D=4 M=100", "steps_per_block": reps, "adam_svgp_us_per_step": a, "collapsed_us_per_step": c,
            "collapsed_over_adam": c / a, "blocks": res}


def convergence(epochs, max_steps):
    """synthetic_power as main.py sets SVGP up (k-means Z, l = 2, s2 = 2, noise 0.05, Lq = sqrt(1e-5) I, lr 0.01)."""
    from tgp.pytorch_amd import config as cg
    from tgp.pytorch_amd.data import return_dataset
    from tgp.pytorch_amd.utils import KMEANS
    cg.set_maximum_precission()
    cg.device = DEV
    loaders, dc = return_dataset("synthetic_power", 10000, use_validation=None, seed=1, options={"shuffle_train": True})
    M, D = 100, dc["Dx"]
    Z = torch.as_tensor(KMEANS(dc["X_tr"], M, n_init=10, seed=cg.config_seed), dtype=F64)
    isp = math.log(math.expm1(2.0))
    params = {"Z": Z, "raw_lengthscale": torch.full((D,), isp, dtype=F64), "raw_outputscale": torch.full((1,), isp, dtype=F64),
              "m": torch.zeros(M, dtype=F64), "Lam": math.sqrt(1e-5) * torch.eye(M, dtype=F64),
              "log_var_noise": torch.full((1,), math.log(0.05), dtype=F64)}
    X, Y = dc["X_tr"].to(DEV, F64), dc["Y_tr"].reshape(-1).to(DEV, F64)
    adam, coll = engines(X, Y, params, float(dc["N_tr"]))
    hist = torch.zeros(epochs, 3, dtype=F64, device=DEV)
    torch.cuda.synchronize()
    t0 = time.time()
    adam.replay_many(epochs, hist)
    torch.cuda.synchronize()
    t_adam = time.time() - t0
    adam.check_status()
    target = float(hist[-1, 0])
    chunk, done, t_coll, passed = 25, 0, 0.0, None
    h = torch.zeros(chunk, 3, dtype=F64, device=DEV)
    first = None
    while done < max_steps and passed is None:
        torch.cuda.synchronize()
        t0 = time.time()
        coll.replay_many(chunk, h)
        torch.cuda.synchronize()
        t_coll += time.time() - t0
        e = h[:, 0].cpu()
        first = float(e[0]) if first is None else first
        over = (e > target).nonzero()
        if len(over):
            passed = done + int(over[0]) + 1         # the scalars of step k are the bound at the hyper-parameters it started from
        done += chunk
    coll.check_status()
    return {"dataset": "synthetic_power seed 1", "M": M, "adam_epochs": epochs, "adam_final_elbo": target, "adam_wall_s": t_adam,
            "adam_first_elbo": float(hist[0, 0]), "collapsed_first_bound": first, "collapsed_steps_to_pass": passed,
            "collapsed_steps_run": done, "collapsed_wall_s_for_steps_run": t_coll, "collapsed_last_bound": float(h[-1, 0])}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50, help="calls (steps) per timed block")
    ap.add_argument("--blocks", type=int, default=7, help="alternating timed blocks per candidate")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--epochs", type=int, default=15000, help="Adam epochs of the SVGP run the collapsed run has to pass")
    ap.add_argument("--max-steps", type=int, default=3000)
    args = ap.parse_args(argv)
    res = {"optimal_qu": [bench_optimal_qu(8611, 4, 100, args.reps, args.blocks, args.warmup),
                          bench_optimal_qu(10000, 8, 1000, max(args.reps // 5, 5), args.blocks, max(args.warmup // 5, 3))],
           "step": bench_step(200, args.blocks, args.warmup), "convergence": convergence(args.epochs, args.max_steps)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
