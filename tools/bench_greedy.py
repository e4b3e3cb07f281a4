"""Measurements of greedy conditional-variance selection of inducing points (tgp_greedy_inducing_f64).  Not a bench.py workload,
no threshold:

  select     ops.greedy_inducing against the same recurrence composed from torch ops on the same device, and against
             utils.KMEANS(n_init=10) as main.py calls it, at the Power shape (N = 8611, D = 4, M = 100); the first two also at
             N = 250000, D = 8, M = 1000.  ALTERNATING blocks in one process, HIP events around work that ends in a synchronise,
             medians with the block spread.
  collapsed  synthetic_power, M = 100, as main.py sets SVGP up: trace[M] / trace[0] of the greedy rows, and the collapsed bound
             at initialisation and after a fixed number of collapsed steps for Z from the greedy selection against Z from k-means
  --once     one selection per shape after one warm-up call, nothing else: the process to put under a kernel trace.
             Achieved bytes/s = N M^2 / 2 x 8 B (the reads of C) over the summed time of k_greedy_step from that trace.

    python tools/bench_greedy.py > profiles/greedy_select.txt
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
SHAPES = ((8611, 4, 100), (250000, 8, 1000))


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


def inputs(N, D, seed=0):
    """Seeded standard-normal rows; the Power shape takes synthetic_power's training inputs instead (what main.py selects from)."""
    if (N, D) == (8611, 4):
        from tgp.pytorch_amd import config as cg
        from tgp.pytorch_amd.data import return_dataset
        cg.set_maximum_precission()
        cg.device = DEV
        _, dc = return_dataset("synthetic_power", 10000, use_validation=None, seed=1, options={"shuffle_train": True})
        assert tuple(dc["X_tr"].shape) == (N, D)
        return dc["X_tr"].to(DEV, F64).contiguous()
    return torch.randn(N, D, dtype=F64, generator=torch.Generator().manual_seed(seed)).to(DEV)


def torch_greedy(X, M, raw_ls, raw_os):
    """The same recurrence from torch ops (RBF): argmax, one kernel column, C[:j]^T C[:j, p] as a matrix-vector product.  No host
    read: the pivot stays a (1,) device tensor and every use of it is an index_select / index_fill (indexing with a 0-dim device
    tensor would read it back on every step)."""
    N = X.shape[0]
    A = X / softplus(raw_ls).reshape(1, -1)
    s2 = softplus(raw_os).reshape(())
    d = torch.full((N,), 1.0, dtype=F64, device=X.device) * s2
    C = torch.empty(M, N, dtype=F64, device=X.device)
    idx = torch.empty(M, dtype=torch.int64, device=X.device)
    trace = torch.empty(M + 1, dtype=F64, device=X.device)
    trace[0] = N * s2
    for j in range(M):
        p = torch.argmax(d, dim=0, keepdim=True)                                  # (1,)
        k = s2 * torch.exp(-0.5 * ((A - A.index_select(0, p)) ** 2).sum(-1))
        Cj = C[:j]
        c = (k - Cj.T @ Cj.index_select(1, p).reshape(j)) / torch.sqrt(d.index_select(0, p))
        C[j] = c
        d = torch.where(d < 0, d, torch.clamp(d - c * c, min=0.0)).index_fill(0, p, -1.0)
        idx[j:j + 1] = p
        trace[j + 1] = torch.clamp(d, min=0.0).sum()
    return idx, trace


def bench_select(N, D, M, blocks, with_kmeans):
    from tgp.pytorch_amd import ops
    from tgp.pytorch_amd.utils import KMEANS
    X = inputs(N, D)
    isp = math.log(math.expm1(2.0))                     # main.py's initial length-scale and kernel scale
    rl, ro = torch.full((D,), isp, dtype=F64, device=DEV), torch.full((1,), isp, dtype=F64, device=DEV)
    fns = {"hip": lambda: ops.greedy_inducing(X, M, rl, ro), "torch": lambda: torch_greedy(X, M, rl, ro)}
    small = N * M < 10 ** 7
    reps = {"hip": 20 if small else 1, "torch": 5 if small else 1}
    if with_kmeans:
        fns["kmeans"] = lambda: KMEANS(X, M, n_init=10, seed=0)
        reps["kmeans"] = 1
    (i1, _, t1, m_eff), (i2, t2) = fns["hip"](), fns["torch"]()
    same = int((i1 == i2[:m_eff]).sum())
    res = alternate(fns, reps, blocks, 2 if small else 1)
    return {"N": N, "D": D, "M": M, "M_eff": m_eff, "trace_ratio": float(t1[-1] / t1[0]), "idx_equal_to_torch": "%d of %d" % (same, M),
            "trace_rel_diff_to_torch": float((t1 - t2[:m_eff + 1]).abs().max() / t1[0]), "C_read_bytes": N * M * M // 2 * 8,
            "hip_over_torch": res["hip"]["median_ms"] / res["torch"]["median_ms"],
            "hip_over_kmeans": res["hip"]["median_ms"] / res["kmeans"]["median_ms"] if with_kmeans else "not measured", "ms": res}


def collapsed_runs(steps):
    """synthetic_power as main.py sets SVGP up (l = 2, s2 = 2, noise 0.05, lr 0.01), the collapsed engine, Z from either initialiser."""
    from tgp.pytorch_amd import config as cg
    from tgp.pytorch_amd.data import return_dataset
    from tgp.pytorch_amd.engine import ElboEngine
    from tgp.pytorch_amd.kernels import instance_kernel
    from tgp.pytorch_amd.utils import GREEDY_VARIANCE, KMEANS
    cg.set_maximum_precission()
    cg.device = DEV
    _, dc = return_dataset("synthetic_power", 10000, use_validation=None, seed=1, options={"shuffle_train": True})
    M, D = 100, dc["Dx"]
    K = instance_kernel("scale_rbf", ard_num_dim=D, num_multioutput=1, kernel_is_shared=False,
                        init_params={"length_scale": 2.0, "kernel_scale": 2.0})
    Zg, info = GREEDY_VARIANCE(dc["X_tr"], M, K, return_info=True)
    Zk = KMEANS(dc["X_tr"], M, n_init=10, seed=cg.config_seed)
    isp = math.log(math.expm1(2.0))
    X, Y = dc["X_tr"].to(DEV, F64), dc["Y_tr"].reshape(-1).to(DEV, F64)
    out = {"dataset": "synthetic_power seed 1", "M": M, "steps": steps, "greedy_trace_ratio": float(info["trace"][-1] / info["trace"][0])}
    # the same residual trace for the k-means centroids, from the package's own dense kernel matrices
    from tgp.pytorch_amd import ops
    rl, ro = K._params()
    rl, ro = rl.to(DEV), ro.to(DEV)
    Kzz, Kzx = ops.kernel_matrix(Zk.to(DEV, F64), None, rl, ro, jitter=1e-8), ops.kernel_matrix(Zk.to(DEV, F64), X, rl, ro)
    s2 = float(softplus(ro))
    out["kmeans_trace_ratio"] = float(1.0 - (Kzx * torch.linalg.solve(Kzz, Kzx)).sum() / (X.shape[0] * s2))
    # where the chosen points sit: mean distance from the mean of the training inputs, in length-scales
    ctr, ell = X.mean(0, keepdim=True), softplus(rl).reshape(1, -1)
    for name, P in (("all_rows", X), ("greedy_rows", Zg.to(DEV, F64)), ("kmeans_centroids", Zk.to(DEV, F64))):
        out["%s_mean_distance_from_centre" % name] = float((((P - ctr) / ell) ** 2).sum(-1).sqrt().mean())
    for name, Z in (("greedy", Zg), ("kmeans", Zk)):
        params = {"Z": torch.as_tensor(Z, dtype=F64).cpu(), "raw_lengthscale": torch.full((D,), isp, dtype=F64),
                  "raw_outputscale": torch.full((1,), isp, dtype=F64), "m": torch.zeros(M, dtype=F64),
                  "Lam": math.sqrt(1e-5) * torch.eye(M, dtype=F64), "log_var_noise": torch.full((1,), math.log(0.05), dtype=F64)}
        eng = ElboEngine(X, Y, params, float(dc["N_tr"]), device=DEV, lr=0.01, collapsed=True)
        eng.capture()
        hist = torch.zeros(steps, 3, dtype=F64, device=DEV)
        eng.replay_many(steps, hist)
        torch.cuda.synchronize()
        eng.check_status()
        out["%s_bound_at_init" % name] = float(hist[0, 0])     # the scalars of step k: the bound at the parameters it started from
        out["%s_bound_after_%d_steps" % (name, steps - 1)] = float(hist[-1, 0])
    return out


def once():
    from tgp.pytorch_amd import ops
    isp = math.log(math.expm1(2.0))
    for N, D, M in SHAPES:
        X = inputs(N, D)
        rl, ro = torch.full((D,), isp, dtype=F64, device=DEV), torch.full((1,), isp, dtype=F64, device=DEV)
        for _ in range(2):
            ops.greedy_inducing(X, M, rl, ro)
        torch.cuda.synchronize()
    print(json.dumps({"once": "2 selections per shape", "shapes": SHAPES}))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=5, help="alternating timed blocks per candidate")
    ap.add_argument("--steps", type=int, default=200, help="collapsed steps of the two runs")
    ap.add_argument("--once", action="store_true", help="two selections per shape and nothing else (for a kernel trace)")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        sys.exit("bench_greedy.py measures on a HIP device: none found")
    if args.once:
        return once()
    res = {"select": [bench_select(*SHAPES[0], args.blocks, True), bench_select(*SHAPES[1], max(args.blocks // 2, 3), False)],
           "collapsed": collapsed_runs(args.steps)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
