"""CPU restatement of greedy conditional-variance selection of inducing points (the pivoted Cholesky factorisation of K_XX; Burt,
Rasmussen, van der Wilk 2020) in float64 torch: test infrastructure only.

Start with d_n = s2 for all rows and no picked rows.  For j = 0 .. M-1:
    1. p_j = argmax_n d_n over rows not yet picked; ties go to the smallest index (step 0 is an exact tie: p_0 = 0)
    2. if d_{p_j} <= min_var, stop: M_eff = j
    3. c_n = (k(x_n, x_{p_j}) - sum_{l<j} C[l,n] C[l,p_j]) / sqrt(d_{p_j}), the sum in the order of l
    4. C[j,n] = c_n
    5. d_n <- max(d_n - c_n^2, 0)
    6. row p_j is marked picked: it never competes again and adds nothing to the trace
    7. trace[j+1] = sum_{n not picked} d_n;  trace[0] = N s2
stated two ways: `greedy` is the recurrence (it chooses, or follows a given sequence without choosing), `dense_route` forms
d^(j) = diag(K - K[:,S] K[S,S]^-1 K[S,:]) by a dense solve and the trace as the sum of the same.  The kernel formulas are the
oracle's (tests/optqu_model.py `kernel`: exact pairwise differences, Matern-3/2 with the max(d^2, 1e-30) clamp).

Every test input comes from `make_case`; `GREEDY_CPU` holds, per CPU case, what this file measured (tools: run this file).
"""
import math

import numpy as np
import torch
from torch.nn.functional import softplus

from optqu_model import SQRT3, kernel

F64 = torch.float64
MIN_VAR = 1e-8            # the first rung of the package's jitter ladder

# (N, M, D, kernel): the cases of tests/test_greedy_host.py, both routes at every step
CPU_CASES = [(1, 1, 1, "scale_rbf"), (2, 2, 1, "scale_matern32"), (65, 17, 13, "scale_rbf"), (65, 17, 4, "scale_matern32"),
             (257, 64, 4, "scale_rbf"), (257, 64, 8, "scale_matern32"), (300, 40, 16, "scale_rbf")]

# Measured by this file on the CPU (python tests/greedy_model.py), float64, worst over the steps:
#   d       max_n |d_recurrence - d_dense| / s2 over the rows not picked
#   trace   |trace_recurrence - trace_dense| / (N s2)
#   cond    cond(K[S,S]) at the last step
GREEDY_CPU = {
    (1, 1, 1, 'scale_rbf'): dict(d=0.0e+00, trace=0.0e+00, cond=1.0e+00),
    (2, 2, 1, 'scale_matern32'): dict(d=0.0e+00, trace=0.0e+00, cond=1.3e+00),
    (65, 17, 13, 'scale_rbf'): dict(d=6.4e-16, trace=2.1e-16, cond=1.5e+00),
    (65, 17, 4, 'scale_matern32'): dict(d=5.4e-16, trace=2.1e-16, cond=2.4e+00),
    (257, 64, 4, 'scale_rbf'): dict(d=1.0e-15, trace=2.1e-16, cond=1.2e+01),
    (257, 64, 8, 'scale_matern32'): dict(d=8.6e-16, trace=2.1e-16, cond=1.0e+01),
    (300, 40, 16, 'scale_rbf'): dict(d=1.1e-15, trace=3.7e-16, cond=1.4e+00),
}

# (N, M, D) of tests/test_gpu_greedy.py, each with both kernels: every N of {1, 2, 63, 64, 65, 257, 1000, 3000, 5000}, every M of
# {1, 2, 17, 64, 129, 200} and every D of {1, 4, 13, 16} (and 8: the third width of the kernel's coordinate loop) at least once
GPU_SHAPES = [(1, 1, 1), (2, 2, 1), (63, 17, 4), (64, 64, 16), (65, 17, 13), (65, 2, 1), (257, 64, 4), (257, 129, 13), (257, 64, 8),
              (1000, 129, 4), (1000, 200, 16), (3000, 129, 13), (3000, 17, 1), (5000, 200, 4), (5000, 64, 16)]
# The cases whose gap between the best and the second-best d stays under 1e-9 s2 at some step after step 0 (this file, CPU:
# 1.1e-10, 0 -- an exact tie --, 3.2e-10, 4.7e-11, 2.4e-14 s2): a device may take either row there, so only the greedy property is
# asked of them.  Every other case clears 1e-9 s2 at every step (the closest: 1.6e-9 s2, RBF 5000 / 64 / 16) and must reproduce
# the CPU's sequence exactly.
NEAR_TIES = {(63, 17, 4, "scale_rbf"), (1000, 129, 4, "scale_rbf"), (1000, 129, 4, "scale_matern32"), (3000, 17, 1, "scale_rbf"),
             (5000, 200, 4, "scale_rbf")}
GAP = 1e-9                # x s2


def inv_softplus(x):
    return math.log(math.expm1(x))


def make_case(N, M, D, kind, seed=0):
    """Seeded inputs: X (N, D) standard normal; softplus length-scales around 1 up to D = 7 and around 2 from D = 8 (K_XX keeps
    off-diagonal mass in every dimension count), s2 = softplus(0.6)."""
    g = torch.Generator().manual_seed(1000003 * seed + 7919 * N + 131 * M + 17 * D + (1 if kind == "scale_matern32" else 0))
    X = torch.randn(N, D, dtype=F64, generator=g)
    raw_ls = torch.full((D,), inv_softplus(1.0 if D < 8 else 2.0), dtype=F64) + 0.1 * torch.randn(D, dtype=F64, generator=g)
    raw_os = torch.tensor([0.6], dtype=F64)
    return dict(X=X, raw_ls=raw_ls, raw_os=raw_os, kernel=kind, N=N, M=M, D=D, s2=float(softplus(raw_os)))


def make_repeats(R, reps, D, kind, seed=0):
    """X of R distinct rows, each repeated `reps` times, in a seeded order: row r sits at 3.5 r length-scales along axis 0, so two distinct rows are at least 3.5 length-scales apart and an unpicked distinct row keeps d of order s2.  Returns the
    case and the group (N,) of every row."""
    p = make_case(R * reps, R, D, kind, seed)
    g = torch.Generator().manual_seed(seed + 5)
    base = torch.randn(R, D, dtype=F64, generator=g)
    base[:, 0] = 3.5 * softplus(p["raw_ls"][0]) * torch.arange(R, dtype=F64)
    base[:, 1:] *= 0.1
    group = torch.arange(R).repeat_interleave(reps)[torch.randperm(R * reps, generator=g)]
    p["X"] = base[group].contiguous()
    return p, group


def kernel_column(A, pj, s2, kind):
    """k(x_n, x_pj) for all n from the scaled rows A = X / length-scale: `kernel`'s formulas in numpy, one column at a time (the
    recurrence needs N values per step, not the N x N matrix; `dense_route` uses `kernel` itself)."""
    d2 = ((A - A[pj:pj + 1]) ** 2).sum(-1)
    if kind == "scale_matern32":
        r = np.sqrt(np.maximum(d2, 1e-30))
        return s2 * (1.0 + SQRT3 * r) * np.exp(-SQRT3 * r)
    return s2 * np.exp(-0.5 * d2)


def greedy(p, M=None, min_var=MIN_VAR, follow=None):
    """The recurrence.  follow = None: it chooses (arg-max, smallest index at a tie) and stops at d_max <= min_var.  follow = a
    sequence of row indices: it takes those pivots as given, never stops and never chooses.  Returns a dict:
      idx (M_eff,), trace (M_eff + 1,), C (M_eff, N), M_eff,
      dmax (M_eff,)  the largest d over the rows not picked, before step j's pick,
      dpiv (M_eff,)  d of the pivot taken at step j,
      gap  (M_eff,)  dmax minus the second largest d over the rows not picked (inf with one row left)."""
    N = p["N"]
    M = p["M"] if M is None else M
    A = (p["X"] / softplus(p["raw_ls"]).reshape(1, -1)).numpy()
    s2 = softplus(p["raw_os"]).reshape(())
    d = torch.full((N,), float(s2), dtype=F64)
    picked = torch.zeros(N, dtype=torch.bool)
    C = torch.zeros(M, N, dtype=F64)
    idx, trace, dmax, dpiv, gap = [], [float(N * s2)], [], [], []
    for j in range(M if follow is None else len(follow)):
        dd = torch.where(picked, torch.full_like(d, -1.0), d)
        top = torch.topk(dd, min(2, N))
        best = float(top.values[0])
        pj = int(torch.nonzero(dd == best)[0]) if follow is None else int(follow[j])       # the smallest index at a tie
        if follow is None and best <= min_var:
            break
        second = float(top.values[1]) if N - j >= 2 else -math.inf
        dp = d[pj]
        acc, tmp, Cn = np.zeros(N), np.empty(N), C.numpy()                  # (in place: the same sums, without N-vectors allocated)
        for l in range(j):
            np.multiply(Cn[l], Cn[l, pj], out=tmp)
            acc += tmp
        acc = torch.from_numpy(acc)
        k = torch.from_numpy(kernel_column(A, pj, float(s2), p["kernel"]))
        c = (k - acc) / torch.sqrt(dp)
        C[j] = c
        d = torch.clamp(d - c * c, min=0.0)
        picked[pj] = True
        idx.append(pj)
        dmax.append(best)
        dpiv.append(float(dp))
        gap.append(best - second)
        trace.append(float(d[~picked].sum()))
    m_eff = len(idx)
    return dict(idx=torch.tensor(idx, dtype=torch.int64), trace=torch.tensor(trace, dtype=F64), C=C[:m_eff], M_eff=m_eff,
                dmax=torch.tensor(dmax, dtype=F64), dpiv=torch.tensor(dpiv, dtype=F64), gap=torch.tensor(gap, dtype=F64))


def dense_route(p, idx):
    """(d (len(idx) + 1, N), trace (len(idx) + 1,), cond(K[S,S]) at the last step): d^(j) = diag(K - K[:,S] K[S,S]^-1 K[S,:]) with
    S the first j rows of idx, by a dense solve; trace = the sum of the same."""
    K = kernel(p["X"], p["X"], p["raw_ls"], p["raw_os"], p["kernel"])
    ds, cond = [torch.diagonal(K).clone()], 1.0
    for j in range(1, len(idx) + 1):
        S = idx[:j]
        Kss, Ksx = K[S][:, S], K[S]
        ds.append(torch.diagonal(K) - (Ksx * torch.linalg.solve(Kss, Ksx)).sum(0))
        if j == len(idx):
            cond = float(torch.linalg.cond(Kss))
    d = torch.stack(ds)
    return d, d.sum(1), cond


def measure(case):
    """The figures `GREEDY_CPU` records for a case."""
    p = make_case(*case)
    r = greedy(p)
    d_dense, tr_dense, cond = dense_route(p, r["idx"])
    s2, N = p["s2"], p["N"]
    # the recurrence's d after j picks: s2 - sum_{l<j} C[l]^2, rebuilt step by step as the recurrence does
    d = torch.full((N,), s2, dtype=F64)
    picked = torch.zeros(N, dtype=torch.bool)
    worst_d = 0.0
    for j in range(r["M_eff"]):
        d = torch.clamp(d - r["C"][j] ** 2, min=0.0)
        picked[r["idx"][j]] = True
        if (~picked).any():
            worst_d = max(worst_d, float((d - d_dense[j + 1])[~picked].abs().max()) / s2)
    worst_tr = float((r["trace"] - tr_dense).abs().max()) / (N * s2)
    return dict(d=worst_d, trace=worst_tr, cond=cond), r


if __name__ == "__main__":
    for case in CPU_CASES:
        m, _ = measure(case)
        print("    %r: dict(d=%.1e, trace=%.1e, cond=%.1e)," % (case, m["d"], m["trace"], m["cond"]))
