"""Time of the full-covariance q(f) (tgp_qf_cov_f64) and of S = 100 joint draws (tgp_qf_joint_sample_f64) at N = 4096 rows, for
M = 100 (D = 4, the Power shape) and M = 1000 (D = 8, the airline shape), with HIP events around the C entries (buffers
allocated once, outside the timed region).  Beside them the SAME algebra composed from torch ops on the same device
(tests/fullcov_model.py: kernel matrices, torch.linalg.cholesky, solve_triangular, matmul) -- the baseline.  Writes
profiles/fullcov.txt (or --out) and prints it.  K_MM gets a jitter of 1e-6 in both versions; the draws factorise
Sigma + 1e-6 I.

    python tools/bench_fullcov.py --steps 20 --warmup 3
"""
import argparse
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import torch                                    # noqa: E402

import fullcov_model as fm                      # noqa: E402
from oracle import tgp_oracle as orc            # noqa: E402
from tgp.pytorch_amd import lib as L            # noqa: E402
from tgp.pytorch_amd import ops                 # noqa: E402

DEV = "cuda:0"
JIT = 1e-6


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(steps):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / steps


def case(N, D, M, S, steps, warmup):
    lib = L.load()
    prob = orc.synthetic_problem(N, D, M, seed=0, flow=None, S=8)
    X = prob["X"].to(DEV)
    p = prob["params"]
    Z, rl, ro, m, Lam = (p[k].to(DEV).contiguous() for k in ("Z", "raw_lengthscale", "raw_outputscale", "m", "Lam"))
    lvn = torch.zeros(1, dtype=torch.float64, device=DEV)
    md, _ = ops._model_struct(X, Z, rl, ro, m, Lam, lvn, 1.0, JIT, 1.0, None, None, None, "scale_rbf")
    nb = lib.tgp_qf_cov_workspace_bytes(N, D, M)
    ws = torch.empty(nb // 8, dtype=torch.float64, device=DEV)
    mu = torch.empty(N, dtype=torch.float64, device=DEV)
    Sigma = torch.empty(N, N, dtype=torch.float64, device=DEV)
    status = torch.zeros(8, dtype=torch.int32, device=DEV)
    st = L.stream_ptr()

    def hip_cov():
        L.check(lib.tgp_qf_cov_f64(md, L.ptr(X), L.ptr(mu), L.ptr(Sigma), L.ptr(status), L.ptr(ws), nb, st), "tgp_qf_cov_f64")

    eps = torch.randn(S, N, dtype=torch.float64, device=DEV, generator=torch.Generator(DEV).manual_seed(1))
    nb2 = lib.tgp_qf_joint_sample_workspace_bytes(N, S)
    ws2 = torch.empty(nb2 // 8, dtype=torch.float64, device=DEV)
    F0 = torch.empty(S, N, dtype=torch.float64, device=DEV)
    status2 = torch.zeros(8, dtype=torch.int32, device=DEV)

    def hip_draw():
        L.check(lib.tgp_qf_joint_sample_f64(L.ptr(mu), L.ptr(Sigma), N, JIT, L.ptr(eps), S, L.ptr(F0), None, L.ptr(status2),
                                            L.ptr(ws2), nb2, st), "tgp_qf_joint_sample_f64")

    ref = {}

    def torch_cov():
        ref["mu"], ref["Sigma"] = fm.qf_cov(X, Z, rl, ro, m, Lam, jitter=JIT, kernel="scale_rbf")

    def torch_draw():
        ref["F0"], _ = fm.joint_draw(ref["mu"], ref["Sigma"], eps, JIT)

    t_hc = timed(hip_cov, steps, warmup)
    t_tc = timed(torch_cov, steps, warmup)
    t_hd = timed(hip_draw, steps, warmup)
    t_td = timed(torch_draw, steps, warmup)
    d_S = float((Sigma - ref["Sigma"]).abs().max())
    return ("N=%d D=%d M=%d S=%d | tgp_qf_cov_f64 %.3f ms, torch ops %.3f ms | tgp_qf_joint_sample_f64 %.3f ms, torch ops %.3f ms | "
            "status %d/%d, max|Sigma - torch| %.2e" % (N, D, M, S, t_hc, t_tc, t_hd, t_td, int(status[0]), int(status2[0]), d_S))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "fullcov.txt"))
    args = ap.parse_args(argv)
    lines = ["tools/bench_fullcov.py --steps %d --warmup %d (%s; HIP events, mean per call; one box, one run)"
             % (args.steps, args.warmup, torch.cuda.get_device_name(0))]
    for N, D, M in ((4096, 4, 100), (4096, 8, 1000)):
        lines.append(case(N, D, M, 100, args.steps, args.warmup))
    text = "\n".join(lines) + "\n"
    with open(args.out, "w") as fh:
        fh.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()
