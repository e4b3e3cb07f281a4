"""Step time of the composed heteroscedastic training step (models._elbo_hetero: two q(f) launches with their adjoints, two KL
terms, one tgp_ell_hetero_f64) on the Power shape (N = 8611, D = 4, M = 100, S = 32, SAL x 1) against the eager TGP_LIK_FLOW step
(ops.ElboFunction, the fused row kernels) of a model with the same chain and the same targets -- both as `ELBO(X, Y)` plus
`backward()` of the model classes, which is what the eager trainer runs per step.  Beside it the two likelihood launches alone:
ops.ell_hetero (k_ell_quad<EllHetero>) against ops.ell_flow (k_ell_quad<EllGauss>) on the same moments, at the same lanes per row
and nodes in flight (ell_plan does not look at the likelihood).  Everything is timed in ALTERNATING blocks in one process on one
device, HIP events around each block (the warm-up / steps convention of bench.py, which this script does not touch).  Prints one
JSON line; not a bench.py workload, and no threshold is attached to its numbers.

    python tools/bench_hetero.py --steps 1000 --warmup 50 --blocks 5 > profiles/hetero_step.txt
"""
import argparse
import json
import math
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import torch                                    # noqa: E402

from oracle import tgp_oracle as orc            # noqa: E402

DEV = "cuda:0"
N, D, M, S = 8611, 4, 100, 32


def build(prob, hetero):
    """A TGP model (SAL x 1) on the problem's rows: HeteroscedasticGaussian over two latent GPs, or GaussianNonLinearMean."""
    from tgp.pytorch_amd import config as cg
    from tgp.pytorch_amd import flows as G
    from tgp.pytorch_amd.kernels import instance_kernel
    from tgp.pytorch_amd.likelihoods import GaussianNonLinearMean, HeteroscedasticGaussian
    from tgp.pytorch_amd.models import sparse_MF_SP
    cg.set_maximum_precission()
    cg.device = DEV
    Dy = 2 if hetero else 1
    K = instance_kernel("scale_rbf", ard_num_dim=D, num_multioutput=Dy, kernel_is_shared=False,
                        init_params={"length_scale": 2.0, "kernel_scale": 2.0, "noisy_variance": 1e-6})
    lik = HeteroscedasticGaussian(0.05, S) if hetero else GaussianNonLinearMean(1, 0.05, False, S)
    flows = [G.SAL(1), [("identity", [])]] if hetero else [G.SAL(1)]
    ip = {"variational_distribution": {"variance_scale": 1e-2, "mean_scale": 0.0}}
    model = sparse_MF_SP(["zero", K], prob["X"], prob["params"]["Z"].clone(), float(N), lik, Dy, True, False, False, False, False,
                         flows, "single", 0.0, init_params=ip)
    return model.to(DEV)


def stepper(model, X, Y):
    def step():
        for q in model.parameters():
            q.grad = None
        elbo, _, _ = model.ELBO(X, Y)
        (-elbo).backward()
        return elbo
    return step


def raw_ell(hetero, y, mu, v, c, spec, theta):
    """A closure around ONE library call -- tgp_ell_hetero_f64 or tgp_ell_flow_f64 with every gradient asked for -- on buffers made
    once: the likelihood kernel and its partial-sum launch, no allocation per call."""
    from tgp.pytorch_amd import lib as L
    from tgp.pytorch_amd import ops
    lib = L.load()
    md, keep = ops._flow_model(y.numel(), S, spec, theta, c, DEV, 1.0, lik=L.LIK_HETERO if hetero else L.LIK_FLOW)
    ws = torch.empty(lib.tgp_ell_workspace_bytes(y.numel(), spec.P, 0) // 8 + 16, dtype=torch.float64, device=DEV)
    out = torch.empty(2, dtype=torch.float64, device=DEV)
    gmu, gv, gth = torch.empty_like(mu), torch.empty_like(v), torch.empty(max(spec.P, 1), dtype=torch.float64, device=DEV)
    entry = lib.tgp_ell_hetero_f64 if hetero else lib.tgp_ell_flow_f64
    args = (md, L.ptr(y), L.ptr(mu), L.ptr(v), None, L.ptr(out), L.ptr(gmu), L.ptr(gv), L.ptr(gth), None, L.ptr(ws), ws.numel() * 8)

    def call():
        L.check(entry(*args, L.stream_ptr()), "likelihood entry")
        return keep, out
    return call


def block(step, steps):
    """microseconds per call over `steps` calls"""
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(steps):
        step()
    t1.record()
    torch.cuda.synchronize()
    return 1e3 * t0.elapsed_time(t1) / steps


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200, help="calls per timed block")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--blocks", type=int, default=5, help="alternating timed blocks per candidate")
    ap.add_argument("--ell-calls", type=int, default=5000, help="likelihood-entry calls per timed block (a call is ~15 us)")
    args = ap.parse_args(argv)
    from tgp.pytorch_amd.flow import compile_flow
    prob =orc.synthetic_problem(N, D, M, seed=0, flow="sal1", S=S)
    X, Y = prob["X"].to(DEV), prob["Y"].to(DEV)
    het, flw = build(prob, True), build(prob, False)
    # the likelihood launches alone, on the hetero model's own moments
    with torch.no_grad():
        mu, v = het.marginal_variational_qf_parameters(X, diagonal=True, is_duvenaud=False)
    mu, v = mu.squeeze(2).contiguous(), v.squeeze(2).contiguous()
    spec, theta_list, _ = compile_flow(het.G_matrix[0])
    theta = torch.stack([q.detach().reshape(()) for q in theta_list])
    c = het.likelihood.log_var_noise.detach().reshape(-1)[:1].contiguous()
    y = Y.reshape(-1).contiguous()
    mu0, v0 = mu[0].contiguous(), v[0].contiguous()
    cands = {"hetero_step": stepper(het, X, Y), "flow_step": stepper(flw, X, Y),
             "ell_hetero": raw_ell(True, y, mu, v, c, spec, theta), "ell_flow": raw_ell(False, y, mu0, v0, c, spec, theta)}
    last = {}
    for k, fn in cands.items():
        for _ in range(args.warmup):
            last[k] = fn()
    torch.cuda.synchronize()
    times = {k: [] for k in cands}
    for _ in range(args.blocks):
        for k, fn in cands.items():
            times[k].append(block(fn, args.ell_calls if k.startswith("ell_") else args.steps))
    res = {"workload": "eager_step_power_sal1", "N": N, "D": D, "M": M, "S": S, "steps": args.steps, "warmup": args.warmup,
           "blocks": args.blocks, "ell_calls": args.ell_calls, "device": torch.cuda.get_device_name(0)}
    for k, ts in times.items():
        res[k + "_us_median"] = sorted(ts)[len(ts) // 2]
        res[k + "_us_blocks"] = ts
    res["hetero_elbo"], res["flow_elbo"] = float(last["hetero_step"].detach()), float(last["flow_step"].detach())
    assert math.isfinite(res["hetero_elbo"]) and math.isfinite(res["flow_elbo"])
    res["hetero_over_flow_step"] = res["hetero_step_us_median"] / res["flow_step_us_median"]
    res["ell_hetero_out"], res["ell_flow_out"] = last["ell_hetero"][1].tolist(), last["ell_flow"][1].tolist()
    res["ell_hetero_over_ell_flow"] = res["ell_hetero_us_median"] / res["ell_flow_us_median"]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
