"""Generate the fixtures of the Bernoulli (probit) likelihood (tests/golden/bern_*.npz) by executing the reference's own
files (build container only; never runs on the GPU box).

Run:  python tools/gen_golden_bernoulli.py

The reference on sys.path with the oracle/shims stand-ins and the parameter recipe come from oracle/gen_golden.py,
imported read-only; the flows' program rows and raw-value perturbation from tools/gen_golden_flows.py.  This file adds
the reference's Bernoulli likelihood (dsp/likelihoods/Bernoulli.py) with sparse_MF_GP / sparse_MF_SP, binary labels from
a seeded Bernoulli draw, and the key schema of the other fixtures (p_*, g_*, program, xs/ws, ELBO/ELL/KLD, history)
plus pred_P / test_logp_sum.  Every case keeps max |G(f0)| <= 6 over the nodes of weight > 1e-14 (asserted): there the
reference's Phi / 1 - Phi rounding stays far below the parity tolerances.  The flowed pred_P is the reference's link and
quadrature with each row's own std, not its marginal_moments (one std for the whole batch).
"""
import math
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)

from oracle import gen_golden as gg        # noqa: E402  (sets up the reference, the shims and float64)

import numpy as np                          # noqa: E402
import torch                                # noqa: E402

import gen_golden_flows as gf               # noqa: E402
from dsp import flows as rflows             # noqa: E402
from dsp.likelihoods import Bernoulli       # noqa: E402
from dsp.models.flow import instance_flow   # noqa: E402
from gpytorch.utils.quadrature import GaussHermiteQuadrature1D   # noqa: E402

from oracle import tgp_oracle as orc        # noqa: E402

# fixture flow name -> (numpy seed, reference spec generator)
FLOWS = {
    "sal_invbcl1": (21, lambda: rflows.build_chain("SAL_InvBCL", 1, constraint=None)),
    "bcl_al2": (22, lambda: rflows.build_chain("BCL_AL", 2, constraint=None)),
    "arcsl2": (23, lambda: rflows.ArcSL(2)),
}


def problem(N, D, M, S, seed=0, band=None):
    """orc.synthetic_problem's recipe with outputscale 0.5 and m scaled by 0.5 (|mu| <~ 3, small v) and binary labels
    y ~ Bernoulli(Phi(2 sin(X w))).  `band`: q(u)'s factor keeps only that many sub-diagonals (a large-M fixture that
    stays under the size limit)."""
    prob = orc.synthetic_problem(N, D, M, seed=seed, flow=None, S=S)
    p = prob["params"]
    if band is not None:
        p["Lam"] = torch.tril(torch.triu(p["Lam"], -band))
    p["raw_outputscale"] = torch.log(torch.expm1(torch.tensor([0.5], dtype=torch.float64)))
    p["m"] = 0.5 * p["m"]
    g = torch.Generator().manual_seed(500 + seed)
    w = torch.randn(D, generator=g, dtype=torch.float64)
    pr = torch.special.ndtr(2.0 * torch.sin(prob["X"] @ w))
    prob["Y"] = torch.bernoulli(pr, generator=g).reshape(N, 1)
    return prob


def bern_lik(S):
    lik = Bernoulli()
    lik.quad_points = S
    lik.quadrature_distribution = GaussHermiteQuadrature1D(S)
    return lik


def attach_flow(prob, flow, seed=0):
    np.random.seed(FLOWS[flow][0])
    specs = FLOWS[flow][1]()
    prog, prm, islam = gf.program_of(instance_flow(specs))
    theta = torch.stack([q.detach().reshape(()) for q in prm]).clone()
    g = torch.Generator().manual_seed(1000 + seed)
    noise = 0.3 * torch.randn(theta.shape, generator=g, dtype=torch.float64)
    theta = torch.where(torch.tensor(islam), (1.0 + noise).clamp(0.5, 2.0), theta + noise)
    prob["program"], prob["params"]["theta"] = prog, theta
    return specs


def build(prob, flow):
    """The reference's SVGP (flow None), TGP (a FLOWS name) or ID_TGP ('idsal1', eval mode) with Bernoulli, prob's values."""
    X, p = prob["X"], prob["params"]
    N, D = X.shape
    M = p["Z"].shape[0]
    S = prob["xs"].shape[0]
    K = gg.instance_kernel("scale_rbf", ard_num_dim=D, num_multioutput=1, kernel_is_shared=False, init_params=gg.KINIT)
    lik = bern_lik(S)
    if flow is None:
        model = gg.sparse_MF_GP(["zero", K], X, p["Z"].clone(), N, lik, 1, True, False, False, False, False, 0.0,
                                init_params=gg.IP)
    elif flow == "idsal1":
        specs = rflows.SAL(1, input_dependent=True, input_dim=D, num_hidden_layers=2, batch_norm=0, dropout=0.25,
                           hidden_dim=50, hidden_activation="relu", inference="MC_dropout")
        specs = instance_flow(specs)
        specs.turn_off_initializer_parameters()
        model = gg.sparse_MF_SP(["zero", K], X, p["Z"].clone(), N, lik, 1, True, False, False, False, False,
                                [specs], "single", 0.0, init_params=gg.IP)
        prob["program"] = [(orc.FLOW_SAL, 0, 0, orc.FLAG_PER_ROW)]
    else:
        specs = attach_flow(prob, flow)
        model = gg.sparse_MF_SP(["zero", K], X, p["Z"].clone(), N, lik, 1, True, False, False, False, False,
                                [specs], "single", 0.0, init_params=gg.IP)
    with torch.no_grad():
        model.Z.data = p["Z"].reshape(1, M, D).clone()
        model.q_U.variational_mean.data = p["m"].reshape(1, M).clone()
        model.q_U.chol_variational_covar.data = p["Lam"].reshape(1, M, M).clone()
        model.covariance_function.raw_outputscale.data = p["raw_outputscale"].reshape(1).clone()
        model.covariance_function.base_kernel.raw_lengthscale.data = p["raw_lengthscale"].reshape(1, 1, D).clone()
        if flow is not None and flow != "idsal1":
            for q, val in zip(gf.program_of(model.G_matrix[0])[1], p["theta"]):
                q.data = val.clone().reshape(q.shape)
    if flow == "idsal1":
        torch.manual_seed(0)
        with torch.no_grad():
            for blk in model.G_matrix[0].flow_arr:
                if hasattr(blk, "NNets_a"):
                    for nm, bias in (("a", 0.0), ("b", 1.0)):
                        last = list(getattr(blk, "NNets_" + nm))[-1].w
                        last.weight.mul_(0.3)
                        last.bias.fill_(bias)
    return model


def warp(model, f0, X):
    """G(f0) for f0 (S, N) through the model's flow (identity for SVGP)."""
    out = model.G_matrix[0](f0, X)
    return out


def node_check(model, mu, v, X, xs, ws):
    keep = ws / math.sqrt(math.pi) > 1e-14
    f0 = mu.reshape(1, -1) + torch.sqrt(2.0 * v.clamp(min=0.0)).reshape(1, -1) * xs[keep].reshape(-1, 1)
    g = warp(model, f0, X)
    gmax = float(g.abs().max())
    assert gmax <= 6.0, "max |G(f0)| = %g > 6: the reference's Phi rounding would show" % gmax
    return gmax


def pred_P(model, mu, v, X, xs, ws, identity):
    """P(y = 1) per row: R&W 3.80 for the identity flow (the reference's marginal_moments), else the reference's link
    and quadrature with each row's own std."""
    if identity:
        return torch.special.ndtr(mu / torch.sqrt(1.0 + v))
    f0 = mu.reshape(1, -1) + torch.sqrt(2.0 * v.clamp(min=0.0)).reshape(1, -1) * xs.reshape(-1, 1)
    P = (model.likelihood.link_function(warp(model, f0, X)) * (ws / math.sqrt(math.pi)).reshape(-1, 1)).sum(0)
    return P.clamp(0.0, 1.0)


def step0(prob, flow, name):
    torch.manual_seed(0)
    model = build(prob, flow)
    model.set_is_training(True)
    X, Y, p = prob["X"], prob["Y"], prob["params"]
    captured = {}
    hooks = []
    if flow == "idsal1":
        model.eval()                          # dropout off: deterministic per-row parameters
        for bi, blk in enumerate(model.G_matrix[0].flow_arr):
            if hasattr(blk, "NNets_a"):
                for nm in ("a", "b"):
                    def hook(mod, inp, out, key=(bi, nm)):
                        if key not in captured and out.requires_grad:
                            out.retain_grad()
                            captured[key] = out
                    hooks.append(getattr(blk, "NNets_" + nm).register_forward_hook(hook))
    elbo, ell, kld = model.ELBO(X, Y)
    elbo.backward()
    for h in hooks:
        h.remove()
    out = {"X": X, "Y": Y, "xs": prob["xs"], "ws": prob["ws"], "N_total": np.float64(prob["N_total"]),
           "ELBO": elbo.detach(), "ELL": ell.detach(), "KLD": kld.detach(),
           "g_Z": model.Z.grad[0], "g_m": model.q_U.variational_mean.grad[0],
           "g_Lam": model.q_U.chol_variational_covar.grad[0],
           "g_raw_outputscale": model.covariance_function.raw_outputscale.grad,
           "g_raw_lengthscale": model.covariance_function.base_kernel.raw_lengthscale.grad.reshape(-1)}
    for k, v in p.items():
        if k != "log_var_noise":
            out["p_" + k] = v
    out["program"] = np.array(prob["program"] if prob.get("program") else np.zeros((0, 4)), dtype=np.int32)
    if flow is not None and flow != "idsal1":
        out["g_theta"] = torch.stack([q.grad.reshape(()) for q in gf.program_of(model.G_matrix[0])[1]])
    if captured:
        keys = sorted(captured.keys())
        out["rowp"] = torch.stack([captured[k].detach().reshape(-1) for k in keys], 1)
        out["g_rowp"] = torch.stack([captured[k].grad.reshape(-1) for k in keys], 1)
    with torch.no_grad():
        mu, v = model.marginal_variational_qf_parameters(X, diagonal=True, is_duvenaud=False, init_Z=None)
        mu, v = mu.reshape(-1), v.reshape(-1)
        out["mu"], out["v"] = mu, v
        X3 = X.reshape(1, *X.shape)
        out["gmax"] = np.float64(node_check(model, mu, v, X3, prob["xs"], prob["ws"]))
        if not captured:
            P = pred_P(model, mu, v, X3, prob["xs"], prob["ws"], flow is None)
            if flow is None:          # the reference's own predictive path gives the same closed form
                model.set_is_training(False)
                Pm, _, _, _ = model.predictive_distribution(X3, diagonal=True)
                assert torch.allclose(Pm.reshape(-1), P, rtol=1e-13, atol=0)
            y = Y.reshape(-1)
            out["pred_P"] = P
            out["test_logp_sum"] = (y * torch.log(P) + (1 - y) * torch.log1p(-P)).sum().reshape(1)
    gg.save(name, out)


def adam_steps(prob, flow, name, steps=5):
    model = build(prob, flow)
    model.set_is_training(True)
    opt = torch.optim.Adam(model.parameters(), lr=0.01)
    hist = []
    for _ in range(steps):
        elbo, ell, kld = model.ELBO(prob["X"], prob["Y"])
        opt.zero_grad()
        (-elbo).backward()
        opt.step()
        hist.append([elbo.item(), ell.item(), kld.item()])
    out = {"X": prob["X"], "Y": prob["Y"], "xs": prob["xs"], "ws": prob["ws"], "N_total": np.float64(prob["N_total"]),
           "history": np.array(hist)}
    for k, v in prob["params"].items():
        if k != "log_var_noise":
            out["p_" + k] = v
    out["program"] = np.array(prob["program"] if prob.get("program") else np.zeros((0, 4)), dtype=np.int32)
    if flow is not None:
        out["final_theta"] = torch.stack([q.detach().reshape(()) for q in gf.program_of(model.G_matrix[0])[1]])
    out["final_Z"] = model.Z.detach()[0]
    out["final_m"] = model.q_U.variational_mean.detach()[0]
    gg.save(name, out)


def main():
    step0(problem(64, 3, 8, 16), None, "bern_tiny_svgp")
    step0(problem(400, 4, 40, 32), None, "bern_med_svgp")
    step0(problem(200, 4, 20, 32), "sal_invbcl1", "bern_med_sal_invbcl1")
    step0(problem(200, 4, 20, 32), "bcl_al2", "bern_med_bcl_al2")
    step0(problem(200, 4, 20, 32), "arcsl2", "bern_med_arcsl2")
    step0(problem(96, 4, 12, 16), "idsal1", "bern_idsal1")
    # general-M path with several row chunks: the GPU test forces 128-row chunks (TGP_PLAN_CHUNK_ROWS)
    step0(problem(400, 6, 200, 16, band=12), "sal_invbcl1", "bern_bigm_sal_invbcl1")
    adam_steps(problem(64, 3, 8, 16), None, "bern_adam5_svgp")
    adam_steps(problem(64, 3, 8, 16), "bcl_al2", "bern_adam5_bcl_al2")


if __name__ == "__main__":
    main()
