"""Generate the fixtures of the warped Gaussian likelihood (tests/golden/warp_*.npz) by executing the reference's own
files (build container only; never runs on the GPU box).

Run:  python tools/gen_golden_warped.py

The reference on sys.path with the oracle/shims stand-ins and the parameter recipe come from oracle/gen_golden.py,
imported read-only; the arcsinh / Box-Cox program rows and raw-value perturbation from tools/gen_golden_flows.py.  The
reference's sparse_MF_SP.ELL cannot call WarpedGaussianLinearMean (it passes flow= and X= keywords the class does not
take), so this file composes the parts itself: the reference's sparse_MF_GP gives marginal_variational_qf_parameters and
KLD, the reference's WarpedGaussianLinearMean gives expected_log_prob / marginal_moments, and

    ELBO = N / MB * lik.expected_log_prob(Y.t(), mu, v) - KLD

is differentiated by autograd with respect to every parameter.  Key schema of the other fixtures (p_*, g_*, program,
xs/ws, ELBO/ELL/KLD, history, final_*) plus t = T(Y), logdet, g_mu / g_v of the likelihood alone, pred_* (moments on a
held-out block of rows) and inv_grid / inv_x (flow.inverse) for the kinds the reference inverts in closed form.

Every case asserts min T'(Y) > 0, finite log T', and (closed-form kinds) |inverse(forward(Y)) - Y| <= 1e-12.
"""
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
from dsp.likelihoods import GaussianLinearMean                      # noqa: E402
from dsp.likelihoods.WarpedGaussianLinearMean import WarpedGaussianLinearMean   # noqa: E402
from dsp.models.flow import AffineFlow, IdentityFlow, StepFlow, instance_flow    # noqa: E402

from oracle import tgp_oracle as orc        # noqa: E402


def _steptanh(nb, ns):
    np.random.seed(0)
    return rflows.StepTanhL(nb, ns, add_f0=True)


# fixture flow name -> (numpy seed, reference spec generator, does the reference invert it in closed form?)
FLOWS = {
    "sal2": (31, lambda: rflows.SAL(2), True),
    "arcsl2": (32, lambda: rflows.ArcSL(2), True),
    "sal_al1": (33, lambda: rflows.build_chain("SAL_AL", 1), True),
    "bcl_al1": (34, lambda: rflows.build_chain("BCL_AL", 1, constraint=None), False),     # BoxCoxFlow.inverse returns None
    "tanh3x2": (35, lambda: _steptanh(3, 2), False),                                        # TanhFlow.inverse raises
}


def program_of(comp):
    """gen_golden_flows.program_of plus the tanh-step blocks: (program rows, [nn.Parameter] in theta order, [is lam])."""
    prog, prm, islam = [], [], []
    for fl in comp.flow_arr:
        if isinstance(fl, StepFlow):
            poff = len(prm)
            K = len(fl.flow_arr)
            prog.append((orc.FLOW_STEPTANH, K, poff, orc.FLAG_ADD_F0 if fl.add_init_f0 else 0))
            for t in fl.flow_arr:
                prm += [t.a, t.b, t.c, t.d]
                islam += [False] * 4
        else:
            one = type("C", (), {"flow_arr": [fl]})
            p1, q1, l1 = gf.program_of(one)
            k, K, _, fl_ = p1[0]
            prog.append((k, K, len(prm), fl_))
            prm += q1
            islam += l1
    return prog, prm, islam


def make_flow(flow, seed=0):
    """Reference CompositeFlow with perturbed raw values, its program and theta."""
    if flow is None:
        return None, [], torch.zeros(0, dtype=torch.float64)
    np.random.seed(FLOWS[flow][0])
    comp = instance_flow(FLOWS[flow][1]())
    prog, prm, islam = program_of(comp)
    theta = torch.stack([q.detach().reshape(()).to(torch.float64) for q in prm]).clone()
    g = torch.Generator().manual_seed(2000 + seed)
    noise = 0.3 * torch.randn(theta.shape, generator=g, dtype=torch.float64)
    if flow != "tanh3x2":        # (the tanh-step generator draws its own random values)
        theta = torch.where(torch.tensor(islam), (1.0 + noise).clamp(0.5, 2.0), theta + noise)
        # every block increasing: |.| of the slopes (AFFINE a, SAL b, ARCSINH b and d) -- a composite T must be strictly
        # increasing on the targets, and a perturbed arcsinh chain is not by itself
        for kind, K, poff, flags in prog:
            for j in {orc.FLOW_AFFINE: (0,), orc.FLOW_SAL: (1,), gf.FLOW_ARCSINH: (1, 3)}.get(kind, ()):
                theta[poff + j] = theta[poff + j].abs()
    with torch.no_grad():
        for q, val in zip(prm, theta):
            q.data = val.clone().reshape(q.shape)
    return comp, prog, theta


def problem(N, D, M, S, seed=0, band=None, away_from_zero=False):
    prob = orc.synthetic_problem(N, D, M, seed=seed, flow=None, S=S)
    if band is not None:
        prob["params"]["Lam"] = torch.tril(torch.triu(prob["params"]["Lam"], -band))
    if away_from_zero:           # Box-Cox with lam < 1: log T'(y) = (lam - 1) log|y| needs |y| away from 0
        Y = prob["Y"]
        prob["Y"] = torch.sign(Y) * (Y.abs() + 0.25)
    g = torch.Generator().manual_seed(700 + seed)
    # held-out rows near the inducing inputs (small q(f) variance): the inverse of an arcsinh chain grows like a double
    # exponential, and with the prior's variance the outer Gauss-Hermite nodes overflow float64 in the reference itself
    Z = prob["params"]["Z"]
    prob["Xte"] = Z[torch.arange(48) % M] + 0.05 * torch.randn(48, D, generator=g, dtype=torch.float64)
    return prob


class _Identity(IdentityFlow):
    def forward(self, f, X=None):
        return f * 1.0     # (a graph node so that forward_grad's autograd call has something to differentiate)


def build(prob, flow, kernel="scale_rbf"):
    """(reference sparse_MF_GP with the reference's WarpedGaussianLinearMean, the flow's parameters in theta order)."""
    X, p = prob["X"], prob["params"]
    N, D = X.shape
    M = p["Z"].shape[0]
    S = prob["xs"].shape[0]
    comp, prog, theta = make_flow(flow)
    prob["program"], p["theta"] = prog, theta
    K = gg.instance_kernel(kernel, ard_num_dim=D, num_multioutput=1, kernel_is_shared=False, init_params=gg.KINIT)
    lik = WarpedGaussianLinearMean(1, 0.05, False, comp if comp is not None else _Identity(), S)
    model = gg.sparse_MF_GP(["zero", K], X, p["Z"].clone(), N, lik, 1, True, False, False, False, False, 0.0,
                            init_params=gg.IP)
    with torch.no_grad():
        model.Z.data = p["Z"].reshape(1, M, D).clone()
        model.q_U.variational_mean.data = p["m"].reshape(1, M).clone()
        model.q_U.chol_variational_covar.data = p["Lam"].reshape(1, M, M).clone()
        model.covariance_function.raw_outputscale.data = p["raw_outputscale"].reshape(1).clone()
        model.covariance_function.base_kernel.raw_lengthscale.data = p["raw_lengthscale"].reshape(1, 1, D).clone()
        model.likelihood.log_var_noise.data = p["log_var_noise"].reshape(1, 1).clone()
    prm = program_of(comp)[1] if comp is not None else []
    return model, prm


def elbo_of(model, X, Y):
    X3 = X.repeat(1, 1, 1)
    kld = model.KLD().sum()
    mu, v = model.marginal_variational_qf_parameters(X3, diagonal=True, is_duvenaud=False, init_Z=None)
    mu, v = mu.squeeze(dim=2), v.squeeze(dim=2)
    ell = model.N / Y.size(0) * model.likelihood.expected_log_prob(Y.t(), mu, v).sum()
    return ell - kld, ell, kld, mu, v


def base_out(prob):
    out = {"X": prob["X"], "Y": prob["Y"], "xs": prob["xs"], "ws": prob["ws"], "N_total": np.float64(prob["N_total"])}
    for k, v in prob["params"].items():
        out["p_" + k] = v
    out["program"] = np.array(prob["program"] if prob["program"] else np.zeros((0, 4)), dtype=np.int32)
    return out


def step0(prob, flow, name, kernel="scale_rbf"):
    torch.manual_seed(0)
    model, prm = build(prob, flow, kernel)
    model.set_is_training(True)
    lik = model.likelihood
    X, Y = prob["X"], prob["Y"]
    fl = lik.flow[0]
    # ---- the generator's own checks
    with torch.no_grad():
        t = fl.forward(Y.t())
    dT = fl.forward_grad(Y.t()).detach()
    assert float(dT.min()) > 0.0, "%s: min T'(Y) = %g" % (name, float(dT.min()))
    assert bool(torch.isfinite(torch.log(dT)).all()), name
    closed = flow is None or FLOWS[flow][2]
    if closed:
        with torch.no_grad():
            rt = float((fl.inverse(t) - Y.t()).abs().max())
        assert rt <= 1e-12, "%s: reference round trip %g" % (name, rt)
    # ---- ELBO and every gradient
    elbo, ell, kld, mu, v = elbo_of(model, X, Y)
    elbo.backward()
    out = base_out(prob)
    if kernel != "scale_rbf":
        out["kernel"] = np.array(kernel)
    out.update({"ELBO": elbo.detach(), "ELL": ell.detach(), "KLD": kld.detach(), "mu": mu.detach().reshape(-1),
                "v": v.detach().reshape(-1), "t": t.reshape(-1), "min_dT": dT.min(),
                "logdet": torch.log(dT).sum(),
                "g_Z": model.Z.grad[0], "g_m": model.q_U.variational_mean.grad[0],
                "g_Lam": model.q_U.chol_variational_covar.grad[0],
                "g_raw_outputscale": model.covariance_function.raw_outputscale.grad,
                "g_raw_lengthscale": model.covariance_function.base_kernel.raw_lengthscale.grad.reshape(-1),
                "g_log_var_noise": lik.log_var_noise.grad.reshape(-1)})
    if prm:
        out["g_theta"] = torch.stack([q.grad.reshape(()) for q in prm])
    # ---- the likelihood alone: gradients with respect to the moments (scale 1), theta and the noise
    mu_l = mu.detach().clone().requires_grad_(True)
    v_l = v.detach().clone().requires_grad_(True)
    for q in list(prm) + [lik.log_var_noise]:
        q.grad = None
    ell1 = lik.expected_log_prob(Y.t(), mu_l, v_l).sum()
    ell1.backward()
    out.update({"lik_ELL": ell1.detach(), "g_mu": mu_l.grad.reshape(-1), "g_v": v_l.grad.reshape(-1),
                "lik_g_log_var_noise": lik.log_var_noise.grad.reshape(-1)})
    if prm:
        out["lik_g_theta"] = torch.stack([q.grad.reshape(()) for q in prm])
    # ---- names (the class surface test compares named_parameters())
    # (a file of its own: the suite's fixture loader turns every array into a tensor, and strings are none)
    if name == "warp_tiny_sal2":
        gg.save("warp_param_names", {"lik_param_names": np.array([n for n, _ in lik.named_parameters()]),
                                     "model_param_names": np.array([n for n, _ in model.named_parameters()])})
    # ---- prediction on a held-out block of rows, and the inverse on a grid
    if closed:
        with torch.no_grad():
            Xte = prob["Xte"]
            pm, pv = model.marginal_variational_qf_parameters(Xte.repeat(1, 1, 1), diagonal=True, is_duvenaud=False, init_Z=None)
            pm, pv = pm.squeeze(dim=2), pv.squeeze(dim=2)
            m1, m2 = lik.marginal_moments(pm, pv, diagonal=True)
            lo, hi = float(t.min()), float(t.max())
            grid = torch.linspace(lo - 0.25 * (hi - lo), hi + 0.25 * (hi - lo), 97, dtype=torch.float64).reshape(1, -1)
            out.update({"Xte": Xte, "pred_mu": pm.reshape(-1), "pred_v": pv.reshape(-1), "pred_m1": m1.reshape(-1),
                        "pred_m2": m2.reshape(-1), "inv_grid": grid.reshape(-1), "inv_x": fl.inverse(grid).reshape(-1)})
            assert bool(torch.isfinite(out["inv_x"]).all()) and bool(torch.isfinite(m1).all()), name
    gg.save(name, out)


def adam_steps(prob, flow, name, steps=5):
    model, prm = build(prob, flow)
    model.set_is_training(True)
    opt = torch.optim.Adam(model.parameters(), lr=0.01)
    hist = []
    for _ in range(steps):
        elbo, ell, kld, _, _ = elbo_of(model, prob["X"], prob["Y"])
        opt.zero_grad()
        (-elbo).backward()
        opt.step()
        hist.append([elbo.item(), ell.item(), kld.item()])
    out = base_out(prob)
    out["history"] = np.array(hist)
    if prm:
        out["final_theta"] = torch.stack([q.detach().reshape(()) for q in prm])
    out["final_Z"] = model.Z.detach()[0]
    out["final_m"] = model.q_U.variational_mean.detach()[0]
    out["final_log_var_noise"] = model.likelihood.log_var_noise.detach().reshape(-1)
    gg.save(name, out)


def main():
    step0(problem(64, 3, 8, 16), "sal2", "warp_tiny_sal2")
    step0(problem(64, 3, 8, 16), None, "warp_tiny_empty")
    step0(problem(64, 3, 8, 16, away_from_zero=True), "bcl_al1", "warp_tiny_bcl_al1")
    step0(problem(400, 4, 40, 32), "sal2", "warp_med_sal2")
    step0(problem(400, 4, 40, 32), "arcsl2", "warp_med_arcsl2")
    step0(problem(200, 4, 20, 32), "sal_al1", "warp_med_sal_al1")
    step0(problem(200, 4, 20, 32), "tanh3x2", "warp_med_tanh3x2")
    step0(problem(200, 4, 20, 32), "sal2", "warp_med_matern_sal2", kernel="scale_matern32")
    step0(problem(400, 6, 200, 16, band=12), "sal2", "warp_bigm_sal2")
    adam_steps(problem(64, 3, 8, 16), "sal2", "warp_adam5_sal2")
    adam_steps(problem(64, 3, 8, 16), "arcsl2", "warp_adam5_arcsl2")


if __name__ == "__main__":
    main()
