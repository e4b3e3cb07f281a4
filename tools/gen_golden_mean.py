"""Generate the fixtures of the linear and identity mean functions (tests/golden/mean_*.npz) by executing the reference's own
files (build container only; never runs on the GPU box).

Run:  python tools/gen_golden_mean.py

The reference on sys.path with the oracle/shims stand-ins comes from oracle/gen_golden.py, the model recipes (parameters, + 0.5 I
on q(u)'s factor, the Bernoulli scaling) from tools/gen_golden_unwhitened.py, both imported read-only.  Each case builds the
reference model with the zero mean and swaps in the reference's own return_mean(name, D, 1, W) -- W from its
return_projection_matrix on the training inputs.  The reference's Linear reads `cg.seed`, which its config.py does not define:
this file sets cg.seed = cg.config_seed AT RUN TIME, here and nowhere else.  The drawn a is scaled by 0.3 (with the Bernoulli
case's milder flow, see problem(), it keeps max |G(f0)| <= 6, asserted with gen_golden_bernoulli.node_check as every Bernoulli fixture does) and b is set to 0.25.

Stored per case: inputs, parameters, a and b (or W), ELBO / ELL / KLD, every gradient, mu and v, and for the regression cases
predictive_distribution's m1, m2 and test_log_likelihood on 16 held-out rows.  The generator prints tests/mean_model.py against
the reference case by case: those figures are the MEAN_CPU table of tests/test_mean_host.py.
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, HERE)

from oracle import gen_golden as gg        # noqa: E402  (sets up the reference, the shims and float64)

import numpy as np                          # noqa: E402
import torch                                # noqa: E402

import gen_golden_unwhitened as gu          # noqa: E402  (gives the stand-in q(u) holder its forward, at run time)
from dsp.models.utils_models import return_mean, return_projection_matrix   # noqa: E402
from conftest import load_golden, rel_err   # noqa: E402
import mean_model as mm                     # noqa: E402
from oracle import tgp_oracle as orc        # noqa: E402

gg.cg.seed = gg.cg.config_seed              # models/means.py Linear reads cg.seed; config.py defines config_seed only

#        fixture                 N    D   M    flow       kernel            likelihood   mean        whiten
CASES = (("mean_tiny_svgp_lin", 37, 4, 5, None, "scale_rbf", "gauss", "linear", True),
         ("mean_tiny_sal1_lin", 37, 4, 5, "sal1", "scale_rbf", "gauss", "linear", True),
         ("mean_med_sal2_lin", 130, 4, 100, "sal2", "scale_rbf", "gauss", "linear", True),
         ("mean_edge128_tanh_id", 130, 13, 128, "tanh3x2", "scale_rbf", "gauss", "identity", True),
         ("mean_bigm_matern_lin", 150, 13, 150, "tanh3x2", "scale_matern32", "gauss", "linear", True),
         ("mean_bern_tiny_lin", 60, 4, 20, "sal1", "scale_rbf", "bernoulli", "linear", True),
         ("mean_unwh_sal2_lin", 130, 4, 100, "sal2", "scale_rbf", "gauss", "linear", False))
A_SCALE, B_INIT, N_TEST, Y_STD = 0.3, 0.25, 16, 1.7
BERN_FLOW_SCALE = 0.25     # the Bernoulli case's SAL x 1 flow: identity initialisation + 0.25 x the recipe's perturbation


def problem(N, D, M, flow, lik):
    """tools/gen_golden_unwhitened.py's recipe.  The Bernoulli case shrinks the flow's perturbation as well: whitened, the recipe's
    SAL block alone takes max |G(f0)| to 6.9 over the quadrature nodes, and the mean adds up to 2.5 to f0 in front of it."""
    prob = gu.problem(N, D, M, flow, lik)
    if lik == "bernoulli":
        ident = orc.sal_program(int(flow[3:]))[1]
        prob["params"]["theta"] = ident + BERN_FLOW_SCALE * (prob["params"]["theta"] - ident)
    return prob


def build(prob, flow, kernel, lik, mean, whiten):
    """The reference's model at prob's values with the reference's own mean function swapped in."""
    model = gu.build(prob, flow, kernel, lik)
    model.is_whiten = bool(whiten)
    D = prob["X"].shape[1]
    W = return_projection_matrix(D, 1, prob["X"]) if mean == "identity" else None
    model.mean_function = return_mean(mean, D, 1, W)
    if mean == "linear":
        with torch.no_grad():
            model.mean_function.a.mul_(A_SCALE)
            model.mean_function.b.fill_(B_INIT)
    return model


def held_out(prob):
    g = torch.Generator().manual_seed(77)
    D = prob["X"].shape[1]
    return torch.randn(N_TEST, D, generator=g, dtype=torch.float64), torch.randn(N_TEST, 1, generator=g, dtype=torch.float64)


def mean_arrays(model, mean, grads):
    mf = model.mean_function
    if mean == "identity":
        return {"mean_W": mf.W.detach().reshape(-1)}
    out = {"mean_a": mf.a.detach().reshape(-1).clone(), "mean_b": mf.b.detach().reshape(-1).clone()}
    if grads:
        out["g_mean_a"], out["g_mean_b"] = mf.a.grad.reshape(-1), mf.b.grad.reshape(-1)
    return out


def one(name, N, D, M, flow, kernel, lik, mean, whiten):
    prob = problem(N, D, M, flow, lik)
    cond = gu.assert_no_ladder(prob, kernel)
    model = build(prob, flow, kernel, lik, mean, whiten)
    X, Y, p = prob["X"], prob["Y"], prob["params"]
    elbo, ell, kld = model.ELBO(X, Y)
    elbo.backward()
    out = {"X": X, "Y": Y, "xs": prob["xs"], "ws": prob["ws"], "N_total": np.float64(prob["N_total"]), "ELBO": elbo.detach(),
           "ELL": ell.detach(), "KLD": kld.detach().reshape(-1), "kernel": np.array(kernel), "bernoulli": np.int32(lik == "bernoulli"),
           "whiten": np.int32(whiten)}
    out.update(gu.ref_grads(model, prob, lik))
    out.update(mean_arrays(model, mean, True))
    for k, v in p.items():
        if not (lik == "bernoulli" and k == "log_var_noise"):
            out["p_" + k] = v
    if prob["program"] is not None:
        out["program"] = np.array(prob["program"], dtype=np.int32)
    with torch.no_grad():
        mu, v = model.marginal_variational_qf_parameters(X, diagonal=True, is_duvenaud=False, init_Z=None)
        out["mu"], out["v"] = mu.reshape(-1), v.reshape(-1)
        if lik == "bernoulli":
            import gen_golden_bernoulli as gb
            out["gmax"] = np.float64(gb.node_check(model, out["mu"], out["v"], X.reshape(1, *X.shape), prob["xs"], prob["ws"]))
        else:
            X_te, Y_te = held_out(prob)
            model.set_is_training(False)
            Y_std = torch.tensor([Y_STD])
            logp, (m1, m2) = model.test_log_likelihood(X_te, Y_te, return_moments=True, Y_std=Y_std, S_MC_NNet=None)
            mu_t, v_t = model.marginal_variational_qf_parameters(X_te, diagonal=True, is_duvenaud=False, init_Z=None)
            out.update(X_te=X_te, Y_te=Y_te, Y_std=Y_std.to(torch.float64), test_logp_sum=logp.reshape(-1), pred_m1=m1.reshape(-1),
                       pred_m2=m2.reshape(-1), mu_te=mu_t.reshape(-1), v_te=v_t.reshape(-1))
    gg.save(name, out)
    if gg.OUT != gg.GOLDEN:
        return
    # tests/mean_model.py against what was just stored
    g = load_golden(name)
    a, b = mm.mean_params(g)
    mu_c, v_c = mm.qf_moments(g, g["X"], g["params"], a, b)
    (e_c, l_c, k_c), gr = mm.elbo_and_grads(g)
    keys = [("Z", "g_Z"), ("m", "g_m"), ("Lam", "g_Lam"), ("raw_outputscale", "g_raw_outputscale"),
            ("raw_lengthscale", "g_raw_lengthscale"), ("log_var_noise", "g_log_var_noise"), ("theta", "g_theta"),
            ("mean_a", "g_mean_a"), ("mean_b", "g_mean_b")]
    worst = max(rel_err(gr[kk], g[gk]) for kk, gk in keys if gk in g and kk in gr)
    vals = max(rel_err(mu_c, g["mu"]), rel_err(v_c, g["v"]), rel_err(e_c, g["ELBO"]), rel_err(l_c, g["ELL"]), rel_err(k_c, g["KLD"]))
    print("%s: cond(K_ZZ) %.2e  ELBO %.6f | CPU model vs reference: worst value %.2e  worst gradient %.2e" % (
        name, cond, float(g["ELBO"]), vals, worst))


def adam5(name, N, D, M, flow):
    """First 5 steps of Trainer_base.train's inner loop with a linear mean, as the adam5_* fixtures."""
    prob = problem(N, D, M, flow, "gauss")
    gu.assert_no_ladder(prob, "scale_rbf")
    model = build(prob, flow, "scale_rbf", "gauss", "linear", True)
    out = mean_arrays(model, "linear", False)
    opt = torch.optim.Adam(model.parameters(), lr=0.01)
    hist = []
    for _ in range(5):
        elbo, ell, kld = model.ELBO(prob["X"], prob["Y"])
        opt.zero_grad()
        (-elbo).backward()
        opt.step()
        hist.append([elbo.item(), ell.item(), kld.item()])
    out.update({"X": prob["X"], "Y": prob["Y"], "xs": prob["xs"], "ws": prob["ws"], "N_total": np.float64(prob["N_total"]),
                "history": np.array(hist), "program": np.array(prob["program"], dtype=np.int32), "whiten": np.int32(1),
                "bernoulli": np.int32(0)})
    for k, v in prob["params"].items():
        out["p_" + k] = v
    k = model.covariance_function
    out["final_theta"] = torch.stack([q.detach().reshape(()) for q in gg.flow_scalar_params(model, prob["program"])])
    out["final_Z"] = model.Z.detach()[0]
    out["final_m"] = model.q_U.variational_mean.detach()[0]
    out["final_Lam"] = model.q_U.chol_variational_covar.detach()[0]
    out["final_mean_a"] = model.mean_function.a.detach().reshape(-1)
    out["final_mean_b"] = model.mean_function.b.detach().reshape(-1)
    out["final_raw_lengthscale"] = k.base_kernel.raw_lengthscale.detach().reshape(-1)
    out["final_raw_outputscale"] = k.raw_outputscale.detach().reshape(-1)
    out["final_log_var_noise"] = model.likelihood.log_var_noise.detach().reshape(-1)
    gg.save(name, out)


def main():
    for case in CASES:
        one(*case)
    adam5("mean_adam5_sal2_lin", 130, 4, 100, "sal2")


if __name__ == "__main__":
    main()
