"""Generate the fixtures of the unwhitened q(u) parameterisation (tests/golden/unwh_*.npz) by executing the reference's own
files with is_whiten = False (build container only; never runs on the GPU box).

Run:  python tools/gen_golden_unwhitened.py

The reference on sys.path with the oracle/shims stand-ins, build_reference_model and the parameter recipe come from
oracle/gen_golden.py, imported read-only.  Each case builds the reference model, sets `model.is_whiten = False` and calls its
marginal_variational_qf_parameters (sparse_MF_SP.py:357-360, :386-389), KLD (:433-453) and ELBO with autograd.  KLD's
unwhitened branch calls `self.q_U()`; the stand-in CholeskyVariationalDistribution of oracle/shims is a parameter holder with
no forward.  This file gives it one AT RUN TIME, here and nowhere else (oracle/ stays as it is): the
torch.distributions.MultivariateNormal(mean, covariance_matrix = tril(C) tril(C)^T) that gpytorch's class returns.

q(u) is N(m, L_q L_q^T) with orc.synthetic_problem's perturbed m and dense L_q (its upper triangle must be ignored) + 0.5 I.  The
generator asserts that the reference's K_ZZ factorises at jitter 0 (the fixtures pin the no-ladder path) and compares
tests/unwhiten_model.py with the reference case by case, printing the worst differences: those figures are the base of the
GPU tests' tolerances where a case is too ill-conditioned for the project's 1e-9 / 1e-7.
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
from gpytorch import variational as shim_var   # noqa: E402  (the stand-in of oracle/shims)

from oracle import tgp_oracle as orc        # noqa: E402
from conftest import load_golden, rel_err   # noqa: E402
import unwhiten_model as um                 # noqa: E402


def _q_u(self):
    C = torch.tril(self.chol_variational_covar)
    return torch.distributions.MultivariateNormal(self.variational_mean, covariance_matrix=C @ C.transpose(-1, -2))


shim_var.CholeskyVariationalDistribution.forward = _q_u
BUILD_REF = gg.build_reference_model      # (tools/gen_golden_flows.py, imported with the Bernoulli tool, rebinds the name)

#        fixture             N    D   M    flow       kernel            likelihood
CASES = (("unwh_tiny_svgp", 37, 4, 5, None, "scale_rbf", "gauss"),
         ("unwh_med_sal2", 130, 4, 100, "sal2", "scale_rbf", "gauss"),
         ("unwh_edge128", 130, 4, 128, None, "scale_rbf", "gauss"),
         ("unwh_bigm_matern", 150, 13, 150, "tanh3x2", "scale_matern32", "gauss"),
         ("unwh_bern_tiny", 60, 4, 20, "sal1", "scale_rbf", "bernoulli"))


BERN_SCALE = 0.1


def shift(prob, scale=1.0):
    """+ 0.5 I on q(u)'s factor: the recipe's diagonal, sqrt(1e-5) + 0.05 N(0, 1), leaves L_q L_q^T numerically singular at
    M >= 100, and the reference's KLD hands that matrix to torch.distributions.MultivariateNormal, which factorises it.
    `scale` shrinks q(u) (m and the factor): the Bernoulli case needs max |G(f0)| <= 6 over the quadrature nodes, as every
    fixture of tools/gen_golden_bernoulli.py does (asserted below with its node_check) -- beyond that the reference's
    log(1 - Phi) loses digits and is no reference any more -- and L^-1 multiplies q(u)'s spread by up to 1 / sqrt(lambda_min(K_ZZ))."""
    M = prob["params"]["m"].numel()
    prob["params"]["Lam"] = scale * (prob["params"]["Lam"] + 0.5 * torch.eye(M, dtype=torch.float64))
    prob["params"]["m"] = scale * prob["params"]["m"]
    return prob


def problem(N, D, M, flow, lik):
    return shift(_problem(N, D, M, flow, lik), BERN_SCALE if lik == "bernoulli" else 1.0)


def _problem(N, D, M, flow, lik):
    if lik == "bernoulli":
        import gen_golden_bernoulli as gb
        prob = gb.problem(N, D, M, 8, seed=3)
        full = orc.synthetic_problem(N, D, M, seed=3, flow=flow, S=8)
        prob["program"], prob["params"]["theta"] = full["program"], full["params"]["theta"]
        return prob
    return orc.synthetic_problem(N, D, M, seed=3, flow=flow, S=8)


def build(prob, flow, kernel, lik):
    """The reference's model with prob's values and is_whiten = False."""
    if lik == "bernoulli":
        import gen_golden_bernoulli as gb
        X, p = prob["X"], prob["params"]
        N, D = X.shape
        M = p["Z"].shape[0]
        K = gg.instance_kernel(kernel, ard_num_dim=D, num_multioutput=1, kernel_is_shared=False, init_params=gg.KINIT)
        model = gg.sparse_MF_SP(["zero", K], X, p["Z"].clone(), N, gb.bern_lik(prob["xs"].shape[0]), 1, True, False, False, False,
                                False, [gg.SAL(int(flow[3:]))], "single", 0.0, init_params=gg.IP)
        with torch.no_grad():
            model.Z.data = p["Z"].reshape(1, M, D).clone()
            model.q_U.variational_mean.data = p["m"].reshape(1, M).clone()
            model.q_U.chol_variational_covar.data = p["Lam"].reshape(1, M, M).clone()
            model.covariance_function.raw_outputscale.data = p["raw_outputscale"].reshape(1).clone()
            model.covariance_function.base_kernel.raw_lengthscale.data = p["raw_lengthscale"].reshape(1, 1, D).clone()
            gg.load_theta(model, prob["program"], p["theta"])
    else:
        model = BUILD_REF(prob, flow, kernel)
    model.is_whiten = False
    model.set_is_training(True)
    return model


def assert_no_ladder(prob, kernel):
    """the reference's own K_ZZ (its kernel's centred expansion) factorises at jitter 0"""
    p = prob["params"]
    K = orc.KERNELS[kernel](p["Z"], p["Z"], p["raw_lengthscale"], p["raw_outputscale"])
    _, info = torch.linalg.cholesky_ex(K)
    assert int(info) == 0, "K_ZZ needs jitter: choose other parameters"
    ev = torch.linalg.eigvalsh(K)
    return float(ev[-1] / ev[0])


def ref_grads(model, prob, lik):
    k = model.covariance_function
    out = {"g_Z": model.Z.grad[0], "g_m": model.q_U.variational_mean.grad[0], "g_Lam": model.q_U.chol_variational_covar.grad[0],
           "g_raw_outputscale": k.raw_outputscale.grad, "g_raw_lengthscale": k.base_kernel.raw_lengthscale.grad.reshape(-1)}
    if lik != "bernoulli":
        out["g_log_var_noise"] = model.likelihood.log_var_noise.grad.reshape(-1)
    if prob["program"] is not None:
        out["g_theta"] = torch.stack([q.grad.reshape(()) for q in gg.flow_scalar_params(model, prob["program"])])
    return out


def one(name, N, D, M, flow, kernel, lik):
    prob = problem(N, D, M, flow, lik)
    cond = assert_no_ladder(prob, kernel)
    model = build(prob, flow, kernel, lik)
    X, Y, p = prob["X"], prob["Y"], prob["params"]
    elbo, ell, kld = model.ELBO(X, Y)
    elbo.backward()
    out = {"X": X, "Y": Y, "xs": prob["xs"], "ws": prob["ws"], "N_total": np.float64(prob["N_total"]), "ELBO": elbo.detach(),
           "ELL": ell.detach(), "KLD": kld.detach().reshape(-1), "kernel": np.array(kernel), "bernoulli": np.int32(lik == "bernoulli")}
    out.update(ref_grads(model, prob, lik))
    for k, v in p.items():
        if not (lik == "bernoulli" and k == "log_var_noise"):
            out["p_" + k] = v
    if prob["program"] is not None:
        out["program"] = np.array(prob["program"], dtype=np.int32)
    with torch.no_grad():
        mu, v = model.marginal_variational_qf_parameters(X, diagonal=True, is_duvenaud=False, init_Z=None)
        out["mu"], out["v"] = mu.reshape(-1), v.reshape(-1)
        assert float((model.KLD().reshape(-1) - out["KLD"]).abs().max()) == 0.0
        if lik == "bernoulli":
            import gen_golden_bernoulli as gb
            out["gmax"] = np.float64(gb.node_check(model, out["mu"], out["v"], X.reshape(1, *X.shape), prob["xs"], prob["ws"]))
    gg.save(name, out)
    # tests/unwhiten_model.py against what was just stored
    g = load_golden(name) if gg.OUT == gg.GOLDEN else None
    if g is None:
        return
    mu_c, v_c = um.qf_moments(g["X"], p["Z"], p["raw_lengthscale"], p["raw_outputscale"], p["m"], p["Lam"], kernel=kernel)
    kl_c = um.kld(p["Z"], p["raw_lengthscale"], p["raw_outputscale"], p["m"], p["Lam"], kernel=kernel)
    line = "%s: cond(K_ZZ) %.2e  max|v| %.3g  KLD %.6g | CPU model vs reference: mu %.2e  v %.2e  KLD %.2e" % (
        name, cond, float(g["v"].abs().max()), float(g["KLD"]), rel_err(mu_c, g["mu"]), rel_err(v_c, g["v"]),
        rel_err(kl_c, g["KLD"]))
    if lik == "gauss":
        (e_c, l_c, k_c), gr = um.elbo_and_grads(g)
        worst = max(rel_err(gr[kk], g[gk]) for kk, gk in (("Z", "g_Z"), ("m", "g_m"), ("Lam", "g_Lam"),
                                                            ("raw_outputscale", "g_raw_outputscale"),
                                                            ("raw_lengthscale", "g_raw_lengthscale"),
                                                            ("log_var_noise", "g_log_var_noise")))
        line += "  ELBO %.2e  ELL %.2e  worst gradient %.2e" % (rel_err(e_c, g["ELBO"]), rel_err(l_c, g["ELL"]), worst)
    print(line)


def adam5(name, N, D, M, flow):
    """First 5 steps of Trainer_base.train's inner loop on the unwhitened model, as the adam5_* fixtures."""
    prob = problem(N, D, M, flow, "gauss")
    assert_no_ladder(prob, "scale_rbf")
    model = build(prob, flow, "scale_rbf", "gauss")
    opt = torch.optim.Adam(model.parameters(), lr=0.01)
    hist = []
    for _ in range(5):
        elbo, ell, kld = model.ELBO(prob["X"], prob["Y"])
        opt.zero_grad()
        (-elbo).backward()
        opt.step()
        hist.append([elbo.item(), ell.item(), kld.item()])
    out = {"X": prob["X"], "Y": prob["Y"], "xs": prob["xs"], "ws": prob["ws"], "N_total": np.float64(prob["N_total"]),
           "history": np.array(hist), "program": np.array(prob["program"], dtype=np.int32)}
    for k, v in prob["params"].items():
        out["p_" + k] = v
    out["final_theta"] = torch.stack([q.detach().reshape(()) for q in gg.flow_scalar_params(model, prob["program"])])
    out["final_Z"] = model.Z.detach()[0]
    out["final_m"] = model.q_U.variational_mean.detach()[0]
    out["final_Lam"] = model.q_U.chol_variational_covar.detach()[0]
    gg.save(name, out)


def main():
    for case in CASES:
        one(*case)
    adam5("unwh_adam5_sal2", 130, 4, 100, "sal2")


if __name__ == "__main__":
    main()
