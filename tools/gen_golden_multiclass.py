"""Generate the fixtures of the multi-class likelihood (tests/golden/mc_*.npz) by executing the reference's own files
(build container only; never runs on the GPU box).

Run:  python tools/gen_golden_multiclass.py

The reference on sys.path with the oracle/shims stand-ins comes from oracle/gen_golden.py, imported read-only; the flow
generators, their program rows and the raw-value perturbation from tools/gen_golden_warped.py.  The reference's
sparse_MF_SP / sparse_MF_GP run BATCHED at num_outputs = C with its MulticlassCategorical (the shim kernels take
batch_shape = [C]); nothing is composed from single-output models.

The reference draws its standard normals inside td.Normal.rsample / .sample.  Each call is made right after
torch.manual_seed(k), and the draws are recorded by re-seeding with k and drawing torch.randn of the same (S, C, MB) shape;
the generator asserts that mu + sqrt(v) eps pushed through the reference's flows and CrossEntropyLoss (softmax for the
prediction) reproduces the reference's own return value to 1e-12, and that v > 0 on every row.

Keys: X, Y (class indices as float64), N_total, S, p_* (Z (C,M,D), raw_lengthscale (C,D), raw_outputscale (C), m (C,M),
Lam (C,M,M), theta), program (all classes' rows, poff relative to the class), blk_off, theta_off, eps (S,C,N), ELBO, ELL,
KLD (C), mu, v (C,N), g_* of the ELBO, lik_ELL / g_mu / g_v / lik_g_theta of the likelihood alone (scale 1), Xte, Yte, eps_te,
pred_mu, pred_v, pred_P (Nte,C), pred_logp = sum_n log P[n, y_n], adam_eps (5,S,C,N), history (5,3), final_*.
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

import gen_golden_warped as gw              # noqa: E402
from dsp.likelihoods.MulticlassCategorical import MulticlassCategorical   # noqa: E402
from dsp.models.flow import instance_flow                                  # noqa: E402

from oracle import tgp_oracle as orc        # noqa: E402


def problem(C, N, D, M, seed, band=None, nte=40):
    g = torch.Generator().manual_seed(9000 + seed)
    X = torch.randn(N + nte, D, generator=g, dtype=torch.float64)
    W = torch.randn(D, C, generator=g, dtype=torch.float64)
    logits = 1.5 * (X @ W) + 0.5 * torch.randn(N + nte, C, generator=g, dtype=torch.float64)
    Y = logits.argmax(1).to(torch.float64).reshape(-1, 1)
    p = {"Z": [], "raw_lengthscale": [], "raw_outputscale": [], "m": [], "Lam": []}
    for c in range(C):
        q = orc.synthetic_problem(N, D, M, seed=100 * seed + c, flow=None, S=4)["params"]
        perm = torch.randperm(N, generator=g)
        p["Z"].append(X[perm[:M]].clone())
        p["raw_lengthscale"].append(q["raw_lengthscale"])
        p["raw_outputscale"].append(q["raw_outputscale"].reshape(()) + 0.1 * c)
        p["m"].append(q["m"])
        p["Lam"].append(torch.tril(torch.triu(q["Lam"], -band)) if band is not None else q["Lam"])
    p = {k: torch.stack(v) for k, v in p.items()}
    return {"X": X[:N], "Y": Y[:N], "Xte": X[N:], "Yte": Y[N:], "params": p, "N_total": float(N)}


def build(prob, flows, S):
    """(reference model at num_outputs = C, [per class: the flow's parameters in theta order], program rows, offsets)."""
    X, p = prob["X"], prob["params"]
    N, D = X.shape
    C, M = p["Z"].shape[0], p["Z"].shape[1]
    comps, prms, prog, blk_off, theta_off, theta = [], [], [], [0], [0], []
    for c, fl in enumerate(flows):
        comp, pr, th = gw.make_flow(fl, seed=10 + c)
        if comp is None:
            comp = instance_flow([("identity", [])])
            prm = []
        else:
            prm = gw.program_of(comp)[1]
        comps.append(comp)
        prms.append(prm)
        prog += [tuple(r) for r in pr]
        blk_off.append(len(prog))
        theta_off.append(theta_off[-1] + len(prm))
        theta.append(th)
    K = gg.instance_kernel("scale_rbf", ard_num_dim=D, num_multioutput=C, kernel_is_shared=False, init_params=gg.KINIT)
    lik = MulticlassCategorical(C)
    lik.SMC = S
    if all(f is None for f in flows):
        model = gg.sparse_MF_GP(["zero", K], X, p["Z"][0].clone(), N, lik, C, True, False, False, False, False, 0.0,
                                init_params=gg.IP)
    else:
        model = gg.sparse_MF_SP(["zero", K], X, p["Z"][0].clone(), N, lik, C, True, False, False, False, False, comps, "single",
                                0.0, init_params=gg.IP)
    with torch.no_grad():
        model.Z.data = p["Z"].clone()
        model.q_U.variational_mean.data = p["m"].clone()
        model.q_U.chol_variational_covar.data = p["Lam"].clone()
        model.covariance_function.raw_outputscale.data = p["raw_outputscale"].reshape(C).clone()
        model.covariance_function.base_kernel.raw_lengthscale.data = p["raw_lengthscale"].reshape(C, 1, D).clone()
    prob["program"], prob["blk_off"], prob["theta_off"] = prog, blk_off, theta_off
    p["theta"] = torch.cat(theta) if theta_off[-1] else torch.zeros(0, dtype=torch.float64)
    return model, prms


def restate(model, Y, mu, v, eps):
    """-CrossEntropyLoss of mu + sqrt(v) eps through the reference's flows: (ELL at scale 1, FK (S,C,MB))."""
    S, C, MB = eps.shape
    F0 = mu.unsqueeze(0) + v.sqrt().unsqueeze(0) * eps
    FK = torch.stack([model.G_matrix[c](F0[:, c, :], None) for c in range(C)], 1)
    nll = torch.nn.CrossEntropyLoss(reduction="none")(FK.transpose(2, 1).reshape(S * MB, C), Y.reshape(-1).long().repeat(S))
    return -nll.view(S, MB).mean(0).sum(), FK


def elbo_seeded(model, X, Y, seed):
    """The reference's ELBO right after torch.manual_seed(seed), and the draws it used."""
    C, S, MB = model.out_dim, model.likelihood.SMC, X.shape[0]
    torch.manual_seed(seed)
    eps = torch.randn(S, C, MB, dtype=torch.float64)
    torch.manual_seed(seed)
    elbo, ell, kld = model.ELBO(X, Y.long())
    with torch.no_grad():
        mu, v = model.marginal_variational_qf_parameters(X.repeat(C, 1, 1), diagonal=True, is_duvenaud=False, init_Z=None)
        mu, v = mu.squeeze(2), v.squeeze(2)
        assert float(v.min()) > 0.0, "v must stay positive: %g" % float(v.min())
        mine = model.N / MB * restate(model, Y, mu, v, eps)[0]
    assert abs(float(mine) - float(ell)) <= 1e-12 * max(1.0, abs(float(ell))), (float(mine), float(ell))
    return elbo, ell, kld, eps, mu, v


def flat_grads(prms):
    th = [q.grad.reshape(()) for prm in prms for q in prm]
    return torch.stack(th) if th else torch.zeros(0, dtype=torch.float64)


def fixture(name, C, N, D, M, S, flows, seed, band=None):
    prob = problem(C, N, D, M, seed, band)
    model, prms = build(prob, flows, S)
    model.set_is_training(True)
    X, Y, p = prob["X"], prob["Y"], prob["params"]
    out = {"X": X, "Y": Y, "N_total": np.float64(prob["N_total"]), "S": np.int32(S),
           "program": np.array(prob["program"] if prob["program"] else np.zeros((0, 4)), dtype=np.int32),
           "blk_off": np.array(prob["blk_off"], dtype=np.int32), "theta_off": np.array(prob["theta_off"], dtype=np.int32)}
    for k, val in p.items():
        out["p_" + k] = val
    # ---- ELBO and every gradient
    elbo, ell, kld, eps, mu, v = elbo_seeded(model, X, Y, 4000 + seed)
    kl_c = model.KLD().detach().reshape(-1)
    assert abs(float(kl_c.sum()) - float(kld)) <= 1e-12 * max(1.0, abs(float(kld)))
    elbo.backward()
    k = model.covariance_function
    out.update({"eps": eps, "ELBO": elbo.detach(), "ELL": ell.detach(), "KLD": kl_c, "mu": mu, "v": v,
                "g_Z": model.Z.grad, "g_m": model.q_U.variational_mean.grad, "g_Lam": model.q_U.chol_variational_covar.grad,
                "g_raw_outputscale": k.raw_outputscale.grad.reshape(-1),
                "g_raw_lengthscale": k.base_kernel.raw_lengthscale.grad.reshape(C, D), "g_theta": flat_grads(prms)})
    # ---- the likelihood alone at scale 1: gradients with respect to the moments and theta
    for prm in prms:
        for q in prm:
            q.grad = None
    mu_l, v_l = mu.clone().requires_grad_(True), v.clone().requires_grad_(True)
    torch.manual_seed(4000 + seed)
    ell1 = model.likelihood.expected_log_prob(Y.long().t(), mu_l, v_l, flow=model.G_matrix, X=X.repeat(C, 1, 1))
    ell1.backward()
    out.update({"lik_ELL": ell1.detach(), "g_mu": mu_l.grad, "g_v": v_l.grad, "lik_g_theta": flat_grads(prms)})
    # ---- prediction on held-out rows with draws of its own
    Xte, Yte = prob["Xte"], prob["Yte"]
    nte = Xte.shape[0]
    with torch.no_grad():
        pm, pv = model.marginal_variational_qf_parameters(Xte.repeat(C, 1, 1), diagonal=True, is_duvenaud=False, init_Z=None)
        pm, pv = pm.squeeze(2), pv.squeeze(2)
        assert float(pv.min()) > 0.0
        torch.manual_seed(5000 + seed)
        eps_te = torch.randn(S, C, nte, dtype=torch.float64)
        torch.manual_seed(5000 + seed)
        P = model.likelihood.marginal_moments(pm, pv, flow=model.G_matrix, X=Xte.repeat(C, 1, 1))
        mineP = torch.softmax(restate(model, Yte, pm, pv, eps_te)[1].transpose(2, 1), dim=2).mean(0)
        assert float((mineP - P).abs().max()) <= 1e-12, float((mineP - P).abs().max())
        logp = torch.log(P.gather(1, Yte.long())).sum()
    out.update({"Xte": Xte, "Yte": Yte, "eps_te": eps_te, "pred_mu": pm, "pred_v": pv, "pred_P": P, "pred_logp": logp})
    # ---- five Adam steps, the draws of each recorded
    model, prms = build(prob, flows, S)
    model.set_is_training(True)
    opt = torch.optim.Adam(model.parameters(), lr=0.01)
    hist, adam_eps = [], []
    for it in range(5):
        elbo, ell, kld, e, _, _ = elbo_seeded(model, X, Y, 6000 + 10 * seed + it)
        opt.zero_grad()
        (-elbo).backward()
        opt.step()
        hist.append([elbo.item(), ell.item(), kld.item()])
        adam_eps.append(e)
    th = [q.detach().reshape(()) for prm in prms for q in prm]
    out.update({"history": np.array(hist), "adam_eps": torch.stack(adam_eps), "final_Z": model.Z.detach(),
                "final_m": model.q_U.variational_mean.detach(),
                "final_theta": torch.stack(th) if th else torch.zeros(0, dtype=torch.float64)})
    gg.save(name, out)


def main():
    fixture("mc_id3", 3, 200, 3, 20, 16, [None] * 3, seed=1)
    fixture("mc_sal2x4", 4, 120, 4, 20, 16, ["sal2"] * 4, seed=2)
    fixture("mc_mixed5", 5, 120, 4, 24, 8, ["tanh3x2", "arcsl2", "bcl_al1", "sal2", "sal_al1"], seed=3)
    fixture("mc_bigm3", 3, 200, 4, 160, 8, ["sal2", None, "sal_al1"], seed=4, band=12)


if __name__ == "__main__":
    main()
