"""Torch restatement of the models with a linear / identity mean function (csrc/tgp_mean.hip and the host logic on top of it)
for the tests, float64 on the CPU, differentiable by autograd.  m(x) = x a + b (identity mean: a = W, b = 0, neither trainable).

  flow likelihoods   the oracle's ELBO with a per-row affine block (a_n, b_n) = (1, m(x_n)) at the head of the program:
                     G(f) becomes G(f + m(x_n)), which is the reference's mu_qf = ... + m(X) (sparse_MF_SP.py:314,355,360)
  Gaussian           the oracle's closed form on Y - m(X)
  Bernoulli          the probit quadrature over the same program
  unwhitened q(u)    tests/unwhiten_model.py at m - m(Z) (sparse_MF_SP.py:359, and the prior mean of :446)
"""
import math

import torch

from oracle import tgp_oracle as orc
import unwhiten_model as um

MEAN_BLOCK = (orc.FLOW_AFFINE, 0, 0, orc.FLAG_PER_ROW)


def mean(X, a, b=None):
    out = X @ a.reshape(-1)
    return out if b is None else out + b.reshape(())


def mean_rowp(X, a, b=None):
    """(N, 2): column 0 the constant 1, column 1 m(x_n)."""
    mx = mean(X, a, b)
    return torch.stack((torch.ones_like(mx), mx), 1)


def mean_program(program):
    return [MEAN_BLOCK] + [tuple(blk) for blk in (program or [])]


def ell_bernoulli(Y, mu, v, program, theta, xs, ws, rowp):
    """sum_n sum_s w_s / sqrt(pi) [y log Phi(g) + (1 - y) log Phi(-g)], g = G(mu + sqrt(2 v) x_s) (likelihoods/Bernoulli.py)."""
    f0 = mu.reshape(1, -1) + torch.sqrt(2.0 * v.clamp(min=0.0)).reshape(1, -1) * xs.reshape(-1, 1)
    g = orc.flow_forward(f0, program, theta, rowp)
    y = Y.reshape(1, -1)
    t = y * torch.special.log_ndtr(g) + (1.0 - y) * torch.special.log_ndtr(-g)
    return (t * (ws / math.sqrt(math.pi)).reshape(-1, 1)).sum()


def qf_moments(g, X, p, a, b):
    """(mu, v) of q(f) at the rows of X, the mean included."""
    args = (p["Z"], p["raw_lengthscale"], p["raw_outputscale"])
    if int(g["whiten"]):
        mu, v = orc.qf_moments(X, *args, p["m"], p["Lam"], kernel=g["kernel"])
    else:
        mu, v = um.qf_moments(X, *args, p["m"] - mean(p["Z"], a, b), p["Lam"], kernel=g["kernel"])
    return mu + mean(X, a, b), v


def elbo(g, p=None, a=None, b=None):
    """(ELBO, ELL, KLD) of fixture `g` (conftest.load_golden) at parameters `p` and mean parameters (a, b)."""
    p = g["params"] if p is None else p
    a, b = mean_params(g) if a is None else (a, b)
    X, y = g["X"], g["Y"].reshape(-1)
    args = (p["Z"], p["raw_lengthscale"], p["raw_outputscale"])
    if int(g["whiten"]):
        mu, v = orc.qf_moments(X, *args, p["m"], p["Lam"], kernel=g["kernel"])
        kl = orc.kld_whitened(p["m"], p["Lam"])
    else:
        mc = p["m"] - mean(p["Z"], a, b)
        mu, v = um.qf_moments(X, *args, mc, p["Lam"], kernel=g["kernel"])
        kl = um.kld(*args, mc, p["Lam"], kernel=g["kernel"])
    if int(g["bernoulli"]):
        ell = ell_bernoulli(y, mu, v, mean_program(g["program"]), p.get("theta"), g["xs"], g["ws"], mean_rowp(X, a, b))
    elif g["program"] is None:
        ell = orc.ell_gauss(y - mean(X, a, b), mu, v, p["log_var_noise"])
    else:
        ell = orc.ell_flow(y, mu, v, p["log_var_noise"], mean_program(g["program"]), p["theta"], g["xs"], g["ws"],
                           mean_rowp(X, a, b))
    ell = float(g["N_total"]) / X.shape[0] * ell
    return ell - kl, ell, kl


def mean_params(g):
    """(a, b) of a fixture: the linear mean's, or (W, None) of the identity mean."""
    if "mean_W" in g:
        return g["mean_W"], None
    return g["mean_a"], g["mean_b"]


def elbo_and_grads(g):
    """((ELBO, ELL, KLD), gradients by name; 'mean_a' / 'mean_b' for a linear mean)."""
    leaves = {k: v.detach().clone().requires_grad_(True) for k, v in g["params"].items()}
    a, b = mean_params(g)
    if b is not None:
        a, b = a.detach().clone().requires_grad_(True), b.detach().clone().requires_grad_(True)
    out = elbo(g, leaves, a, b)
    out[0].backward()
    grads = {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in leaves.items()}
    if b is not None:
        grads["mean_a"], grads["mean_b"] = a.grad, b.grad
    return tuple(o.detach() for o in out), grads
