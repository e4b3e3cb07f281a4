"""CPU restatement of the negative-binomial likelihood (TGP_LIK_NEGBIN, include/tgp_hip.h) in torch, the autograd oracle of
tests/test_negbin_host.py and tests/test_gpu_negbin.py.  With g = G(f0) the log-mean, lam = log r the log dispersion,
u = g - lam and sp(u) = log(1 + e^u):

    log p(y | g) = lgamma(y + r) - lgamma(r) - lgamma(y + 1) + y u - (y + r) sp(u)
    d/dg         = y - (y + r) sigmoid(u)
    d/dlam       = r [psi(y + r) - psi(r)] - r sp(u) - d/dg

`ell_torch` is the Gauss-Hermite expected log-likelihood, `pred_torch` the predictive mean, variance and log pmf (the latter
by torch.logsumexp), `step_torch` the ELBO of one training step (oracle q(f) moments -> ell_torch - whitened KL).  The flow
and node helpers are those of tests/poisson_model.py.

RANGE CONDITIONS, stated once; every comparison first asserts `in_range(...)`:
  * `max_log_rate(...) <= GMAX` = 10 over the nodes whose normalised weight exceeds 1e-14 (Poisson's condition, for the same
    reason: the restatement forms exp(G) in plain float64 for the moments, and past it two overflowing sums are compared);
  * RMIN = 1e-3 <= r <= RMAX = 1e3: the terms of d/dlam cancel as r grows (relative error 2e-10 at 1e3, 2e-7 at 1e4)."""
import math

import torch

from oracle import tgp_oracle as O
from poisson_model import GMAX, _nodes, flow_any, max_log_rate      # noqa: F401  (re-exported for the tests)

F64 = torch.float64
RMIN, RMAX = 1e-3, 1e3


def in_range(lam, mu, v, program, theta, xs, ws, rowp=None):
    """The two range conditions: (ok, max G, r)."""
    r = float(torch.exp(torch.as_tensor(lam, dtype=F64).detach().reshape(-1)[0]))
    gmax = max_log_rate(mu, v, program, theta, xs, ws, rowp)
    return (gmax <= GMAX and RMIN * (1 - 1e-12) <= r <= RMAX * (1 + 1e-12)), gmax, r


def softplus(u):
    """log(1 + e^u), stable: u > 0 ? u + log1p(e^-u) : log1p(e^u)."""
    return torch.where(u > 0, u + torch.log1p(torch.exp(-u.abs())), torch.log1p(torch.exp(-u.abs())))


def row_term(y, lam):
    """lgamma(y + r) - lgamma(r) - lgamma(y + 1): the part of log p that depends on y and r only."""
    r = torch.exp(lam)
    return torch.lgamma(y + r) - torch.lgamma(r) - torch.lgamma(y + 1.0)


def log_p(y, g, lam):
    """log NB(y | mean = exp(g), dispersion r = exp(lam)); broadcasts."""
    u = g - lam
    return row_term(y, lam) + y * u - (y + torch.exp(lam)) * softplus(u)


def dlog_p_dg(y, g, lam):
    return y - (y + torch.exp(lam)) * torch.sigmoid(g - lam)


def dlog_p_dlam(y, g, lam):
    r = torch.exp(lam)
    return r * (torch.digamma(y + r) - torch.digamma(r)) - r * softplus(g - lam) - dlog_p_dg(y, g, lam)


def ell_rows(Y, mu, v, lam, program, theta, xs, ws, rowp=None):
    """(N,): sum_s wn_s log p(y_n | g_ns), g_ns = G(mu_n + sqrt(2 max(v_n, 0)) x_s)."""
    g = _nodes(mu, v, program, theta, xs, rowp)
    y = Y.reshape(1, -1)
    lam = lam.reshape(())
    u = g - lam
    wn = (ws / math.sqrt(math.pi)).reshape(-1, 1)
    return (wn * (y * u - (y + torch.exp(lam)) * softplus(u))).sum(0) + row_term(Y.reshape(-1), lam)


def ell_torch(Y, mu, v, lam, program, theta, xs, ws, rowp=None, scale=1.0):
    """scale * sum_n ell_rows."""
    return scale * ell_rows(Y, mu, v, lam, program, theta, xs, ws, rowp).sum()


def dlam_rows(Y, mu, v, lam, program, theta, xs, ws, rowp=None):
    """(N,): each row's contribution to dELL/dlam (unscaled), from the closed form."""
    with torch.no_grad():
        g = _nodes(mu, v, program, theta, xs, rowp)
        wn = (ws / math.sqrt(math.pi)).reshape(-1, 1)
        return (wn * dlog_p_dlam(Y.reshape(1, -1), g, lam.reshape(()))).sum(0)


def pred_terms(Y, mu, v, lam, program, theta, xs, ws, rowp=None):
    """(S, N): log wn_s + log p(y_n | g_ns), the terms of the log predictive pmf."""
    g = _nodes(mu, v, program, theta, xs, rowp)
    return torch.log(ws / math.sqrt(math.pi)).reshape(-1, 1) + log_p(Y.reshape(1, -1), g, lam.reshape(()))


def pred_torch(mu, v, lam, program, theta, xs, ws, rowp=None, Y=None):
    """(m1, m2, logp): E[y] = sum wn exp(g), Var[y] = m1 + (1 + 1/r) sum wn exp(2 g) - m1^2 (the empty program: the log-normal
    closed forms E[mean] = exp(mu + v / 2), E[mean^2] = exp(2 mu + 2 v)), logp = logsumexp_s of pred_terms (None without Y)."""
    g = _nodes(mu, v, program, theta, xs, rowp)
    wn = (ws / math.sqrt(math.pi)).reshape(-1, 1)
    c = 1.0 + torch.exp(-lam.reshape(()))
    if len(program) == 0:
        vc = v.clamp(min=0.0)
        m1 = torch.exp(mu + 0.5 * vc)
        e2 = torch.exp(2.0 * mu + 2.0 * vc)
    else:
        m1 = (wn * torch.exp(g)).sum(0)
        e2 = (wn * torch.exp(2.0 * g)).sum(0)
    m2 = m1 + c * e2 - m1 * m1
    logp = None if Y is None else torch.logsumexp(pred_terms(Y, mu, v, lam, program, theta, xs, ws, rowp), 0)
    return m1, m2, logp


def step_torch(X, Y, params, N_total, program, xs, ws, kernel="scale_rbf", jitter=None):
    """((ELBO, ELL, KLD), grads, (ok, max G, r)) of one negative-binomial training step under autograd: O.qf_moments, ell_torch
    scaled by N_total / N, minus O.kld_whitened.  `params`: Z, raw_lengthscale, raw_outputscale, m, Lam, log_var_noise (= log r)
    [, theta]."""
    lv = {k: t.detach().clone().requires_grad_(True) for k, t in params.items()}
    mu, v = O.qf_moments(X, lv["Z"], lv["raw_lengthscale"], lv["raw_outputscale"], lv["m"], lv["Lam"], jitter, kernel)
    prog = program or []
    ell = ell_torch(Y.reshape(-1), mu, v, lv["log_var_noise"], prog, lv.get("theta"), xs, ws, None, float(N_total) / X.shape[0])
    kld = O.kld_whitened(lv["m"], lv["Lam"])
    elbo = ell - kld
    elbo.backward()
    rng = in_range(lv["log_var_noise"], mu.detach(), v.detach(), prog, None if "theta" not in lv else lv["theta"].detach(), xs, ws)
    return (elbo.detach(), ell.detach(), kld.detach()), {k: t.grad for k, t in lv.items()}, rng
