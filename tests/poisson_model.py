"""CPU restatement of the Poisson likelihood (TGP_LIK_POISSON, include/tgp_hip.h) in torch, the autograd oracle of
tests/test_poisson_host.py and tests/test_gpu_poisson.py:

    log p(y | f0) = y G(f0) - exp(G(f0)) - lgamma(y + 1),   G the flow of the latent GP = the log-rate

`ell_torch` is the Gauss-Hermite expected log-likelihood, `pred_torch` the predictive mean, variance and log pmf (the latter
by torch.logsumexp), `step_torch` the ELBO of one training step (oracle q(f) moments -> ell_torch - whitened KL).

RANGE CONDITION, stated once: the restatement forms exp(G) in plain float64, so every comparison first asserts
`max_log_rate(...) <= GMAX` = 10 over the nodes whose normalised weight exceeds 1e-14 -- inputs past it would compare two
overflowing sums, not two likelihoods."""
import math

import torch

from oracle import tgp_oracle as O
from test_bernoulli_host import flow_torch

from tgp.pytorch_amd import lib as L

F64 = torch.float64
GMAX = 10.0


def flow_any(f, program, theta, rowp=None):
    """G(f): flow_torch for the SAL, affine, arcsinh and Box-Cox kinds, the oracle's flow_forward for programs with tanh steps."""
    program = [tuple(int(v) for v in b) for b in program]
    if len(program) == 0:
        return f
    if any(b[0] == L.FLOW_STEPTANH for b in program):
        return O.flow_forward(f, program, theta, rowp)
    return flow_torch(f, program, theta, rowp)


def _nodes(mu, v, program, theta, xs, rowp):
    f0 = mu.reshape(1, -1) + torch.sqrt(2.0 * v.clamp(min=0.0)).reshape(1, -1) * xs.reshape(-1, 1)
    return flow_any(f0, program, theta, rowp)


def max_log_rate(mu, v, program, theta, xs, ws, rowp=None):
    """max G(f0) over the nodes with wn > 1e-14 (the range condition's left-hand side)."""
    with torch.no_grad():
        g = _nodes(mu, v, program, theta, xs, rowp)
        keep = (ws / math.sqrt(math.pi)) > 1e-14
        return float(g[keep].max())


def ell_torch(Y, mu, v, program, theta, xs, ws, rowp=None, scale=1.0):
    """scale * sum_n [sum_s wn_s (y g_ns - exp(g_ns)) - lgamma(y_n + 1)], g_ns = G(mu_n + sqrt(2 max(v_n, 0)) x_s)."""
    g = _nodes(mu, v, program, theta, xs, rowp)
    y = Y.reshape(1, -1)
    t = (y * g - torch.exp(g)) * (ws / math.sqrt(math.pi)).reshape(-1, 1)
    return scale * (t.sum() - torch.lgamma(Y.reshape(-1) + 1.0).sum())


def pred_terms(Y, mu, v, program, theta, xs, ws, rowp=None):
    """(S, N): log wn_s + y g_ns - exp(g_ns) - lgamma(y + 1), the terms of the log predictive pmf."""
    g = _nodes(mu, v, program, theta, xs, rowp)
    y = Y.reshape(1, -1)
    return torch.log(ws / math.sqrt(math.pi)).reshape(-1, 1) + y * g - torch.exp(g) - torch.lgamma(y + 1.0)


def pred_torch(mu, v, program, theta, xs, ws, rowp=None, Y=None):
    """(m1, m2, logp): E[y] = sum wn exp(g), Var[y] = m1 + sum wn exp(2 g) - m1^2 (the empty program: exp(mu + v / 2) and
    m1 + (exp(v) - 1) m1^2), logp = logsumexp_s of pred_terms (None without Y)."""
    g = _nodes(mu, v, program, theta, xs, rowp)
    wn = (ws / math.sqrt(math.pi)).reshape(-1, 1)
    if len(program) == 0:
        vc = v.clamp(min=0.0)
        m1 = torch.exp(mu + 0.5 * vc)
        m2 = m1 + torch.expm1(vc) * m1 * m1
    else:
        m1 = (wn * torch.exp(g)).sum(0)
        m2 = m1 + (wn * torch.exp(2.0 * g)).sum(0) - m1 * m1
    logp = None if Y is None else torch.logsumexp(pred_terms(Y, mu, v, program, theta, xs, ws, rowp), 0)
    return m1, m2, logp


def step_torch(X, Y, params, N_total, program, xs, ws, kernel="scale_rbf", jitter=None):
    """((ELBO, ELL, KLD), grads, max log-rate) of one Poisson training step under autograd: O.qf_moments, ell_torch scaled by
    N_total / N, minus O.kld_whitened.  `params`: Z, raw_lengthscale, raw_outputscale, m, Lam[, theta]."""
    lv = {k: t.detach().clone().requires_grad_(True) for k, t in params.items() if k != "log_var_noise"}
    mu, v = O.qf_moments(X, lv["Z"], lv["raw_lengthscale"], lv["raw_outputscale"], lv["m"], lv["Lam"], jitter, kernel)
    prog = program or []
    ell = ell_torch(Y.reshape(-1), mu, v, prog, lv.get("theta"), xs, ws, None, float(N_total) / X.shape[0])
    kld = O.kld_whitened(lv["m"], lv["Lam"])
    elbo = ell - kld
    elbo.backward()
    gmax = max_log_rate(mu.detach(), v.detach(), prog, None if "theta" not in lv else lv["theta"].detach(), xs, ws)
    return (elbo.detach(), ell.detach(), kld.detach()), {k: t.grad for k, t in lv.items()}, gmax
