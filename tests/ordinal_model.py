"""CPU restatement of the ordinal (cumulative-probit) likelihood (TGP_LIK_ORDINAL, include/tgp_hip.h) in torch, the autograd
oracle of tests/test_ordinal_host.py and tests/test_gpu_ordinal.py.  With K - 1 fixed, increasing bin edges b_1 < .. < b_{K-1}
(b_0 = -inf, b_K = +inf), sigma^2 = exp(lvn), g = G(f0), u = (b_{y+1} - g) / sigma and l = (b_y - g) / sigma:

    log p(y | g) = log(Phi(u) - Phi(l)) = log_ndtr(a) + log(-expm1(log_ndtr(b) - log_ndtr(a))),

(a, b) = (u, l), or (-l, -u) when l > 0: the difference is taken on the side where both tails are small.  An infinite edge
drops its term (log_ndtr(-inf) = -inf, expm1 = -1, log 1 = 0), formed without any arithmetic on the infinity so that autograd
stays finite.  Gradients come from autograd.

`ell_torch` is the Gauss-Hermite expected log-likelihood, `pred_torch` the predictive mean, variance and log pmf (the empty
program: the closed form, every edge at (b_j - mu) / sqrt(sigma^2 + max(v, 0))), `step_torch` the ELBO of one training step
(oracle q(f) moments -> ell_torch - whitened KL).

RANGE CONDITION, stated once: every bin of a comparison has width / sigma >= MIN_WIDTH = 1e-3 (`min_bin_width`; each
comparison asserts it on its inputs first).  Against 60-digit arithmetic, at that width the restatement is within 8e-14 (value)
and 1.4e-12 (gradient) of exact; at width / sigma = 1e-6 only 5e-11 / 1.5e-9, which is why narrower bins are not compared.  For
|u| up to 160 it is within 1e-15."""
import math

import torch

from oracle import tgp_oracle as O
from poisson_model import flow_any

F64 = torch.float64
MIN_WIDTH = 1e-3


def default_edges(K):
    """b_j = j - K / 2, j = 1 .. K-1: unit spacing, centred."""
    return torch.tensor([j - K / 2.0 for j in range(1, K)], dtype=F64)


def min_bin_width(lvn, edges):
    """min_j (b_{j+1} - b_j) / sigma over the finite bins (inf for K = 2, which has none): the range condition's left-hand side."""
    e = torch.as_tensor(edges, dtype=F64).reshape(-1)
    if e.numel() < 2:
        return math.inf
    return float((e[1:] - e[:-1]).min() * torch.exp(-0.5 * torch.as_tensor(lvn, dtype=F64).detach().reshape(-1)[0]))


def log_p(g, y, lvn, edges):
    """log p(y | g) elementwise: g (S, N) or (N,), y (N,) classes (integers in [0, K-1]), lvn the log noise variance (one
    element, or (N,): a row's own), edges (K-1,)."""
    e = torch.as_tensor(edges, dtype=F64).reshape(-1)
    K = e.numel() + 1
    yi = y.reshape(-1).long()
    assert bool(((yi >= 0) & (yi <= K - 1)).all())
    lo_inf, hi_inf = yi == 0, yi == K - 1
    lo_b = e[(yi - 1).clamp(min=0)]
    hi_b = e[yi.clamp(max=K - 2)]
    isig = torch.exp(-0.5 * lvn.reshape(-1))
    zero = torch.zeros_like(g)
    # (an infinite edge stands at g itself, l = 0 or u = 0, and its terms are masked below)
    l = torch.where(lo_inf, zero, (lo_b - g) * isig)
    u = torch.where(hi_inf, zero, (hi_b - g) * isig)
    flip = l > 0.0
    a, b = torch.where(flip, -l, u), torch.where(flip, -u, l)
    a_inf = torch.where(flip, lo_inf, hi_inf).expand_as(a)      # the edge behind a (b) is infinite
    b_inf = torch.where(flip, hi_inf, lo_inf).expand_as(b)
    la = torch.where(a_inf, zero, torch.special.log_ndtr(a))
    d = torch.where(b_inf, -torch.ones_like(g), torch.special.log_ndtr(b) - la)
    return la + torch.where(b_inf, zero, torch.log(-torch.expm1(d)))


def _nodes(mu, v, program, theta, xs, rowp):
    f0 = mu.reshape(1, -1) + torch.sqrt(2.0 * v.clamp(min=0.0)).reshape(1, -1) * xs.reshape(-1, 1)
    return flow_any(f0, program, theta, rowp)


def ell_torch(Y, mu, v, lvn, edges, program, theta, xs, ws, rowp=None, scale=1.0):
    """scale * sum_n sum_s wn_s log p(y_n | g_ns), g_ns = G(mu_n + sqrt(2 max(v_n, 0)) x_s)."""
    g = _nodes(mu, v, program, theta, xs, rowp)
    return scale * (log_p(g, Y, lvn, edges) * (ws / math.sqrt(math.pi)).reshape(-1, 1)).sum()


def ell_rows(Y, mu, v, lvn, edges, program, theta, xs, ws, rowp=None):
    """(N,): the rows of ell_torch."""
    g = _nodes(mu, v, program, theta, xs, rowp)
    return (log_p(g, Y, lvn, edges) * (ws / math.sqrt(math.pi)).reshape(-1, 1)).sum(0)


def _moments(g, isig, edges):
    """E[y | g] = sum_j (1 - Phi_j), E[y^2 | g] = sum_j (2j - 1)(1 - Phi_j), Phi_j = Phi((b_j - g) isig): shape of g."""
    e = torch.as_tensor(edges, dtype=F64).reshape(-1)
    sf = torch.special.ndtr((g.unsqueeze(-1) - e) * isig.unsqueeze(-1))
    j = torch.arange(1, e.numel() + 1, dtype=F64)
    return sf.sum(-1), (sf * (2.0 * j - 1.0)).sum(-1)


def pred_torch(mu, v, lvn, edges, program, theta, xs, ws, rowp=None, Y=None):
    """(m1, m2, logp): E[y], Var[y] = E[y^2] - m1^2 and the log predictive pmf of class Y (None without Y), by the quadrature
    (logp by torch.logsumexp) -- or, for the empty program, in closed form."""
    lvn = torch.as_tensor(lvn, dtype=F64).reshape(-1)[:1]
    if len(program) == 0:
        s2 = torch.exp(lvn) + v.clamp(min=0.0)
        e1, e2 = _moments(mu, 1.0 / torch.sqrt(s2), edges)
        logp = None if Y is None else log_p(mu, Y, torch.log(s2), edges)
        return e1, e2 - e1 * e1, logp
    g = _nodes(mu, v, program, theta, xs, rowp)
    wn = (ws / math.sqrt(math.pi)).reshape(-1, 1)
    c1, c2 = _moments(g, torch.exp(-0.5 * lvn).expand_as(g), edges)
    e1, e2 = (wn * c1).sum(0), (wn * c2).sum(0)
    logp = None if Y is None else torch.logsumexp(torch.log(wn) + log_p(g, Y, lvn, edges), 0)
    return e1, e2 - e1 * e1, logp


def pmf_closed(mu, v, lvn, edges):
    """(N, K): the class probabilities of the empty program, differences of P(y <= k) = Phi((b_{k+1} - mu) / sqrt(sigma^2 + max(v, 0)))."""
    e = torch.as_tensor(edges, dtype=F64).reshape(-1)
    s = torch.sqrt(torch.exp(torch.as_tensor(lvn, dtype=F64).reshape(-1)[0]) + v.clamp(min=0.0))
    cdf = torch.special.ndtr((e.reshape(1, -1) - mu.reshape(-1, 1)) / s.reshape(-1, 1))
    cdf = torch.cat((torch.zeros_like(cdf[:, :1]), cdf, torch.ones_like(cdf[:, :1])), 1)
    return cdf[:, 1:] - cdf[:, :-1]


def sample_classes(g, lvn, edges, gen):
    """y = #{j : g + sigma eps > b_j}: a draw from the model at the latent values g."""
    e = torch.as_tensor(edges, dtype=F64).reshape(-1)
    z = g + torch.exp(0.5 * torch.as_tensor(lvn, dtype=F64).reshape(-1)[0]) * torch.randn(g.shape, generator=gen, dtype=F64)
    return (z.unsqueeze(-1) > e).sum(-1).to(F64)


def step_torch(X, Y, params, edges, N_total, program, xs, ws, kernel="scale_rbf", jitter=None):
    """((ELBO, ELL, KLD), grads) of one ordinal training step under autograd: O.qf_moments, ell_torch scaled by N_total / N, minus
    O.kld_whitened.  `params`: Z, raw_lengthscale, raw_outputscale, m, Lam, log_var_noise[, theta]."""
    lv = {k: t.detach().clone().requires_grad_(True) for k, t in params.items()}
    mu, v = O.qf_moments(X, lv["Z"], lv["raw_lengthscale"], lv["raw_outputscale"], lv["m"], lv["Lam"], jitter, kernel)
    prog = program or []
    ell = ell_torch(Y.reshape(-1), mu, v, lv["log_var_noise"], edges, prog, lv.get("theta") if prog else None, xs, ws, None,
                    float(N_total) / X.shape[0])
    kld = O.kld_whitened(lv["m"], lv["Lam"])
    elbo = ell - kld
    elbo.backward()
    return (elbo.detach(), ell.detach(), kld.detach()), {k: t.grad for k, t in lv.items()}
