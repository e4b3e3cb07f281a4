"""CPU restatement of the heteroscedastic Gaussian likelihood (TGP_LIK_HETERO, include/tgp_hip.h) in float64 torch, the
autograd oracle of tests/test_hetero_host.py and tests/test_gpu_hetero.py:

    y | f, h ~ N(G(f), exp(c + h)),   q(f_n) = N(mu1, v1),  q(h_n) = N(mu2, v2) independent,  c = log_var_noise

`ell_torch` is the expected log-likelihood with h integrated out in closed form (a = c + mu2, p = exp(-a + v2 / 2)) and f by
Gauss-Hermite; `ell_product_rule` the same expectation by an independent S x S Gauss-Hermite product rule over (f, h), which
nothing of the closed form enters; `pred_torch` the predictive mean, variance and the S x S mixture log density (by
torch.logsumexp); `step_torch` the ELBO of one composed training step (two q(f) restatements -> ell_torch - the two KL terms)
under autograd.  Variances <= 0 count as 0 everywhere, as in the kernels."""
import math

import numpy as np
import torch

from oracle import tgp_oracle as O
from poisson_model import flow_any

F64 = torch.float64
LOG_2PI_REF = math.log(2.0 * float(np.float32(np.pi)))     # the constant of the Gaussian ELL kernels: the reference's float32 pi
LOG_2PI = math.log(2.0 * math.pi)                          # the predictive density's: double precision


def _nodes(mu, v, program, theta, xs, rowp):
    f0 = mu.reshape(1, -1) + torch.sqrt(2.0 * v.clamp(min=0.0)).reshape(1, -1) * xs.reshape(-1, 1)
    return flow_any(f0, program, theta, rowp)


def ell_torch(Y, mu, v, c, program, theta, xs, ws, rowp=None, scale=1.0):
    """scale * sum_n (-log(2 pi) / 2 - a_n / 2 - p_n A_n / 2); mu, v (2, N), c a 1-element tensor."""
    g = _nodes(mu[0], v[0], program, theta, xs, rowp)
    wn = (ws / math.sqrt(math.pi)).reshape(-1, 1)
    A = (wn * (Y.reshape(1, -1) - g) ** 2).sum(0)
    a = c.reshape(()) + mu[1]
    p = torch.exp(-a + 0.5 * v[1].clamp(min=0.0))
    return scale * (-0.5 * LOG_2PI_REF - 0.5 * a - 0.5 * p * A).sum()


def ell_product_rule(Y, mu, v, c, program, theta, xs, ws, rowp=None, scale=1.0):
    """The same expectation as a product rule: sum_s sum_t wn_s wn_t log N(y | g_s, exp(c + mu2 + sqrt(2 v2) xs_t))."""
    g = _nodes(mu[0], v[0], program, theta, xs, rowp)                                             # (S, N)
    wn = ws / math.sqrt(math.pi)
    lv = c.reshape(()) + mu[1].reshape(1, -1) + torch.sqrt(2.0 * v[1].clamp(min=0.0)).reshape(1, -1) * xs.reshape(-1, 1)   # (T, N)
    r2 = (Y.reshape(1, -1) - g) ** 2                                                                # (S, N)
    logn = -0.5 * (LOG_2PI_REF + lv.unsqueeze(0) + r2.unsqueeze(1) * torch.exp(-lv).unsqueeze(0))   # (S, T, N)
    return scale * (wn.reshape(-1, 1, 1) * wn.reshape(1, -1, 1) * logn).sum()


def pred_torch(mu, v, c, program, theta, xs, ws, rowp=None, Y=None, Y_std=1.0):
    """(m1, m2, logp) in standardised units: m1 = sum wn g, m2 = sum wn g^2 - m1^2 + exp(a + v2 / 2) (the empty program: mu1
    and max(v1, 0) + exp(a + v2 / 2)), logp = logsumexp_{s,t}(log wn_s + log wn_t + log N(y | g_s, e^{a + sqrt(2 v2) xs_t})) -
    log Y_std (None without Y).  Nodes of weight 0 (underflowed) do not enter."""
    g = _nodes(mu[0], v[0], program, theta, xs, rowp)
    wn = ws / math.sqrt(math.pi)
    v2 = v[1].clamp(min=0.0)
    a = c.reshape(()) + mu[1]
    noise = torch.exp(a + 0.5 * v2)
    if len(program) == 0:
        m1, m2 = mu[0].clone(), v[0].clamp(min=0.0) + noise
    else:
        m1 = (wn.reshape(-1, 1) * g).sum(0)
        m2 = (wn.reshape(-1, 1) * g * g).sum(0) - m1 * m1 + noise
    logp = None
    if Y is not None:
        lv = a.reshape(1, -1) + torch.sqrt(2.0 * v2).reshape(1, -1) * xs.reshape(-1, 1)              # (T, N)
        r2 = (Y.reshape(1, -1) - g) ** 2
        lw = torch.log(wn)                                                                           # -inf at weight 0
        t = lw.reshape(-1, 1, 1) + lw.reshape(1, -1, 1) - 0.5 * (LOG_2PI + lv.unsqueeze(0) + r2.unsqueeze(1) * torch.exp(-lv).unsqueeze(0))
        logp = torch.logsumexp(t.reshape(-1, t.shape[-1]), 0) - math.log(Y_std)
    return m1, m2, logp


def step_torch(X, Y, params_f, params_h, c, N_total, program, xs, ws, kernel="scale_rbf", jitter=None, whiten=True):
    """((ELBO, ELL, KLD), grads_f, grads_h, grad_c) of one composed heteroscedastic step under autograd.  `params_f`, `params_h`:
    Z, raw_lengthscale, raw_outputscale, m, Lam of the two latent GPs (`params_f` also theta); whitened: O.qf_moments and
    O.kld_whitened per GP; unwhitened (m, Lam describe q(u) itself): tests/unwhiten_model.py's moments and KL."""
    keys = ("Z", "raw_lengthscale", "raw_outputscale", "m", "Lam")
    lf = {k: t.detach().clone().requires_grad_(True) for k, t in params_f.items() if k in keys + ("theta",)}
    lh = {k: t.detach().clone().requires_grad_(True) for k, t in params_h.items() if k in keys}
    cc = c.detach().clone().requires_grad_(True)
    mus, vs, kld = [], [], 0.0
    for lv in (lf, lh):
        args = [lv[k] for k in keys]
        if whiten:
            mu, v = O.qf_moments(X, *args, jitter, kernel)
            kld = kld + O.kld_whitened(lv["m"], lv["Lam"])
        else:
            import unwhiten_model as um
            mu, v = um.qf_moments(X, *args, kernel=kernel)
            kld = kld + um.kld(*args, kernel=kernel)
        mus.append(mu)
        vs.append(v)
    ell = ell_torch(Y.reshape(-1), torch.stack(mus), torch.stack(vs), cc, program or [], lf.get("theta"), xs, ws, None,
                    float(N_total) / X.shape[0])
    elbo = ell - kld
    elbo.backward()
    return ((elbo.detach(), ell.detach(), kld.detach()), {k: t.grad for k, t in lf.items()}, {k: t.grad for k, t in lh.items()},
            cc.grad)
