"""CPU restatement of the Student-t likelihood (TGP_LIK_STUDENT, include/tgp_hip.h) in torch, the autograd oracle of
tests/test_student_host.py and tests/test_gpu_student.py:

    y | f0 ~ StudentT(nu, loc = G(f0), scale = sigma),  eta = log sigma^2 (log_var_noise), nu fixed
    log p(y | g) = lgamma((nu+1)/2) - lgamma(nu/2) - log(nu pi)/2 - eta/2 - (nu+1)/2 log1p((y - g)^2 / (nu sigma^2))

`ell_torch` is the Gauss-Hermite expected log-likelihood, `pred_torch` the predictive mean, variance and log density (the
latter by torch.logsumexp), `step_torch` the ELBO of one training step (oracle q(f) moments -> ell_torch - whitened KL) under
autograd, the gradient in log_var_noise included."""
import math

import torch

from oracle import tgp_oracle as O
from poisson_model import flow_any

F64 = torch.float64


def log_p(y, g, eta, nu):
    """The node term: log StudentT(y | nu, g, exp(eta / 2)), every constant included.  `eta` a tensor, `nu` a float."""
    nu = float(nu)
    r = y - g
    const = math.lgamma(0.5 * (nu + 1.0)) - math.lgamma(0.5 * nu) - 0.5 * math.log(nu * math.pi)
    return const - 0.5 * eta - 0.5 * (nu + 1.0) * torch.log1p(r * r / (nu * torch.exp(eta)))


def _nodes(mu, v, program, theta, xs, rowp):
    f0 = mu.reshape(1, -1) + torch.sqrt(2.0 * v.clamp(min=0.0)).reshape(1, -1) * xs.reshape(-1, 1)
    return flow_any(f0, program, theta, rowp)


def ell_torch(Y, mu, v, eta, nu, program, theta, xs, ws, rowp=None, scale=1.0):
    """scale * sum_n sum_s wn_s log p(y_n | g_ns), g_ns = G(mu_n + sqrt(2 max(v_n, 0)) x_s)."""
    g = _nodes(mu, v, program, theta, xs, rowp)
    t = log_p(Y.reshape(1, -1), g, eta.reshape(()), nu) * (ws / math.sqrt(math.pi)).reshape(-1, 1)
    return scale * t.sum()


def pred_torch(mu, v, eta, nu, program, theta, xs, ws, rowp=None, Y=None, Y_std=1.0):
    """(m1, m2, logp) in standardised units: m1 = sum wn g, m2 = sum wn g^2 - m1^2 + sigma^2 nu / (nu - 2) (+inf for nu <= 2),
    logp = logsumexp_s(log wn_s + log p(y | g_s)) - log Y_std (None without Y)."""
    g = _nodes(mu, v, program, theta, xs, rowp)
    wn = (ws / math.sqrt(math.pi)).reshape(-1, 1)
    m1 = (wn * g).sum(0)
    tail = torch.exp(eta.reshape(())) * nu / (nu - 2.0) if nu > 2.0 else torch.tensor(float("inf"), dtype=F64)
    m2 = (wn * g * g).sum(0) - m1 * m1 + tail
    logp = None
    if Y is not None:
        logp = torch.logsumexp(torch.log(wn) + log_p(Y.reshape(1, -1), g, eta.reshape(()), nu), 0) - math.log(Y_std)
    return m1, m2, logp


def step_torch(X, Y, params, nu, N_total, program, xs, ws, kernel="scale_rbf", jitter=None):
    """((ELBO, ELL, KLD), grads) of one Student-t training step under autograd: O.qf_moments, ell_torch scaled by
    N_total / N, minus O.kld_whitened.  `params`: Z, raw_lengthscale, raw_outputscale, m, Lam, log_var_noise[, theta]."""
    lv = {k: t.detach().clone().requires_grad_(True) for k, t in params.items()}
    mu, v = O.qf_moments(X, lv["Z"], lv["raw_lengthscale"], lv["raw_outputscale"], lv["m"], lv["Lam"], jitter, kernel)
    ell = ell_torch(Y.reshape(-1), mu, v, lv["log_var_noise"], nu, program or [], lv.get("theta"), xs, ws, None,
                    float(N_total) / X.shape[0])
    kld = O.kld_whitened(lv["m"], lv["Lam"])
    elbo = ell - kld
    elbo.backward()
    return (elbo.detach(), ell.detach(), kld.detach()), {k: t.grad for k, t in lv.items()}
