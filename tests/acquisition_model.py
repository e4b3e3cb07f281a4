"""Torch restatement of the acquisition kernels (k_pred_acq / k_acq_gauss of csrc/tgp_quantile.hip) for the tests, float64 on
the CPU.  With c = +1 to maximise and -1 to minimise, sigma^2 = exp(log_var_noise), g_ns = G(mu_n + sqrt(2 v_n) xs_s),
z_ns = c (g_ns - best) / sigma and h(z) = z Phi(z) + phi(z):

    EI_n = sigma sum_s wn_s h(z_ns),   PI_n = sum_s wn_s Phi(z_ns),   logEI_n = log sigma + logsumexp_s(log wn_s + log h(z_ns))

and the partials of each in mu and v at fixed flow parameters (a row with v <= 0 counts as v = 0, zeros in the v row).  `log_h`
states the kernel's three branches of log h; the node table is quantile_model.nodes (values) or the oracle's flow with its
slope (input_grad_model.flow_value_and_slope) when the partials are asked for.  The empty program: one Gaussian, closed form."""
import math

import torch

from quantile_model import G, nodes  # noqa: F401  (G: re-exported for the tests)

SQRT1_2 = 0.70710678118654752440
INV_SQRT_2PI = 0.39894228040143267794
SQRT_PI_2 = 1.25331413731550025121
LOG_SQRT_2PI = 0.91893853320467274178
Z_DIRECT, Z_SERIES = -1.0, -30.0      # the branch points: z > -1 as written, (-30, -1] log1p(z q), z <= -30 the series
KINDS = ("ei", "log_ei", "pi")


def Phi(z):
    small = 0.5 * torch.erfc(z.abs() * SQRT1_2)
    return torch.where(z < 0.0, small, 1.0 - small)


def phi(z):
    return INV_SQRT_2PI * torch.exp(-0.5 * z * z)


def log_h(z):
    """(log h, Phi / h, phi / h, h) elementwise, h(z) = z Phi(z) + phi(z) = phi(z) (1 + z q(z)), q = Phi / phi =
    sqrt(pi / 2) erfcx(-z / sqrt 2): the kernel's branches."""
    z = torch.as_tensor(z, dtype=torch.float64)
    zd = z.clamp_min(Z_DIRECT)                               # (each branch on arguments inside its own range)
    P, p = 0.5 * torch.erfc(-zd * SQRT1_2), phi(zd)
    hd = zd * P + p
    zl = z.clamp_max(Z_DIRECT)
    q = SQRT_PI_2 * torch.special.erfcx(-zl * SQRT1_2)
    u = 1.0 / (zl * zl)
    series = u * (1.0 - 3.0 * u * (1.0 - 5.0 * u * (1.0 - 7.0 * u * (1.0 - 9.0 * u * (1.0 - 11.0 * u)))))
    far = zl <= Z_SERIES
    t = torch.where(far, series, 1.0 + zl * q)
    logt = torch.where(far, torch.log(series), torch.log1p((zl * q).clamp_min(-1.0 + 1e-300)))
    low = z <= Z_DIRECT
    logh = torch.where(low, -0.5 * zl * zl - LOG_SQRT_2PI + logt, torch.log(hd))
    return (logh, torch.where(low, q / t, P / hd), torch.where(low, 1.0 / t, p / hd),
            torch.where(low, phi(zl) * t, hd))


def acquisition(mu, v, lvn, kind, best, c, xs, wn, program, theta, rowp=None, want_partials=False):
    """value (N,), or (value, partials (2, N)): the three acquisition functions and their partials in mu (row 0), v (row 1)."""
    assert kind in KINDS and c in (1.0, -1.0)
    var = math.exp(float(lvn))
    sigma = math.sqrt(var)
    pos = v > 0.0
    if program is None or len(program) == 0:
        sd = torch.sqrt(v.clamp_min(0.0) + var)
        z = c * (mu - best) / sd
        lh, Ph, ph, h = log_h(z)
        if kind == "ei":
            val, a_mu, a_v = sd * h, c * Phi(z), phi(z) / (2.0 * sd)
        elif kind == "pi":
            val, a_mu, a_v = Phi(z), c * phi(z) / sd, -z * phi(z) / (2.0 * sd * sd)
        else:
            val, a_mu, a_v = torch.log(sd) + lh, c * Ph / sd, ph / (2.0 * sd * sd)
        return (val, torch.stack((a_mu, torch.where(pos, a_v, torch.zeros_like(a_v))))) if want_partials else val
    w = wn.reshape(-1, 1)
    xcol = xs.reshape(-1, 1)
    sq = torch.sqrt(2.0 * v.clamp_min(0.0))
    if want_partials:
        from input_grad_model import flow_value_and_slope
        g, gp = flow_value_and_slope(mu.unsqueeze(0) + sq.unsqueeze(0) * xcol, program, theta, rowp)
    else:
        g, gp = nodes(mu, v, xs, program, theta, rowp), None
    z = c * ((g - best) / sigma)
    if kind == "log_ei":
        lh, Ph, _, _ = log_h(z)
        terms = torch.log(w) + lh                            # (log 0 = -inf: a weight of 0 does not enter)
        lse = torch.logsumexp(terms, 0)
        val = math.log(sigma) + lse
        dg = torch.exp(terms - lse.unsqueeze(0)) * Ph * (c / sigma) if want_partials else None
    elif kind == "ei":
        val = sigma * (w * log_h(z)[3]).sum(0)
        dg = c * w * Phi(z)
    else:
        val = (w * Phi(z)).sum(0)
        dg = (c / sigma) * w * phi(z)
    if not want_partials:
        return val
    inv = torch.where(pos, 1.0 / sq.clamp_min(1e-300), torch.zeros_like(sq))
    return val, torch.stack(((dg * gp).sum(0), (dg * gp * xcol).sum(0) * inv))
