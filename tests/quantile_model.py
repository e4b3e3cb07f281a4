"""Torch restatement of the predictive CDF / quantile kernels (csrc/tgp_quantile.hip) for the tests, float64 on the CPU:

    F_n(t) = sum_s wn_s Phi((t - g_ns) / sigma),   g_ns = G(mu_n + sqrt(2 v_n) xs_s),   sigma^2 = exp(log_var_noise)

`tails` is the kernel's evaluation of F (Phi through erfc on the side where it is small, the lower and the upper sum each on
its own), `quantiles` its root rule -- start G(mu + zq sqrt v) + zq sigma, bracket by doubling steps of
max(sigma, |t0| 2^-20), Newton steps with the density, bisection whenever a step leaves the bracket, stop at an exact hit or
a step <= 2^-50 max(1, |t|), at most 128 evaluations per phase, p <= 0.5 on the lower-tail equation and p > 0.5 on the
upper-tail one -- and `bisect_quantiles` an independent solver: plain bisection on F until the bracket no longer shrinks.
The flow itself is warp_model.flow_forward (the same block table)."""
import math

import torch

from warp_model import flow_forward

MAXIT = 128
STEP_TOL = 8.8817841970012523e-16    # 2^-50
START_REL = 9.5367431640625e-07      # 2^-20
SQRT1_2 = 0.70710678118654752440
INV_SQRT_2PI = 0.39894228040143267794


def G(f, program, theta, rowp=None):
    """The flow at f of shape (N,) or (K,N) (row n uses rowp[n, :]); the empty program is the identity."""
    if not len(program):
        return f
    return flow_forward(f, [tuple(int(x) for x in b) for b in program], theta, rowp)[0]


def nodes(mu, v, xs, program, theta, rowp=None):
    """(S,N) node values g_ns; a row with v <= 0 counts as v = 0."""
    vn = v.clamp_min(0.0)
    return G(mu.unsqueeze(0) + torch.sqrt(2.0 * vn).unsqueeze(0) * xs.unsqueeze(1), program, theta, rowp)


def tails(g, wn, sigma, t):
    """(lower, upper, density) at t of shape (N,) from the node values g (S,N): sum wn Phi(z), sum wn Phi(-z), F'(t)."""
    z = (t.unsqueeze(0) - g) / sigma
    small = 0.5 * torch.erfc(z.abs() * SQRT1_2)
    big = 1.0 - small
    neg = z < 0.0
    w = wn.unsqueeze(1)
    lower = (w * torch.where(neg, small, big)).sum(0)
    upper = (w * torch.where(neg, big, small)).sum(0)
    dens = (w * torch.exp(-0.5 * z * z)).sum(0) * INV_SQRT_2PI / sigma
    return lower, upper, dens


def residual(g, wn, sigma, t, p):
    """|F(t) - p| / min(p, 1 - p) per row, F from the tail that is small at p (the rule the tests hold every root to)."""
    lower, upper, _ = tails(g, wn, sigma, t)
    if p > 0.5:
        return (upper - (1.0 - p)).abs() / (1.0 - p)
    return (lower - p).abs() / p


def _signed(g, wn, sigma, t, p):
    """F(t) - p from the small tail (increasing in t on both sides) and the density."""
    lower, upper, dens = tails(g, wn, sigma, t)
    return ((1.0 - p) - upper if p > 0.5 else lower - p), dens


def start(mu, v, sigma, zq, program, theta, rowp=None):
    return G(mu + zq * torch.sqrt(v.clamp_min(0.0)), program, theta, rowp) + zq * sigma


def quantiles(mu, v, lvn, probs, xs, wn, program, theta, rowp=None):
    """(t of shape (Q,N), number of roots that ran out of evaluations): the kernel's rule, all rows at once."""
    sigma = math.sqrt(math.exp(float(lvn)))
    probs = [float(p) for p in probs]
    zqs = torch.special.ndtri(torch.tensor(probs, dtype=torch.float64))
    if not len(program):
        sd = torch.sqrt(v.clamp_min(0.0) + math.exp(float(lvn)))
        return mu.unsqueeze(0) + zqs.unsqueeze(1) * sd.unsqueeze(0), 0
    g = nodes(mu, v, xs, program, theta, rowp)
    out, failed = [], 0
    for p, zq in zip(probs, zqs):
        x = start(mu, v, sigma, zq, program, theta, rowp)
        fx, dn = _signed(g, wn, sigma, x, p)
        done = ~(v > 0.0) | (fx == 0.0)
        # ---- bracket
        step = torch.maximum(torch.full_like(x, sigma), x.abs() * START_REL)
        up = fx < 0.0
        lo, hi = torch.where(up, x, x - step), torch.where(up, x + step, x)
        ok = done.clone()
        for _ in range(MAXIT):
            if bool(ok.all()):
                break
            probe = torch.where(ok, x, torch.where(up, hi, lo))
            fb, _d = _signed(g, wn, sigma, probe, p)
            hit = torch.where(up, fb >= 0.0, fb <= 0.0)
            grow = ~ok & ~hit
            ok = ok | hit
            step = torch.where(grow, step * 2.0, step)
            lo_n = torch.where(up, hi, lo - step)
            hi_n = torch.where(up, hi + step, lo)
            lo, hi = torch.where(grow, lo_n, lo), torch.where(grow, hi_n, hi)
        fail = ~ok
        done = done | fail
        # ---- Newton with bisection
        for _ in range(MAXIT):
            act = ~done
            zero = act & (fx == 0.0)
            mv = act & ~zero
            lo = torch.where(mv & (fx < 0.0), x, lo)
            hi = torch.where(mv & ~(fx < 0.0), x, hi)
            xn = x - fx / dn
            xn = torch.where((xn > lo) & (xn < hi), xn, 0.5 * (lo + hi))
            dx = (xn - x).abs()
            x = torch.where(mv, xn, x)
            done = done | zero | (mv & (dx <= STEP_TOL * x.abs().clamp_min(1.0)))
            if bool(done.all()):
                break
            f2, d2 = _signed(g, wn, sigma, x, p)
            fx, dn = torch.where(done, fx, f2), torch.where(done, dn, d2)
        fail = fail | ~done
        failed += int(fail.sum())
        out.append(torch.where(fail, torch.full_like(x, float("nan")), x))
    return torch.stack(out), failed


def bisect_quantiles(mu, v, lvn, probs, xs, wn, program, theta, rowp=None):
    """The same roots by plain bisection on F, from a bracket 40 sigma outside the node values, until the midpoint is one of
    the two ends (the bracket no longer shrinks).  Shares `tails` with the rule above and nothing else."""
    sigma = math.sqrt(math.exp(float(lvn)))
    if not len(program):
        g = mu.unsqueeze(0)
        sigma = None
    else:
        g = nodes(mu, v, xs, program, theta, rowp)
    out = []
    for p in probs:
        p = float(p)
        if sigma is None:      # one Gaussian of its own width per row: bisect on the standardised variable
            sd = torch.sqrt(v.clamp_min(0.0) + math.exp(float(lvn)))
            lo, hi = torch.full_like(mu, -40.0), torch.full_like(mu, 40.0)
            one = torch.ones(1, dtype=torch.float64)
            f = lambda z: _signed(torch.zeros(1, z.numel(), dtype=torch.float64), one, 1.0, z, p)[0]
        else:
            lo, hi = g.min(0).values - 40.0 * sigma, g.max(0).values + 40.0 * sigma
            f = lambda t: _signed(g, wn, sigma, t, p)[0]
        for _ in range(4000):
            mid = 0.5 * (lo + hi)
            stuck = (mid <= lo) | (mid >= hi)
            if bool(stuck.all()):
                break
            below = f(mid) < 0.0
            lo = torch.where(~stuck & below, mid, lo)
            hi = torch.where(~stuck & ~below, mid, hi)
        t = 0.5 * (lo + hi)
        out.append(mu + t * sd if sigma is None else t)
    return torch.stack(out)


def cdf(mu, v, lvn, Y, xs, wn, program, theta, rowp=None):
    """(cdf, sf) at Y per row."""
    if not len(program):
        sd = torch.sqrt(v.clamp_min(0.0) + math.exp(float(lvn)))
        lower, upper, _ = tails(torch.zeros(1, mu.numel(), dtype=torch.float64), torch.ones(1, dtype=torch.float64), 1.0,
                                (Y - mu) / sd)
        return lower, upper
    g = nodes(mu, v, xs, program, theta, rowp)
    lower, upper, _ = tails(g, wn, math.sqrt(math.exp(float(lvn))), Y)
    return lower, upper
