"""Torch restatement of the CRPS kernels (csrc/tgp_quantile.hip: k_pred_crps, k_crps_gauss) for the tests, float64 on the CPU.

    a(z) = z erf(z / sqrt 2) + sqrt(2 / pi) exp(-z^2 / 2)
    T1 = sigma sum_s wn_s a((y - g_s) / sigma)                                                      (E|Y - y|)
    T2 = sigma / sqrt(pi) sum_s wn_s^2 + sqrt(2) sigma sum_{s<t} wn_s wn_t a((g_s - g_t) / (sqrt(2) sigma))   (E|Y - Y'| / 2)
    CRPS = T1 - T2 = int (F(t) - 1{t >= y})^2 dt,   F the CDF of quantile_model.tails

`crps_parts` adds in the kernel's order.  T1 and sum wn^2: lane l of 16 adds the nodes l, l + 16, ... in that order, the 16
partials are joined by the butterfly (x[l] + x[l + 8], then + 4, + 2, + 1).  The pairs: pair k = 0 .. S (S - 1) / 2 - 1 is
(s, t) = (k mod S, (k mod S + k div S + 1) mod S) (cyclic offsets: each unordered pair once); with WAVES waves on a row, lane l
of wave w adds the pairs k = 16 w + l + 16 WAVES j, j = 0, 1, ... in that order, each wave's 16 partials are joined by the
butterfly and the waves' sums are added in the order w = 0, 1, ...  `crps_quadrature` shares nothing with it but
quantile_model.tails: composite Gauss-Legendre of F^2 left of y and (1 - F)^2 right of it.

`bound` is the accuracy bound every comparison is held to; it follows from the formula and the number format:
    |delta| <= (16 + S (S + 1) / 2) 2^-52 (T1 + T2) + 2 node_tol max(1, max_s |g_s|)
* every term is positive; n = S + S (S - 1) / 2 terms added in any order err by at most n ulp of their total, and each term
  carries a few ulp of its own from erf, exp and the rounding of z (|da/dz| <= 1 <= a / |z|);
* |dCRPS / dg_s| <= 2 wn_s; node_tol = 1e-9 (the project's value tolerance) when the two sides ran different flow code, else 0.
"""
import math

import numpy as np
import torch

import quantile_model as qm

WAVES = 4                 # CRPS_WAVES of the build
LANES = 16
SQRT1_2 = 0.70710678118654752440
SQRT2 = 1.41421356237309504880
SQRT_2_OVER_PI = 0.79788456080286535588
INV_SQRT_PI = 0.56418958354775628695
F64 = torch.float64


def a(z):
    return z * torch.erf(z * SQRT1_2) + SQRT_2_OVER_PI * torch.exp(-0.5 * z * z)


def _butterfly(x):
    """(16, N) -> (N,): x[l] + x[l + 8], then + 4, + 2, + 1."""
    for h in (8, 4, 2, 1):
        x = x[:h] + x[h:]
    return x[0]


def _dealt_sum(terms, waves):
    """terms (K, N) in index order -> (N,): the kernel's order for `waves` waves of 16 lanes (see the module docstring)."""
    K, N = terms.shape
    step = LANES * waves
    J = -(-K // step)
    x = torch.cat([terms, torch.zeros(J * step - K, N, dtype=F64)]).reshape(J, waves, LANES, N)
    acc = torch.zeros(waves, LANES, N, dtype=F64)
    for j in range(J):
        acc = acc + x[j]
    tot = _butterfly(acc[0])
    for w in range(1, waves):
        tot = tot + _butterfly(acc[w])
    return tot


def pair_indices(S):
    """(s, t) of the pairs k = 0 .. S (S - 1) / 2 - 1 in the kernel's numbering."""
    k = torch.arange(S * (S - 1) // 2)
    s = k % S
    return s, (s + k // S + 1) % S


def crps_parts(g, wn, sigma, y):
    """(crps, T1, T2), each (N,), from the node values g (S,N), the weights wn (S,), sigma and the targets y (N,)."""
    S, N = g.shape
    w = wn.unsqueeze(1)
    t1 = _dealt_sum(w * a((y.unsqueeze(0) - g) / sigma), 1)
    w2 = _dealt_sum((w * w).expand(S, N), 1)
    sig2 = SQRT2 * sigma
    if S > 1:
        s, t = pair_indices(S)
        pr = _dealt_sum((wn[s] * wn[t]).unsqueeze(1) * a((g[s] - g[t]) / sig2), WAVES)
    else:
        pr = torch.zeros(N, dtype=F64)
    T1 = sigma * t1
    T2 = sigma * INV_SQRT_PI * w2 + sig2 * pr
    return T1 - T2, T1, T2


def gauss_parts(mu, v, lvn, y):
    """The closed form of one Gaussian (TGP_LIK_GAUSS / the empty program): sd (a(z) - 1 / sqrt pi) as T1 - T2."""
    sd = torch.sqrt(v.clamp_min(0.0) + math.exp(float(lvn)))
    T1 = sd * a((y - mu) / sd)
    T2 = sd * INV_SQRT_PI
    return T1 - T2, T1, T2


def crps(mu, v, lvn, y, xs, wn, program, theta, rowp=None):
    """(crps, T1, T2) as tgp_predict_crps_f64 returns them."""
    if not len(program):
        return gauss_parts(mu, v, lvn, y)
    return crps_parts(qm.nodes(mu, v, xs, program, theta, rowp), wn, math.sqrt(math.exp(float(lvn))), y)


def bound(S, T1, T2, gmax=None, node_tol=0.0):
    """The module docstring's bound, per row."""
    b = (16.0 + S * (S + 1) / 2.0) * 2.0 ** -52 * (T1 + T2)
    if node_tol:
        b = b + 2.0 * node_tol * gmax.clamp_min(1.0)
    return b


def quadrature_rule(g, sigma, y, panels=400, order=16, reach=12.0):
    """Abscissae and weights of the composite Gauss-Legendre rule: (t_lo, w_lo, t_hi, w_hi), each (panels * order, N) --
    [min(g, y) - reach sigma, y] and [y, max(g, y) + reach sigma] per row, `panels` equal panels a side."""
    x, w = np.polynomial.legendre.leggauss(order)
    x, w = torch.tensor(x, dtype=F64), torch.tensor(w, dtype=F64)
    lo = torch.minimum(g.min(0).values, y) - reach * sigma
    hi = torch.maximum(g.max(0).values, y) + reach * sigma

    def side(a_, b_):
        h = (b_ - a_) / panels                                                    # (N,)
        left = a_.unsqueeze(0) + torch.arange(panels, dtype=F64).unsqueeze(1) * h.unsqueeze(0)       # (panels, N)
        t = left.unsqueeze(1) + 0.5 * h.reshape(1, 1, -1) * (x.reshape(1, -1, 1) + 1.0)
        wt = (0.5 * h.reshape(1, 1, -1) * w.reshape(1, -1, 1)).expand_as(t)
        return t.reshape(panels * order, -1), wt.reshape(panels * order, -1)

    t_lo, w_lo = side(lo, y)
    t_hi, w_hi = side(y, hi)
    return t_lo, w_lo, t_hi, w_hi


def crps_quadrature(g, wn, sigma, y, panels=400, order=16, chunk=400):
    """int (F - 1{t >= y})^2 dt per row: the lower tail squared left of y, the upper tail squared right of it (each from
    quantile_model.tails' own sum, so neither side subtracts from 1)."""
    S, N = g.shape
    t_lo, w_lo, t_hi, w_hi = quadrature_rule(g, sigma, y, panels, order)
    out = torch.zeros(N, dtype=F64)
    for t, w, which in ((t_lo, w_lo, 0), (t_hi, w_hi, 1)):
        for c0 in range(0, t.shape[0], chunk):
            tc = t[c0:c0 + chunk]                                                 # (K, N)
            K = tc.shape[0]
            tail = qm.tails(g.repeat(1, K), wn, sigma, tc.reshape(-1))[which].reshape(K, N)
            out = out + (w[c0:c0 + chunk] * tail * tail).sum(0)
    return out


def poisson_crps(pmf, y):
    """sum_k (cdf_k - 1{k >= y})^2 over the counts k = 0 .. pmf.shape[1] - 1, pmf (N, K + 1), y (N,)."""
    cdf = pmf.cumsum(1)
    k = torch.arange(pmf.shape[1], dtype=pmf.dtype, device=pmf.device).unsqueeze(0)
    return ((cdf - (k >= y.reshape(-1, 1).to(pmf.dtype)).to(pmf.dtype)) ** 2).sum(1)
