"""Torch restatement of the input-gradient kernels (csrc/tgp_xgrad.hip, k_pred_mgrad of csrc/tgp_quantile.hip) for the tests,
float64 on whatever device the inputs live on.  The four covariance functions as k(d2) with the weight k_g = -2 dk/d(d2) and the
max(d2, 1e-30) clamp of the device code (DESIGN.md "The covariance family"), then
  J[n,m,d] = -k_g(d2_nm) (x_nd - z_md) / l_d^2,   a = L^-T m,   U = L^-T W L^-1 K(Z, X),
  dmu[n,d] = sum_m J[n,m,d] a_m,   dv[n,d] = 2 sum_m J[n,m,d] U_mn,
and the partials of the predictive moments in mu and v through the flow.  Nothing here uses autograd on the kernels; the flow's
derivative G' is taken elementwise from the oracle's flow_forward (the one place the restatement leans on autograd)."""
import math

import torch
import torch.nn.functional as F

from oracle import tgp_oracle as orc

KERNELS = ("scale_rbf", "scale_matern32", "scale_matern52", "scale_rq")


def _scaled_d2(X1, X2, raw_ls):
    ils = 1.0 / F.softplus(raw_ls.reshape(-1))
    diff = (X1 * ils).unsqueeze(1) - (X2 * ils).unsqueeze(0)      # (N1, N2, D): formed directly, an equal pair gives exact zeros
    return diff, (diff ** 2).sum(-1), ils


def cov_pair(d2, s2, kernel, alpha=None):
    """(k, k_g) at the squared scaled distance d2: the table of DESIGN.md, with r = sqrt(max(d2, 1e-30))."""
    if kernel == "scale_rbf":
        k = s2 * torch.exp(-0.5 * d2)
        return k, k
    if kernel == "scale_matern32":
        ar = math.sqrt(3.0) * torch.sqrt(d2.clamp_min(1e-30))
        e = torch.exp(-ar)
        return s2 * (1.0 + ar) * e, 3.0 * s2 * e
    if kernel == "scale_matern52":
        r = torch.sqrt(d2.clamp_min(1e-30))
        ar = math.sqrt(5.0) * r
        e = torch.exp(-ar)
        return s2 * (1.0 + ar + (5.0 / 3.0) * r * r) * e, (5.0 / 3.0) * s2 * (1.0 + ar) * e
    assert kernel == "scale_rq" and alpha is not None, kernel
    base = 1.0 + d2 / (2.0 * alpha)
    return s2 * base ** (-alpha), s2 * base ** (-alpha - 1.0)


def kernel_matrix(X1, X2, raw_ls, raw_os, kernel="scale_rbf", alpha=None):
    """K(X1, X2); raw_os holds the raw output scale in its first entry (the RQ kernel's alpha is passed apart)."""
    _, d2, _ = _scaled_d2(X1, X2, raw_ls)
    return cov_pair(d2, F.softplus(raw_os.reshape(-1)[0]), kernel, alpha)[0]


def kernel_jacobian(X, Z, raw_ls, raw_os, kernel="scale_rbf", alpha=None):
    """J (N, M, D) = dk(x_n, z_m) / dx_nd."""
    diff, d2, ils = _scaled_d2(X, Z, raw_ls)
    kg = cov_pair(d2, F.softplus(raw_os.reshape(-1)[0]), kernel, alpha)[1]
    return -kg.unsqueeze(-1) * diff * ils


def operands(X, Z, raw_ls, raw_os, m, Lam, jitter=0.0, kernel="scale_rbf", alpha=None):
    """(a (M), U (M, N)): a = L^-T m, U = L^-T W L^-1 K(Z, X) with L L^T = K(Z, Z) + jitter I, W = tril(Lam) tril(Lam)^T - I."""
    M = Z.shape[0]
    eye = torch.eye(M, dtype=X.dtype, device=X.device)
    L = torch.linalg.cholesky(kernel_matrix(Z, Z, raw_ls, raw_os, kernel, alpha) + jitter * eye)
    A = torch.linalg.solve_triangular(L, kernel_matrix(Z, X, raw_ls, raw_os, kernel, alpha), upper=False)
    Lq = torch.tril(Lam)
    U = torch.linalg.solve_triangular(L.t(), (Lq @ Lq.t() - eye) @ A, upper=True)
    a = torch.linalg.solve_triangular(L.t(), m.reshape(-1, 1), upper=True).reshape(-1)
    return a, U


def qf_moments(X, Z, raw_ls, raw_os, m, Lam, jitter=0.0, kernel="scale_rbf", alpha=None):
    """mu (N), v (N) in the form the Jacobians differentiate: mu_n = sum_m k_nm a_m, v_n = s2 + sum_m k_nm U_mn."""
    a, U = operands(X, Z, raw_ls, raw_os, m, Lam, jitter, kernel, alpha)
    K = kernel_matrix(X, Z, raw_ls, raw_os, kernel, alpha)
    return K @ a, F.softplus(raw_os.reshape(-1)[0]) + (K * U.t()).sum(1)


def qf_input_grad(X, Z, raw_ls, raw_os, m, Lam, jitter=0.0, kernel="scale_rbf", alpha=None):
    """(dmu, dv), each (N, D)."""
    a, U = operands(X, Z, raw_ls, raw_os, m, Lam, jitter, kernel, alpha)
    J = kernel_jacobian(X, Z, raw_ls, raw_os, kernel, alpha)
    return torch.einsum("nmd,m->nd", J, a), 2.0 * torch.einsum("nmd,mn->nd", J, U)


def flow_value_and_slope(f, program, theta, rowp=None):
    """(G(f), G'(f)) elementwise for f of shape (S, N): the oracle's flow and its derivative in f."""
    with torch.enable_grad():
        fr = f.detach().clone().requires_grad_(True)
        g = orc.flow_forward(fr, program, theta.detach(), rowp)
        (gp,) = torch.autograd.grad(g.sum(), fr)
    return g.detach(), gp


def moment_partials(mu, v, program, theta, xs, ws, rowp=None):
    """(dm1, dm2), each (2, N): row 0 the partial in mu, row 1 the partial in v, of m1 = sum wn g and m2 = sum wn g^2 - m1^2 (+ the
    noise, a constant).  A row with v <= 0 counts as v = 0: its v-partials are zeros.  The empty program: (1, 0), (0, 1)."""
    n = mu.numel()
    if program is None or len(program) == 0:
        one, zero = torch.ones(n, dtype=mu.dtype, device=mu.device), torch.zeros(n, dtype=mu.dtype, device=mu.device)
        return torch.stack((one, zero)), torch.stack((zero, (v > 0).to(mu.dtype)))
    S = xs.numel()
    wn = (ws / math.sqrt(math.pi)).reshape(S, 1)
    vc = v.clamp_min(0.0)
    sq = torch.sqrt(2.0 * vc)
    g, gp = flow_value_and_slope(sq.reshape(1, n) * xs.reshape(S, 1) + mu.reshape(1, n), program, theta, rowp)
    inv = torch.where(v > 0, 1.0 / sq.clamp_min(1e-300), torch.zeros_like(sq))
    xcol = xs.reshape(S, 1)
    m1 = (wn * g).sum(0)
    d1m, d1v = (wn * gp).sum(0), (wn * gp * xcol).sum(0) * inv
    d2m = 2.0 * (wn * g * gp).sum(0) - 2.0 * m1 * d1m
    d2v = 2.0 * (wn * g * gp * xcol).sum(0) * inv - 2.0 * m1 * d1v
    return torch.stack((d1m, d1v)), torch.stack((d2m, d2v))
