"""Torch restatement of the posterior derivative kernels for the tests, float64 on whatever device the inputs live on: the variance
of the derivative process under q(f) (k_xgrad_va / k_xgrad_vcol of csrc/tgp_xgrad.hip) and the input gradient of a pathwise draw
(k_pw_grad of csrc/tgp_pathwise.hip).  Closed form and vectorised; autograd appears only in the tests that hold these to it
(tests/test_derivative_host.py).

With l = softplus(raw_ls), K_ZZ + jitter I = L L^T, W = tril(Lam) tril(Lam)^T - I, B = L^-T W L^-1 and
J[n,m,d] = dk(x_n, z_m) / dx_nd = -k_g(d2_nm) (x_nd - z_md) / l_d^2 (input_grad_model.kernel_jacobian):
    Sigma(x, x') = k(x, x') + k(x, Z) B k(Z, x')
    dvar[n,d]    = k_g(0) / l_d^2 + sum_{m,m'} J[n,m,d] B[m,m'] J[n,m',d]          (the mixed derivative in x_d, x'_d at x' = x)
and, with the symbols of tests/pathwise_model.py (coef rows [0, R2) = amp W[s,j], [R2, 2 R2) = amp W[s,R2+j], [2 R2, ..) = nu_s):
    d f0_s(x) / dx_d = sum_{j < R2} (omega_jd / l_d) [ -sin a_j(x) coef[j,s] + cos a_j(x) coef[R2+j,s] ] + sum_i J[.,i,d] coef[2 R2+i,s]

`python tests/derivative_model.py` prints what LINK_GAP_CPU records."""
import torch
import torch.nn.functional as F

import input_grad_model as IG
import pathwise_model as PM

F64 = torch.float64

# k_g(0) / s2: cov_gweight at d2 = 0
KG0 = {"scale_rbf": 1.0, "scale_matern32": 3.0, "scale_matern52": 5.0 / 3.0, "scale_rq": 1.0}

# The link between the two halves (slope_var_fourier against slope_var at link_case's inputs: N = 65, D = 4, M = 20, seed 0):
# max over rows and inputs of |gap| / (k_g(0) / l_d^2), measured by this file on the CPU, float64.  The inducing-point update is
# exact, so the gap is that of the Fourier features' slope variance s2 / R2 sum_j omega_jd^2 / l_d^2 to the prior's.
# tests/test_derivative_host.py asserts each within a margin of 2 x and that the R2 = 2048 gap is below the R2 = 256 gap.
#   (kernel, R2): gap
LINK_GAP_CPU = {
    ('scale_rbf', 256): 1.299e-01,
    ('scale_rbf', 2048): 6.230e-02,
    ('scale_matern32', 256): 4.396e-01,
    ('scale_matern32', 2048): 1.908e-01,
}


def _factor(Z, raw_ls, raw_os, jitter, kernel, alpha):
    M = Z.shape[0]
    eye = torch.eye(M, dtype=Z.dtype, device=Z.device)
    return torch.linalg.cholesky(IG.kernel_matrix(Z, Z, raw_ls, raw_os, kernel, alpha) + jitter * eye), eye


def b_matrix(Z, raw_ls, raw_os, Lam, jitter=0.0, kernel="scale_rbf", alpha=None):
    """B = L^-T W L^-1 (M, M), symmetric."""
    L, eye = _factor(Z, raw_ls, raw_os, jitter, kernel, alpha)
    Linv = torch.linalg.solve_triangular(L, eye, upper=False)
    Lq = torch.tril(Lam)
    return Linv.t() @ (Lq @ Lq.t() - eye) @ Linv


def prior_slope_var(raw_ls, raw_os, kernel="scale_rbf"):
    """(D,): k_g(0) / l_d^2, the slope variance of the prior."""
    ils = 1.0 / F.softplus(raw_ls.reshape(-1))
    return KG0[kernel] * F.softplus(raw_os.reshape(-1)[0]) * ils * ils


def posterior_slope_var(X, Z, raw_ls, raw_os, Lam, jitter=0.0, kernel="scale_rbf", alpha=None):
    """(N, D): sum_{m,m'} J[n,m,d] B[m,m'] J[n,m',d] through A_d = L^-1 J_d^T and W, the form the kernels use."""
    L, eye = _factor(Z, raw_ls, raw_os, jitter, kernel, alpha)
    J = IG.kernel_jacobian(X, Z, raw_ls, raw_os, kernel, alpha)                     # (N, M, D)
    Lq = torch.tril(Lam)
    W = Lq @ Lq.t() - eye
    out = torch.empty(X.shape[0], X.shape[1], dtype=X.dtype, device=X.device)
    for d in range(X.shape[1]):
        A = torch.linalg.solve_triangular(L, J[:, :, d].t(), upper=False)          # (M, N)
        out[:, d] = (A * (W @ A)).sum(0)
    return out


def slope_var(X, Z, raw_ls, raw_os, m, Lam, jitter=0.0, kernel="scale_rbf", alpha=None):
    """dvar (N, D); never clamped.  (m does not enter: the signature is ops.qf_input_grad_var's.)"""
    return prior_slope_var(raw_ls, raw_os, kernel).reshape(1, -1) + posterior_slope_var(X, Z, raw_ls, raw_os, Lam, jitter, kernel,
                                                                                       alpha)


def rowwise_cov_posterior(X1, X2, Z, raw_ls, raw_os, Lam, jitter=0.0, kernel="scale_rbf", alpha=None):
    """(N,): k(x1_n, Z) B k(Z, x2_n), the posterior part of Sigma(x1_n, x2_n), for autograd in both arguments."""
    B = b_matrix(Z, raw_ls, raw_os, Lam, jitter, kernel, alpha)
    K1 = IG.kernel_matrix(X1, Z, raw_ls, raw_os, kernel, alpha)
    K2 = IG.kernel_matrix(X2, Z, raw_ls, raw_os, kernel, alpha)
    return ((K1 @ B) * K2).sum(1)


def _rowwise_d2(X1, X2, raw_ls):
    ils = 1.0 / F.softplus(raw_ls.reshape(-1))
    diff = (X1 - X2) * ils
    return diff, (diff ** 2).sum(-1), ils


def rowwise_cov_prior(X1, X2, raw_ls, raw_os, kernel="scale_rbf", alpha=None):
    """(N,): k(x1_n, x2_n).  For the kernels that are smooth in d2 at 0 (RBF, RQ) autograd can take its mixed second derivative
    at x2 = x1."""
    _, d2, _ = _rowwise_d2(X1, X2, raw_ls)
    return IG.cov_pair(d2, F.softplus(raw_os.reshape(-1)[0]), kernel, alpha)[0]


def rowwise_slope_prior(X1, X2, raw_ls, raw_os, kernel="scale_rbf", alpha=None):
    """(N, D): dk(x1_n, x2_n) / dx1_nd = -k_g(d2_n) (x1_nd - x2_nd) / l_d^2 -- the restated first derivative, which autograd
    differentiates once more in x2 (Matern-5/2: k holds an r^3 term whose second derivative autograd loses to cancellation at
    r = 0, while k_g is finite and differentiable there)."""
    diff, d2, ils = _rowwise_d2(X1, X2, raw_ls)
    kg = IG.cov_pair(d2, F.softplus(raw_os.reshape(-1)[0]), kernel, alpha)[1]
    return -kg.unsqueeze(-1) * diff * ils


def draw_grad(p, coef, X=None):
    """(S, N, D): the input gradients of the draws of coef on the rows of X (p: a pathwise_model case)."""
    X = p["X"] if X is None else X
    omega, raw_ls, raw_os = p["omega"].to(X.device), p["raw_ls"].to(X.device), p["raw_os"].to(X.device)
    R2, D = omega.shape
    ils = 1.0 / F.softplus(raw_ls.reshape(-1))
    Xs = X * ils.reshape(1, -1)
    a = torch.zeros(X.shape[0], R2, dtype=X.dtype, device=X.device)
    for d in range(D):                       # (summed in the order of d, as pathwise_model.features)
        a = a + Xs[:, d:d + 1] * omega[:, d].reshape(1, -1)
    wd = omega * ils.reshape(1, -1)                                                 # (R2, D): omega_jd / l_d
    cf = coef.to(X.device)
    four = torch.einsum("nj,jd,js->snd", -torch.sin(a), wd, cf[:R2]) + torch.einsum("nj,jd,js->snd", torch.cos(a), wd, cf[R2:2 * R2])
    J = IG.kernel_jacobian(X, p["Z"].to(X.device), raw_ls, raw_os, p["kernel"])    # (N, M, D)
    return four + torch.einsum("nmd,ms->snd", J, cf[2 * R2:])


def link_case(kind, R2, N=65, seed=0):
    """The inputs of the link check: N = 65, D = 4, M = 20 -- the same X, Z and parameters at every R2, pathwise_model's
    frequencies from a generator seeded with R2."""
    p = PM.make_case(N, 4, 20, 1, 1, kind, seed)
    p["omega"] = PM.spectral_frequencies(kind, R2, 4, torch.Generator().manual_seed(R2))
    p["R2"] = R2
    return p


def slope_var_fourier(p):
    """(N, D): the variance of the draws' slopes, sum_s (g_s - g_0)^2 over the 2 R2 + M draws whose [W, eps] rows are the unit
    vectors, g_0 the draw of the zero row (the draws are affine in [W, eps], whose entries are independent standard normals).
    Deterministic: nothing is sampled."""
    R2, M = p["omega"].shape[0], p["M"]
    n = 2 * R2 + M
    E = torch.cat([torch.eye(n, dtype=F64), torch.zeros(1, n, dtype=F64)], 0)
    g = draw_grad(p, PM.coeff(p, E[:, :2 * R2].contiguous(), E[:, 2 * R2:].contiguous()))
    return ((g[:n] - g[n:]) ** 2).sum(0)


def link_gap(p):
    """max |slope_var_fourier - slope_var| / (k_g(0) / l_d^2)."""
    exact = slope_var(p["X"], p["Z"], p["raw_ls"], p["raw_os"], p["m"], p["Lam"], p["jitter"], p["kernel"])
    return float(((slope_var_fourier(p) - exact).abs() / prior_slope_var(p["raw_ls"], p["raw_os"], p["kernel"]).reshape(1, -1)).max())


if __name__ == "__main__":
    print("LINK_GAP_CPU = {")
    for kind in PM.KINDS:
        for R2 in (256, 2048):
            print("    (%r, %d): %.3e," % (kind, R2, link_gap(link_case(kind, R2))))
    print("}")
