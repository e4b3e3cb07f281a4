"""Torch restatement of the full-covariance kernels (csrc/tgp_cov.hip) for the tests, float64 on whatever device the inputs
live on: the covariance element function with its max(d2, 1e-30) clamp, A = L^-1 K(Z, X), W = L_q L_q^T - I,
mu = A^T m, Sigma = K(X, X) + A^T W A (its strict upper triangle mirrored from the lower one, as the kernel writes it), and
the joint draw mu + eps chol(Sigma + jitter I)^T."""
import math

import torch
import torch.nn.functional as F


def kernel_matrix(X1, X2, raw_ls, raw_os, kernel="scale_rbf"):
    """K(X1, X2) from the squared scaled distance summed dimension by dimension (no centred expansion)."""
    ils = 1.0 / F.softplus(raw_ls.reshape(-1))
    s2 = F.softplus(raw_os.reshape(()))
    d2 = (((X1 * ils).unsqueeze(1) - (X2 * ils).unsqueeze(0)) ** 2).sum(-1)
    if kernel == "scale_matern32":
        ar = math.sqrt(3.0) * torch.sqrt(d2.clamp_min(1e-30))
        return s2 * (1.0 + ar) * torch.exp(-ar)
    assert kernel == "scale_rbf", kernel
    return s2 * torch.exp(-0.5 * d2)


def operands(X, Z, raw_ls, raw_os, m, Lam, jitter=0.0, kernel="scale_rbf"):
    """(A, W): A = L^-1 K(Z, X) with L L^T = K(Z, Z) + jitter I;  W = tril(Lam) tril(Lam)^T - I."""
    M = Z.shape[0]
    eye = torch.eye(M, dtype=X.dtype, device=X.device)
    L = torch.linalg.cholesky(kernel_matrix(Z, Z, raw_ls, raw_os, kernel) + jitter * eye)
    A = torch.linalg.solve_triangular(L, kernel_matrix(Z, X, raw_ls, raw_os, kernel), upper=False)
    Lq = torch.tril(Lam)
    return A, Lq @ Lq.t() - eye


def qf_cov(X, Z, raw_ls, raw_os, m, Lam, jitter=0.0, kernel="scale_rbf"):
    """mu (N), Sigma (N, N); Sigma is symmetric by construction (lower triangle mirrored)."""
    A, W = operands(X, Z, raw_ls, raw_os, m, Lam, jitter, kernel)
    mu = A.t() @ m.reshape(-1)
    full = kernel_matrix(X, X, raw_ls, raw_os, kernel) + A.t() @ (W @ A)
    low = torch.tril(full)
    return mu, low + torch.tril(full, -1).t()


def joint_draw(mu, Sigma, eps, jitter=0.0):
    """(F0 (S, N) = mu + eps L^T, L = chol(Sigma + jitter I))."""
    N = Sigma.shape[0]
    L = torch.linalg.cholesky(Sigma + jitter * torch.eye(N, dtype=Sigma.dtype, device=Sigma.device))
    return mu.reshape(1, -1) + eps @ L.t(), L
