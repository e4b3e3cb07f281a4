"""Torch restatement of the unwhitened q(u) parameterisation (csrc/tgp_unwhiten.hip and the host logic on top of it) for the
tests, float64 on whatever device the inputs live on, differentiable by autograd:

    L L^T = K(Z, Z) + jitter I,   m_w = L^-1 m,   Lam_w = L^-1 tril(L_q)

q(f) of the unwhitened model = the whitened q(f) at (m_w, Lam_w); KL(q(u) || N(0, L L^T)) = the whitened KL at (m_w, Lam_w)."""
import torch

import fullcov_model as fm

KL_PRIOR_JITTERS = tuple(1e-8 * (10 ** i) for i in range(5))


def factor(Z, raw_ls, raw_os, jitter=0.0, kernel="scale_rbf"):
    M = Z.shape[0]
    K = fm.kernel_matrix(Z, Z, raw_ls, raw_os, kernel) + jitter * torch.eye(M, dtype=Z.dtype, device=Z.device)
    return torch.linalg.cholesky(K)


def unwhiten(Z, raw_ls, raw_os, m, L_q, jitter=0.0, kernel="scale_rbf"):
    """(m_w (M), Lam_w (M, M) lower, L)."""
    L = factor(Z, raw_ls, raw_os, jitter, kernel)
    m_w = torch.linalg.solve_triangular(L, m.reshape(-1, 1), upper=False).reshape(-1)
    Lam_w = torch.linalg.solve_triangular(L, torch.tril(L_q), upper=False)
    return m_w, Lam_w, L


def kl_whitened(m, Lam):
    """sparse_MF_SP.py:406-431."""
    Lq = torch.tril(Lam)
    return 0.5 * (-torch.log(torch.diagonal(Lq) ** 2).sum() + (m * m).sum() + (Lq * Lq).sum() - float(m.numel()))


def kld(Z, raw_ls, raw_os, m, L_q, jitter=KL_PRIOR_JITTERS[0], kernel="scale_rbf"):
    """KL(N(m, L_q L_q^T) || N(0, K(Z, Z) + jitter I)): sparse_MF_SP.py:433-453 with add_jitter_MultivariateNormal's prior."""
    m_w, Lam_w, _ = unwhiten(Z, raw_ls, raw_os, m, L_q, jitter, kernel)
    return kl_whitened(m_w, Lam_w)


def qf_moments(X, Z, raw_ls, raw_os, m, L_q, jitter=0.0, kernel="scale_rbf"):
    """mu, v (N) of sparse_MF_SP.py:357-360, :386-389: the whitened moments at (m_w, Lam_w)."""
    m_w, Lam_w, L = unwhiten(Z, raw_ls, raw_os, m, L_q, jitter, kernel)
    A = torch.linalg.solve_triangular(L, fm.kernel_matrix(Z, X, raw_ls, raw_os, kernel), upper=False)
    kxx = torch.nn.functional.softplus(raw_os.reshape(())) * torch.ones(X.shape[0], dtype=X.dtype, device=X.device)
    return A.t() @ m_w, kxx - (A * A).sum(0) + ((Lam_w.t() @ A) ** 2).sum(0)


def qf_cov(X, Z, raw_ls, raw_os, m, L_q, jitter=0.0, kernel="scale_rbf"):
    """Full covariance of the unwhitened model: tests/fullcov_model.py at (m_w, Lam_w)."""
    m_w, Lam_w, _ = unwhiten(Z, raw_ls, raw_os, m, L_q, jitter, kernel)
    return fm.qf_cov(X, Z, raw_ls, raw_os, m_w, Lam_w, jitter, kernel)


def elbo(g, params=None, jitter=0.0, jitter_p=KL_PRIOR_JITTERS[0]):
    """(ELBO, ELL, KLD) of a Gaussian-likelihood fixture `g` (conftest.load_golden) at `params` (default: the fixture's): the
    oracle's likelihood terms on the moments above."""
    from oracle import tgp_oracle as orc
    p = g["params"] if params is None else params
    kern = g["kernel"]
    mu, v = qf_moments(g["X"], p["Z"], p["raw_lengthscale"], p["raw_outputscale"], p["m"], p["Lam"], jitter, kern)
    y = g["Y"].reshape(-1)
    if g["program"] is None:
        ell = orc.ell_gauss(y, mu, v, p["log_var_noise"])
    else:
        ell = orc.ell_flow(y, mu, v, p["log_var_noise"], g["program"], p["theta"], g["xs"], g["ws"])
    ell = float(g["N_total"]) / g["X"].shape[0] * ell
    kl = kld(p["Z"], p["raw_lengthscale"], p["raw_outputscale"], p["m"], p["Lam"], jitter_p, kern)
    return ell - kl, ell, kl


def elbo_and_grads(g):
    leaves = {k: v.detach().clone().requires_grad_(True) for k, v in g["params"].items()}
    out = elbo(g, leaves)
    out[0].backward()
    return tuple(o.detach() for o in out), {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in leaves.items()}
