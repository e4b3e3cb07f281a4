"""CPU restatement of pathwise posterior function draws (Wilson et al. 2020, "Efficiently sampling functions from Gaussian process
posteriors") for the whitened sparse GP, in float64 torch: test infrastructure only.

With l = softplus(raw_ls), s2 = softplus(raw_os), K = K_ZZ + jitter I = L L^T, Lam = tril(Lam), amp = sqrt(s2 / R2) and
a_j(x) = sum_d omega[j,d] x_d / l_d summed in the order of d:
    phi_j(x) = amp cos a_j(x),   phi_{R2+j}(x) = amp sin a_j(x)                    j < R2
    u_s      = L (m + Lam eps_s)
    nu_s     = K^-1 (u_s - Phi_Z W_s^T) = L^-T (m + Lam eps_s - L^-1 Phi_Z W_s^T)
    f0_s(x)  = sum_{j < 2 R2} phi_j(x) W[s,j] + sum_{i < M} k(x, z_i) nu_s[i]
coef (2 R2 + M, S): rows [0, 2 R2) hold amp W[s,j], rows [2 R2, 2 R2 + M) hold nu_s[i].  The kernel is the oracle's
(tests/optqu_model.py `kernel`: exact pairwise differences of the scaled rows, Matern-3/2 with the max(d^2, 1e-30) clamp, as
cov_value evaluates it).

Every test input comes from `make_case`; `PATHWISE_CPU` holds, per case, what this file measured (python tests/pathwise_model.py).
"""
import math

import torch
from torch.nn.functional import softplus

from optqu_model import kernel

F64 = torch.float64
KINDS = ("scale_rbf", "scale_matern32")

# (N, D, M, R2, S, kernel): every N of {1, 63, 65, 257, 1000}, D of {1, 4, 13, 16} (and 8: the third width of the kernels'
# coordinate loops), M of {1, 16, 65, 129, 200} (both factorisation routes), R2 of {1, 15, 64, 130, 1024}, S of {1, 3, 64, 65, 100}
# (and 130: the widest sample tiling of the row kernel) at least once, both kernels; and four cases of N = 16 450, above the
# row count up to which the row kernel gives a workgroup 16 rows instead of 64: one per sample tiling of the 64-row form
CASES = [
    (1, 1, 1, 1, 1, "scale_rbf"),
    (1, 4, 16, 15, 3, "scale_matern32"),
    (63, 1, 16, 64, 3, "scale_matern32"),
    (63, 4, 65, 130, 64, "scale_rbf"),
    (65, 13, 129, 15, 65, "scale_rbf"),
    (65, 16, 200, 64, 100, "scale_matern32"),
    (65, 8, 65, 130, 130, "scale_rbf"),
    (257, 4, 129, 64, 1, "scale_matern32"),
    (257, 13, 200, 130, 3, "scale_rbf"),
    (257, 16, 16, 1024, 64, "scale_rbf"),
    (257, 8, 129, 15, 100, "scale_matern32"),
    (1000, 4, 200, 1024, 100, "scale_matern32"),
    (1000, 13, 65, 1, 65, "scale_matern32"),
    (1000, 16, 129, 130, 64, "scale_rbf"),
    (1000, 1, 1, 15, 100, "scale_rbf"),
    (16450, 4, 16, 15, 3, "scale_rbf"),
    (16450, 8, 65, 15, 64, "scale_matern32"),
    (16450, 16, 16, 15, 100, "scale_rbf"),
    (16450, 13, 16, 1, 130, "scale_matern32"),
]
COND_MAX = 1e5

# Measured by this file on the CPU, float64:
#   cond    cond(K_ZZ), jitter 0
#   interp  max |f0_s(Z) - u_s| / max |u|
#   coef    max |coef|            F0   max |F0|
PATHWISE_CPU = {
    (1, 1, 1, 1, 1, 'scale_rbf'): dict(cond=1.0e+00, interp=1.1e-15, coef=8.2e-01, F0=1.7e-02),
    (1, 4, 16, 15, 3, 'scale_matern32'): dict(cond=3.3e+00, interp=1.7e-16, coef=7.1e+00, F0=1.0e+00),
    (63, 1, 16, 64, 3, 'scale_matern32'): dict(cond=6.0e+00, interp=4.0e-16, coef=5.3e+00, F0=4.4e+00),
    (63, 4, 65, 130, 64, 'scale_rbf'): dict(cond=4.8e+00, interp=7.2e-16, coef=6.6e+00, F0=6.2e+00),
    (65, 13, 129, 15, 65, 'scale_rbf'): dict(cond=1.6e+02, interp=1.9e-15, coef=1.2e+01, F0=4.9e+00),
    (65, 16, 200, 64, 100, 'scale_matern32'): dict(cond=7.3e+01, interp=1.7e-15, coef=9.1e+00, F0=4.8e+00),
    (65, 8, 65, 130, 130, 'scale_rbf'): dict(cond=1.5e+02, interp=1.7e-15, coef=1.7e+01, F0=4.7e+00),
    (257, 4, 129, 64, 1, 'scale_matern32'): dict(cond=3.2e+00, interp=3.7e-16, coef=4.5e+00, F0=2.9e+00),
    (257, 13, 200, 130, 3, 'scale_rbf'): dict(cond=2.0e+02, interp=3.0e-15, coef=9.3e+00, F0=3.9e+00),
    (257, 16, 16, 1024, 64, 'scale_rbf'): dict(cond=4.9e+00, interp=6.1e-16, coef=6.0e+00, F0=4.5e+00),
    (257, 8, 129, 15, 100, 'scale_matern32'): dict(cond=1.0e+02, interp=2.4e-15, coef=1.0e+01, F0=5.5e+00),
    (1000, 4, 200, 1024, 100, 'scale_matern32'): dict(cond=5.0e+00, interp=1.1e-15, coef=8.5e+00, F0=5.3e+00),
    (1000, 13, 65, 1, 65, 'scale_matern32'): dict(cond=2.8e+01, interp=1.0e-15, coef=7.1e+00, F0=3.6e+00),
    (1000, 16, 129, 130, 64, 'scale_rbf'): dict(cond=1.3e+02, interp=2.0e-15, coef=9.8e+00, F0=4.9e+00),
    (1000, 1, 1, 15, 100, 'scale_rbf'): dict(cond=1.0e+00, interp=8.0e-16, coef=3.8e+00, F0=3.3e+00),
    (16450, 4, 16, 15, 3, 'scale_rbf'): dict(cond=2.6e+00, interp=3.9e-16, coef=3.5e+00, F0=3.6e+00),
    (16450, 8, 65, 15, 64, 'scale_matern32'): dict(cond=4.9e+01, interp=8.7e-16, coef=8.0e+00, F0=5.9e+00),
    (16450, 16, 16, 15, 100, 'scale_rbf'): dict(cond=3.9e+00, interp=6.4e-16, coef=5.7e+00, F0=5.5e+00),
    (16450, 13, 16, 1, 130, 'scale_matern32'): dict(cond=5.0e+00, interp=6.6e-16, coef=9.0e+00, F0=7.1e+00),
}

# Draw covariance against the exact q(f) covariance K_XX + A^T (Lam Lam^T - I) A at N = 300, D = 4, M = 40 (seed 0), largest
# entry error / s2, measured by this file on the CPU (tests/test_pathwise_host.py asserts each within a margin of 2 x):
#   (kernel, R2): error
DRAW_COV_CPU = {
    ('scale_rbf', 256): 1.797e-01,   # cond 5.2e+00
    ('scale_rbf', 2048): 5.677e-02,   # cond 5.2e+00
    ('scale_matern32', 256): 1.882e-01,   # cond 3.3e+00
    ('scale_matern32', 2048): 5.875e-02,   # cond 3.3e+00
}
# Phi_X Phi_X^T against K_XX with pathwise.spectral_frequencies (generator seed 0), same inputs, largest entry error / s2
SPECTRAL_CPU = {
    ('scale_rbf', 256): 1.767e-01,
    ('scale_rbf', 2048): 5.883e-02,
    ('scale_matern32', 256): 1.811e-01,
    ('scale_matern32', 2048): 7.663e-02,
}


def inv_softplus(x):
    return math.log(math.expm1(x))


def make_case(N, D, M, R2, S, kind, seed=0):
    """Seeded inputs.  Length-scales around 1.5 up to D = 7 and around 0.6 sqrt(D) from D = 8.  Z: up to D = 4 a jittered grid
    along axis 0 with a spacing of 1.2 length-scales (standard normal in the other axes) -- random points in so few dimensions
    come arbitrarily close and cond(K_ZZ) explodes --, standard normal draws above.  X: standard normal draws scaled to cover Z.
    s2 = softplus(0.6); m, Lam (lower, positive diagonal) of order one."""
    g = torch.Generator().manual_seed(1000003 * seed + 7919 * N + 131 * M + 17 * D + 3 * R2 + 5 * S + (1 if kind == KINDS[1] else 0))
    ls = 1.5 if D < 8 else 0.6 * math.sqrt(D)
    raw_ls = torch.full((D,), inv_softplus(ls), dtype=F64) + 0.1 * torch.randn(D, dtype=F64, generator=g)
    raw_os = torch.tensor([0.6], dtype=F64)
    Z = torch.randn(M, D, dtype=F64, generator=g)
    if D <= 4:
        step = 1.2 * float(softplus(raw_ls[0]))
        Z[:, 0] = step * (torch.arange(M, dtype=F64) - 0.5 * (M - 1)) + 0.15 * step * torch.randn(M, dtype=F64, generator=g)
    X = torch.randn(N, D, dtype=F64, generator=g)
    X[:, 0] *= max(1.0, float(Z[:, 0].abs().max()) / 2.0)
    m = torch.randn(M, dtype=F64, generator=g)
    Lam = torch.tril(0.3 * torch.randn(M, M, dtype=F64, generator=g) / math.sqrt(M))
    Lam.diagonal().copy_(0.5 + torch.rand(M, dtype=F64, generator=g))
    omega = spectral_frequencies(kind, R2, D, g)
    W = torch.randn(S, 2 * R2, dtype=F64, generator=g)
    eps = torch.randn(S, M, dtype=F64, generator=g)
    return dict(X=X, Z=Z, raw_ls=raw_ls, raw_os=raw_os, m=m, Lam=Lam, omega=omega, W=W, eps=eps, kernel=kind, jitter=0.0,
                N=N, D=D, M=M, R2=R2, S=S, s2=float(softplus(raw_os)))


def spectral_frequencies(kind, R2, D, g):
    """omega (R2, D) of the unit-length-scale kernel: N(0, I) for the RBF; g sqrt(3 / c), c ~ chi^2(3), for Matern-3/2."""
    om = torch.randn(R2, D, dtype=F64, generator=g)
    if kind == "scale_matern32":
        c = torch.randn(R2, 3, dtype=F64, generator=g).pow(2).sum(1, keepdim=True)
        om = om * torch.sqrt(3.0 / c)
    return om


def features(X, raw_ls, raw_os, omega):
    """Phi (N, 2 R2) = amp [cos a, sin a], a_j(x) summed in the order of d."""
    R2, D = omega.shape
    Xs = X * (1.0 / softplus(raw_ls)).reshape(1, -1)
    a = torch.zeros(X.shape[0], R2, dtype=F64)
    for d in range(D):
        a = a + Xs[:, d:d + 1] * omega[:, d].reshape(1, -1)
    amp = math.sqrt(float(softplus(raw_os)) / R2)
    return amp * torch.cat([torch.cos(a), torch.sin(a)], 1)


def k_zz(p, jitter=None):
    j = p["jitter"] if jitter is None else jitter
    return kernel(p["Z"], p["Z"], p["raw_ls"], p["raw_os"], p["kernel"]) + j * torch.eye(p["M"], dtype=F64)


def cond_K(p):
    return float(torch.linalg.cond(k_zz(p, 0.0)))


def inducing_values(p, eps=None, jitter=None):
    """u (M, S): u_s = L (m + Lam eps_s)."""
    L = torch.linalg.cholesky(k_zz(p, jitter))
    eps = p["eps"] if eps is None else eps
    return L @ (p["m"].reshape(-1, 1) + torch.tril(p["Lam"]) @ eps.T)


def coeff(p, W=None, eps=None, jitter=None):
    """coef (2 R2 + M, S)."""
    W = p["W"] if W is None else W
    eps = p["eps"] if eps is None else eps
    R2 = p["omega"].shape[0]
    amp = math.sqrt(float(softplus(p["raw_os"])) / R2)
    L = torch.linalg.cholesky(k_zz(p, jitter))
    PhiZ = features(p["Z"], p["raw_ls"], p["raw_os"], p["omega"])
    v = p["m"].reshape(-1, 1) + torch.tril(p["Lam"]) @ eps.T - torch.linalg.solve_triangular(L, PhiZ @ W.T, upper=False)
    nu = torch.linalg.solve_triangular(L.T, v, upper=True)
    return torch.cat([amp * W.T, nu], 0)


def evaluate(p, coef, X=None):
    """F0 (S, N) = the draws of coef on the rows of X."""
    X = p["X"] if X is None else X
    R2 = p["omega"].shape[0]
    amp = math.sqrt(float(softplus(p["raw_os"])) / R2)
    Phi = features(X, p["raw_ls"], p["raw_os"], p["omega"]) / amp
    Kxz = kernel(X, p["Z"], p["raw_ls"], p["raw_os"], p["kernel"])
    return (Phi @ coef[:2 * R2] + Kxz @ coef[2 * R2:]).T


def exact_cov(p, X=None):
    """K_XX + A^T (Lam Lam^T - I) A, A = L^-1 K_ZX: the covariance of q(f) on the rows of X."""
    X = p["X"] if X is None else X
    L = torch.linalg.cholesky(k_zz(p))
    A = torch.linalg.solve_triangular(L, kernel(p["Z"], X, p["raw_ls"], p["raw_os"], p["kernel"]), upper=False)
    Lq = torch.tril(p["Lam"])
    return kernel(X, X, p["raw_ls"], p["raw_os"], p["kernel"]) + A.T @ (Lq @ Lq.T - torch.eye(p["M"], dtype=F64)) @ A


def draw_cov(p):
    """J_w J_w^T + J_e J_e^T: the covariance of the draws on the rows of X, from the Jacobians of F0 with respect to (W, eps)
    recovered by feeding unit vectors (the draws are affine in both)."""
    R2, M = p["omega"].shape[0], p["M"]
    zero_w, zero_e = torch.zeros(1, 2 * R2, dtype=F64), torch.zeros(1, M, dtype=F64)
    base = evaluate(p, coeff(p, zero_w, zero_e))                                          # (1, N): the mean
    Jw = evaluate(p, coeff(p, torch.eye(2 * R2, dtype=F64), torch.zeros(2 * R2, M, dtype=F64))) - base
    Je = evaluate(p, coeff(p, torch.zeros(M, 2 * R2, dtype=F64), torch.eye(M, dtype=F64))) - base
    return Jw.T @ Jw + Je.T @ Je


def cov_case(kind, R2, seed=0, omega=None):
    """The inputs of the draw-covariance check: N = 300, D = 4, M = 40 -- the same X, Z and parameters at every R2; `omega`
    (R2, 4), or this file's own frequencies from a generator seeded with R2."""
    p = make_case(300, 4, 40, 1, 1, kind, seed)
    p["omega"] = spectral_frequencies(kind, R2, 4, torch.Generator().manual_seed(R2)) if omega is None else omega
    p["R2"] = R2
    return p


def spectral_error(p):
    """max |Phi_X Phi_X^T - K_XX| / s2 for the frequencies of p."""
    Phi = features(p["X"], p["raw_ls"], p["raw_os"], p["omega"])
    return float((Phi @ Phi.T - kernel(p["X"], p["X"], p["raw_ls"], p["raw_os"], p["kernel"])).abs().max() / p["s2"])


if __name__ == "__main__":
    print("PATHWISE_CPU = {")
    for c in CASES:
        p = make_case(*c)
        cf = coeff(p)
        F0 = evaluate(p, cf)
        u = inducing_values(p)
        interp = float((evaluate(p, cf, p["Z"]).T - u).abs().max() / u.abs().max())
        print("    %r: dict(cond=%.1e, interp=%.1e, coef=%.1e, F0=%.1e)," % (c, cond_K(p), interp, float(cf.abs().max()),
                                                                          float(F0.abs().max())))
    print("}\nDRAW_COV_CPU = {")
    for kind in KINDS:
        for R2 in (256, 2048):
            p = cov_case(kind, R2)
            err = float((draw_cov(p) - exact_cov(p)).abs().max() / p["s2"])
            print("    (%r, %d): %.3e,   # cond %.1e" % (kind, R2, err, cond_K(p)))
    print("}\nSPECTRAL_CPU = {")
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from tgp.pytorch_amd.pathwise import spectral_frequencies as product_frequencies
    for kind in KINDS:
        for R2 in (256, 2048):
            p = cov_case(kind, R2, omega=product_frequencies(kind, R2, 4, torch.Generator().manual_seed(0)))
            print("    (%r, %d): %.3e," % (kind, R2, spectral_error(p)))
    print("}")
