"""CPU restatement of the closed-form optimal q(u) (Titsias' collapsed bound) in float64 torch: test infrastructure only.

Whitened q(u) = N(m, Lam Lam^T), zero prior mean, sigma^2 = exp(log_var_noise), c = N_total / N, K = K_ZZ + j I = L L^T:
    C = K_ZX K_XZ,  b = K_ZX y,  B = I + (c / sigma^2) L^-1 C L^-T,  Lam* Lam*^T = B^-1,  m* = (c / sigma^2) B^-1 L^-1 b
stated two ways (`closed_form_rev`: one Cholesky of the index-reversed B; `closed_form_inv`: inv / solve / cholesky), the
Gaussian ELBO the training step computes (`elbo`, differentiable) and the dense collapsed bound (`dense_bound`, c = 1).

Every test input comes from `make_case`; `OPT_CPU` holds, per case, what this file measured on the CPU (tools: run this file).
"""
import math
import zlib

import torch
from torch.nn.functional import softplus

F64 = torch.float64
SQRT3 = math.sqrt(3.0)
# log(2 * float32(pi)): the constant of the project's Gaussian density (the reference's pi is a float32 tensor; TGP_LOG_2PI_REF).
# Both the ELBO and the dense bound below are stated with it: they are the same function of the same density.
LOG_2PI_REF = 1.8378770942368803

# name: (N, D, M, c, kernel, jitter)
CASES = {
    "m1_d1": (17, 1, 1, 1.0, "scale_rbf", 0.0),
    "m16": (257, 4, 16, 1.0, "scale_rbf", 0.0),
    "m63_mat": (300, 4, 63, 1.0, "scale_matern32", 0.0),
    "m64_c": (257, 13, 64, 2.5, "scale_rbf", 1e-6),
    "m65": (1100, 16, 65, 1.0, "scale_rbf", 0.0),
    "m100_c_mat": (1100, 4, 100, 2.5, "scale_matern32", 0.0),
    "m128": (300, 4, 128, 1.0, "scale_rbf", 1e-6),
    "m129": (257, 4, 129, 1.0, "scale_rbf", 0.0),
    "m129_c_mat": (1100, 8, 129, 2.5, "scale_matern32", 0.0),
    "m200": (300, 13, 200, 1.0, "scale_rbf", 0.0),
}
# the targets of a case as a model with a mean function or a warped likelihood hands them to the Gaussian step: the base case's
# inputs with Y replaced by Y - (X a + b) ("linear") or by T(Y), T one sinh-arcsinh + affine block ("warp")
VARIANTS = {"m16_linear": ("m16", "linear"), "m16_warp": ("m16", "warp")}
CASES.update({k: CASES[b] for k, (b, _) in VARIANTS.items()})
WARP_PROGRAM = [(1, 0, 0, 0), (0, 0, 2, 0)]           # (kind, K, poff, flags): TGP_FLOW_SAL, TGP_FLOW_AFFINE, shared parameters
WARP_THETA = (0.3, 1.2, 0.8, 0.1)                     # SAL a, b; affine a, b
DENSE_CASES = tuple(k for k, v in CASES.items() if v[0] <= 300 and v[3] == 1.0 and k not in VARIANTS)      # the dense bound: N <= 300, c = 1

# Measured by this file on the CPU (python tests/optqu_model.py), float64:
#   route   max relative discrepancy of (m*, Lam*, Lam* Lam*^T) between the two routes
#   ratio   max |g_m|, |tril g_Lam| of the ELBO at the optimum over the same at m = 0, Lam = I: the larger of the two routes
#   bound   relative error of the ELBO at the optimum against the dense collapsed bound (None: c != 1 or N > 300)
#   cond    cond(K_ZZ + j I)
OPT_CPU = {
    "m1_d1": dict(route=0.0e+00, ratio=4.1e-17, bound=1.7e-16, cond=1.0e+00),
    "m16": dict(route=5.9e-16, ratio=2.7e-16, bound=1.7e-16, cond=7.2e+00),
    "m63_mat": dict(route=2.5e-15, ratio=3.3e-15, bound=1.9e-16, cond=8.2e+01),
    "m64_c": dict(route=1.3e-15, ratio=1.1e-15, bound=None, cond=5.0e+00),
    "m65": dict(route=8.1e-16, ratio=9.2e-16, bound=None, cond=4.0e+00),
    "m100_c_mat": dict(route=7.9e-15, ratio=1.0e-14, bound=None, cond=1.0e+02),
    "m128": dict(route=3.2e-15, ratio=1.4e-13, bound=0.0e+00, cond=1.1e+04),
    "m129": dict(route=2.8e-15, ratio=8.1e-14, bound=3.5e-16, cond=8.1e+03),
    "m129_c_mat": dict(route=8.0e-15, ratio=5.6e-15, bound=None, cond=4.9e+01),
    "m200": dict(route=2.7e-15, ratio=5.8e-15, bound=0.0e+00, cond=2.5e+01),
    "m16_linear": dict(route=5.4e-16, ratio=3.9e-16, bound=None, cond=7.2e+00),
    "m16_warp": dict(route=6.9e-16, ratio=5.7e-16, bound=None, cond=7.2e+00),
}


def kernel(X1, X2, raw_ls, raw_os, kind):
    a = X1 / softplus(raw_ls).reshape(1, -1)
    b = X2 / softplus(raw_ls).reshape(1, -1)
    d2 = ((a.unsqueeze(1) - b.unsqueeze(0)) ** 2).sum(-1)
    s2 = softplus(raw_os).reshape(())
    if kind == "scale_matern32":
        r = d2.clamp_min(1e-30).sqrt()
        return s2 * (1.0 + SQRT3 * r) * torch.exp(-SQRT3 * r)
    return s2 * torch.exp(-0.5 * d2)


def make_case(name):
    """Seeded inputs of a case: X (N, D), Y (N), Z (M, D) standard normal draws (Y a smooth function of X plus noise)."""
    N, D, M, c, kind, jitter = CASES[name]
    base, variant = VARIANTS.get(name, (name, None))
    g = torch.Generator().manual_seed(zlib.crc32(base.encode()) % 100000)
    X = torch.randn(N, D, dtype=F64, generator=g)
    Z = torch.randn(M, D, dtype=F64, generator=g)
    w = torch.randn(D, dtype=F64, generator=g)
    Y = torch.sin(X @ w) + 0.3 * torch.randn(N, dtype=F64, generator=g)
    # length-scales near 0.85 up to D = 4 and near 0.5 sqrt(D) above: K_ZZ keeps off-diagonal mass, cond(K_ZZ) stays <= 1e5
    raw_ls = torch.full((D,), 0.3 if D <= 4 else 0.4 * math.sqrt(D), dtype=F64) + 0.2 * torch.randn(D, dtype=F64, generator=g)
    raw_os = torch.tensor([0.6], dtype=F64)
    lvn = torch.tensor([-1.5], dtype=F64)
    p = dict(name=name, X=X, Y=Y, Z=Z, raw_ls=raw_ls, raw_os=raw_os, lvn=lvn, c=c, N_total=c * N, kernel=kind, jitter=jitter,
             N=N, D=D, M=M, Y_raw=Y)
    if variant == "linear":
        p["mean_a"], p["mean_b"] = 0.3 * torch.randn(D, dtype=F64, generator=g), torch.tensor([0.2], dtype=F64)
        p["Y"] = Y - X @ p["mean_a"] - p["mean_b"]
    elif variant == "warp":
        sa, sb, aa, ab = WARP_THETA
        p["Y"] = aa * torch.sinh(sb * torch.asinh(Y) - sa) + ab
    return p


def k_zz(p):
    return kernel(p["Z"], p["Z"], p["raw_ls"], p["raw_os"], p["kernel"]) + p["jitter"] * torch.eye(p["M"], dtype=F64)


def cond_K(p):
    return float(torch.linalg.cond(k_zz(p)))


def c_and_b(p):
    Kzx = kernel(p["Z"], p["X"], p["raw_ls"], p["raw_os"], p["kernel"])
    return Kzx @ Kzx.T, Kzx @ p["Y"]


def _b_matrix(p):
    C, b = c_and_b(p)
    L = torch.linalg.cholesky(k_zz(p))
    Li = torch.linalg.solve_triangular(L, torch.eye(p["M"], dtype=F64), upper=False)
    s = p["c"] * math.exp(-float(p["lvn"]))
    Phi = Li @ C @ Li.T
    Phi = 0.5 * (Phi + Phi.T)
    return torch.eye(p["M"], dtype=F64) + s * Phi, Li @ b, s


def closed_form_rev(p):
    """(m*, Lam*) by the reversed Cholesky: J B J = L' L'^T, Lam* = J L'^-T J."""
    B, v1, s = _b_matrix(p)
    Lp = torch.linalg.cholesky(B.flip(0, 1))
    Lpi = torch.linalg.solve_triangular(Lp, torch.eye(p["M"], dtype=F64), upper=False)
    Lam = Lpi.T.flip(0, 1)
    return s * (Lam @ (Lam.T @ v1)), Lam


def closed_form_inv(p):
    """(m*, Lam*) by inv / solve: S* = B^-1, Lam* = chol(S*), m* = (c / sigma^2) B^-1 L^-1 b."""
    B, v1, s = _b_matrix(p)
    S = torch.linalg.inv(B)
    Lam = torch.linalg.cholesky(0.5 * (S + S.T))
    return s * torch.linalg.solve(B, v1), Lam


def elbo(p, m, Lam, Z=None, raw_ls=None, raw_os=None, lvn=None):
    """(ELBO, ELL, KLD) of the Gaussian step at q(u) = N(m, tril(Lam) tril(Lam)^T); differentiable in every argument."""
    Z = p["Z"] if Z is None else Z
    raw_ls = p["raw_ls"] if raw_ls is None else raw_ls
    raw_os = p["raw_os"] if raw_os is None else raw_os
    lvn = p["lvn"] if lvn is None else lvn
    N, M = p["N"], p["M"]
    K = kernel(Z, Z, raw_ls, raw_os, p["kernel"]) + p["jitter"] * torch.eye(M, dtype=F64)
    L = torch.linalg.cholesky(K)
    A = torch.linalg.solve_triangular(L, kernel(Z, p["X"], raw_ls, raw_os, p["kernel"]), upper=False)
    Lq = torch.tril(Lam)
    mu = A.T @ m
    v = softplus(raw_os).reshape(()) - (A * A).sum(0) + ((Lq.T @ A) ** 2).sum(0)
    eta = lvn.reshape(())
    ell = p["c"] * (-0.5 * N * LOG_2PI_REF - 0.5 * N * eta - 0.5 * torch.exp(-eta) * (((p["Y"] - mu) ** 2) + v).sum())
    kld = 0.5 * (-torch.log(torch.diagonal(Lq) ** 2).sum() + (m * m).sum() + (Lq * Lq).sum() - M)
    return ell - kld, ell, kld


def dense_bound(p, Z=None, raw_ls=None, raw_os=None, lvn=None):
    """log N(y | 0, Q + sigma^2 I) - tr(K_XX - Q) / (2 sigma^2), Q = K_XZ K^-1 K_ZX (c = 1); differentiable."""
    assert p["c"] == 1.0
    Z = p["Z"] if Z is None else Z
    raw_ls = p["raw_ls"] if raw_ls is None else raw_ls
    raw_os = p["raw_os"] if raw_os is None else raw_os
    lvn = p["lvn"] if lvn is None else lvn
    N, M = p["N"], p["M"]
    K = kernel(Z, Z, raw_ls, raw_os, p["kernel"]) + p["jitter"] * torch.eye(M, dtype=F64)
    L = torch.linalg.cholesky(K)
    A = torch.linalg.solve_triangular(L, kernel(Z, p["X"], raw_ls, raw_os, p["kernel"]), upper=False)
    s2n = torch.exp(lvn.reshape(()))
    Q = A.T @ A
    Lc = torch.linalg.cholesky(Q + s2n * torch.eye(N, dtype=F64))
    a = torch.linalg.solve_triangular(Lc, p["Y"].reshape(-1, 1), upper=False)
    logn = -0.5 * N * LOG_2PI_REF - torch.log(torch.diagonal(Lc)).sum() - 0.5 * (a * a).sum()
    return logn - 0.5 * (N * softplus(raw_os).reshape(()) - torch.diagonal(Q).sum()) / s2n


def qu_grads(p, m, Lam):
    """(g_m, tril g_Lam) of the ELBO at (m, Lam)."""
    m = m.detach().clone().requires_grad_(True)
    Lam = Lam.detach().clone().requires_grad_(True)
    elbo(p, m, Lam)[0].backward()
    return m.grad, torch.tril(Lam.grad)


def grad_ratio(p, m, Lam):
    """max(|g_m|, |tril g_Lam|) at (m, Lam) over the same at m = 0, Lam = I."""
    gm, gL = qu_grads(p, m, Lam)
    gm0, gL0 = qu_grads(p, torch.zeros(p["M"], dtype=F64), torch.eye(p["M"], dtype=F64))
    return float(max(gm.abs().max(), gL.abs().max()) / max(gm0.abs().max(), gL0.abs().max()))


def rel(a, b):
    return float((a - b).abs().max() / b.abs().max())


def measure(name):
    """The figures `OPT_CPU` records for a case."""
    p = make_case(name)
    (m1, L1), (m2, L2) = closed_form_rev(p), closed_form_inv(p)
    route = max(rel(m1, m2), rel(L1, L2), rel(L1 @ L1.T, L2 @ L2.T))
    ratio = max(grad_ratio(p, m1, L1), grad_ratio(p, m2, L2))
    bound = None
    if name in DENSE_CASES:
        d = dense_bound(p)
        bound = float(abs(elbo(p, m1, L1)[0] - d) / abs(d))
    return dict(route=route, ratio=ratio, bound=bound, cond=cond_K(p))


if __name__ == "__main__":
    for name in CASES:
        r = measure(name)
        print('    "%s": dict(route=%.1e, ratio=%.1e, bound=%s, cond=%.1e),' % (
            name, r["route"], r["ratio"], "None" if r["bound"] is None else "%.1e" % r["bound"], r["cond"]))
