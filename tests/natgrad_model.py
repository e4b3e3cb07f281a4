"""CPU restatement of the natural-gradient step of q(u) (conjugate-computation form) in float64 torch: test infrastructure only.

Whitened q(u) = N(m, Lam Lam^T), zero prior mean, K = K_ZZ + j I = L L^T, a_n = L^-1 k_Z(x_n), mu_n = a_n^T m,
v_n = k_nn - a_n^T a_n + |Lam^T a_n|^2.  With mu_bar = d(c ELL)/d mu, v_bar = d(c ELL)/d v (they hold c):
    lambda = max(-2 v_bar, floor),  r = mu_bar + lambda mu
    B = I + L^-1 K_ZX diag(lambda) K_XZ L^-T,  h = L^-1 K_ZX r,  P = (Lam Lam^T)^-1
    P' = (1 - rho) P + rho B,  h' = (1 - rho) P m + rho h,  Lam' Lam'^T = P'^-1 (Lam' lower, positive diagonal),  m' = P'^-1 h'
stated two ways (`update_inv`: explicit inverses; `update_rev`: solves on the factor of the index-reversed P'), the sites of the
Gaussian and the Poisson likelihood in closed form and of any row-wise ELL by autograd, and the ELBOs the checks need.

The inputs are optqu_model's cases plus two small ones of this file; `NAT_CPU` holds, per case and scenario, what this file
measured on the CPU (tools: run this file).
"""
import math
import zlib

import numpy as np
import torch

import optqu_model as om

F64 = om.F64
# the cases of the operator tests (optqu_model.CASES): the 63 / 64 / 65 and 128 / 129 tile edges, ragged last groups, D = 1 and 16
OP_CASES = ("m1_d1", "m16", "m63_mat", "m65", "m129_c_mat", "m200")
# name: (N, D, M, c, kernel, jitter) -- the host checks' case and the models' smallest shapes
SMALL = {
    "n40_m6": (40, 2, 6, 2.5, "scale_rbf", 0.0),
    "n60_m8": (60, 3, 8, 1.0, "scale_rbf", 0.0),
    "n60_m8_mat": (60, 3, 8, 1.0, "scale_matern32", 0.0),
}
RHOS = (0.25, 1.0)

# Measured by this file on the CPU (python tests/natgrad_model.py), float64, per case and scenario:
#   route   max relative discrepancy of (m', Lam', Lam' Lam'^T) between the two routes (kxwxk: of C between two summation orders)
#   cond    cond(P') (kxwxk: None)
# Scenarios: gauss = Gaussian sites, rho 1; pois_<rho> = Poisson sites at state(p); floor = mixed-sign sites clamped at 0, rho 0.25
NAT_CPU = {
    "m1_d1": {"kxwxk": dict(route=4.6e-17, cond=None), "gauss": dict(route=2.0e-16, cond=1.0e+00), "pois_0.25": dict(route=0.0e+00, cond=1.0e+00), "pois_1": dict(route=0.0e+00, cond=1.0e+00), "floor": dict(route=1.4e-16, cond=1.0e+00)},
    "m16": {"kxwxk": dict(route=6.0e-17, cond=None), "gauss": dict(route=3.9e-16, cond=3.8e+01), "pois_0.25": dict(route=5.6e-16, cond=1.3e+01), "pois_1": dict(route=5.9e-16, cond=3.7e+01), "floor": dict(route=3.1e-16, cond=6.2e+00)},
    "m63_mat": {"kxwxk": dict(route=1.1e-16, cond=None), "gauss": dict(route=3.4e-15, cond=1.3e+02), "pois_0.25": dict(route=1.6e-15, cond=2.9e+01), "pois_1": dict(route=1.2e-15, cond=5.3e+01), "floor": dict(route=9.6e-16, cond=2.9e+01)},
    "m65": {"kxwxk": dict(route=1.1e-16, cond=None), "gauss": dict(route=7.5e-16, cond=8.3e+01), "pois_0.25": dict(route=1.8e-15, cond=2.7e+01), "pois_1": dict(route=4.7e-15, cond=3.1e+01), "floor": dict(route=8.2e-16, cond=3.0e+01)},
    "m129_c_mat": {"kxwxk": dict(route=9.6e-17, cond=None), "gauss": dict(route=7.1e-15, cond=9.2e+02), "pois_0.25": dict(route=4.7e-15, cond=1.6e+02), "pois_1": dict(route=7.4e-15, cond=3.3e+02), "floor": dict(route=3.4e-15, cond=1.8e+02)},
    "m200": {"kxwxk": dict(route=1.8e-16, cond=None), "gauss": dict(route=1.5e-15, cond=5.7e+01), "pois_0.25": dict(route=1.5e-14, cond=6.8e+02), "pois_1": dict(route=2.5e-15, cond=2.3e+01), "floor": dict(route=1.6e-14, cond=7.2e+02)},
    "n40_m6": {"kxwxk": dict(route=3.7e-16, cond=None), "gauss": dict(route=6.8e-16, cond=1.3e+01), "pois_0.25": dict(route=1.4e-16, cond=8.4e+00), "pois_1": dict(route=4.6e-16, cond=1.5e+01), "floor": dict(route=3.2e-16, cond=3.9e+00)},
    "n60_m8": {"kxwxk": dict(route=1.5e-16, cond=None), "gauss": dict(route=2.9e-16, cond=3.8e+01), "pois_0.25": dict(route=3.5e-16, cond=3.7e+00), "pois_1": dict(route=4.9e-16, cond=1.4e+01), "floor": dict(route=3.2e-16, cond=3.3e+00)},
    "n60_m8_mat": {"kxwxk": dict(route=1.6e-16, cond=None), "gauss": dict(route=3.7e-16, cond=3.1e+01), "pois_0.25": dict(route=7.3e-16, cond=4.0e+00), "pois_1": dict(route=3.6e-16, cond=1.3e+01), "floor": dict(route=4.3e-16, cond=3.2e+00)},
}
TOL = 1e-9            # the project's tolerance for a float64 kernel against its restatement


def tolerance(route):
    """The project's rule: 1e-9 where the two CPU routes agree to a tenth of it, else 10 x their discrepancy."""
    return TOL if route < 0.1 * TOL else 10.0 * route


def make_case(name):
    """optqu_model.make_case for its cases; the small cases of this file the same way.  Adds the counts `Yc` (Poisson draws at the
    rate exp(Y / 2), seeded)."""
    if name in SMALL:
        om.CASES[name] = SMALL[name]
        try:
            p = om.make_case(name)
        finally:
            del om.CASES[name]
    else:
        p = om.make_case(name)
    g = torch.Generator().manual_seed(zlib.crc32(("counts " + name).encode()) % 100000)
    p["Yc"] = torch.poisson(torch.exp(0.5 * p["Y"]), generator=g)
    return p


def state(p, seed=3):
    """A seeded q(u) away from the prior: m, and a lower factor whose diagonal has one negative entry (Lam Lam^T decides)."""
    g = torch.Generator().manual_seed(seed + p["M"])
    M = p["M"]
    m = 0.3 * torch.randn(M, dtype=F64, generator=g)
    Lam = 0.8 * torch.eye(M, dtype=F64) + 0.1 * torch.tril(torch.randn(M, M, dtype=F64, generator=g))
    Lam[M // 2, M // 2] = -Lam[M // 2, M // 2]
    return m, Lam


def factor(p):
    """(L^-1, A = L^-1 K_ZX (M, N))"""
    L = torch.linalg.cholesky(om.k_zz(p))
    Li = torch.linalg.solve_triangular(L, torch.eye(p["M"], dtype=F64), upper=False)
    return Li, Li @ om.kernel(p["Z"], p["X"], p["raw_ls"], p["raw_os"], p["kernel"])


def moments(p, m, Lam):
    """(mu, v) of q(f) at the rows of X"""
    _, A = factor(p)
    Lq = torch.tril(Lam)
    s2 = torch.nn.functional.softplus(p["raw_os"]).reshape(())
    return A.T @ m, s2 - (A * A).sum(0) + ((Lq.T @ A) ** 2).sum(0)


# ---- sites: (mu_bar, v_bar) = d(c ELL) / d(mu, v) -----------------------------------------------------------------------
def gauss_sites(p, mu, v):
    s = p["c"] * math.exp(-float(p["lvn"]))
    return s * (p["Y"] - mu), torch.full_like(v, -0.5 * s)


def poisson_sites(p, mu, v):
    e = torch.exp(mu + 0.5 * v)
    return p["c"] * (p["Yc"] - e), -0.5 * p["c"] * e


def gauss_hermite(S):
    x, w = np.polynomial.hermite.hermgauss(int(S))
    return torch.tensor(x, dtype=F64), torch.tensor(w / math.sqrt(math.pi), dtype=F64)


def bernoulli_ell(p, mu, v, S=50):
    """c sum_n E_q(f)[y log Phi(f) + (1 - y) log Phi(-f)], labels y = (Y > 0), by Gauss-Hermite quadrature; differentiable."""
    xs, wn = gauss_hermite(S)
    f = mu.unsqueeze(1) + torch.sqrt(2.0 * v).unsqueeze(1) * xs.unsqueeze(0)
    y = (p["Y"] > 0).to(F64).unsqueeze(1)
    lp = y * torch.special.log_ndtr(f) + (1.0 - y) * torch.special.log_ndtr(-f)
    return p["c"] * (lp * wn.unsqueeze(0)).sum()


def poisson_ell(p, mu, v):
    return p["c"] * (p["Yc"] * mu - torch.exp(mu + 0.5 * v) - torch.lgamma(p["Yc"] + 1.0)).sum()


def gauss_ell(p, mu, v):
    eta, N = float(p["lvn"]), p["N"]
    return p["c"] * (-0.5 * N * om.LOG_2PI_REF - 0.5 * N * eta - 0.5 * math.exp(-eta) * (((p["Y"] - mu) ** 2) + v).sum())


ELLS = {"gauss": gauss_ell, "poisson": poisson_ell, "bernoulli": bernoulli_ell}


def autograd_sites(ell, p, mu, v):
    mu, v = mu.detach().clone().requires_grad_(True), v.detach().clone().requires_grad_(True)
    g = torch.autograd.grad(ell(p, mu, v), (mu, v))
    return g[0], g[1]


def elbo(p, m, Lam, lik):
    """ELBO = c ELL - KL of likelihood `lik` (a key of ELLS) at q(u) = N(m, tril(Lam) tril(Lam)^T); differentiable in m, Lam."""
    mu, v = moments(p, m, Lam)
    Lq = torch.tril(Lam)
    kld = 0.5 * (-torch.log(torch.diagonal(Lq) ** 2).sum() + (m * m).sum() + (Lq * Lq).sum() - p["M"])
    return ELLS[lik](p, mu, v) - kld


def grad_m(p, m, Lam, lik):
    m = m.detach().clone().requires_grad_(True)
    return torch.autograd.grad(elbo(p, m, Lam, lik), m)[0]


# ---- the update, two routes ------------------------------------------------------------------------------------------------
def sites(mu, mu_bar, v_bar, floor):
    lam = -2.0 * v_bar
    if floor is not None:
        lam = lam.clamp_min(floor)
    return lam, mu_bar + lam * mu


def _system(p, m, Lam, mu, mu_bar, v_bar, rho, floor):
    """(P', h')"""
    M = p["M"]
    Li, _ = factor(p)
    lam, r = sites(mu, mu_bar, v_bar, floor)
    C, b, _ = kxwxk(p, lam, r)
    Phi = Li @ C @ Li.T                     # (optqu_model._b_matrix's order of operations: Gaussian sites give its B)
    B = torch.eye(M, dtype=F64) + 0.5 * (Phi + Phi.T)
    h = Li @ b
    if rho == 1.0:
        return B, h
    Lq = torch.tril(Lam)
    S = Lq @ Lq.T
    P = torch.linalg.inv(0.5 * (S + S.T))
    P = 0.5 * (P + P.T)
    return (1.0 - rho) * P + rho * B, (1.0 - rho) * (P @ m) + rho * h


def p_prime(p, m, Lam, mu, mu_bar, v_bar, rho=1.0, floor=0.0):
    return _system(p, m, Lam, mu, mu_bar, v_bar, rho, floor)[0]


def update_inv(p, m, Lam, mu, mu_bar, v_bar, rho=1.0, floor=0.0):
    """(m', Lam') by explicit inverses: S' = P'^-1, Lam' = chol(S'), m' = S' h'."""
    Pn, hn = _system(p, m, Lam, mu, mu_bar, v_bar, rho, floor)
    S = torch.linalg.inv(Pn)
    S = 0.5 * (S + S.T)
    return S @ hn, torch.linalg.cholesky(S)


def update_rev(p, m, Lam, mu, mu_bar, v_bar, rho=1.0, floor=0.0):
    """(m', Lam') by the reversed Cholesky: J P' J = L' L'^T, Lam' = J L'^-T J, m' = Lam' (Lam'^T h')."""
    Pn, hn = _system(p, m, Lam, mu, mu_bar, v_bar, rho, floor)
    Lp = torch.linalg.cholesky(Pn.flip(0, 1))
    Lpi = torch.linalg.solve_triangular(Lp, torch.eye(p["M"], dtype=F64), upper=False)
    Ln = Lpi.T.flip(0, 1)
    return Ln @ (Ln.T @ hn), Ln


def step(p, m, Lam, lik, rho=1.0, floor=0.0):
    """One step with the sites of `lik` at (m, Lam): the reversed route."""
    mu, v = moments(p, m, Lam)
    mb, vb = {"gauss": gauss_sites, "poisson": poisson_sites}[lik](p, mu, v) if lik != "bernoulli" else autograd_sites(bernoulli_ell, p, mu, v)
    return update_rev(p, m, Lam, mu, mb, vb, rho, floor)


# ---- the inputs of the operator tests ------------------------------------------------------------------------------------
def weights(p, seed=5):
    """(w, r): normal draws, w with both signs and exact zeros"""
    g = torch.Generator().manual_seed(seed + p["N"])
    w = torch.randn(p["N"], dtype=F64, generator=g)
    w[::5] = 0.0
    return w, torch.randn(p["N"], dtype=F64, generator=g)


def kxwxk(p, w, r):
    """(C, b, C of |w|)"""
    K = om.kernel(p["Z"], p["X"], p["raw_ls"], p["raw_os"], p["kernel"])
    return (K * w.unsqueeze(0)) @ K.T, K @ r, (K * w.abs().unsqueeze(0)) @ K.T


def mixed_sites(p, m, seed=9):
    """(mu, mu_bar, v_bar) with lambda = -2 v_bar of both signs"""
    g = torch.Generator().manual_seed(seed + p["N"])
    _, A = factor(p)
    return A.T @ m, torch.randn(p["N"], dtype=F64, generator=g), torch.randn(p["N"], dtype=F64, generator=g)


def scenario(p, name):
    """(m, Lam, mu, mu_bar, v_bar, rho, floor) of a scenario of NAT_CPU"""
    M = p["M"]
    if name == "gauss":
        m, Lam = torch.zeros(M, dtype=F64), torch.eye(M, dtype=F64)
        mu, v = moments(p, m, Lam)
        return (m, Lam, mu, *gauss_sites(p, mu, v), 1.0, 0.0)
    m, Lam = state(p)
    if name == "floor":
        return (m, Lam, *mixed_sites(p, m), 0.25, 0.0)
    mu, v = moments(p, m, Lam)
    return (m, Lam, mu, *poisson_sites(p, mu, v), float(name.split("_")[1]), 0.0)


SCENARIOS = ("gauss",) + tuple("pois_%g" % r for r in RHOS) + ("floor",)


def route_discrepancy(p, args):
    (m1, L1), (m2, L2) = update_rev(p, *args), update_inv(p, *args)
    return max(om.rel(m1, m2), om.rel(L1, L2), om.rel(L1 @ L1.T, L2 @ L2.T))


def measure(name):
    """The figures `NAT_CPU` records for a case."""
    p = make_case(name)
    w, r = weights(p)
    C1, _, Cabs = kxwxk(p, w, r)
    K = om.kernel(p["Z"], p["X"], p["raw_ls"], p["raw_os"], p["kernel"])
    C2 = torch.einsum("in,n,jn->ij", K.flip(1), w.flip(0), K.flip(1))      # the rows summed in the opposite order
    out = {"kxwxk": dict(route=float((C1 - C2).abs().max() / Cabs.abs().max()), cond=None)}
    for sc in SCENARIOS:
        args = scenario(p, sc)
        Pn = p_prime(p, *args)
        out[sc] = dict(route=route_discrepancy(p, args), cond=float(torch.linalg.cond(Pn)))
    return out


if __name__ == "__main__":
    for name in OP_CASES + tuple(SMALL):
        res = measure(name)
        print('    "%s": {%s},' % (name, ", ".join(
            '"%s": dict(route=%.1e, cond=%s)' % (k, v["route"], "None" if v["cond"] is None else "%.1e" % v["cond"])
            for k, v in res.items())))
