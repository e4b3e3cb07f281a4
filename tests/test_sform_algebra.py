"""CPU: the two forms of the row kernel's q(f) variance and of its adjoint agree to rounding.

B form (two triangular products with L_q):   v = s2 - sum A^2 + sum (L_q^T A)^2
                                             Abar = m mubar^T - 2 A diag(vbar) + 2 L_q (L_q^T A diag(vbar))
S form (one product with S - I, S = L_q L_q^T from the prepare stage -- csrc/tgp_rows.hpp):
                                             C = (S - I) A ;  v = s2 + sum A o C ;  Abar = m mubar^T + 2 C diag(vbar)

Both are evaluated in float64 torch with algebra_model.prepare's operands on committed fixtures, the initialisation
(Lam = sqrt(1e-5) I: S - I ~ -I) among them.  The bound is not fitted to the result: every entry of either form is a sum of
at most 2 M + 2 products whose absolute values add up to `mag` below, so each form is within (2 M + 2) eps mag of the exact
value (the standard bound for recursive summation, gamma_n ~ n eps).  The operand A carries its own rounding into BOTH forms
identically (same tensor), so it does not enter the difference; S = fl(L_q L_q^T) against the B form's exact-L_q products
adds another M eps |L_q||L_q^T| per entry of S, which the same `mag` (built from |L_q||L_q^T|, not from |S|) covers with one
more multiple of M eps: n_terms = 3 M + 2 per form, and the two forms are within twice that of each other."""
import pytest
import torch

import algebra_model as am
from conftest import load_golden

CASES = ["power_tanh3x2", "tiny_svgp", "tiny_sal2", "tiny_tanh3x2", "tiny_idsal3", "init_sal2_identity", "power_init_sal2"]
EPS = 2.0 ** -53


def _forms(g):
    p = g["params"]
    st = am.prepare(p)
    X = g["X"]
    Xs = X / st["ls"]
    d2 = ((Xs[:, None, :] - st["Zs"][None, :, :]) ** 2).sum(-1)
    K = st["s2"] * torch.exp(-0.5 * d2)
    A = torch.linalg.solve_triangular(st["L"], K.T, upper=False)        # (M, N), by substitution as the kernel does
    return st, p, A


@pytest.mark.parametrize("name", CASES)
def test_v_and_abar_agree_between_b_form_and_s_form(name):
    g = load_golden(name)
    st, p, A = _forms(g)
    Lq, S = st["Lq"], st["S"]
    M, N = A.shape
    eye = torch.eye(M, dtype=A.dtype)
    # adjoints of (mu, v): the closed-form Gaussian ones (what the SVGP mode feeds in) with a seeded per-row factor on vbar,
    # so that diag(vbar) is not a multiple of the identity; the identity under test holds for ANY (mubar, vbar)
    gen = torch.Generator().manual_seed(7)
    e = torch.exp(-p["log_var_noise"].reshape(()))
    mu = A.T @ p["m"]
    mub = e * (g["Y"].reshape(-1) - mu)
    vb = -0.5 * e * (0.5 + torch.rand(N, generator=gen, dtype=A.dtype))

    B = Lq.T @ A
    v_b = st["s2"] - (A * A).sum(0) + (B * B).sum(0)
    ab_b = p["m"][:, None] * mub[None, :] - 2 * A * vb[None, :] + 2 * Lq @ (B * vb[None, :])

    C = (S - eye) @ A
    v_s = st["s2"] + (A * C).sum(0)
    ab_s = p["m"][:, None] * mub[None, :] + 2 * C * vb[None, :]

    absA = A.abs()
    SA = Lq.abs() @ (Lq.abs().T @ absA)                       # |L_q| |L_q^T| |A|  >=  |S| |A| entrywise
    n_terms = 3 * M + 2
    mag_v = st["s2"].abs() + (absA * absA).sum(0) + (absA * SA).sum(0)
    mag_ab = p["m"].abs()[:, None] * mub.abs()[None, :] + 2 * (absA + SA) * vb.abs()[None, :]
    dv = (v_b - v_s).abs()
    dab = (ab_b - ab_s).abs()
    print("%s: max |dv| / bound = %.3g, max |dAbar| / bound = %.3g, min v = %.3g, max |S - I| = %.3g" % (
        name, float((dv / (2 * n_terms * EPS * mag_v)).max()), float((dab / (2 * n_terms * EPS * mag_ab + 1e-300)).max()),
        float(v_s.min()), float((S - eye).abs().max())))
    assert bool((dv <= 2 * n_terms * EPS * mag_v).all())
    assert bool((dab <= 2 * n_terms * EPS * mag_ab).all())
    # and, where the fixture records it, against the reference-executed variance at the bar of test_algebra_model.py
    # (the full-size Power fixtures hold the ELBO and its gradients only)
    if "v" in g:
        assert float((v_s - g["v"]).abs().max()) < 1e-8 * float(g["v"].abs().max())
