"""Torch restatement of the warped-GP likelihood kernels (csrc/tgp_warp.hip) for the tests: the block table with autograd
derivatives (`flow_forward`), the likelihood (`ell_warp_torch`), the block-by-block inverse with the kernel's bracketed
Newton rule (`inverse_torch`) and the prediction (`predict_torch`).  Float64 on whatever device the inputs live on."""
import math

import torch
import torch.nn.functional as F

AFFINE, SAL, STEPTANH, ARCSINH, BOXCOX, INV_BOXCOX = 0, 1, 2, 3, 4, 5
RESTRICT, ADD_F0, PER_ROW = 1, 2, 4
LOG_2PI_REF = 1.8378770942368803     # log(2 * float32(pi)), the reference's constant
MAXIT = 128                          # WARP_INV_MAXIT
STEP_TOL = 8.8817841970012523e-16    # 2^-50


def _asinh(x):
    return torch.log(x + torch.sqrt(x * x + 1.0))


def _restricted(kind, flags, j):
    if kind == ARCSINH:
        return bool(flags & RESTRICT) and bool(j & 1)
    if kind in (BOXCOX, INV_BOXCOX):
        return False
    if kind == STEPTANH:
        return bool(j & 1)
    return bool(flags & RESTRICT) and j == (0 if kind == AFFINE else 1)


def _params(kind, K, poff, flags, theta, rowp):
    n = {AFFINE: 2, SAL: 2, STEPTANH: 4 * K, ARCSINH: 4}.get(kind, 1)
    out = []
    for j in range(n):
        p = rowp[:, poff + j] if flags & PER_ROW else theta[poff + j]
        out.append(F.softplus(p, threshold=20.0) if _restricted(kind, flags, j) else p)
    return out


def block(kind, K, flags, p, x):
    """(g(x), g'(x)) of one block with transformed parameters p."""
    addf = bool(flags & ADD_F0) and kind != AFFINE
    if kind == AFFINE:
        return p[0] * x + p[1], p[0] * torch.ones_like(x)
    if kind == SAL:
        s = torch.sqrt(x * x + 1.0)
        tau = p[1] * _asinh(x) - p[0]
        g, g1 = torch.sinh(tau), p[1] * torch.cosh(tau) / s
    elif kind == STEPTANH:
        g, g1 = torch.zeros_like(x), torch.zeros_like(x)
        for k in range(K):
            a, B, c, D = p[4 * k:4 * k + 4]
            th = torch.tanh((x - c) / D)
            g = g + a + B * th
            g1 = g1 + B * (1.0 - th * th) / D
    elif kind == ARCSINH:
        a, b, c, d = p
        z = (x - c) / d
        g, g1 = a + b * _asinh(z), b / (d * torch.sqrt(z * z + 1.0))
    elif kind == BOXCOX:
        lam = p[0] if float(p[0].detach()) != 0.0 else p[0] + 1e-11
        ax = x.abs()
        pw = torch.exp(lam * torch.log(ax))
        g, g1 = (torch.sign(x) * pw - 1.0) / lam, pw / ax
    else:
        lam = p[0] if float(p[0].detach()) != 0.0 else p[0] + 1e-11
        w = lam * x + 1.0
        aw = w.abs()
        q = torch.exp(torch.log(aw) / lam)
        g, g1 = torch.sign(w) * q, q / aw
    if addf:
        g, g1 = g + x, g1 + 1.0
    return g, g1


def flow_forward(y, program, theta, rowp=None):
    """(t = T(y), sum of log g_k' per element)."""
    x, ld = y, torch.zeros_like(y)
    for kind, K, poff, flags in program:
        g, g1 = block(kind, K, flags, _params(kind, K, poff, flags, theta, rowp), x)
        x, ld = g, ld + torch.log(g1)
    return x, ld


def ell_warp_torch(Y, mu, v, lvn, program, theta, scale=1.0):
    """(ELL_w, scale * sum log T', t): differentiable in mu, v, lvn, theta."""
    t, ld = flow_forward(Y, program, theta)
    eta = lvn.reshape(())
    e = -0.5 * LOG_2PI_REF - 0.5 * eta - 0.5 * torch.exp(-eta) * ((t - mu) ** 2 + v)
    return scale * e.sum() + scale * ld.sum(), scale * ld.sum(), t


def _newton(kind, K, flags, p, t):
    """The kernel's rule (warp_newton), element-wise with masks.  Returns (x, failed mask)."""
    with torch.no_grad():
        f = lambda x: block(kind, K, flags, p, x)
        x = t.clone()
        g, g1 = f(x)
        done = g == t
        up = g < t
        step = torch.clamp(x.abs(), min=1.0)
        lo = torch.where(up, x, x - step)
        hi = torch.where(up, x + step, x)
        ok = done.clone()
        for _ in range(MAXIT):
            probe = torch.where(up, hi, lo)
            gp = f(probe)[0]
            hit = torch.where(up, gp >= t, gp <= t)
            ok = ok | hit
            if bool(ok.all()):
                break
            grow = ~ok
            step = torch.where(grow, step * 2.0, step)
            lo2 = torch.where(grow & up, hi, torch.where(grow & ~up, lo - step, lo))
            hi2 = torch.where(grow & up, hi + step, torch.where(grow & ~up, lo, hi))
            lo, hi = lo2, hi2
        fail = ~ok
        conv = done | fail
        for _ in range(MAXIT):
            fx = g - t
            conv = conv | (fx == 0.0)
            lo = torch.where(~conv & (fx < 0.0), x, lo)
            hi = torch.where(~conv & ~(fx < 0.0), x, hi)
            xn = x - fx / g1
            bad = ~((xn > lo) & (xn < hi))
            xn = torch.where(bad, 0.5 * (lo + hi), xn)
            dx = (xn - x).abs()
            x = torch.where(conv, x, xn)
            conv = conv | (dx <= STEP_TOL * torch.clamp(x.abs(), min=1.0))
            if bool(conv.all()):
                break
            g, g1 = f(x)
        return x, fail | ~conv


def inverse_torch(t, program, theta, rowp=None):
    """(x = T^-1(t), number of elements that did not converge); t of shape (N,) or (S, N)."""
    x = t
    nfail = torch.zeros_like(t, dtype=torch.bool)
    for kind, K, poff, flags in reversed([tuple(int(q) for q in b) for b in program]):
        p = _params(kind, K, poff, flags, theta, rowp)
        addf = bool(flags & ADD_F0) and kind != AFFINE
        if addf or kind == STEPTANH:
            x, fl = _newton(kind, K, flags, p, x)
            nfail = nfail | fl
        elif kind == AFFINE:
            x = (x - p[1]) / p[0]
        elif kind == SAL:
            x = torch.sinh((_asinh(x) + p[0]) / p[1])
        elif kind == ARCSINH:
            x = p[2] + p[3] * torch.sinh((x - p[0]) / p[1])
        elif kind == BOXCOX:
            x = block(INV_BOXCOX, 0, 0, p, x)[0]
        else:
            x = block(BOXCOX, 0, 0, p, x)[0]
    return x, int(nfail.sum())


def predict_torch(mu, v, lvn, program, theta, xs, wn, Y=None, Y_std=1.0):
    """(m1, m2, logp) of tgp_predict_f64 with TGP_LIK_WARPED."""
    var = v + torch.exp(lvn.reshape(()))
    f = mu.reshape(1, -1) + torch.sqrt(2.0 * var).reshape(1, -1) * xs.reshape(-1, 1)
    x, nfail = inverse_torch(f, program, theta)
    assert nfail == 0
    m1 = (wn.reshape(-1, 1) * x).sum(0)
    m2 = (wn.reshape(-1, 1) * x * x).sum(0) - m1 * m1
    logp = None
    if Y is not None:
        t, ld = flow_forward(Y, program, theta)
        logp = -0.5 * (LOG_2PI_REF + torch.log(var) + (t - mu) ** 2 / var) + ld - math.log(Y_std)
    return m1, m2, logp


def load_case(d, device="cpu"):
    """npz fixture -> dict of float64 tensors (+ program as a list of int tuples)."""
    import numpy as np
    out = {}
    for k in d.files:
        a = d[k]
        if k == "program":
            out[k] = [tuple(int(q) for q in b) for b in a.reshape(-1, 4)]
        elif a.dtype.kind == "f":
            out[k] = torch.tensor(np.asarray(a, dtype=np.float64), dtype=torch.float64, device=device)
        else:
            out[k] = a
    return out
