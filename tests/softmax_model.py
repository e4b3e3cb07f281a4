"""Torch restatement of the multi-class likelihood kernels (csrc/tgp_softmax.hip) for the tests, float64 with autograd:

    f0[s,c,n] = mu[c,n] + sqrt(max(v[c,n], 0)) eps[s,c,n],   g = G_c(f0),
    ELL = scale/S sum_n sum_s (g[s,y_n,n] - logsumexp_c g[s,c,n])

(`ell_softmax_torch`), the prediction (`predict_torch`), and the kernels' counter-based standard normals restated in plain
integer arithmetic and `math` (`mc_hash`, `mc_normal`, `mc_normals`).  The block table is the one of warp_model.py.
`programs` is a list of C programs (rows kind, K, poff, flags; poff relative to the class's own slice of theta), `theta_off`
the C + 1 offsets of those slices."""
import math

import torch

import warp_model as wm

MASK64 = (1 << 64) - 1
GOLD = 0x9E3779B97F4A7C15


def flows_forward(f0, programs, theta, theta_off):
    """g (S, C, N) from f0 (S, C, N)."""
    cols = []
    for c, prog in enumerate(programs):
        th = theta[int(theta_off[c]):int(theta_off[c + 1])] if theta is not None else None
        x = f0[:, c, :]
        for kind, K, poff, flags in prog:
            x, _ = wm.block(int(kind), int(K), int(flags), wm._params(int(kind), int(K), int(poff), int(flags), th, None), x)
        cols.append(x)
    return torch.stack(cols, dim=1)


def f0_of(mu, v, eps):
    # (a row with v <= 0 takes no derivative with respect to v, as in the kernel)
    sd = torch.where(v > 0, torch.sqrt(torch.where(v > 0, v, torch.ones_like(v))), torch.zeros_like(v))
    return mu.unsqueeze(0) + sd.unsqueeze(0) * eps


def ell_softmax_torch(Y, mu, v, eps, programs, theta, theta_off, scale=1.0):
    """ELL as a 0-dim tensor; Y (N) class indices, mu, v (C, N), eps (S, C, N)."""
    g = flows_forward(f0_of(mu, v, eps), programs, theta, theta_off)
    S, C, N = g.shape
    y = Y.reshape(-1).long()
    gy = g.gather(1, y.reshape(1, 1, N).expand(S, 1, N)).squeeze(1)
    lse = torch.logsumexp(g, dim=1)
    return (scale / S) * (gy - lse).sum()


def predict_torch(mu, v, eps, programs, theta, theta_off, Y=None):
    """P (N, C) and, with Y, log P[n, y_n]."""
    g = flows_forward(f0_of(mu, v, eps), programs, theta, theta_off)
    P = torch.softmax(g, dim=1).mean(0).t()
    if Y is None:
        return P, None
    return P, torch.log(P.gather(1, Y.reshape(-1, 1).long())).reshape(-1)


# ---- the counter recipe of csrc/tgp_softmax.hip's header comment ------------------------------------------------
def _fin(z):
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK64
    return z ^ (z >> 31)


def mc_hash(seed, step, s, c, row):
    """(h1, h2): the two 64-bit words of one draw."""
    x = (seed + GOLD * (step & 0xFFFFFFFF)) & MASK64
    x ^= ((s << 56) ^ (c << 48) ^ (row & 0xFFFFFFFFFFFF)) & MASK64
    h1 = _fin(x)
    return h1, _fin((h1 + GOLD) & MASK64)


def mc_normal(seed, step, s, c, row):
    h1, h2 = mc_hash(seed, step, s, c, row)
    u1 = float((h1 >> 11) + 1) * 2.0 ** -53
    u2 = float(h2 >> 11) * 2.0 ** -53
    return math.sqrt(-2.0 * math.log(u1)) * math.cos(6.283185307179586 * u2)


def mc_normals(S, C, N, seed=0, step=0, row0=0):
    out = torch.empty(S, C, N, dtype=torch.float64)
    for s in range(S):
        for c in range(C):
            for n in range(N):
                out[s, c, n] = mc_normal(seed, step, s, c, row0 + n)
    return out


def mc_normals_np(count, seed=0, step=0):
    """`count` draws of consecutive rows of (s, c) = (0, 0), vectorised with numpy's uint64 (the statistics test)."""
    import numpy as np
    with np.errstate(over="ignore"):
        row = np.arange(count, dtype=np.uint64)
        x = np.uint64((seed + GOLD * (step & 0xFFFFFFFF)) & MASK64) ^ (row & np.uint64(0xFFFFFFFFFFFF))

        def fin(z):
            z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
            z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
            return z ^ (z >> np.uint64(31))
        h1 = fin(x)
        h2 = fin(h1 + np.uint64(GOLD))
    u1 = ((h1 >> np.uint64(11)) + np.uint64(1)).astype(np.float64) * 2.0 ** -53
    u2 = (h2 >> np.uint64(11)).astype(np.float64) * 2.0 ** -53
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(6.283185307179586 * u2)


def train_blobs_cpu(split_seed=1, M=20, S=16, epochs=300, lr=0.01):
    """The CPU counterpart of `main.py --likelihood multiclass --dataset synthetic_blobs --model TGP --num_inducing M`: C
    latent GPs from the CPU oracle (oracle/tgp_oracle.py qf_moments / kld_whitened), SAL x 2 flows at their identity
    initialisation, this file's likelihood with torch.randn draws, Adam on -ELBO over the whole training split.  Z starts at
    the first M training rows (the CLI uses k-means).  Returns (test NLL per row, test accuracy, majority-class share)."""
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from oracle import tgp_oracle as orc
    from tgp.pytorch_amd import config as cg
    from tgp.pytorch_amd.data import return_dataset
    cg.set_maximum_precission()
    _, dc = return_dataset("synthetic_blobs", 10000, seed=split_seed)
    X, Y, Xte, Yte = dc["X_tr"], dc["Y_tr"].reshape(-1), dc["X_te"], dc["Y_te"].reshape(-1)
    C, D, N = dc["num_classes"], X.shape[1], X.shape[0]
    f64 = torch.float64
    prog1, th1 = orc.sal_program(2)
    progs = [[tuple(int(t) for t in r) for r in prog1]] * C
    theta_off = [c * th1.numel() for c in range(C + 1)]
    P = {"Z": X[:M].clone().repeat(C, 1, 1), "rl": orc.inv_softplus(torch.full((C, D), 2.0, dtype=f64)),
         "ro": orc.inv_softplus(torch.full((C, 1), 2.0, dtype=f64)), "m": torch.zeros(C, M, dtype=f64),
         "Lam": (1e-5 ** 0.5) * torch.eye(M, dtype=f64).repeat(C, 1, 1), "theta": th1.to(f64).repeat(C)}
    P = {k: t.clone().requires_grad_(True) for k, t in P.items()}
    opt = torch.optim.Adam(P.values(), lr=lr)
    gen = torch.Generator().manual_seed(0)

    def moments(Xq):
        mv = [orc.qf_moments(Xq, P["Z"][c], P["rl"][c], P["ro"][c], P["m"][c], P["Lam"][c]) for c in range(C)]
        return torch.stack([a[0].reshape(-1) for a in mv]), torch.stack([a[1].reshape(-1) for a in mv])
    for _ in range(epochs):
        mu, v = moments(X)
        eps = torch.randn(S, C, N, generator=gen, dtype=f64)
        ell = ell_softmax_torch(Y, mu, v, eps, progs, P["theta"], theta_off)
        kl = sum(orc.kld_whitened(P["m"][c], P["Lam"][c]).reshape(()) for c in range(C))
        opt.zero_grad()
        (-(ell - kl)).backward()
        opt.step()
    with torch.no_grad():
        mu, v = moments(Xte)
        eps = torch.randn(100, C, Xte.shape[0], generator=gen, dtype=f64)
        Pte, lp = predict_torch(mu, v, eps, progs, P["theta"], theta_off, Yte)
    acc = float((Pte.argmax(1) == Yte.long()).to(f64).mean())
    return -float(lp.mean()), acc, float(torch.bincount(Yte.long()).max()) / Yte.numel()
