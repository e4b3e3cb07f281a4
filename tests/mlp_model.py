"""The packed per-row networks of the input-dependent flows (tgp_mlp_forward_f64 / tgp_mlp_backward_f64) in numpy.longdouble:
forward, and a hand-written backward -- the reference of tests/test_gpu_mlp_variants.py, pinned to torch autograd by
tests/test_mlp_host.py.

Per net, torch parameter order: [W1 (H, D) | b1 (H) | W2 (H, H) | b2 (H) | ... | Wout (H) | bout]; every hidden layer is
Linear -> activation -> keep mask / (1 - p).  out (N, nnets); g_W = d sum(out * G) / dW, packed like W.

GPU tolerances (the project's, test_mlp_kernels_match_torch): 1e-12 for the outputs, 1e-11 for g_W, relative to the largest entry.
Measured by tests/test_mlp_host.py::test_float64_torch_is_well_inside_the_gpu_tolerances over every case of CASES below (x86-64,
torch CPU): float64 torch autograd is at most 5.93e-16 (outputs) and 1.39e-15 (g_W) from this model -- the host test holds
every case to a tenth of the tolerances (1e-13, 1e-12) and to twice the measured figures (F64_*), so the GPU tolerance is never
spent on the reference.
"""
import numpy as np

LD = np.longdouble
TOL_OUT, TOL_GW = 1e-12, 1e-11
F64_OUT, F64_GW = 1.2e-15, 2.8e-15           # 2 x measured (5.93e-16, 1.39e-15), see above

# (N, D, H, L, nnets, act, p): every case of the GPU test, shared with the host test that measures float64 torch on them.
_UPPER, _FIRST = (32, 52, 64), (1, 33, 53)                 # the H classes' upper edges, and the first size of each class


def _variants():
    out = []
    for L in (1, 2, 3):
        for act in ("relu", "tanh"):
            # L = 1 upper edges, L = 2 first sizes, L = 3 one of each per activation: every class sees both across the depths.
            # (L = 3 at H = 64 is beyond the backward kernel's LDS -- 179 376 bytes of the 162 816 a kernel may have -- and is
            # refused with TGP_E_LDS: LDS_LIMIT_CASES below and test_backward_runs_exactly_what_its_lds_sizing_admits; the widest
            # trainable three-layer net has H = 53, so that is the third class's size at L = 3 under both activations.)
            hs = _UPPER if L == 1 else _FIRST if L == 2 else (_FIRST if act == "relu" else (32, 52, 53))
            out += [(129, 5, H, L, 2, act, 0.25) for H in hs]
    return out


CASES = {
    "variants": _variants(),                                                       # all 18 (L, NKS, act) instantiations
    "small_H": [(129, 5, H, 2, 2, "tanh", 0.25) for H in (1, 2, 3, 4, 17)],
    "wide_D": [(129, D, 33, 2, 2, "relu", 0.25) for D in (1, 4, 16, 17, 64)],
    "short_N": [(N, 4, 50, 2, 2, "tanh", 0.25) for N in (1, 15, 16, 17, 63, 64, 65)],
    # 20 chunks of 64 rows, the last holds one row: forward 2 chunks per workgroup, backward 3 (last workgroup short, 7 slots)
    "chunks": [(1217, 4, 17, 1, 60, "relu", 0.25)],
}
ALL_CASES = [c for group in CASES.values() for c in group]
# around the backward kernel's LDS ceiling, with mlp_lds(D, H, L, bwd)'s bytes worked out by hand from tgp_mlp.hip:
# (case, bytes); 160 KiB - 1 KiB = 162 816 are granted
LDS_LIMIT_CASES = [((129, 5, 53, 3, 2, "tanh", 0.25), 161600), ((129, 5, 54, 3, 2, "tanh", 0.25), 163216),
                   ((129, 5, 64, 3, 2, "tanh", 0.25), 179376), ((129, 4, 50, 2, 2, "relu", 0.25), 81104)]
W_SCALE = 0.4


def weights_per_net(D, H, L):
    return D * H + H + (L - 1) * (H * H + H) + H + 1


def make_case(case, seed=3):
    """X (N, D), W (packed, scale 0.4), G (N, nnets): float64, seeded per case."""
    N, D, H, L, nnets, act, p = case
    rng = np.random.default_rng([seed, N, D, H, L, nnets])
    X = rng.standard_normal((N, D))
    W = W_SCALE * rng.standard_normal(nnets * weights_per_net(D, H, L))
    G = rng.standard_normal((N, nnets))
    return X, W, G


def _act(z, act):
    return np.maximum(z, 0) if act == "relu" else np.tanh(z)


def _dact(z, a, act):
    return (z > 0).astype(LD) if act == "relu" else 1 - a * a


def forward_backward(X, W, G, D, H, L, nnets, act, p=0.0, masks=None):
    """(out, g_W) in longdouble.  masks[k][l]: (N, H) keep masks (bool / 0-1) or None for eval mode."""
    X, W, G = np.asarray(X, LD), np.asarray(W, LD), np.asarray(G, LD)
    N, pw = X.shape[0], weights_per_net(D, H, L)
    scale = LD(1) / (LD(1) - LD(p)) if masks is not None else LD(1)
    out, gW = np.zeros((N, nnets), LD), np.zeros(nnets * pw, LD)
    for k in range(nnets):
        w, o, nin = W[k * pw:(k + 1) * pw], 0, D
        hs, zs, fs, offs = [X], [], [], []
        for l in range(L):
            Wl, bl = w[o:o + H * nin].reshape(H, nin), w[o + H * nin:o + H * nin + H]
            offs.append((o, nin))
            o += H * nin + H
            z = hs[-1] @ Wl.T + bl
            a = _act(z, act)
            f = (np.asarray(masks[k][l], LD) * scale) if masks is not None else np.ones((N, H), LD)
            zs.append((z, a))
            fs.append(f)
            hs.append(a * f)
            nin = H
        wout = w[o:o + H]
        out[:, k] = hs[-1] @ wout + w[o + H]
        g = gW[k * pw:(k + 1) * pw]
        g[o:o + H] = hs[-1].T @ G[:, k]
        g[o + H] = G[:, k].sum()
        dh = G[:, k:k + 1] * wout[None, :]
        for l in range(L - 1, -1, -1):
            z, a = zs[l]
            delta = dh * fs[l] * _dact(z, a, act)
            ol, nin = offs[l]
            g[ol:ol + H * nin] = (delta.T @ hs[l]).reshape(-1)
            g[ol + H * nin:ol + H * nin + H] = delta.sum(0)
            dh = delta @ w[ol:ol + H * nin].reshape(H, nin)
    return out, gW


def rel(a, ref):
    """max|a - ref| / max|ref|, formed in longdouble."""
    a, ref = np.asarray(a, LD), np.asarray(ref, LD)
    return float(np.abs(a - ref).max() / (np.abs(ref).max() + LD(1e-300)))
