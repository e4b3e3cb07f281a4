"""Float64 torch restatement of the Matern-5/2 and rational-quadratic covariance functions: test infrastructure only.

With d2 = |(x - z) / l|^2, l = softplus(raw_lengthscale), s2 = softplus(raw_outputscale), r = sqrt(max(d2, 1e-30)):
    scale_matern52   s2 (1 + sqrt5 r + 5/3 r^2) exp(-sqrt5 r)       gpytorch 1.1.1 MaternKernel(nu=2.5) under a ScaleKernel
    scale_rq         s2 (1 + d2 / (2 alpha))^-alpha                 gpytorch 1.1.1 RQKernel under a ScaleKernel, alpha fixed

A test names a kernel SETTING by a `kind` string: "scale_matern52", or "scale_rq@<alpha>" -- the restatements of the other test
modules carry one kernel name and a one-element raw output scale, and so do these; `hip_args` turns a kind into what the package
takes (the name 'scale_rq' and ops.rq_scale's two doubles).

At import the settings of K4 are added to `oracle.tgp_oracle.KERNELS` under their kind strings, in gpytorch's op order
(mean-centred inputs, the centred a^2 - 2ab + b^2 expansion, clamp_min(1e-30).sqrt()): orc.elbo_and_grads(..., kernel=kind) and
orc.qf_moments(..., kernel=kind) are then the autograd oracle, as for 'scale_matern32'.  Keys are added at run time; no file of
the oracle changes.  `patched(module)` lends the same formulas to the CPU restatements of the other test modules (optqu_model,
pathwise_model, greedy_model, fullcov_model) for the length of a `with` block."""
import contextlib
import math

import numpy as np
import torch
from torch.nn.functional import softplus

from oracle import tgp_oracle as orc

F64 = torch.float64
SQRT5 = math.sqrt(5.0)
K4 = ("scale_matern52", "scale_rq@0.5", "scale_rq@2", "scale_rq@50")


def is_mine(kind):
    return isinstance(kind, str) and (kind == "scale_matern52" or kind.startswith("scale_rq@"))


def alpha_of(kind):
    return float(kind.split("@")[1]) if kind.startswith("scale_rq@") else None


def hip_name(kind):
    return kind.split("@")[0]


def hip_args(kind, raw_os):
    """(kernel name, raw_os) as the package takes them: alpha packed behind the raw output scale for the RQ settings."""
    if alpha_of(kind) is None:
        return kind, raw_os
    return "scale_rq", torch.cat((raw_os.reshape(-1)[:1], torch.tensor([alpha_of(kind)], dtype=F64, device=raw_os.device)))


def from_d2(d2, s2, kind):
    """k from the squared scaled distance (a torch tensor)."""
    if kind == "scale_matern52":
        r = d2.clamp_min(1e-30).sqrt()
        return s2 * (SQRT5 * r + 1.0 + (5.0 / 3.0) * r ** 2) * torch.exp(-SQRT5 * r)
    a = alpha_of(kind)
    return s2 * (1.0 + d2 / (2.0 * a)).pow(-a)


def gweight(d2, s2, kind):
    """k_g = -2 dk/d(d2), closed form (the table of include/tgp_hip.h's implementation)."""
    if kind == "scale_matern52":
        r = d2.clamp_min(1e-30).sqrt()
        return s2 * (5.0 / 3.0) * (1.0 + SQRT5 * r) * torch.exp(-SQRT5 * r)
    a = alpha_of(kind)
    return s2 * (1.0 + d2 / (2.0 * a)).pow(-a - 1.0)


def kernel(X1, X2, raw_ls, raw_os, kind):
    """K(X1, X2) from exact pairwise differences of the scaled rows (optqu_model.kernel's form); differentiable."""
    ls = softplus(raw_ls).reshape(1, -1)
    d2 = (((X1 / ls).unsqueeze(1) - (X2 / ls).unsqueeze(0)) ** 2).sum(-1)
    return from_d2(d2, softplus(raw_os).reshape(()), kind)


def gpytorch_kernel(kind):
    """f(X1, X2, raw_lengthscale, raw_outputscale) in gpytorch's op order, the form of oracle.tgp_oracle.scale_matern32."""
    def f(X1, X2, raw_lengthscale, raw_outputscale):
        ls = softplus(raw_lengthscale).reshape(1, -1)
        mean = X1.reshape(-1, X1.shape[-1]).mean(0, keepdim=True)
        a = (X1 - mean) / ls
        b = (X2 - mean) / ls
        shift = a.mean(-2, keepdim=True)
        a = a - shift
        b = b - shift
        sq = a.pow(2).sum(-1, keepdim=True) - 2.0 * a.matmul(b.transpose(-2, -1)) + b.pow(2).sum(-1, keepdim=True).transpose(-2, -1)
        # (gpytorch's RQKernel takes the squared distance, clamped at zero by its postprocess; MaternKernel the clamped root)
        return from_d2(sq.clamp_min(0.0), softplus(raw_outputscale).reshape(()), kind)
    return f


for _kind in K4:
    orc.KERNELS.setdefault(_kind, gpytorch_kernel(_kind))


@contextlib.contextmanager
def patched(module):
    """Inside the block `module`'s kernel formulas know the kinds of this file as well: optqu_model / pathwise_model.kernel,
    greedy_model.kernel and kernel_column, fullcov_model.kernel_matrix.  Their own kinds go to their own code."""
    saved = {}

    def wrap(name, mine):
        orig = getattr(module, name, None)
        if orig is None:
            return
        saved[name] = orig

        def f(*a, **kw):
            kind = kw.get("kernel", a[-1] if a and isinstance(a[-1], str) else None)
            return mine(*a, **kw) if is_mine(kind) else orig(*a, **kw)
        setattr(module, name, f)

    def column(A, pj, s2, kind):      # greedy_model.kernel_column: numpy in, numpy out
        A = torch.from_numpy(np.asarray(A))
        return from_d2(((A - A[pj:pj + 1]) ** 2).sum(-1), s2, kind).numpy()

    wrap("kernel", kernel)
    wrap("kernel_column", column)
    wrap("kernel_matrix", lambda X1, X2, raw_ls, raw_os, kernel="scale_rbf": globals()["kernel"](X1, X2, raw_ls, raw_os, kernel))
    try:
        yield module
    finally:
        for name, orig in saved.items():
            setattr(module, name, orig)


def oracle_case(N, D, M, flow, S, kind, seed=6, lengthscale=None):
    """orc.synthetic_problem + the oracle's ELBO and gradients under `kind`, in the dict test_gpu_parity.run_hip and compare
    take; `hip` is the same dict with the kernel's name and raw output scale as the package takes them.  `lengthscale`: every
    dimension's, in place of the problem's own (about 2); `cond` = cond(K_ZZ)."""
    prob = orc.synthetic_problem(N, D, M, seed=seed, flow=flow, S=S)
    if lengthscale is not None:
        prob["params"]["raw_lengthscale"] = torch.log(torch.expm1(torch.full((D,), float(lengthscale), dtype=F64)))
    (elbo, ell, kld), og = orc.elbo_and_grads(prob["X"], prob["Y"], prob["params"], prob["N_total"], prob["program"], prob["xs"],
                                              prob["ws"], prob["rowp"], kernel=kind)
    g = dict(prob)
    pp = prob["params"]
    g["cond"] = float(torch.linalg.cond(kernel(pp["Z"], pp["Z"], pp["raw_lengthscale"], pp["raw_outputscale"], kind)))
    g.update(kernel=kind, ELBO=elbo, ELL=ell, KLD=kld, g_Z=og["Z"], g_raw_lengthscale=og["raw_lengthscale"],
             g_raw_outputscale=og["raw_outputscale"], g_m=og["m"], g_Lam=og["Lam"], g_log_var_noise=og["log_var_noise"])
    if "theta" in og:
        g["g_theta"] = og["theta"]
    if "rowp" in og:
        g["g_rowp"] = og["rowp"]
    hip = dict(g)
    name, ro = hip_args(kind, prob["params"]["raw_outputscale"])
    hip["kernel"], hip["params"] = name, dict(prob["params"], raw_outputscale=ro)
    return g, hip


# ---- greedy conditional-variance selection: the recurrence and the runner-up margin ----------------------------------------
GREEDY_CASES = ((65, 4, 17), (257, 8, 64))        # (N, D, M)
GREEDY_MARGIN = 1e-6                              # x the pick's d: below it, two rounding routes may pick different rows


# The seed of each case: the first of 1, 2, ... whose CPU recurrence keeps the runner-up more than 2e-6 away at every pick (far rows
# of a light-tailed kernel all sit at d = s2 (1 - 1e-10): most seeds have a near tie somewhere).  Chosen from the CPU recurrence
# alone; the not-gpu test asserts the margin of every one.
GREEDY_SEEDS = {(65, 4, 17, "scale_matern52"): 4, (65, 4, 17, "scale_rq@50"): 12, (257, 8, 64, "scale_matern52"): 2}


def greedy_case(N, D, M, kind):
    import greedy_model as gm
    return dict(gm.make_case(N, M, D, "scale_rbf", seed=GREEDY_SEEDS.get((N, D, M, kind), 1)), kernel=kind)


def greedy(p):
    """greedy_model.greedy (the CPU recurrence) under `p["kernel"]`, plus `margin` = min of gap / dmax over the picks after the
    first: before any pick every row has d = s2 exactly, an exact tie that both sides break by the smallest index."""
    import greedy_model as gm
    with patched(gm):
        r = gm.greedy(p)
    r["margin"] = float((r["gap"] / r["dmax"])[1:].min())
    return r


def spectral_error(kind, R2, omega, seed=0):
    """max |Phi Phi^T - K| / s2 on 64 seeded rows in D = 4 at unit length-scales: what the frequencies `omega` (R2, 4) leave."""
    import pathwise_model as pm
    g = torch.Generator().manual_seed(11 + seed)
    X = torch.randn(64, 4, dtype=F64, generator=g)
    raw_ls = torch.full((4,), math.log(math.expm1(1.0)), dtype=F64)
    raw_os = torch.tensor([0.6], dtype=F64)
    Phi = pm.features(X, raw_ls, raw_os, omega)
    return float((Phi @ Phi.T - kernel(X, X, raw_ls, raw_os, kind)).abs().max() / softplus(raw_os))
