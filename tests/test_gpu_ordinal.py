"""GPU (-m gpu): the ordinal (cumulative-probit) likelihood (TGP_LIK_ORDINAL: ordered classes, fixed bin edges, the flow learns
their spacing) through every layer -- the stand-alone ELL kernel and its gradients against torch autograd (tests/ordinal_model.py
restates the formula), the extremes, targets outside the classes, the prediction kernel, the training step (general-M path at
every M) against the CPU restatement, K = 2 against the Bernoulli kernel, the model classes with predictive_pmf, the refusals,
the natural-gradient step, a short training run on synthetic_ratings and the CLI.

Every comparison first asserts the range condition of tests/ordinal_model.py on its inputs: every bin at least 1e-3 sigma wide."""
import math
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import REPO, rel_err

import ordinal_model as OM
from oracle import tgp_oracle as O
from test_gpu_poisson import _case, _dev, _hermite, _spec

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL_VAL, TOL_GRAD = 1e-9, 1e-7
F64 = torch.float64
AFFINE = 0


@pytest.fixture(autouse=True)
def _f64():
    from tgp.pytorch_amd import config as cg
    old = torch.get_default_dtype()
    cg.set_maximum_precission()
    cg.device = DEV
    yield
    torch.set_default_dtype(old)


def _lvn(var):
    return torch.tensor([math.log(var)], dtype=F64)


def _flow_inverse(t, program, theta, rowp):
    """mu with G(mu) = t, by bisection on [-2000, 2000] (the flows are monotone; flows_med_arcsl2 decreases, and grows like a
    logarithm): where the latent has to sit for the classes of the centred default edges to occur, whatever the flow's own
    direction, offset and scale."""
    G = lambda x: OM.flow_any(x.reshape(1, -1), program, theta, rowp).reshape(-1)
    lo, hi = torch.full_like(t, -2000.0), torch.full_like(t, 2000.0)
    rising = G(hi) > G(lo)
    for _ in range(80):
        mid = 0.5 * (lo + hi)
        left = (G(mid) < t) == rising                   # the root lies to the right of mid
        lo, hi = torch.where(left, mid, lo), torch.where(left, hi, mid)
    return 0.5 * (lo + hi)


def _inputs(case, N, K, var):
    """The inputs of the likelihood comparisons, seeded by N: mu with G(mu) = 1.2 randn, v = 0.3 rand (the first seven rows at
    -1e-12), the default edges of K classes and Y drawn from the model at G(mu)."""
    g = torch.Generator().manual_seed(N)
    t = 1.2 * torch.randn(N, generator=g, dtype=F64)
    v = 0.3 * torch.rand(N, generator=g, dtype=F64)
    v[:7] = -1e-12
    program, theta, rowp = _case(case, N, g)
    mu = _flow_inverse(t, program, theta, rowp)
    edges, lvn = OM.default_edges(K), _lvn(var)
    Y = OM.sample_classes(OM.flow_any(mu.reshape(1, -1), program, theta, rowp).reshape(-1), lvn, edges, g)
    return mu, v, Y, program, theta, rowp, edges, lvn


def _lp_close(a, b):
    """Row by row |a - b| / max(1, |b|): a log-probability near 0 says p = 1 - 1e-16, so its absolute scale is 1."""
    return float(((a - b).abs() / b.abs().clamp(min=1.0)).max())


# ---- 1. the stand-alone ELL kernel against autograd --------------------------------------------------------------------
CASES = ["empty", "sal2", "tanh3x2", "flows_med_arcsl2", "idsal"]


# 32, 16 and 4 lanes per row; then four nodes in flight per lane at 32 and at 16 lanes per row
@pytest.mark.parametrize("var", [0.07, 1.0])
@pytest.mark.parametrize("K", [5, 2])
@pytest.mark.parametrize("N,S", [(300, 32), (4000, 32), (13000, 32), (300, 80), (4000, 40)],
                         ids=["300", "4000", "13000", "300-S80", "4000-S40"])
@pytest.mark.parametrize("case", CASES)
def test_ell_kernel_matches_autograd(case, N, S, K, var):
    from tgp.pytorch_amd import ops
    mu, v, Y, program, theta, rowp, edges, lvn = _inputs(case, N, K, var)
    assert OM.min_bin_width(lvn, edges) >= OM.MIN_WIDTH
    assert sorted(set(Y.tolist())) == [float(k) for k in range(K)]          # drawn from the model: every class occurs
    xs, ws = _hermite(S)
    P, RP = (0 if theta is None else theta.numel()), (0 if rowp is None else rowp.shape[1])
    scale = 3.5
    res = ops.ell_ordinal(Y.to(DEV), mu.to(DEV), v.to(DEV), lvn.to(DEV), edges.to(DEV), _spec(program, P, RP), _dev(theta), S,
                          _dev(rowp), scale=scale)
    wrt = [mu.clone().requires_grad_(True), v.clone().requires_grad_(True), lvn.clone().requires_grad_(True)]
    th = theta.clone().requires_grad_(True) if theta is not None else None
    rp = rowp.clone().requires_grad_(True) if rowp is not None else None
    ell = OM.ell_torch(Y, wrt[0], wrt[1], wrt[2], edges, program, th, xs, ws, rp, scale)
    extra = [t for t in (th, rp) if t is not None]
    grads = torch.autograd.grad(ell, wrt + extra)
    gv = grads[1].clone()
    gv[:7] = 0.0                                        # v <= 0: the adjoint of v is 0
    errs = {"ell": rel_err(res["ell"].cpu(), ell.detach()), "g_mu": rel_err(res["g_mu"].cpu(), grads[0]),
            "g_v": rel_err(res["g_v"].cpu(), gv), "g_lvn": rel_err(res["g_lvn"].cpu(), grads[2])}
    if th is not None:
        errs["g_theta"] = rel_err(res["g_theta"].cpu(), grads[3])
    if rp is not None:
        errs["g_rowp"] = rel_err(res["g_rowp"].cpu(), grads[-1])
    print(errs)
    assert errs.pop("ell") < TOL_VAL
    assert torch.all(res["g_v"][:7].cpu() == 0)
    for k, e in errs.items():
        assert e < TOL_GRAD, (k, e)


# ---- 2. extremes ----------------------------------------------------------------------------------------------------------
X_EDGES = [-1.5, 0.0, 1e-3, 1.5]           # K = 5 at sigma = 1: the middle bin is 1e-3 sigma wide
X_MU = [1.5 + 1e8, 1.5 + 1e8, -1.5 - 1e8, -1.5 - 1e8, 0.3]
X_V = [0.0, 0.3, 2.0, 0.3, 0.3]
X_Y = [0.0, 4.0, 4.0, 0.0, 2.0]            # far class, near class, far class, near class, the narrow bin


def test_extremes():
    """g 1e8 sigma above the top edge and below the bottom one, at the far class (rows 0, 2; row 0 with v = 0) and at the near
    class (rows 1, 3), and the narrow middle bin (row 4), each row in a launch of its own so that the sums are the row's: every
    output is finite; the value of every row and the gradients of rows 1, 3, 4 equal the restatement and its autograd.

    The gradients of the far rows are held against Mills' ratio instead.  There p = Phi(-a_s) with a_s = |g_s - b| / sigma ~ 1e8 at
    every node, so d log p / dg = -+lambda(a_s) / sigma and d log p / d eta = a_s lambda(a_s) / 2 with lambda(a) = phi(a) / Phi(-a) =
    a + 1/a - 2/a^3 + ..: a + 1/a to far below one rounding.  Autograd of the restatement cannot serve at that distance:
    torch's backward of log_ndtr forms exp(-x^2 / 2 - log_ndtr(x)), the difference of two numbers near 5e15 whose spacing is 1, and
    returns 1.94e8 for lambda(1e8) (its forward value is right and is what the rows' values are compared with)."""
    from tgp.pytorch_amd import lib as L
    from tgp.pytorch_amd import ops
    S = 16
    xs, ws = _hermite(S)
    wn = ws / math.sqrt(math.pi)
    edges, lvn = torch.tensor(X_EDGES, dtype=F64), torch.zeros(1, dtype=F64)
    assert OM.min_bin_width(lvn, edges) >= OM.MIN_WIDTH
    ident = [(AFFINE, 0, 0, 0)]                                      # G(f) = 1 f + 0: the predictive's sweep instead of its closed form
    th1 = torch.tensor([1.0, 0.0], dtype=F64)
    for n in range(5):
        mu, v, Y = (torch.tensor([t[n]], dtype=F64) for t in (X_MU, X_V, X_Y))
        res = ops.ell_ordinal(Y.to(DEV), mu.to(DEV), v.to(DEV), lvn.to(DEV), edges.to(DEV), _spec([], 0), None, S)
        out = {k: res[k].cpu().reshape(-1) for k in ("ell", "g_mu", "g_v", "g_lvn")}
        for k, t in out.items():
            assert torch.isfinite(t).all(), (n, k)
        m, vv, ll = (t.clone().requires_grad_(True) for t in (mu, v, lvn))
        ell = OM.ell_torch(Y, m, vv, ll, edges, [], None, xs, ws)
        print("row", n, {k: float(t) for k, t in out.items()}, "restatement ell", float(ell.detach()))
        assert _lp_close(out["ell"], ell.detach().reshape(-1)) < TOL_VAL
        if n in (0, 2):
            b, sign = (X_EDGES[0], -1.0) if n == 0 else (X_EDGES[-1], 1.0)
            gs = mu + torch.sqrt(2.0 * v) * xs
            a = (gs - b).abs()
            lam = a + 1.0 / a
            ref = {"g_mu": (wn * sign * lam).sum(), "g_lvn": (wn * 0.5 * a * lam).sum(),
                   "g_v": (wn * sign * lam * xs).sum() / torch.sqrt(2.0 * v) if float(v) > 0 else torch.zeros(())}
        else:
            gm, gv, gl = torch.autograd.grad(ell, [m, vv, ll])
            ref = {"g_mu": gm, "g_v": gv, "g_lvn": gl}
        for k, r in ref.items():
            assert rel_err(out[k], r.reshape(-1)) < TOL_GRAD, (n, k, float(out[k]), float(r))
        if float(v) == 0.0:
            assert float(out["g_v"]) == 0.0
        # the predictive log pmf of the row: the closed form of the empty program, and the sweep's log-sum-exp
        for prog, th in (([], None), (ident, th1)):
            _, _, lp = ops.predict(mu.to(DEV), v.to(DEV), lvn.to(DEV), _spec(prog, 0 if th is None else 2), _dev(th), S, Y=Y.to(DEV),
                                   lik=L.LIK_ORDINAL, df=edges.to(DEV))
            _, _, rlp = OM.pred_torch(mu, v, lvn, edges, prog, th, xs, ws, Y=Y)
            print("row", n, "logp", float(lp), "restatement", float(rlp))
            assert torch.isfinite(lp).all() and _lp_close(lp.cpu(), rlp) < TOL_VAL


def test_the_second_double_behind_the_noise_pointer_is_the_number_of_classes():
    """A raw _ell_quad call with {eta, 3, -0.7, 0.9, 1, 6} behind the noise pointer is the K = 3 likelihood with edges (-0.7, 0.9):
    the two doubles past the K - 1 edges are not read (were K taken for 5, class 2 would end at the edge 1)."""
    from tgp.pytorch_amd import lib as L
    from tgp.pytorch_amd import ops
    N, S = 300, 32
    g = torch.Generator().manual_seed(5)
    mu, v = 1.2 * torch.randn(N, generator=g, dtype=F64), 0.3 * torch.rand(N, generator=g, dtype=F64)
    edges, lvn = torch.tensor([-0.7, 0.9], dtype=F64), _lvn(0.3)
    assert OM.min_bin_width(lvn, edges) >= OM.MIN_WIDTH
    Y = OM.sample_classes(mu, lvn, edges, g)
    assert sorted(set(Y.tolist())) == [0.0, 1.0, 2.0]
    xs, ws = _hermite(S)
    noise = torch.cat((lvn, torch.tensor([3.0], dtype=F64), edges, torch.tensor([1.0, 6.0], dtype=F64))).to(DEV)
    res = ops._ell_quad(Y.to(DEV), mu.to(DEV), v.to(DEV), noise, _spec([], 0), None, S, None, 1.0, L.LIK_ORDINAL)
    m = mu.clone().requires_grad_(True)
    ell = OM.ell_torch(Y, m, v, lvn, edges, [], None, xs, ws)
    assert rel_err(res["ell"].cpu(), ell.detach()) < TOL_VAL
    assert rel_err(res["g_mu"].cpu(), torch.autograd.grad(ell, m)[0]) < TOL_GRAD
    other = OM.ell_torch(Y, mu, v, lvn, torch.tensor([-0.7, 0.9, 1.0, 6.0], dtype=F64), [], None, xs, ws)
    assert rel_err(res["ell"].cpu(), other) > 1e-3


# ---- 3. targets outside the classes stay in bounds ----------------------------------------------------------------------
def test_out_of_range_targets_are_clamped():
    """Y = (-3, K + 7, NaN) through ops._ell_quad (check_targets is the likelihood class's and is not on this route): the kernel
    takes them for the classes (0, K - 1, 0) -- finite, and the same bits.  An ordinary run: it reads the K - 1 edges only."""
    from tgp.pytorch_amd import lib as L
    from tgp.pytorch_amd import ops
    K, S = 5, 32
    edges, lvn = OM.default_edges(K), _lvn(0.3)
    mu = torch.tensor([0.3, -0.2, 1.1], dtype=F64, device=DEV)
    v = torch.tensor([0.2, 0.1, 0.3], dtype=F64, device=DEV)
    noise = ops.ordinal_noise(lvn.to(DEV), edges)
    run = lambda Y: ops._ell_quad(torch.tensor(Y, dtype=F64, device=DEV), mu, v, noise, _spec([], 0), None, S, None, 1.0, L.LIK_ORDINAL)
    bad, good = run([-3.0, K + 7.0, float("nan")]), run([0.0, K - 1.0, 0.0])
    for k in ("ell", "g_lvn", "g_mu", "g_v"):
        assert torch.isfinite(bad[k]).all() and torch.equal(bad[k], good[k]), k
    _, _, lp_bad = ops.predict(mu, v, lvn.to(DEV), _spec([], 0), None, S, Y=torch.tensor([-3.0, K + 7.0, float("nan")], dtype=F64, device=DEV),
                               lik=L.LIK_ORDINAL, df=edges)
    _, _, lp_good = ops.predict(mu, v, lvn.to(DEV), _spec([], 0), None, S, Y=torch.tensor([0.0, K - 1.0, 0.0], dtype=F64, device=DEV),
                                lik=L.LIK_ORDINAL, df=edges)
    assert torch.isfinite(lp_bad).all() and torch.equal(lp_bad, lp_good)


# ---- 4. the prediction kernel ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [20, 50, 1, 5])      # (1: one partly filled group of four nodes; 5: a full group and a one-node tail)
@pytest.mark.parametrize("case", ["empty", "sal2", "flows_med_arcsl2", "idsal"])
def test_predict_matches_restatement(case, S):
    _predict_matches_restatement(case, S, 1000)
    if S == 5:      # the first row past a workgroup of 256, and a single row
        _predict_matches_restatement(case, S, 257)
        _predict_matches_restatement(case, S, 1)


def _predict_matches_restatement(case, S, N):
    """m1 and m2 in the project's norm (m2 = E[y^2] - m1^2 is a difference: its rounding is that of E[y^2], so a row is held to
    the largest row), logp row by row."""
    from tgp.pytorch_amd import lib as L
    from tgp.pytorch_amd import ops
    K = 5
    mu, v, Y, program, theta, rowp, edges, lvn = _inputs(case, N, K, 0.07)
    assert OM.min_bin_width(lvn, edges) >= OM.MIN_WIDTH
    xs, ws = _hermite(S)
    P, RP = (0 if theta is None else theta.numel()), (0 if rowp is None else rowp.shape[1])
    args = (mu.to(DEV), v.to(DEV), lvn.to(DEV), _spec(program, P, RP), _dev(theta), S, _dev(rowp))
    m1, m2, lp = ops.predict(*args, Y=Y.to(DEV), Y_std=7.0, lik=L.LIK_ORDINAL, df=edges.to(DEV))          # (Y_std is ignored)
    r1, r2, rlp = OM.pred_torch(mu, v, lvn, edges, program, theta, xs, ws, rowp, Y=Y)
    errs = [rel_err(m1.cpu(), r1), rel_err(m2.cpu(), r2), _lp_close(lp.cpu(), rlp)]
    print("errors m1, m2, logp:", errs)
    assert max(errs) < TOL_VAL
    if case == "empty":      # the closed form, for every class
        pmf = OM.pmf_closed(mu, v, lvn, edges)
        for k in range(K):
            _, _, lpk = ops.predict(*args, Y=torch.full((N,), float(k), dtype=F64, device=DEV), lik=L.LIK_ORDINAL, df=edges.to(DEV),
                                    want_moments=False)
            assert float((torch.exp(lpk).cpu() - pmf[:, k]).abs().max()) < TOL_VAL, k
    # without targets: moments only
    m1b, m2b, none = ops.predict(*args, lik=L.LIK_ORDINAL, df=edges.to(DEV))
    assert none is None and torch.equal(m1b, m1) and torch.equal(m2b, m2)


# ---- 5. the training step against the CPU restatement -------------------------------------------------------------------
STEPS = [(200, 3, 20, 5, "sal2", 20, "scale_rbf"), (300, 4, 150, 0, "tanh3x2", 32, "scale_rbf"),
         (256, 3, 128, 2, "none", 16, "scale_rbf"), (200, 3, 33, 2, "sal1", 20, "scale_matern32")]


@pytest.mark.parametrize("N,D,M,seed,flow,S,kernel", STEPS, ids=["sal2-M20", "tanh3x2-M150", "svgp-M128", "sal1-M33-matern32"])
def test_step_matches_cpu(N, D, M, seed, flow, S, kernel):
    """ops.elbo_step(lik=LIK_ORDINAL) against step_torch.  Both factorise K_ZZ as it stands; 1e-6 is the base of the
    restatement's jitter ladder, which a factorisation that succeeds never reaches (the step's status words are asserted 0)."""
    from tgp.pytorch_amd import lib as L
    from tgp.pytorch_amd import ops
    K = 5
    prob = O.synthetic_problem(N, D, M, seed, flow, S)
    p = {k: t.clone() for k, t in prob["params"].items()}
    p["raw_outputscale"] = O.inv_softplus(0.8).reshape(1)
    # half the problem's length-scales: 128 inducing points in three dimensions at length-scale 2 give K_ZZ a condition number of
    # 2.6e12, and the two factorisations (CPU, GPU) then differ by 7e-8 in dELBO/dZ; at length-scale 1 it is 5.7e7
    p["raw_lengthscale"] = O.inv_softplus(0.5 * torch.nn.functional.softplus(p["raw_lengthscale"]))
    p["m"] = 0.5 * p["m"]
    p["log_var_noise"] = _lvn(0.3)
    edges = OM.default_edges(K)
    assert OM.min_bin_width(p["log_var_noise"], edges) >= OM.MIN_WIDTH
    g = torch.Generator().manual_seed(100 + seed)
    w = torch.randn(D, generator=g, dtype=F64)
    Y = OM.sample_classes(1.5 * torch.sin(prob["X"] @ w), p["log_var_noise"], edges, g).reshape(N, 1)
    assert sorted(set(Y.reshape(-1).tolist())) == [float(k) for k in range(K)]
    program = prob["program"]
    if program is None:
        p.pop("theta", None)
    (elbo, ell, kld), rg = OM.step_torch(prob["X"], Y, p, edges, float(N), program, prob["xs"], prob["ws"], kernel, jitter=1e-6)
    theta = p.get("theta") if program is not None else None
    spec = _spec(program, 0 if theta is None else theta.numel())

    def run():
        out, grads, status, _ = ops.elbo_step(prob["X"].to(DEV), Y.to(DEV), _dev(p["Z"]), _dev(p["raw_lengthscale"]),
                                              _dev(p["raw_outputscale"]), _dev(p["m"]), _dev(p["Lam"]), _dev(p["log_var_noise"]),
                                              float(N), flow=spec, theta=_dev(theta), S=S, kernel=kernel, lik=L.LIK_ORDINAL,
                                              df=edges.to(DEV))
        torch.cuda.synchronize()
        assert int(status[0]) == 0 and int(status[1]) == 0
        return out.cpu(), {k: t.cpu() for k, t in grads.items()}

    out, grads = run()
    errs = {"elbo": rel_err(out[0], elbo), "ell": rel_err(out[1], ell), "kld": rel_err(out[2], kld)}
    pairs = [("Z", "Z"), ("raw_ls", "raw_lengthscale"), ("raw_os", "raw_outputscale"), ("m", "m"), ("Lam", "Lam"),
             ("lvn", "log_var_noise")]
    if theta is not None:
        pairs.append(("theta", "theta"))
    for k_hip, k_ref in pairs:
        errs["g_" + k_hip] = rel_err(grads[k_hip], rg[k_ref])
    print(errs)
    for k in ("elbo", "ell", "kld"):
        assert errs.pop(k) < TOL_VAL, k
    for k, e in errs.items():
        assert e < TOL_GRAD, (k, e)
    assert grads["lvn"].numel() == 1 and float(grads["lvn"].abs().max()) > 0.0
    assert float(torch.triu(grads["Lam"], 1).abs().max()) == 0.0
    out2, grads2 = run()
    assert torch.equal(out, out2) and all(torch.equal(grads[k], grads2[k]) for k in grads)


# ---- 6. K = 2 is the Bernoulli likelihood ---------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["empty", "sal2", "idsal"])
def test_two_classes_are_bernoulli(case):
    """Edge 0 and sigma = 1: class 1 has probability Phi(G(f0)), the Bernoulli kernel's, on the same rows."""
    from tgp.pytorch_amd import ops
    N, S = 300, 32
    mu, v, Y, program, theta, rowp, edges, lvn = _inputs(case, N, 2, 1.0)
    assert edges.tolist() == [0.0] and float(lvn) == 0.0
    P, RP = (0 if theta is None else theta.numel()), (0 if rowp is None else rowp.shape[1])
    args = (_spec(program, P, RP), _dev(theta), S, _dev(rowp))
    a = ops.ell_ordinal(Y.to(DEV), mu.to(DEV), v.to(DEV), lvn.to(DEV), edges.to(DEV), *args, scale=2.0)
    b = ops.ell_bernoulli(Y.to(DEV), mu.to(DEV), v.to(DEV), *args, scale=2.0)
    assert rel_err(a["ell"].cpu(), b["ell"].cpu()) < TOL_VAL
    for k in ("g_mu", "g_v") + (("g_theta",) if P else ()) + (("g_rowp",) if RP else ()):
        assert rel_err(a[k].cpu(), b[k].cpu()) < TOL_GRAD, k


# ---- 7. the model classes ---------------------------------------------------------------------------------------------------
def _build_model(X, M=20, tgp=False, mean="zero", var_scale=1e-5, num_outputs=1, flow=None):
    from tgp.pytorch_amd import flows as G
    from tgp.pytorch_amd.kernels import instance_kernel
    from tgp.pytorch_amd.likelihoods import Ordinal
    from tgp.pytorch_amd.models import sparse_MF_GP, sparse_MF_SP
    D = X.shape[1]
    K = instance_kernel("scale_rbf", ard_num_dim=D, num_multioutput=num_outputs, kernel_is_shared=False,
                        init_params={"length_scale": 2.0, "kernel_scale": 2.0, "noisy_variance": 1e-6})
    ip = {"variational_distribution": {"variance_scale": var_scale, "mean_scale": 0.0}}
    lik = Ordinal(5, noise_init=0.3)
    if tgp:
        model = sparse_MF_SP([mean, K], X, X[:M].clone(), X.shape[0], lik, num_outputs, True, False, False, False, False,
                             [G.SAL(1) if flow is None else flow] * num_outputs, "single", 0.0, init_params=ip)
    else:
        model = sparse_MF_GP([mean, K], X, X[:M].clone(), X.shape[0], lik, num_outputs, True, False, False, False, False, 0.0,
                             init_params=ip)
    return model.to(DEV)


@pytest.fixture(scope="module")
def ratings():
    from tgp.pytorch_amd import synthetic
    X, Y = synthetic.synthetic_ratings()
    return torch.tensor(X, dtype=F64), torch.tensor(Y, dtype=F64)


@pytest.mark.parametrize("tgp", [False, True], ids=["svgp", "tgp"])
def test_model_and_pmf(ratings, tgp):
    from tgp.pytorch_amd import ops
    from tgp.pytorch_amd.flow import compile_flow
    X, Y = ratings
    X, Y = X[:300], Y[:300]
    K = 5
    model = _build_model(X, tgp=tgp)
    gen = torch.Generator().manual_seed(11)
    with torch.no_grad():       # a q(u) away from its initial value
        model.q_U.variational_mean.data = (0.5 * torch.randn(1, 20, generator=gen, dtype=F64)).to(DEV)
        model.q_U.chol_variational_covar.data = (0.2 * torch.eye(20, dtype=F64) +
                                                 0.02 * torch.randn(20, 20, generator=gen, dtype=F64).tril()).reshape(1, 20, 20).to(DEV)
    Xd, Yd = X.to(DEV), Y.to(DEV)
    model.set_is_training(True)
    elbo, ell, kld = model.ELBO(Xd, Yd)
    Z, rl, ro, m, Lam, lvn = (None if t is None else t.detach() for t in model._raw_params())
    edges = model.likelihood.bin_edges
    assert lvn.numel() == 1 and OM.min_bin_width(lvn.cpu(), edges.cpu()) >= OM.MIN_WIDTH
    spec, theta_list, _ = compile_flow(model.G_matrix[0])
    theta = torch.stack([q.detach().reshape(()) for q in theta_list]) if theta_list else None
    assert (spec.nblk > 0) == tgp
    mu, v = ops.qf_moments(Xd, Z, rl, ro, m, Lam, kernel="scale_rbf")
    comp = ops.ell_ordinal(Yd, mu, v, lvn, edges, spec, theta, model.quad_points, scale=1.0)
    kl = ops.kl_whitened(m, Lam)[0]
    assert rel_err(ell.detach().cpu(), comp["ell"].cpu()) < TOL_VAL and rel_err(kld.detach().cpu(), kl.cpu()) < TOL_VAL
    assert rel_err(elbo.detach().cpu(), (comp["ell"] - kl).cpu()) < TOL_VAL
    (-elbo).backward()
    assert all(q.grad is not None and torch.isfinite(q.grad).all() for q in model.parameters())
    glv = model.likelihood.log_var_noise.grad
    assert float(glv.abs().max()) > 0 and rel_err(-glv.reshape(-1).cpu(), comp["g_lvn"].reshape(-1).cpu()) < TOL_GRAD
    if tgp:
        assert all(float(q.grad.abs().max()) > 0 for n, q in model.named_parameters() if n.startswith("G_matrix"))
    assert model.likelihood.bin_edges.grad is None and not model.likelihood.bin_edges.requires_grad

    model.set_is_training(False)
    n = 50
    lp_sum, (m1, m2) = model.test_log_likelihood(Xd[:n], Yd[:n], return_moments=True, Y_std=torch.ones(1, device=DEV))
    _, _, lp = ops.predict(mu[:n], v[:n], lvn, spec, theta, model.quad_points, Y=Yd[:n].reshape(-1), lik=ops.L.LIK_ORDINAL, df=edges)
    assert lp_sum.shape == (1,) and m1.shape == (1, n) and m2.shape == (1, n) and rel_err(lp_sum.cpu(), lp.sum().cpu()) < TOL_VAL
    pm1, pm2, _, _ = model.predictive_distribution(Xd[:n])
    assert pm1.shape == (1, n) and torch.equal(pm1, m1) and torch.equal(pm2, m2)
    pmf = model.predictive_pmf(Xd[:n], K - 1)
    assert pmf.shape == (n, K) and not pmf.requires_grad and bool((pmf >= 0).all())
    assert float((pmf.sum(1) - 1.0).abs().max()) < 1e-12
    xs, ws = _hermite(model.quad_points)
    program = [tuple(int(t) for t in b) for b in spec.blocks]
    th = None if theta is None else theta.cpu()
    ref = torch.stack([torch.exp(OM.pred_torch(mu[:n].cpu(), v[:n].cpu(), lvn.cpu(), edges.cpu(), program, th, xs, ws,
                                               Y=torch.full((n,), float(k), dtype=F64))[2]) for k in range(K)], 1)
    assert float((pmf.cpu() - ref).abs().max()) < TOL_VAL
    kk = torch.arange(K, dtype=F64, device=DEV)
    assert rel_err((pmf * kk).sum(1).cpu(), m1.reshape(-1).cpu()) < TOL_VAL
    assert rel_err(((pmf * kk * kk).sum(1) - (pmf * kk).sum(1) ** 2).cpu(), m2.reshape(-1).cpu()) < TOL_VAL
    at_y = pmf[torch.arange(n, device=DEV), Yd[:n].reshape(-1).long()]
    assert rel_err(at_y.cpu(), torch.exp(lp).cpu()) < TOL_VAL
    rps = model.predictive_crps(Xd[:n], Yd[:n], kmax=K - 1)             # the ranked probability score
    assert rps.shape == (1, n) and bool((rps >= 0).all()) and bool((rps <= K - 1).all())
    s, _, _ = model.sample_from_predictive_distribution(Xd[:n], S=4)
    assert s.shape == (1, 4, n, 1) and bool((s >= 0).all()) and bool((s <= K - 1).all()) and bool((s == torch.round(s)).all())


def test_refusals(ratings):
    from tgp.pytorch_amd import flows as G
    X, Y = ratings
    X, Y = X[:100], Y[:100]
    with pytest.raises(NotImplementedError, match="ordinal"):           # ID_TGP
        _build_model(X, tgp=True, flow=G.SAL(1, input_dependent=True, input_dim=X.shape[1], num_hidden_layers=1, batch_norm=0,
                                             dropout=0.5, hidden_dim=8, hidden_activation="tanh", inference="MC_dropout"))
    with pytest.raises(NotImplementedError, match="one output"):
        _build_model(X, num_outputs=2)
    model = _build_model(X)
    with pytest.raises(NotImplementedError, match="ordinal"):
        model.set_optimal_qu(X.to(DEV), Y.to(DEV))
    model.set_is_training(False)
    with pytest.raises(NotImplementedError, match="ordinal"):
        model.predictive_quantiles(X.to(DEV), [0.5])
    with pytest.raises(ValueError, match="integer in"):
        model.ELBO(X.to(DEV), Y.to(DEV) + 0.5)
    with pytest.raises(ValueError, match="integer in"):
        model.ELBO(X.to(DEV), Y.to(DEV) + 5.0)
    q = model.posterior_quantiles(X.to(DEV), [0.1, 0.9])                  # the quantiles of G(f) go through the unchanged code
    assert q.shape == (1, 2, 100) and bool((q[0, 0] < q[0, 1]).all())


def test_linear_mean_takes_the_affine_head_block(ratings):
    """A linear mean goes the route of the other flow likelihoods: a per-row affine block (1, m(x_n)) at the head of the
    program in training, m(X) inside mu in prediction.  The ELBO equals the stand-alone likelihood at mu + m(X)."""
    from tgp.pytorch_amd import ops
    X, Y = ratings
    X, Y = X[:300].to(DEV), Y[:300].to(DEV)
    model = _build_model(X.cpu(), mean="linear")
    with torch.no_grad():
        model.mean_function.a.data.copy_(torch.tensor([0.2, -0.1], dtype=F64).reshape(model.mean_function.a.shape))
        model.mean_function.b.data.fill_(0.3)
    model.set_is_training(True)
    elbo, ell, kld = model.ELBO(X, Y)
    (-elbo).backward()
    ga = model.mean_function.a.grad
    assert ga is not None and torch.isfinite(ga).all() and float(ga.abs().max()) > 0
    lik = model.likelihood
    with torch.no_grad():
        mu, v = model.marginal_variational_qf_parameters(X, diagonal=True, is_duvenaud=False)
        comp = ops.ell_ordinal(Y, mu.reshape(-1).contiguous(), v.reshape(-1).contiguous(), lik.noise().detach().contiguous(),
                               lik.bin_edges, _spec([], 0), None, model.quad_points)
    assert rel_err(ell.detach().cpu(), comp["ell"].cpu()) < TOL_VAL
    # dELL/da = X^T dELL/dmu: the adjoint of mu from the same launch
    assert rel_err(-ga.reshape(-1).cpu(), (X.t() @ comp["g_mu"]).cpu()) < TOL_GRAD
    model.set_is_training(False)
    m1, _, mq, _ = model.predictive_distribution(X[:20])
    assert m1.shape == (1, 20) and rel_err(mq.reshape(-1).cpu(), mu.reshape(-1)[:20].cpu()) < TOL_VAL


# ---- 8. the natural-gradient step of q(u) -----------------------------------------------------------------------------------
@pytest.mark.parametrize("tgp", [False, True], ids=["svgp", "tgp"])
def test_one_natgrad_step_from_the_constructors_qu_raises_the_elbo(ratings, tgp):
    """natgrad_step_qu(lr = 1) from q(u) = N(0, I): q_U afterwards is ops.qf_moments -> ops.ell_ordinal at scale N / MB ->
    ops.natgrad_qu on the same inputs, and the ELBO is higher (cumulative probit is log-concave in g: no site is clamped for
    SVGP)."""
    from tgp.pytorch_amd import ops
    from tgp.pytorch_amd.flow import compile_flow
    X, Y = ratings
    X, Y = X[:300].to(DEV), Y[:300].to(DEV)
    model = _build_model(X.cpu(), tgp=tgp, var_scale=1.0)
    Z, rl, ro, m, Lam, lvn = (t.detach().contiguous() for t in model._raw_params())
    assert torch.equal(m.cpu(), torch.zeros(20, dtype=F64)) and torch.equal(Lam.cpu(), torch.eye(20, dtype=F64))
    spec, theta_list, _ = compile_flow(model.G_matrix[0])
    theta = torch.stack([q.detach().reshape(()) for q in theta_list]) if theta_list else None
    mu, v = ops.qf_moments(X, Z, rl, ro, m, Lam, kernel="scale_rbf")
    res = ops.ell_ordinal(Y, mu, v, lvn, model.likelihood.bin_edges, spec, theta, model.quad_points, scale=1.0)
    if not tgp:
        assert bool((res["g_v"] <= 0).all())
    m_ref, Lam_ref = ops.natgrad_qu(X, Z, rl, ro, m, Lam, mu, res["g_mu"], res["g_v"], rho=1.0, site_floor=0.0, kernel="scale_rbf")
    before = float(model.ELBO(X, Y)[0].detach())
    info = model.natgrad_step_qu(X, Y, lr=1.0)
    after = float(model.ELBO(X, Y)[0].detach())
    print("ELBO", before, "->", after)
    assert info["jitter"] == 0.0
    assert torch.equal(model.q_U.variational_mean.detach()[0], m_ref) and torch.equal(model.q_U.chol_variational_covar.detach()[0], Lam_ref)
    assert after > before


# ---- 9. a short training run ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tgp", [False, True], ids=["svgp", "tgp"])
def test_short_training_run_beats_the_class_frequencies(tgp):
    """300 Adam epochs on the seed-1 split of synthetic_ratings: the test negative log-likelihood is below that of the baseline
    that predicts the training class frequencies everywhere."""
    from tgp.pytorch_amd import config as cg
    from tgp.pytorch_amd.data import return_dataset
    from tgp.pytorch_amd.trainers import Trainer_SP_regression
    loaders, dc = return_dataset("synthetic_ratings", 10000, seed=1, options={"shuffle_train": False})
    Xtr, Ytr, Xte, Yte = dc["X_tr"], dc["Y_tr"], dc["X_te"], dc["Y_te"]
    torch.manual_seed(1)
    model = _build_model(Xtr, tgp=tgp)
    tr = Trainer_SP_regression(model, loaders, 1e20, False, False, torch.ones(1, device=DEV), -1, 100, True)
    tr.train(epochs=300, lr_ALL=0.05, opt="adam", keep_parameter_groups=True)
    assert tr._engine is None                           # the ordinal likelihood trains on the eager path
    assert len(tr.loss_arr) == 300 and -tr.loss_arr[-1] > -tr.loss_arr[0]
    model.set_is_training(False)
    lp, _ = model.test_log_likelihood(Xte.to(DEV), Yte.to(DEV), return_moments=False, Y_std=torch.ones(1, device=DEV))
    y = Yte.reshape(-1)
    freq = torch.bincount(Ytr.reshape(-1).long(), minlength=5).to(F64) / Ytr.numel()
    base_nll = -float(torch.log(freq[y.long()]).mean())
    nll = -float(lp) / y.numel()
    pmf = model.predictive_pmf(Xte.to(DEV), 4).cpu()
    acc = float((pmf.argmax(1).to(F64) == y).double().mean())
    print("%s: ELBO %.2f -> %.2f; test NLL %.4f (class frequencies %.4f); accuracy of the modal class %.3f"
          % ("TGP" if tgp else "SVGP", -tr.loss_arr[0], -tr.loss_arr[-1], nll, base_nll, acc))
    assert nll < base_nll
    res = tr.compute_metrics()                          # the trainer reports the same number
    assert abs(-res[6] - nll) < 1e-9 * abs(nll)


# ---- 10. the CLI ----------------------------------------------------------------------------------------------------------
def test_cli():
    cmd = [sys.executable, "-m", "tgp.pytorch_amd.main", "--model", "TGP", "--likelihood", "ordinal", "--dataset",
           "synthetic_ratings", "--train_test_seed_split", "1", "--num_inducing", "20", "--epochs", "30"]
    r = subprocess.run(["timeout", "-k", "10", "300"] + cmd, cwd=REPO, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert r.stdout.count("Test Negative LOGL") == 2 and "Test Accuracy (modal class)" in r.stdout
    assert "Test MAE (median class)" in r.stdout and "class frequencies" in r.stdout
