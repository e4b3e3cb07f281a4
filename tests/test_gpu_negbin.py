"""GPU (-m gpu): the negative-binomial likelihood (TGP_LIK_NEGBIN: over-dispersed counts, the flow as the log-mean, a trained
dispersion r in the noise slot) through every layer -- the stand-alone ELL kernel and its gradients, dELL/dlog r among them,
against torch autograd (tests/negbin_model.py restates the formula), the extremes, the prediction kernel, the Poisson limit at
r = 1e3, the training step (general-M path at every M) against the CPU restatement, the model classes with predictive_pmf and
predictive_crps, determinism and the CLI.

Every comparison first asserts the range conditions of tests/negbin_model.py on the CPU restatement: max G(f0) <= 10 over the
nodes with wn > 1e-14, and 1e-3 <= r <= 1e3.  The extremes are the one exception to the first (the restatement's log p forms
no exp(G)); they state their own inputs."""
import math
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import REPO, rel_err

import negbin_model as NM
import poisson_model as PM
from oracle import tgp_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL_VAL, TOL_GRAD = 1e-9, 1e-7
F64 = torch.float64
SAL, PER_ROW = 1, 4
LVN_MIN_SHARE = 1e-3       # |dELL/dlam| of the restatement must be at least this share of the rows' summed magnitudes


@pytest.fixture(autouse=True)
def _f64():
    from tgp.pytorch_amd import config as cg
    old = torch.get_default_dtype()
    cg.set_maximum_precission()
    cg.device = DEV
    yield
    torch.set_default_dtype(old)


def _spec(program, P, RP=0):
    from tgp.pytorch_amd import ops
    return ops.FlowSpec([tuple(int(v) for v in b) for b in (program or [])], P, RP, DEV)


def _hermite(S):
    return tuple(torch.tensor(a) for a in np.polynomial.hermite.hermgauss(S))


def _dev(t):
    return None if t is None else t.to(DEV).contiguous()


def _lam(r):
    return torch.tensor([math.log(r)], dtype=F64)


_CASE_CACHE = {}


def _case(case, N, g):
    """(program, theta, rowp) of a named flow case, as tests/test_gpu_poisson.py builds them; the per-row parameters of `idsal`
    come from the generator `g`."""
    if case == "idsal":
        rowp = torch.stack([0.1 * torch.randn(N, generator=g, dtype=F64), 0.8 + 0.05 * torch.randn(N, generator=g, dtype=F64)], 1)
        return [(SAL, 0, 0, PER_ROW)], None, rowp
    if case not in _CASE_CACHE:
        if case == "empty":
            _CASE_CACHE[case] = ([], None)
        else:
            prob = O.synthetic_problem(64, 4, 8, seed=5 if case == "sal2" else 0, flow=case)
            _CASE_CACHE[case] = ([tuple(int(v) for v in b) for b in prob["program"]], prob["params"]["theta"].clone())
    program, theta = _CASE_CACHE[case]
    return program, theta, None


def gamma_poisson(mean, r, g):
    """y ~ NB(mean, r) as a Gamma-Poisson mixture from the seeded generator."""
    lam = torch._standard_gamma(torch.full_like(mean, float(r)), generator=g) / float(r)
    return torch.poisson(mean * lam, generator=g)


# seeds of the inputs, by (case, N, r), where the default (N) would not satisfy the g_lvn condition on the restatement.  Checked on
# the CPU from NM.dlam_rows alone: at the default every case below has a share of 1.1e-2 or more, ten times the condition
SEEDS = {}


def _inputs(case, N, r, with_v0=True):
    """The inputs of the likelihood comparisons: mu = 0.5 randn, v = 0.3 rand (the first seven rows at -1e-12),
    Y ~ NB(exp(min(G(mu), 6)), r) as a Gamma-Poisson mixture."""
    g = torch.Generator().manual_seed(SEEDS.get((case, N, r), N))
    mu = 0.5 * torch.randn(N, generator=g, dtype=F64)
    v = 0.3 * torch.rand(N, generator=g, dtype=F64)
    if with_v0:
        v[:7] = -1e-12
    program, theta, rowp = _case(case, N, g)
    mean = torch.exp(PM.flow_any(mu.reshape(1, -1), program, theta, rowp).reshape(-1).clamp(max=6.0))
    Y = gamma_poisson(mean, r, g)
    return mu, v, Y, program, theta, rowp


def _assert_range(lam, mu, v, program, theta, xs, ws, rowp=None):
    ok, gmax, r = NM.in_range(lam, mu, v, program, theta, xs, ws, rowp)
    print("max G = %.3f, r = %g" % (gmax, r))
    assert ok, (gmax, r)


def lvn_share(Y, mu, v, lam, program, theta, xs, ws, rowp=None):
    """|sum of the rows' dELL/dlam| over the sum of their magnitudes, on the restatement."""
    rows = NM.dlam_rows(Y, mu, v, lam, program, theta, xs, ws, rowp)
    return float(rows.sum().abs() / rows.abs().sum())


# ---- 1. the stand-alone ELL kernel against autograd --------------------------------------------------------------------
CASES = ["empty", "sal2", "tanh3x2", "idsal"]


# 32, 16 and 4 lanes per row; then four nodes in flight per lane
@pytest.mark.parametrize("r", [0.5, 3.0, 50.0])
@pytest.mark.parametrize("N,S", [(300, 32), (4000, 32), (13000, 32), (300, 80)], ids=["300", "4000", "13000", "300-S80"])
@pytest.mark.parametrize("case", CASES)
def test_ell_kernel_matches_autograd(case, N, S, r):
    from tgp.pytorch_amd import ops
    mu, v, Y, program, theta, rowp = _inputs(case, N, r)
    xs, ws = _hermite(S)
    lam = _lam(r)
    _assert_range(lam, mu, v, program, theta, xs, ws, rowp)
    share = lvn_share(Y, mu, v, lam, program, theta, xs, ws, rowp)
    print("|dELL/dlam| / sum of the rows' magnitudes = %.3e" % share)
    assert share >= LVN_MIN_SHARE
    P, RP = (0 if theta is None else theta.numel()), (0 if rowp is None else rowp.shape[1])
    scale = 3.5
    res = ops.ell_negbin(Y.to(DEV), mu.to(DEV), v.to(DEV), lam.to(DEV), _spec(program, P, RP), _dev(theta), S, _dev(rowp),
                         scale=scale)
    wrt = [mu.clone().requires_grad_(True), v.clone().requires_grad_(True), lam.clone().requires_grad_(True)]
    th = theta.clone().requires_grad_(True) if theta is not None else None
    rp = rowp.clone().requires_grad_(True) if rowp is not None else None
    ell = NM.ell_torch(Y, wrt[0], wrt[1], wrt[2], program, th, xs, ws, rp, scale)
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
@pytest.mark.parametrize("r", [1e-3, 1e3])
def test_extremes(r):
    """Means from e^-30 to e^20, counts up to 10^6, r at both ends of its range: value, g_mu and logp finite and equal to the
    restatement; the predictive log pmf is finite on the rows where a plain log(sum(exp(terms))) is -inf (at r = 1e3 the rows
    y = 3 at mean e^20, y = 10^6 at mean 1 and y = 10^4 at mean e^2, whose terms lie near -1.3e4, -7e6 and -5e3; at r = 1e-3
    the tails are power laws and nothing underflows)."""
    from tgp.pytorch_amd import lib as L
    from tgp.pytorch_amd import ops
    mu = torch.tensor([-30.0, 20.0, 0.0, 2.0], dtype=F64)
    v = torch.tensor([0.0, 0.0, 1e-3, 0.5], dtype=F64)
    Y = torch.tensor([0.0, 3.0, 1e6, 1e4], dtype=F64)
    S = 16
    xs, ws = _hermite(S)
    lam = _lam(r)
    assert NM.RMIN * (1 - 1e-12) <= r <= NM.RMAX * (1 + 1e-12)
    res = ops.ell_negbin(Y.to(DEV), mu.to(DEV), v.to(DEV), lam.to(DEV), _spec([], 0), None, S)
    m, vv = mu.clone().requires_grad_(True), v.clone().requires_grad_(True)
    ell = NM.ell_torch(Y, m, vv, lam, [], None, xs, ws)
    gm, gv = torch.autograd.grad(ell, [m, vv])
    gv[:2] = 0.0                                        # v = 0: the adjoint of v is 0
    for k in ("ell", "g_mu", "g_v", "g_lvn"):
        assert torch.isfinite(res[k]).all(), k
    print("ell %.17g restatement %.17g" % (float(res["ell"]), float(ell.detach())))
    assert rel_err(res["ell"].cpu(), ell.detach()) < TOL_VAL
    assert rel_err(res["g_mu"].cpu(), gm) < TOL_GRAD and rel_err(res["g_v"].cpu(), gv) < TOL_GRAD
    _, _, lp = ops.predict(mu.to(DEV), v.to(DEV), lam.to(DEV), _spec([], 0), None, S, Y=Y.to(DEV), lik=L.LIK_NEGBIN)
    terms = NM.pred_terms(Y, mu, v, lam, [], None, xs, ws)
    lp_ref = torch.logsumexp(terms, 0)
    print("logp", lp.cpu().tolist(), "restatement", lp_ref.tolist())
    assert torch.isfinite(lp).all() and torch.isfinite(lp_ref).all()
    # row by row.  logp = max + log(sum) of terms log wn_s + log p_s of magnitude ~1 at the heaviest nodes, so it carries a few
    # roundings of O(1) numbers whatever its own size: the row y = 0 at mean e^-30 has logp ~ -1e-13 and is held to 1e-15 absolute
    assert bool(((lp.cpu() - lp_ref).abs() <= TOL_VAL * lp_ref.abs() + 1e-15).all())
    naive = torch.log(torch.exp(terms).sum(0))
    under = torch.isinf(naive) & (naive < 0)
    print("rows where the plain sum underflows:", under.tolist())
    if r == 1e3:
        assert under.tolist() == [False, True, True, True]
    assert torch.isfinite(lp.cpu()[under]).all()


# ---- 3. the prediction kernel ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [32, 80, 1, 5])      # (1: one partly filled group of four nodes; 5: a full group and a one-node tail)
@pytest.mark.parametrize("case", CASES)
def test_predict_matches_restatement(case, S):
    from tgp.pytorch_amd import lib as L
    from tgp.pytorch_amd import ops
    N, r = 257, 3.0                                     # a ragged last workgroup
    mu, v, Y, program, theta, rowp = _inputs(case, N, r)
    xs, ws = _hermite(S)
    lam = _lam(r)
    _assert_range(lam, mu, v, program, theta, xs, ws, rowp)
    P, RP = (0 if theta is None else theta.numel()), (0 if rowp is None else rowp.shape[1])
    m1, m2, lp = ops.predict(mu.to(DEV), v.to(DEV), lam.to(DEV), _spec(program, P, RP), _dev(theta), S, _dev(rowp), Y=Y.to(DEV),
                             Y_std=7.0, lik=L.LIK_NEGBIN)           # (Y_std is ignored)
    r1, r2, rlp = NM.pred_torch(mu, v, lam, program, theta, xs, ws, rowp, Y=Y)
    errs = [float(((a.cpu() - b).abs() / b.abs().clamp(min=1e-300)).max()) for a, b in ((m1, r1), (m2, r2), (lp, rlp))]
    print("per-row relative errors m1, m2, logp:", errs)
    assert max(errs) < TOL_VAL
    if case == "empty":
        vc = v.clamp(min=0.0)
        c1, c2 = torch.exp(mu + 0.5 * vc), torch.exp(2.0 * mu + 2.0 * vc)
        assert rel_err(m1.cpu(), c1) < TOL_VAL and rel_err(m2.cpu(), c1 + (1.0 + 1.0 / r) * c2 - c1 * c1) < TOL_VAL
        # ... which the quadrature of the restatement reproduces (from 32 nodes on)
        wn = (ws / np.sqrt(np.pi)).reshape(-1, 1)
        gq = mu.reshape(1, -1) + torch.sqrt(2.0 * vc).reshape(1, -1) * xs.reshape(-1, 1)
        assert S < 32 or (rel_err((wn * torch.exp(gq)).sum(0), c1) < TOL_VAL and rel_err((wn * torch.exp(2.0 * gq)).sum(0), c2) < TOL_VAL)
    # without targets: moments only, no logp
    m1b, m2b, none = ops.predict(mu.to(DEV), v.to(DEV), lam.to(DEV), _spec(program, P, RP), _dev(theta), S, _dev(rowp),
                                 lik=L.LIK_NEGBIN)
    assert none is None and torch.equal(m1b, m1) and torch.equal(m2b, m2)


# ---- 4. the Poisson limit -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["empty", "sal2"])
def test_poisson_limit(case):
    """At r = 1e3 the new policy is tied to the existing one: log NB(y | mean, r) - log Poisson(y | mean) =
    -((y - mean)^2 - y) / (2 r) + O(r^-2).  ell lies within twice the next-order term |(y - mean)^2 - y| / (2 r), summed over
    nodes and rows by the restatement, of ops.ell_poisson on the same inputs; logp, row by row, within twice the row's largest
    node term of the Poisson ops.predict (on the restatement both hold with a factor of 0.51 in place of 2)."""
    from tgp.pytorch_amd import lib as L
    from tgp.pytorch_amd import ops
    N, S, r = 300, 32, 1e3
    mu, v, Y, program, theta, rowp = _inputs(case, N, r)
    xs, ws = _hermite(S)
    lam = _lam(r)
    _assert_range(lam, mu, v, program, theta, xs, ws, rowp)
    P = 0 if theta is None else theta.numel()
    spec = _spec(program, P)
    nb = ops.ell_negbin(Y.to(DEV), mu.to(DEV), v.to(DEV), lam.to(DEV), spec, _dev(theta), S)
    po = ops.ell_poisson(Y.to(DEV), mu.to(DEV), v.to(DEV), spec, _dev(theta), S)
    g = NM._nodes(mu, v, program, theta, xs, None)
    wn = (ws / math.sqrt(math.pi)).reshape(-1, 1)
    y = Y.reshape(1, -1)
    term = ((y - torch.exp(g)) ** 2 - y).abs() / (2.0 * r)                              # (S, N)
    bound_rows = 2.0 * (wn * term).sum(0)
    diff = abs(float(nb["ell"] - po["ell"]))
    print("ell: |NB - Poisson| = %.6e, bound %.6e" % (diff, float(bound_rows.sum())))
    assert 0.0 < diff <= float(bound_rows.sum())
    zero = torch.zeros(1, dtype=F64, device=DEV)
    _, _, lp_nb = ops.predict(mu.to(DEV), v.to(DEV), lam.to(DEV), spec, _dev(theta), S, Y=Y.to(DEV), lik=L.LIK_NEGBIN)
    _, _, lp_po = ops.predict(mu.to(DEV), v.to(DEV), zero, spec, _dev(theta), S, Y=Y.to(DEV), lik=L.LIK_POISSON)
    # a row's logp difference is the log of a weighted mean of the nodes' ratios p_NB / p_Poisson (weighted by the Poisson
    # posterior over the nodes, not by wn), so it lies between the smallest and the largest node term of the row: row by row
    dlp = (lp_nb - lp_po).abs().cpu()
    bound_lp = 2.0 * term.max(0).values
    print("logp: largest |NB - Poisson| / bound over the rows = %.4f, smallest |NB - Poisson| = %.3e"
          % (float((dlp / bound_lp).max()), float(dlp.min())))
    assert bool((dlp > 0.0).all()) and bool((dlp <= bound_lp).all())


# ---- 5. the training step against the CPU restatement -------------------------------------------------------------------
STEPS = [(300, 4, 20, 5, "sal2", 20, "scale_rbf", 3.0), (300, 5, 150, 0, "tanh3x2", 32, "scale_rbf", 0.5),
         (300, 3, 33, 2, "sal1", 20, "scale_matern32", 50.0)]


@pytest.mark.parametrize("N,D,M,seed,flow,S,kernel,r", STEPS, ids=["sal2-M20", "tanh3x2-M150", "sal1-M33-matern32"])
def test_step_matches_cpu(N, D, M, seed, flow, S, kernel, r):
    """ops.elbo_step(lik=LIK_NEGBIN) against step_torch, log_var_noise (= log r) among the gradients.  Both factorise K_ZZ as it
    stands; 1e-6 is the base of the restatement's jitter ladder, which a factorisation that succeeds never reaches (the step's
    status words are asserted 0).  M = 20 lies below the fused path's limit: the workspace the step asks for is the general-M
    path's, the one a Poisson step of the shape takes, not the fused one's."""
    from tgp.pytorch_amd import lib as L
    from tgp.pytorch_amd import ops
    prob = O.synthetic_problem(N, D, M, seed, flow, S)
    p = {k: t.clone() for k, t in prob["params"].items()}
    p["raw_outputscale"] = O.inv_softplus(0.3).reshape(1)
    p["m"] = 0.3 * p["m"]
    p["log_var_noise"] = _lam(r)
    g = torch.Generator().manual_seed(100 + seed)
    w = torch.randn(D, generator=g, dtype=F64)
    Y = gamma_poisson(torch.exp(0.5 + 0.8 * torch.sin(prob["X"] @ w)), r, g).reshape(N, 1)
    program = prob["program"]
    (elbo, ell, kld), rg, (ok, gmax, rr) = NM.step_torch(prob["X"], Y, p, float(N), program, prob["xs"], prob["ws"], kernel,
                                                         jitter=1e-6)
    print("max G = %.3f, r = %g" % (gmax, rr))
    assert ok
    theta = p.get("theta") if program is not None else None
    spec = _spec(program, 0 if theta is None else theta.numel())
    h = L.load()
    shape = (N, D, M, S, spec.nblk, spec.P, 0, L.KERNELS[kernel], 0)
    assert h.tgp_workspace_bytes_lik(*shape, L.LIK_NEGBIN) == h.tgp_workspace_bytes_lik(*shape, L.LIK_POISSON)
    if M <= 128 and kernel == "scale_rbf":
        assert h.tgp_workspace_bytes_lik(*shape, L.LIK_NEGBIN) != h.tgp_workspace_bytes_lik(*shape, L.LIK_FLOW)

    def run():
        out, grads, status, _ = ops.elbo_step(prob["X"].to(DEV), Y.to(DEV), _dev(p["Z"]), _dev(p["raw_lengthscale"]),
                                              _dev(p["raw_outputscale"]), _dev(p["m"]), _dev(p["Lam"]), _dev(p["log_var_noise"]),
                                              float(N), flow=spec, theta=_dev(theta), S=S, kernel=kernel, lik=L.LIK_NEGBIN)
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
    assert grads["lvn"].numel() == 1 and float(grads["lvn"].abs()) > 0.0
    assert float(torch.triu(grads["Lam"], 1).abs().max()) == 0.0
    out2, grads2 = run()
    assert torch.equal(out, out2) and all(torch.equal(grads[k], grads2[k]) for k in grads)


# ---- 6. the model classes -------------------------------------------------------------------------------------------------
N_MODEL, M_MODEL, R_MODEL = 200, 10, 3.0
# predicted means of a few counts and a q(f) variance below 0.15, so that the log-normal mixture over the log-mean keeps a light
# tail: on the CPU oracle's moments the restatement's pmf then has its mass (1e-10) and its first two moments (1e-6) by kmax = 52
KERNEL_SCALE, Q_MEAN_SCALE = 0.3, 1.0


def _build_model(X, tgp=False, mean="zero", whiten=True):
    from tgp.pytorch_amd import flows as G
    from tgp.pytorch_amd.kernels import instance_kernel
    from tgp.pytorch_amd.likelihoods import NegativeBinomial
    from tgp.pytorch_amd.models import sparse_MF_GP, sparse_MF_SP
    D, M = X.shape[1], M_MODEL
    K = instance_kernel("scale_rbf", ard_num_dim=D, num_multioutput=1, kernel_is_shared=False,
                        init_params={"length_scale": 2.0, "kernel_scale": KERNEL_SCALE, "noisy_variance": 1e-6})
    ip = {"variational_distribution": {"variance_scale": 1e-5, "mean_scale": 0.0}}
    lik = NegativeBinomial(dispersion_init=R_MODEL)
    if tgp:
        model = sparse_MF_SP([mean, K], X, X[:M].clone(), X.shape[0], lik, 1, whiten, False, False, False, False,
                             [G.SAL(1)], "single", 0.0, init_params=ip)
    else:
        model = sparse_MF_GP([mean, K], X, X[:M].clone(), X.shape[0], lik, 1, whiten, False, False, False, False, 0.0,
                             init_params=ip)
    model = model.to(DEV)
    gen = torch.Generator().manual_seed(11)
    mw = (Q_MEAN_SCALE * torch.randn(M, generator=gen, dtype=F64)).to(DEV)
    Lw = (0.1 * torch.eye(M, dtype=F64) + 0.02 * torch.randn(M, M, generator=gen, dtype=F64).tril()).to(DEV)
    if not whiten:             # the same q(f): u = L_Z v, with L_Z the factor of K_ZZ (+ the kernel's 1e-6 on the diagonal)
        from tgp.pytorch_amd import ops
        cf = model.covariance_function
        Kzz = ops.kmm(model.Z.detach()[0], cf.base_kernel.raw_lengthscale.detach().reshape(-1), cf.raw_outputscale.detach().reshape(-1))
        Lz = torch.linalg.cholesky(Kzz + 1e-6 * torch.eye(M, dtype=F64, device=DEV))
        mw, Lw = Lz @ mw, Lz @ Lw
    with torch.no_grad():      # a q(u) away from its initial value
        model.q_U.variational_mean.data = mw.reshape(1, M)
        model.q_U.chol_variational_covar.data = Lw.reshape(1, M, M)
    return model


@pytest.fixture(scope="module")
def counts():
    from tgp.pytorch_amd import synthetic
    X, Y = synthetic.overdispersed_dataset()
    return torch.tensor(X[:N_MODEL], dtype=F64), torch.tensor(Y[:N_MODEL], dtype=F64)


def _flow_of(model):
    from tgp.pytorch_amd.flow import compile_flow
    spec, theta_list, _ = compile_flow(model.G_matrix[0])
    theta = torch.stack([q.detach().reshape(()) for q in theta_list]) if theta_list else None
    return spec, theta


@pytest.mark.parametrize("tgp", [False, True], ids=["svgp", "tgp"])
def test_model_and_pmf(counts, tgp):
    from tgp.pytorch_amd import ops
    X, Y = counts
    model = _build_model(X, tgp=tgp)
    Xd, Yd = X.to(DEV), Y.to(DEV)
    model.set_is_training(True)
    elbo, ell, kld = model.ELBO(Xd, Yd)
    Z, rl, ro, m, Lam, lvn = (None if t is None else t.detach() for t in model._raw_params())
    assert lvn.data_ptr() == model.likelihood.log_dispersion.data_ptr()
    spec, theta = _flow_of(model)
    assert (spec.nblk > 0) == tgp
    S = model.quad_points
    mu, v = ops.qf_moments(Xd, Z, rl, ro, m, Lam, kernel="scale_rbf")
    lam = model.likelihood.log_dispersion.detach()
    comp = ops.ell_negbin(Yd, mu, v, lam, spec, theta, S, scale=1.0)
    kl = ops.kl_whitened(m, Lam)[0]
    assert rel_err(ell.detach().cpu(), comp["ell"].cpu()) < TOL_VAL and rel_err(kld.detach().cpu(), kl.cpu()) < TOL_VAL
    assert rel_err(elbo.detach().cpu(), (comp["ell"] - kl).cpu()) < TOL_VAL
    # ... and the restatement at the same moments
    xs, ws = _hermite(S)
    prog = [tuple(int(q) for q in b) for b in spec.blocks]
    th = None if theta is None else theta.cpu()
    _assert_range(lam.cpu(), mu.cpu(), v.cpu(), prog, th, xs, ws)
    assert rel_err(ell.detach().cpu(), NM.ell_torch(Y.reshape(-1), mu.cpu(), v.cpu(), lam.cpu(), prog, th, xs, ws)) < TOL_VAL
    (-elbo).backward()
    assert all(q.grad is not None and torch.isfinite(q.grad).all() for q in model.parameters())
    gl = model.likelihood.log_dispersion.grad
    assert gl.shape == (1,) and rel_err(-gl.cpu(), comp["g_lvn"].cpu()) < TOL_GRAD and float(gl.abs()) > 0

    model.set_is_training(False)
    n = 50
    lp_sum, (m1, m2) = model.test_log_likelihood(Xd[:n], Yd[:n], return_moments=True, Y_std=7.0 * torch.ones(1, device=DEV))
    _, _, lp = ops.predict(mu[:n], v[:n], lam, spec, theta, S, Y=Yd[:n].reshape(-1), lik=ops.L.LIK_NEGBIN)
    assert m1.shape == (1, n) and m2.shape == (1, n) and rel_err(lp_sum.cpu(), lp.sum().cpu()) < TOL_VAL     # (no log Y_std)
    pm1, pm2, _, _ = model.predictive_distribution(Xd[:n])
    assert pm1.shape == (1, n) and torch.equal(pm1, m1) and torch.equal(pm2, m2)
    # kmax from the restatement: the first count at which its pmf sums to within 1e-10 of 1 on every row
    KTOP = 400
    k = torch.arange(KTOP + 1, dtype=F64)
    mu_c, v_c = mu[:n].cpu(), v[:n].cpu()
    terms = NM.pred_terms(k.repeat_interleave(n), mu_c.repeat(KTOP + 1), v_c.repeat(KTOP + 1), lam.cpu(), prog, th, xs, ws)
    pmf_ref = torch.exp(torch.logsumexp(terms, 0)).reshape(KTOP + 1, n).t()              # (n, KTOP + 1)
    done = ((pmf_ref.cumsum(1) - 1.0).abs() <= 1e-10).all(0)
    assert bool(done.any()), "the restatement's pmf does not sum to 1 within 1e-10 by k = %d" % KTOP
    kmax = int(torch.nonzero(done)[0])
    print("kmax = %d" % kmax)
    assert kmax <= KTOP
    pmf = model.predictive_pmf(Xd[:n], kmax)
    assert pmf.shape == (n, kmax + 1) and not pmf.requires_grad and bool((pmf >= 0).all())
    assert float((pmf.sum(1) - 1.0).abs().max()) < 1e-9
    kd = torch.arange(kmax + 1, dtype=F64, device=DEV)
    assert rel_err((pmf * kd).sum(1).cpu(), m1.reshape(-1).cpu()) < 1e-6
    assert rel_err(((pmf * kd * kd).sum(1) - (pmf * kd).sum(1) ** 2).cpu(), m2.reshape(-1).cpu()) < 1e-6
    at_y = pmf[torch.arange(n, device=DEV), Yd[:n].reshape(-1).long()]
    assert rel_err(at_y.cpu(), torch.exp(lp).cpu()) < TOL_VAL
    err_pmf = float(((pmf.cpu() - pmf_ref[:, :kmax + 1]).abs() / pmf_ref[:, :kmax + 1]).max())
    # the CRPS of the pmf: sum_k (cdf_k - 1{k >= y})^2, against the same sum from the restatement's pmf, row by row
    crps = model.predictive_crps(Xd[:n], Yd[:n], kmax=kmax)
    assert crps.shape == (1, n)
    dev_ref = pmf_ref[:, :kmax + 1].cumsum(1) - (k[:kmax + 1].unsqueeze(0) >= Y[:n].reshape(-1, 1)).to(F64)
    crps_ref = (dev_ref ** 2).sum(1)
    err_crps = float(((crps[0].cpu() - crps_ref).abs() / crps_ref).max())
    print("pmf: largest relative error of an entry %.3e; CRPS: largest relative error of a row %.3e" % (err_pmf, err_crps))
    assert err_pmf < TOL_VAL                            # (every entry, down to ~1e-12 of its row)
    assert rel_err(crps[0].cpu(), crps_ref) < TOL_VAL and err_crps < TOL_VAL
    with pytest.raises(ValueError, match="negative-binomial model needs kmax"):
        model.predictive_crps(Xd[:n], Yd[:n])
    q = model.posterior_quantiles(Xd[:n], [0.1, 0.9])
    assert q.shape == (1, 2, n) and bool((q[0, 0] < q[0, 1]).all())
    paths = model.posterior_paths(3, num_frequencies=64, generator=torch.Generator().manual_seed(0))
    draws = paths(Xd[:n])                               # G(f) of three coherent draws: the log-mean
    assert draws.numel() == 3 * n and torch.isfinite(draws).all()
    s, _, _ = model.sample_from_predictive_distribution(Xd[:n], S=4)
    assert s.shape == (1, 4, n, 1) and bool((s >= 0).all()) and bool((s == torch.round(s)).all())


@pytest.mark.parametrize("variant", ["linear-mean", "unwhitened"])
def test_model_variants_match_the_restatement(counts, variant):
    """A linear mean (the per-row affine head block, as for Poisson) and is_whiten=False: the ELBO is the restatement's ELL at
    the model's q(f) moments minus the model's KL, and the dispersion gets its gradient."""
    X, Y = counts
    Xd, Yd = X.to(DEV), Y.to(DEV)
    model = _build_model(X, mean="linear" if variant == "linear-mean" else "zero", whiten=variant != "unwhitened")
    if variant == "linear-mean":
        with torch.no_grad():
            model.mean_function.a.data.copy_(torch.tensor([0.2, -0.1], dtype=F64).reshape(model.mean_function.a.shape))
            model.mean_function.b.data.fill_(0.3)
    model.set_is_training(True)
    elbo, ell, kld = model.ELBO(Xd, Yd)
    (-elbo).backward()
    gl = model.likelihood.log_dispersion.grad
    assert gl is not None and torch.isfinite(gl).all() and float(gl.abs()) > 0
    if variant == "linear-mean":
        ga = model.mean_function.a.grad
        assert ga is not None and torch.isfinite(ga).all() and float(ga.abs().max()) > 0
    with torch.no_grad():
        mu, v = model.marginal_variational_qf_parameters(Xd, diagonal=True, is_duvenaud=False)
        kl = model.KLD().sum()
    S = model.quad_points
    xs, ws = _hermite(S)
    lam = model.likelihood.log_dispersion.detach().cpu()
    mu, v = mu.reshape(-1).cpu(), v.reshape(-1).cpu()
    _assert_range(lam, mu, v, [], None, xs, ws)
    ref = NM.ell_torch(Y.reshape(-1), mu, v, lam, [], None, xs, ws)
    assert rel_err(ell.detach().cpu(), ref) < TOL_VAL
    assert rel_err(kld.detach().cpu(), kl.cpu()) < TOL_VAL and rel_err(elbo.detach().cpu(), ref - kl.cpu()) < TOL_VAL
    gref = NM.dlam_rows(Y.reshape(-1), mu, v, lam, [], None, xs, ws).sum()
    assert rel_err(-gl.cpu(), gref) < TOL_GRAD


# ---- 7. determinism -------------------------------------------------------------------------------------------------------
def test_same_input_same_bits():
    from tgp.pytorch_amd import lib as L
    from tgp.pytorch_amd import ops
    N, S, r = 4000, 32, 3.0
    mu, v, Y, program, theta, rowp = _inputs("sal2", N, r)
    lam = _lam(r).to(DEV)
    spec = _spec(program, theta.numel())
    a = ops.ell_negbin(Y.to(DEV), mu.to(DEV), v.to(DEV), lam, spec, _dev(theta), S, scale=2.0)
    b = ops.ell_negbin(Y.to(DEV), mu.to(DEV), v.to(DEV), lam, spec, _dev(theta), S, scale=2.0)
    for k in ("ell", "g_lvn", "g_mu", "g_v", "g_theta"):
        assert torch.equal(a[k], b[k]), k
    pa = ops.predict(mu.to(DEV), v.to(DEV), lam, spec, _dev(theta), S, Y=Y.to(DEV), lik=L.LIK_NEGBIN)
    pb = ops.predict(mu.to(DEV), v.to(DEV), lam, spec, _dev(theta), S, Y=Y.to(DEV), lik=L.LIK_NEGBIN)
    assert all(torch.equal(x, y) for x, y in zip(pa, pb))


# ---- 8. the CLI -----------------------------------------------------------------------------------------------------------
CLI = ["--model", "TGP", "--likelihood", "negbinomial", "--dataset", "synthetic_overdispersed", "--train_test_seed_split", "1",
       "--num_inducing", "10", "--epochs", "20"]
NUM = r"(-?(?:\d+\.\d+|nan|inf))"


def test_cli(monkeypatch, capsys):
    """The command line in a child process: exit 0, finite NLL, RMSE and r.  The same arguments in this process, with the
    trainer's model kept: the NLL it prints is -mean logp of one predict launch on the test rows, and the child's line is the
    same line (the run is seeded)."""
    r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, "-m", "tgp.pytorch_amd.main"] + CLI, cwd=REPO,
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert r.stdout.count("Test Negative LOGL") == 2 and "constant rate" in r.stdout
    line = re.search(r"model TGP, Test Negative LOGL %s, Test RMSE %s" % (NUM, NUM), r.stdout)
    disp = re.search(r"learned dispersion r %s \(true r 2\.000\)" % NUM, r.stdout)
    assert line and disp, r.stdout[-2000:]
    nll, rmse, rr = float(line.group(1)), float(line.group(2)), float(disp.group(1))
    assert math.isfinite(nll) and math.isfinite(rmse) and math.isfinite(rr) and rr > 0

    from tgp.pytorch_amd import main, trainers
    kept = {}

    class Keeping(trainers.Trainer_SP_regression):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            kept["model"], kept["loaders"] = kw["model"], kw["data_loaders"]

    monkeypatch.setattr(main, "Trainer_SP_regression", Keeping)
    res = main.main(CLI)
    out = capsys.readouterr().out
    assert line.group(0) in out and disp.group(0) in out
    model = kept["model"]
    from tgp.pytorch_amd import data
    _, dc = data.return_dataset("synthetic_overdispersed", 10000, seed=1)
    Xte, Yte = dc["X_te"].to(DEV), dc["Y_te"].to(DEV)
    model.set_is_training(False)
    lp, (m1, _) = model.test_log_likelihood(Xte, Yte, return_moments=True, Y_std=torch.ones(1, device=DEV))
    mean_nll = -float(lp) / Yte.numel()
    assert abs(-res[6] - mean_nll) <= 1e-9 * abs(mean_nll) and abs(nll - mean_nll) <= 5.1e-4        # (three printed decimals)
    assert abs(res[7] - float(((m1.reshape(-1) - Yte.reshape(-1)) ** 2).mean().sqrt())) <= 1e-9 * res[7]
    assert abs(float(model.likelihood.dispersion) - rr) <= 5.1e-4
