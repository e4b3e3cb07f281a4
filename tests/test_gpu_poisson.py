"""GPU (-m gpu): the Poisson likelihood (TGP_LIK_POISSON: counts, the flow as the log-rate) through every layer -- the
stand-alone ELL kernel and its gradients against torch autograd (tests/poisson_model.py restates the formula), the extremes
(the log-sum-exp of the predictive pmf), the prediction kernel, the training step (general-M path at every M) against the
CPU restatement, the refusals, the model classes with predictive_pmf, a short training run on synthetic_counts and the CLI.

Every comparison first asserts the range condition of tests/poisson_model.py on the CPU restatement: max G(f0) <= 10 over the
nodes with wn > 1e-14."""
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import REPO, load_golden, rel_err

import poisson_model as PM
from oracle import tgp_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL_VAL, TOL_GRAD = 1e-9, 1e-7
F64 = torch.float64
SAL, PER_ROW = 1, 4


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


_CASE_CACHE = {}


def _case(case, N, g):
    """(program, theta, rowp) of a named flow case; the per-row parameters of `idsal` come from the generator `g`."""
    if case == "idsal":
        rowp = torch.stack([0.1 * torch.randn(N, generator=g, dtype=F64), 0.8 + 0.05 * torch.randn(N, generator=g, dtype=F64)], 1)
        return [(SAL, 0, 0, PER_ROW)], None, rowp
    if case not in _CASE_CACHE:
        if case == "empty":
            _CASE_CACHE[case] = ([], None)
        elif case in ("sal2", "tanh3x2"):
            prob = O.synthetic_problem(64, 4, 8, seed=5 if case == "sal2" else 0, flow=case)
            _CASE_CACHE[case] = ([tuple(int(v) for v in b) for b in prob["program"]], prob["params"]["theta"].clone())
        else:
            z = load_golden(case)
            _CASE_CACHE[case] = (z["program"], z["p_theta"].clone())
    program, theta = _CASE_CACHE[case]
    return program, theta, None


def _inputs(case, N, with_v0=True):
    """The inputs of the likelihood comparisons: seeded by N; mu = 0.5 randn, v = 0.3 rand (the first seven rows at -1e-12),
    Y ~ Poisson(exp(min(G(mu), 6)))."""
    g = torch.Generator().manual_seed(N)
    mu = 0.5 * torch.randn(N, generator=g, dtype=F64)
    v = 0.3 * torch.rand(N, generator=g, dtype=F64)
    if with_v0:
        v[:7] = -1e-12
    program, theta, rowp = _case(case, N, g)
    rate = torch.exp(PM.flow_any(mu.reshape(1, -1), program, theta, rowp).reshape(-1).clamp(max=6.0))
    Y = torch.poisson(rate, generator=g)
    return mu, v, Y, program, theta, rowp


# ---- 1. the stand-alone ELL kernel against autograd --------------------------------------------------------------------
CASES = ["empty", "sal2", "tanh3x2", "flows_med_arcsl2", "bern_med_sal_invbcl1", "flows_med_invbcl_al1", "idsal"]


# 32, 16 and 4 lanes per row; then four nodes in flight per lane at 32 and at 16 lanes per row
@pytest.mark.parametrize("N,S", [(300, 32), (4000, 32), (13000, 32), (300, 80), (4000, 40)],
                         ids=["300", "4000", "13000", "300-S80", "4000-S40"])
@pytest.mark.parametrize("case", CASES)
def test_ell_kernel_matches_autograd(case, N, S):
    from tgp.pytorch_amd import ops
    mu, v, Y, program, theta, rowp = _inputs(case, N)
    xs, ws = _hermite(S)
    gmax = PM.max_log_rate(mu, v, program, theta, xs, ws, rowp)
    print("max G = %.3f" % gmax)
    assert gmax <= PM.GMAX
    P, RP = (0 if theta is None else theta.numel()), (0 if rowp is None else rowp.shape[1])
    scale = 3.5
    res = ops.ell_poisson(Y.to(DEV), mu.to(DEV), v.to(DEV), _spec(program, P, RP), _dev(theta), S, _dev(rowp), scale=scale)
    wrt = [mu.clone().requires_grad_(True), v.clone().requires_grad_(True)]
    th = theta.clone().requires_grad_(True) if theta is not None else None
    rp = rowp.clone().requires_grad_(True) if rowp is not None else None
    ell = PM.ell_torch(Y, wrt[0], wrt[1], program, th, xs, ws, rp, scale)
    extra = [t for t in (th, rp) if t is not None]
    grads = torch.autograd.grad(ell, wrt + extra)
    gv = grads[1].clone()
    gv[:7] = 0.0                                        # v <= 0: the adjoint of v is 0
    errs = {"ell": rel_err(res["ell"].cpu(), ell.detach()), "g_mu": rel_err(res["g_mu"].cpu(), grads[0]),
            "g_v": rel_err(res["g_v"].cpu(), gv)}
    if th is not None:
        errs["g_theta"] = rel_err(res["g_theta"].cpu(), grads[2])
    if rp is not None:
        errs["g_rowp"] = rel_err(res["g_rowp"].cpu(), grads[-1])
    print(errs)
    assert "g_lvn" not in res
    assert errs.pop("ell") < TOL_VAL
    assert torch.all(res["g_v"][:7].cpu() == 0)
    for k, e in errs.items():
        assert e < TOL_GRAD, (k, e)


# ---- 2. extremes ----------------------------------------------------------------------------------------------------------
def test_extremes():
    """Rates from e^-30 to e^20 and counts up to 10^6: everything finite and equal to the restatement; the predictive log pmf
    is finite where a plain log(sum(exp(terms))) is -inf (every term underflows; asserted on the last two rows)."""
    from tgp.pytorch_amd import lib as L
    from tgp.pytorch_amd import ops
    mu = torch.tensor([-30.0, 20.0, 0.0, 2.0], dtype=F64)
    v = torch.tensor([0.0, 0.0, 1e-3, 0.5], dtype=F64)
    Y = torch.tensor([0.0, 3.0, 1e6, 1e4], dtype=F64)
    S = 16
    xs, ws = _hermite(S)
    res = ops.ell_poisson(Y.to(DEV), mu.to(DEV), v.to(DEV), _spec([], 0), None, S)
    m, vv = mu.clone().requires_grad_(True), v.clone().requires_grad_(True)
    ell = PM.ell_torch(Y, m, vv, [], None, xs, ws)
    gm, gv = torch.autograd.grad(ell, [m, vv])
    gv[:2] = 0.0                                        # v = 0: the adjoint of v is 0
    for k in ("ell", "g_mu", "g_v"):
        assert torch.isfinite(res[k]).all(), k
    assert rel_err(res["ell"].cpu(), ell.detach()) < TOL_VAL
    assert rel_err(res["g_mu"].cpu(), gm) < TOL_GRAD and rel_err(res["g_v"].cpu(), gv) < TOL_GRAD
    lvn = torch.zeros(1, dtype=F64, device=DEV)
    _, _, lp = ops.predict(mu.to(DEV), v.to(DEV), lvn, _spec([], 0), None, S, Y=Y.to(DEV), lik=L.LIK_POISSON)
    terms = PM.pred_terms(Y, mu, v, [], None, xs, ws)
    lp_ref = torch.logsumexp(terms, 0)
    print("logp", lp.cpu().tolist(), "restatement", lp_ref.tolist())
    assert torch.isfinite(lp).all() and torch.isfinite(lp_ref).all()
    assert rel_err(lp.cpu(), lp_ref) < TOL_VAL
    assert float((lp[1:].cpu() - lp_ref[1:]).abs().div(lp_ref[1:].abs()).max()) < TOL_VAL     # ... the large rows one by one
    naive = torch.log(torch.exp(terms).sum(0))
    assert torch.isinf(naive[2]) and torch.isinf(naive[3]) and naive[2] < 0 and naive[3] < 0


# ---- 3. the prediction kernel ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [20, 50, 1, 5])      # (1: one partly filled group of four nodes; 5: a full group and a one-node tail)
@pytest.mark.parametrize("case", ["empty", "sal2", "flows_med_arcsl2", "idsal"])
def test_predict_matches_restatement(case, S):
    _predict_matches_restatement(case, S, 1000)
    if S == 5:      # the first row past a workgroup of 256, and a single row
        _predict_matches_restatement(case, S, 257)
        _predict_matches_restatement(case, S, 1)


def _predict_matches_restatement(case, S, N):
    from tgp.pytorch_amd import lib as L
    from tgp.pytorch_amd import ops
    mu, v, Y, program, theta, rowp = _inputs(case, N)
    xs, ws = _hermite(S)
    assert PM.max_log_rate(mu, v, program, theta, xs, ws, rowp) <= PM.GMAX
    P, RP = (0 if theta is None else theta.numel()), (0 if rowp is None else rowp.shape[1])
    lvn = torch.zeros(1, dtype=F64, device=DEV)
    m1, m2, lp = ops.predict(mu.to(DEV), v.to(DEV), lvn, _spec(program, P, RP), _dev(theta), S, _dev(rowp), Y=Y.to(DEV),
                             Y_std=7.0, lik=L.LIK_POISSON)          # (Y_std is ignored)
    r1, r2, rlp = PM.pred_torch(mu, v, program, theta, xs, ws, rowp, Y=Y)
    errs = [float(((a.cpu() - b).abs() / b.abs().clamp(min=1e-300)).max()) for a, b in ((m1, r1), (m2, r2), (lp, rlp))]
    print("per-row relative errors m1, m2, logp:", errs)
    assert max(errs) < TOL_VAL
    if case == "empty":
        vc = v.clamp(min=0.0)
        c1 = torch.exp(mu + 0.5 * vc)
        assert rel_err(m1.cpu(), c1) < TOL_VAL and rel_err(m2.cpu(), c1 + torch.expm1(vc) * c1 * c1) < TOL_VAL
        # ... which the quadrature of the restatement reproduces (from 20 nodes on)
        wn = (ws / np.sqrt(np.pi)).reshape(-1, 1)
        gq = mu.reshape(1, -1) + torch.sqrt(2.0 * vc).reshape(1, -1) * xs.reshape(-1, 1)
        assert S < 20 or rel_err((wn * torch.exp(gq)).sum(0), c1) < TOL_VAL
    # without targets: moments only
    m1b, m2b, none = ops.predict(mu.to(DEV), v.to(DEV), lvn, _spec(program, P, RP), _dev(theta), S, _dev(rowp), lik=L.LIK_POISSON)
    assert none is None and torch.equal(m1b, m1) and torch.equal(m2b, m2)


# ---- 4. the training step against the CPU restatement -------------------------------------------------------------------
STEPS = [(300, 4, 20, 5, "sal2", 20, "scale_rbf"), (700, 5, 150, 0, "tanh3x2", 32, "scale_rbf"),
         (257, 13, 128, 2, "none", 16, "scale_rbf"), (300, 3, 33, 2, "sal1", 20, "scale_matern32")]


@pytest.mark.parametrize("N,D,M,seed,flow,S,kernel", STEPS, ids=["sal2-M20", "tanh3x2-M150", "svgp-M128", "sal1-M33-matern32"])
def test_step_matches_cpu(N, D, M, seed, flow, S, kernel):
    """ops.elbo_step(lik=LIK_POISSON) against step_torch.  Both factorise K_ZZ as it stands; 1e-6 is the base of the
    restatement's jitter ladder, which a factorisation that succeeds never reaches (the step's status words are asserted 0)."""
    from tgp.pytorch_amd import lib as L
    from tgp.pytorch_amd import ops
    prob = O.synthetic_problem(N, D, M, seed, flow, S)
    p = {k: t.clone() for k, t in prob["params"].items()}
    p["raw_outputscale"] = O.inv_softplus(0.3).reshape(1)
    p["m"] = 0.3 * p["m"]
    g = torch.Generator().manual_seed(100 + seed)
    w = torch.randn(D, generator=g, dtype=F64)
    Y = torch.poisson(torch.exp(0.5 + 0.8 * torch.sin(prob["X"] @ w)), generator=g).reshape(N, 1)
    program = prob["program"]
    (elbo, ell, kld), rg, gmax = PM.step_torch(prob["X"], Y, p, float(N), program, prob["xs"], prob["ws"], kernel, jitter=1e-6)
    print("max G = %.3f" % gmax)
    assert gmax <= PM.GMAX
    theta = p.get("theta") if program is not None else None
    spec = _spec(program, 0 if theta is None else theta.numel())
    lvn = torch.zeros(1, dtype=F64, device=DEV)

    def run():
        out, grads, status, _ = ops.elbo_step(prob["X"].to(DEV), Y.to(DEV), _dev(p["Z"]), _dev(p["raw_lengthscale"]),
                                              _dev(p["raw_outputscale"]), _dev(p["m"]), _dev(p["Lam"]), lvn, float(N), flow=spec,
                                              theta=_dev(theta), S=S, kernel=kernel, lik=L.LIK_POISSON)
        torch.cuda.synchronize()
        assert int(status[0]) == 0 and int(status[1]) == 0
        return out.cpu(), {k: t.cpu() for k, t in grads.items()}

    out, grads = run()
    errs = {"elbo": rel_err(out[0], elbo), "ell": rel_err(out[1], ell), "kld": rel_err(out[2], kld)}
    pairs = [("Z", "Z"), ("raw_ls", "raw_lengthscale"), ("raw_os", "raw_outputscale"), ("m", "m"), ("Lam", "Lam")]
    if theta is not None:
        pairs.append(("theta", "theta"))
    for k_hip, k_ref in pairs:
        errs["g_" + k_hip] = rel_err(grads[k_hip], rg[k_ref])
    print(errs)
    for k in ("elbo", "ell", "kld"):
        assert errs.pop(k) < TOL_VAL, k
    for k, e in errs.items():
        assert e < TOL_GRAD, (k, e)
    assert float(grads["lvn"].abs().max()) == 0.0
    assert float(torch.triu(grads["Lam"], 1).abs().max()) == 0.0
    out2, grads2 = run()
    assert torch.equal(out, out2) and all(torch.equal(grads[k], grads2[k]) for k in grads)


# ---- 5. refusals ----------------------------------------------------------------------------------------------------------
def _build_model(X, Y, M=20, tgp=False, mean="zero"):
    from tgp.pytorch_amd import flows as G
    from tgp.pytorch_amd.kernels import instance_kernel
    from tgp.pytorch_amd.likelihoods import Poisson
    from tgp.pytorch_amd.models import sparse_MF_GP, sparse_MF_SP
    D = X.shape[1]
    K = instance_kernel("scale_rbf", ard_num_dim=D, num_multioutput=1, kernel_is_shared=False,
                        init_params={"length_scale": 2.0, "kernel_scale": 2.0, "noisy_variance": 1e-6})
    ip = {"variational_distribution": {"variance_scale": 1e-5, "mean_scale": 0.0}}
    if tgp:
        model = sparse_MF_SP([mean, K], X, X[:M].clone(), X.shape[0], Poisson(), 1, True, False, False, False, False,
                             [G.SAL(1)], "single", 0.0, init_params=ip)
    else:
        model = sparse_MF_GP([mean, K], X, X[:M].clone(), X.shape[0], Poisson(), 1, True, False, False, False, False, 0.0,
                             init_params=ip)
    return model.to(DEV)


@pytest.fixture(scope="module")
def counts():
    from tgp.pytorch_amd import synthetic
    X, Y = synthetic.counts_dataset()
    return torch.tensor(X, dtype=F64), torch.tensor(Y, dtype=F64)


def test_refusals(counts):
    from tgp.pytorch_amd import lib as L
    from tgp.pytorch_amd import ops
    h = L.load()
    mu = torch.zeros(9, dtype=F64, device=DEV)
    v = torch.ones(9, dtype=F64, device=DEV)
    lvn = torch.zeros(1, dtype=F64, device=DEV)
    md, keep = ops._flow_model(9, 8, _spec([], 0), None, lvn, DEV, lik=L.LIK_POISSON)
    assert md.lik == 6
    p, zq = ops.quantile_probs([0.5], DEV)
    t = torch.empty(1, 9, dtype=F64, device=DEV)
    st = torch.zeros(1, dtype=torch.int32, device=DEV)
    rc = h.tgp_predict_quantile_f64(md, L.ptr(mu), L.ptr(v), None, L.ptr(p), L.ptr(zq), 1, L.ptr(t), L.ptr(st), L.stream_ptr())
    assert rc == L.E_UNSUPPORTED and b"TGP_LIK_POISSON" in h.tgp_last_error()
    rc = h.tgp_predict_cdf_f64(md, L.ptr(mu), L.ptr(v), None, L.ptr(mu), L.ptr(t), None, L.stream_ptr())
    assert rc == L.E_UNSUPPORTED and b"TGP_LIK_POISSON" in h.tgp_last_error()
    X, Y = counts
    model = _build_model(X[:100], Y[:100])
    assert [n for n, _ in model.named_parameters() if "noise" in n] == []
    with pytest.raises(NotImplementedError, match="Poisson"):
        model.set_optimal_qu(X[:100].to(DEV), Y[:100].to(DEV))
    model.set_is_training(False)
    with pytest.raises(NotImplementedError, match="Poisson"):
        model.predictive_quantiles(X[:100].to(DEV), [0.5])
    with pytest.raises(ValueError, match="counts"):
        model.ELBO(X[:100].to(DEV), Y[:100].to(DEV) + 0.5)
    # the log-rate's quantiles go through the unchanged code
    q = model.posterior_quantiles(X[:100].to(DEV), [0.1, 0.9])
    assert q.shape == (1, 2, 100) and bool((q[0, 0] < q[0, 1]).all())


# ---- 6. the model classes and the predictive pmf --------------------------------------------------------------------------
@pytest.mark.parametrize("tgp", [False, True], ids=["svgp", "tgp"])
def test_model_and_pmf(counts, tgp):
    from tgp.pytorch_amd import ops
    from tgp.pytorch_amd.flow import compile_flow
    X, Y = counts
    X, Y = X[:300], Y[:300]
    model = _build_model(X, Y, tgp=tgp)
    gen = torch.Generator().manual_seed(11)
    # a q(u) away from its initial value whose predictive keeps its mass below kmax = 60: the CPU restatement puts the rows' sums
    # over k <= 60 within 5e-16 of 1 at this state (at m ~ 0.5 N(0, 1), L_q = 0.3 I + ... the mass past 60 is 1.5e-9, there too)
    with torch.no_grad():
        model.q_U.variational_mean.data = (0.3 * torch.randn(1, 20, generator=gen, dtype=F64)).to(DEV)
        model.q_U.chol_variational_covar.data = (0.1 * torch.eye(20, dtype=F64) +
                                                 0.02 * torch.randn(20, 20, generator=gen, dtype=F64).tril()).reshape(1, 20, 20).to(DEV)
    Xd, Yd = X.to(DEV), Y.to(DEV)
    model.set_is_training(True)
    elbo, ell, kld = model.ELBO(Xd, Yd)
    Z, rl, ro, m, Lam, _ = (None if t is None else t.detach() for t in model._raw_params())
    spec, theta_list, _ = compile_flow(model.G_matrix[0])
    theta = torch.stack([q.detach().reshape(()) for q in theta_list]) if theta_list else None
    assert (spec.nblk > 0) == tgp
    mu, v = ops.qf_moments(Xd, Z, rl, ro, m, Lam, kernel="scale_rbf")
    comp = ops.ell_poisson(Yd, mu, v, spec, theta, model.quad_points, scale=1.0)
    kl = ops.kl_whitened(m, Lam)[0]
    assert rel_err(ell.detach().cpu(), comp["ell"].cpu()) < TOL_VAL and rel_err(kld.detach().cpu(), kl.cpu()) < TOL_VAL
    assert rel_err(elbo.detach().cpu(), (comp["ell"] - kl).cpu()) < TOL_VAL
    (-elbo).backward()
    assert all(q.grad is not None and torch.isfinite(q.grad).all() for q in model.parameters())

    model.set_is_training(False)
    n, kmax = 50, 60
    lp_sum, (m1, m2) = model.test_log_likelihood(Xd[:n], Yd[:n], return_moments=True, Y_std=torch.ones(1, device=DEV))
    _, _, lp = ops.predict(mu[:n], v[:n], torch.zeros(1, dtype=F64, device=DEV), spec, theta, model.quad_points, Y=Yd[:n].reshape(-1),
                           lik=ops.L.LIK_POISSON)
    assert m1.shape == (1, n) and m2.shape == (1, n) and rel_err(lp_sum.cpu(), lp.sum().cpu()) < TOL_VAL
    pm1, pm2, _, _ = model.predictive_distribution(Xd[:n])
    assert pm1.shape == (1, n) and torch.equal(pm1, m1) and torch.equal(pm2, m2)
    pmf = model.predictive_pmf(Xd[:n], kmax)
    assert pmf.shape == (n, kmax + 1) and not pmf.requires_grad and bool((pmf >= 0).all())
    assert float((pmf.sum(1) - 1.0).abs().max()) < 1e-9
    k = torch.arange(kmax + 1, dtype=F64, device=DEV)
    assert rel_err((pmf * k).sum(1).cpu(), m1.reshape(-1).cpu()) < 1e-6
    assert rel_err(((pmf * k * k).sum(1) - (pmf * k).sum(1) ** 2).cpu(), m2.reshape(-1).cpu()) < 1e-6
    at_y = pmf[torch.arange(n, device=DEV), Yd[:n].reshape(-1).long()]
    assert rel_err(at_y.cpu(), torch.exp(lp).cpu()) < TOL_VAL
    # the README's 95 % count interval from the cumulative sum
    cdf = pmf.cumsum(1)
    lo, hi = (cdf < 0.025).sum(1), (cdf < 0.975).sum(1)
    assert bool((lo <= hi).all()) and bool((hi <= kmax).all())
    s, _, _ = model.sample_from_predictive_distribution(Xd[:n], S=4)
    assert s.shape == (1, 4, n, 1) and bool((s >= 0).all()) and bool((s == torch.round(s)).all())


def test_linear_mean_takes_the_affine_head_block(counts):
    """A linear mean goes the route of the other flow likelihoods: a per-row affine block (1, m(x_n)) at the head of the
    program in training, m(X) inside mu in prediction.  The ELBO equals the stand-alone likelihood at mu + m(X)."""
    from tgp.pytorch_amd import ops
    X, Y = counts
    X, Y = X[:300].to(DEV), Y[:300].to(DEV)
    model = _build_model(X.cpu(), Y.cpu(), mean="linear")
    with torch.no_grad():
        model.mean_function.a.data.copy_(torch.tensor([0.2, -0.1], dtype=F64).reshape(model.mean_function.a.shape))
        model.mean_function.b.data.fill_(0.3)
    model.set_is_training(True)
    elbo, ell, kld = model.ELBO(X, Y)
    (-elbo).backward()
    ga = model.mean_function.a.grad
    assert ga is not None and torch.isfinite(ga).all() and float(ga.abs().max()) > 0
    with torch.no_grad():
        mu, v = model.marginal_variational_qf_parameters(X, diagonal=True, is_duvenaud=False)
        comp = ops.ell_poisson(Y, mu.reshape(-1).contiguous(), v.reshape(-1).contiguous(), _spec([], 0), None, model.quad_points)
    assert rel_err(ell.detach().cpu(), comp["ell"].cpu()) < TOL_VAL
    # dELL/da = X^T dELL/dmu: the adjoint of mu from the same launch
    assert rel_err(-ga.reshape(-1).cpu(), (X.t() @ comp["g_mu"]).cpu()) < TOL_GRAD
    model.set_is_training(False)
    m1, _, mq, _ = model.predictive_distribution(X[:20])
    assert m1.shape == (1, 20) and rel_err(mq.reshape(-1).cpu(), mu.reshape(-1)[:20].cpu()) < TOL_VAL


# ---- 7. a short training run ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tgp", [False, True], ids=["svgp", "tgp"])
def test_short_training_run_beats_constant_rate(counts, tgp):
    from tgp.pytorch_amd.data import DeviceLoader
    from tgp.pytorch_amd.trainers import Trainer_SP_regression
    X, Y = counts
    Xtr, Ytr, Xte, Yte = X[:600], Y[:600], X[600:], Y[600:]
    model = _build_model(Xtr, Ytr, tgp=tgp)
    loaders = [DeviceLoader(Xtr, Ytr, 10000, shuffle=False, device=DEV), DeviceLoader(Xte, Yte, 10000, device=DEV)]
    tr = Trainer_SP_regression(model, loaders, 1e20, False, False, torch.ones(1, device=DEV), -1, 100, True)
    tr.train(epochs=150, lr_ALL=0.05, opt="adam", keep_parameter_groups=True)
    assert tr._engine is None                           # Poisson trains on the eager path
    assert len(tr.loss_arr) == 150 and -tr.loss_arr[-1] > -tr.loss_arr[0]
    model.set_is_training(False)
    lp, (m1, _) = model.test_log_likelihood(Xte.to(DEV), Yte.to(DEV), return_moments=True, Y_std=torch.ones(1, device=DEV))
    rate, y = Ytr.mean(), Yte.reshape(-1)
    base_lp = float((y * torch.log(rate) - rate - torch.lgamma(y + 1.0)).mean())
    base_rmse = float(((y - rate) ** 2).mean().sqrt())
    mean_lp = float(lp) / y.numel()
    rmse = float(((m1.reshape(-1).cpu() - y) ** 2).mean().sqrt())
    print("ELBO %.2f -> %.2f; test mean logp %.3f (constant rate %.3f); RMSE %.3f (constant rate %.3f)"
          % (-tr.loss_arr[0], -tr.loss_arr[-1], mean_lp, base_lp, rmse, base_rmse))
    assert mean_lp >= base_lp + 1.0
    assert rmse <= 0.7 * base_rmse
    res = tr.compute_metrics()                          # the trainer reports the same two numbers, in raw counts
    assert abs(res[6] - mean_lp) < 1e-9 * abs(mean_lp) and abs(res[7] - rmse) < 1e-9 * rmse


# ---- 8. the CLI -----------------------------------------------------------------------------------------------------------
def test_cli():
    cmd = [sys.executable, "-m", "tgp.pytorch_amd.main", "--model", "TGP", "--likelihood", "poisson", "--dataset",
           "synthetic_counts", "--train_test_seed_split", "1", "--num_inducing", "20", "--epochs", "30"]
    r = subprocess.run(["timeout", "-k", "10", "300"] + cmd, cwd=REPO, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert r.stdout.count("Test Negative LOGL") == 2 and "constant rate" in r.stdout
