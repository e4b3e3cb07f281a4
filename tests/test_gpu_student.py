"""GPU (-m gpu): the Student-t likelihood (TGP_LIK_STUDENT: Student-t noise of nu degrees of freedom and scale sigma around
the flow) through every layer -- the stand-alone ELL kernel and its gradients against torch autograd (tests/student_model.py
restates the formula), the extremes, the prediction kernel, the training step (general-M path at every M) against the CPU
restatement, the model classes and the CLI."""
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import REPO, load_golden, rel_err

import student_model as SM
from oracle import tgp_oracle as O
from poisson_model import flow_any

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


_INPUT_CACHE = {}


def _inputs(case, N):
    """The inputs of the likelihood comparisons, seeded by N and made once per (case, N): mu = 0.5 randn, v = 0.3 rand (the
    first seven rows at -1e-12), Y = G(mu) + 0.3 randn with every tenth row moved by a gross error of +-(5 to 15)."""
    if (case, N) not in _INPUT_CACHE:
        g = torch.Generator().manual_seed(N)
        mu = 0.5 * torch.randn(N, generator=g, dtype=F64)
        v = 0.3 * torch.rand(N, generator=g, dtype=F64)
        v[:7] = -1e-12
        program, theta, rowp = _case(case, N, g)
        Y = flow_any(mu.reshape(1, -1), program, theta, rowp).reshape(-1) + 0.3 * torch.randn(N, generator=g, dtype=F64)
        Y[::10] += torch.sign(torch.randn(Y[::10].shape, generator=g, dtype=F64)) * (5.0 + 10.0 * torch.rand(Y[::10].shape, generator=g, dtype=F64))
        _INPUT_CACHE[(case, N)] = (mu, v, Y, program, theta, rowp)
    return _INPUT_CACHE[(case, N)]


# ---- 1. the stand-alone ELL kernel against autograd --------------------------------------------------------------------
CASES = ["empty", "sal2", "tanh3x2", "flows_med_arcsl2", "idsal"]


# 32, 16 and 4 lanes per row; then four nodes in flight per lane at 32 and at 16 lanes per row
@pytest.mark.parametrize("nu", [2.5, 30.0])
@pytest.mark.parametrize("N,S", [(300, 32), (4000, 32), (13000, 32), (300, 80), (4000, 40)],
                         ids=["300", "4000", "13000", "300-S80", "4000-S40"])
@pytest.mark.parametrize("case", CASES)
def test_ell_kernel_matches_autograd(case, N, S, nu):
    from tgp.pytorch_amd import ops
    mu, v, Y, program, theta, rowp = _inputs(case, N)
    xs, ws = _hermite(S)
    P, RP = (0 if theta is None else theta.numel()), (0 if rowp is None else rowp.shape[1])
    scale = 3.5
    lvn = torch.tensor([np.log(0.07)], dtype=F64)
    res = ops.ell_student(Y.to(DEV), mu.to(DEV), v.to(DEV), lvn.to(DEV), nu, _spec(program, P, RP), _dev(theta), S, _dev(rowp),
                          scale=scale)
    wrt = [mu.clone().requires_grad_(True), v.clone().requires_grad_(True), lvn.clone().requires_grad_(True)]
    th = theta.clone().requires_grad_(True) if theta is not None else None
    rp = rowp.clone().requires_grad_(True) if rowp is not None else None
    ell = SM.ell_torch(Y, wrt[0], wrt[1], wrt[2], nu, program, th, xs, ws, rp, scale)
    extra = [t for t in (th, rp) if t is not None]
    grads = torch.autograd.grad(ell, wrt + extra)
    gv = grads[1].clone()
    gv[:7] = 0.0                                        # v <= 0: the adjoint of v is 0
    errs = {"ell": rel_err(res["ell"].cpu(), ell.detach()), "g_mu": rel_err(res["g_mu"].cpu(), grads[0]),
            "g_v": rel_err(res["g_v"].cpu(), gv), "out[1]": rel_err(res["g_lvn"].cpu().reshape(1), grads[2])}
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
def test_extremes():
    """Residuals of 10^8 sigma stay finite and equal to the restatement (value, every gradient, the predictive density); rows
    with v = 0 have g_v = 0; the second double behind log_var_noise is really read as nu."""
    from tgp.pytorch_amd import lib as L
    from tgp.pytorch_amd import ops
    sig2, nu, S = 0.04, 4.0, 16
    sig = float(np.sqrt(sig2))
    mu = torch.tensor([0.0, 0.0, 0.3, -0.2, 1.0], dtype=F64)
    v = torch.tensor([0.0, 1e-3, 0.5, 0.0, 0.2], dtype=F64)
    Y = torch.tensor([1e8 * sig, -1e8 * sig, 1e8 * sig, -0.25, 1.1], dtype=F64)
    lvn = torch.tensor([np.log(sig2)], dtype=F64)
    xs, ws = _hermite(S)
    res = ops.ell_student(Y.to(DEV), mu.to(DEV), v.to(DEV), lvn.to(DEV), nu, _spec([], 0), None, S)
    m, vv, lv = (t.clone().requires_grad_(True) for t in (mu, v, lvn))
    ell = SM.ell_torch(Y, m, vv, lv, nu, [], None, xs, ws)
    gm, gv, gl = torch.autograd.grad(ell, [m, vv, lv])
    zero_v = v == 0
    gv[zero_v] = 0.0                                    # v = 0: the adjoint of v is 0
    for k in ("ell", "g_mu", "g_v", "g_lvn"):
        assert torch.isfinite(res[k]).all(), k
    assert rel_err(res["ell"].cpu(), ell.detach()) < TOL_VAL
    assert rel_err(res["g_mu"].cpu(), gm) < TOL_GRAD and rel_err(res["g_v"].cpu(), gv) < TOL_GRAD
    assert float(((res["g_mu"].cpu() - gm).abs() / gm.abs()).max()) < TOL_GRAD        # ... row by row: 1e-8 beside O(1)
    assert rel_err(res["g_lvn"].cpu().reshape(1), gl) < TOL_GRAD
    assert torch.all(res["g_v"].cpu()[zero_v] == 0)
    _, _, lp = ops.predict(mu.to(DEV), v.to(DEV), lvn.to(DEV), _spec([], 0), None, S, Y=Y.to(DEV), Y_std=3.0, lik=L.LIK_STUDENT,
                           df=nu)
    _, _, lp_ref = SM.pred_torch(mu, v, lvn, nu, [], None, xs, ws, Y=Y, Y_std=3.0)
    print("logp", lp.cpu().tolist(), "restatement", lp_ref.tolist())
    assert torch.isfinite(lp).all() and float(((lp.cpu() - lp_ref).abs() / lp_ref.abs()).max()) < TOL_VAL
    # nu is read from log_var_noise[1]: the raw two-element call equals ell_student at that nu, and another nu another value
    two = {}
    for d in (4.0, 9.0):
        noise = torch.tensor([float(lvn), d], dtype=F64, device=DEV)
        two[d] = ops._ell_quad(Y.to(DEV), mu.to(DEV), v.to(DEV), noise, _spec([], 0), None, S, None, 1.0, L.LIK_STUDENT)
    assert torch.equal(two[4.0]["ell"], res["ell"]) and torch.equal(two[4.0]["g_mu"], res["g_mu"])
    ell9 = SM.ell_torch(Y, mu, v, lvn, 9.0, [], None, xs, ws)
    assert rel_err(two[9.0]["ell"].cpu(), ell9) < TOL_VAL and abs(float(two[9.0]["ell"]) - float(two[4.0]["ell"])) > 1.0


# ---- 3. the prediction kernel ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nu", [2.5, 30.0])
@pytest.mark.parametrize("S", [20, 50, 1, 5])      # (1: one partly filled group of four nodes; 5: a full group and a one-node tail)
@pytest.mark.parametrize("case", ["empty", "sal2", "flows_med_arcsl2", "idsal"])
def test_predict_matches_restatement(case, S, nu):
    from tgp.pytorch_amd import lib as L
    from tgp.pytorch_amd import ops
    N = 1000
    mu, v, Y, program, theta, rowp = _inputs(case, N)
    xs, ws = _hermite(S)
    P, RP = (0 if theta is None else theta.numel()), (0 if rowp is None else rowp.shape[1])
    lvn = torch.tensor([np.log(0.07)], dtype=F64)
    m1, m2, lp = ops.predict(mu.to(DEV), v.to(DEV), lvn.to(DEV), _spec(program, P, RP), _dev(theta), S, _dev(rowp), Y=Y.to(DEV),
                             Y_std=7.0, lik=L.LIK_STUDENT, df=nu)
    r1, r2, rlp = SM.pred_torch(mu, v, lvn, nu, program, theta, xs, ws, rowp, Y=Y, Y_std=7.0)
    # m1 is a mean of either sign, so its error is rel_err's (against the largest entry); m2 and logp row by row
    errs = [rel_err(m1.cpu(), r1), float(((m2.cpu() - r2).abs() / r2).max()), float(((lp.cpu() - rlp).abs() / rlp.abs()).max())]
    print("errors m1, m2 (per row), logp (per row):", errs)
    assert max(errs) < TOL_VAL
    if case == "empty":
        vc = v.clamp(min=0.0)
        assert float((m1.cpu() - mu).abs().max()) < TOL_VAL
        # (one node carries no spread: S = 1 gives sigma^2 nu / (nu - 2) alone; from S = 2 on the rule is exact for f^2)
        assert rel_err(m2.cpu(), (vc if S > 1 else 0.0 * vc) + 0.07 * nu / (nu - 2.0)) < TOL_VAL
    # without targets: moments only
    m1b, m2b, none = ops.predict(mu.to(DEV), v.to(DEV), lvn.to(DEV), _spec(program, P, RP), _dev(theta), S, _dev(rowp),
                                 lik=L.LIK_STUDENT, df=nu)
    assert none is None and torch.equal(m1b, m1) and torch.equal(m2b, m2)


def test_predict_has_no_variance_at_two_degrees():
    """nu <= 2 is outside the supported range; the kernel cannot refuse (nu lives on the device) and writes m2 = +inf."""
    from tgp.pytorch_amd import lib as L
    from tgp.pytorch_amd import ops
    mu, v = torch.zeros(5, dtype=F64, device=DEV), torch.ones(5, dtype=F64, device=DEV)
    noise = torch.tensor([0.0, 2.0], dtype=F64, device=DEV)
    md, keep = ops._flow_model(5, 8, _spec([], 0), None, noise, DEV, lik=L.LIK_STUDENT)
    m1, m2 = torch.empty_like(mu), torch.empty_like(mu)
    L.check(L.load().tgp_predict_f64(md, L.ptr(mu), L.ptr(v), None, None, 1.0, L.ptr(m1), L.ptr(m2), None, L.stream_ptr()),
            "tgp_predict_f64")
    assert bool(torch.isinf(m2).all()) and bool((m2 > 0).all()) and float(m1.abs().max()) < 1e-15


# ---- 4. the training step against the CPU restatement -------------------------------------------------------------------
STEPS = [(300, 4, 20, 5, "sal2", 20, "scale_rbf"), (700, 5, 150, 0, "tanh3x2", 32, "scale_rbf"),
         (257, 13, 128, 2, "none", 16, "scale_rbf"), (300, 3, 33, 2, "sal1", 20, "scale_matern32")]


@pytest.mark.parametrize("N,D,M,seed,flow,S,kernel", STEPS, ids=["sal2-M20", "tanh3x2-M150", "svgp-M128", "sal1-M33-matern32"])
def test_step_matches_cpu(N, D, M, seed, flow, S, kernel):
    """ops.elbo_step(lik=LIK_STUDENT) against step_torch.  Both factorise K_ZZ as it stands; 1e-6 is the base of the
    restatement's jitter ladder, which a factorisation that succeeds never reaches (the step's status words are asserted 0)."""
    from tgp.pytorch_amd import lib as L
    from tgp.pytorch_amd import ops
    nu = 4.0
    prob = O.synthetic_problem(N, D, M, seed, flow, S)
    p = {k: t.clone() for k, t in prob["params"].items()}
    Y = prob["Y"].clone()
    Y[::10] += 8.0                                       # gross errors in a tenth of the (standardised) targets
    program = prob["program"]
    if program is None:
        p.pop("theta", None)
    (elbo, ell, kld), rg = SM.step_torch(prob["X"], Y, p, nu, float(N), program, prob["xs"], prob["ws"], kernel, jitter=1e-6)
    theta = p.get("theta")
    spec = _spec(program, 0 if theta is None else theta.numel())

    def run():
        out, grads, status, _ = ops.elbo_step(prob["X"].to(DEV), Y.to(DEV), _dev(p["Z"]), _dev(p["raw_lengthscale"]),
                                              _dev(p["raw_outputscale"]), _dev(p["m"]), _dev(p["Lam"]), _dev(p["log_var_noise"]),
                                              float(N), flow=spec, theta=_dev(theta), S=S, kernel=kernel, lik=L.LIK_STUDENT, df=nu)
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


# ---- 5. the model classes -------------------------------------------------------------------------------------------------
def _build_model(X, M=20, tgp=False, mean="zero", whiten=True, df=4.0):
    from tgp.pytorch_amd import flows as G
    from tgp.pytorch_amd.kernels import instance_kernel
    from tgp.pytorch_amd.likelihoods import StudentT
    from tgp.pytorch_amd.models import sparse_MF_GP, sparse_MF_SP
    D = X.shape[1]
    K = instance_kernel("scale_rbf", ard_num_dim=D, num_multioutput=1, kernel_is_shared=False,
                        init_params={"length_scale": 2.0, "kernel_scale": 2.0, "noisy_variance": 1e-6})
    ip = {"variational_distribution": {"variance_scale": 1e-5, "mean_scale": 0.0}}
    lik = StudentT(1, 0.05, False, 20, df=df)
    if tgp:
        model = sparse_MF_SP([mean, K], X, X[:M].clone(), X.shape[0], lik, 1, whiten, False, False, False, False,
                             [G.SAL(1)], "single", 0.0, init_params=ip)
    else:
        model = sparse_MF_GP([mean, K], X, X[:M].clone(), X.shape[0], lik, 1, whiten, False, False, False, False, 0.0,
                             init_params=ip)
    return model.to(DEV)


@pytest.fixture(scope="module")
def outliers():
    """300 rows of synthetic_outliers' inputs with a tenth of the targets replaced by gross errors, standardised."""
    from tgp.pytorch_amd import synthetic
    X, Y = synthetic.outliers_dataset()
    Y, _ = synthetic.gross_errors(Y[:300], seed=1)
    Y = (Y - Y.mean()) / Y.std()
    return torch.tensor(X[:300], dtype=F64), torch.tensor(Y, dtype=F64)


def _move_qu(model, M=20):
    gen = torch.Generator().manual_seed(11)
    with torch.no_grad():
        model.q_U.variational_mean.data = (0.3 * torch.randn(1, M, generator=gen, dtype=F64)).to(DEV)
        model.q_U.chol_variational_covar.data = (0.1 * torch.eye(M, dtype=F64) +
                                                 0.02 * torch.randn(M, M, generator=gen, dtype=F64).tril()).reshape(1, M, M).to(DEV)


@pytest.mark.parametrize("tgp", [False, True], ids=["svgp", "tgp"])
def test_model(outliers, tgp):
    from tgp.pytorch_amd import ops
    from tgp.pytorch_amd.flow import compile_flow
    X, Y = outliers
    model = _build_model(X, tgp=tgp, df=5.0)
    _move_qu(model)
    Xd, Yd = X.to(DEV), Y.to(DEV)
    model.set_is_training(True)
    elbo, ell, kld = model.ELBO(Xd, Yd)
    Z, rl, ro, m, Lam, lvn = (t.detach() for t in model._raw_params())
    spec, theta_list, _ = compile_flow(model.G_matrix[0])
    theta = torch.stack([q.detach().reshape(()) for q in theta_list]) if theta_list else None
    assert (spec.nblk > 0) == tgp
    mu, v = ops.qf_moments(Xd, Z, rl, ro, m, Lam, kernel="scale_rbf")
    comp = ops.ell_student(Yd, mu, v, lvn, 5.0, spec, theta, model.quad_points, scale=1.0)
    kl = ops.kl_whitened(m, Lam)[0]
    assert rel_err(ell.detach().cpu(), comp["ell"].cpu()) < TOL_VAL and rel_err(kld.detach().cpu(), kl.cpu()) < TOL_VAL
    assert rel_err(elbo.detach().cpu(), (comp["ell"] - kl).cpu()) < TOL_VAL
    (-elbo).backward()
    assert all(q.grad is not None and torch.isfinite(q.grad).all() for q in model.parameters())
    assert rel_err(-model.likelihood.log_var_noise.grad.reshape(1).cpu(), comp["g_lvn"].reshape(1).cpu()) < TOL_GRAD
    assert float(model.likelihood.df) == 5.0 and not model.likelihood.df.requires_grad
    # the likelihood's own method: the same value, differentiable in the noise
    e2 = model.likelihood.expected_log_prob(Yd.t(), mu.reshape(1, -1), v.reshape(1, -1), flow=model.G_matrix, X=Xd.unsqueeze(0))
    assert rel_err(e2.detach().cpu(), comp["ell"].reshape(1).cpu()) < TOL_VAL and e2.requires_grad

    model.set_is_training(False)
    n, ystd = 50, 2.5
    lp_sum, (m1, m2) = model.test_log_likelihood(Xd[:n], Yd[:n], return_moments=True, Y_std=torch.full((1,), ystd, device=DEV))
    r1, r2, lp = ops.predict(mu[:n], v[:n], lvn, spec, theta, model.quad_points, Y=Yd[:n].reshape(-1), Y_std=ystd,
                             lik=ops.L.LIK_STUDENT, df=5.0)
    assert m1.shape == (1, n) and m2.shape == (1, n) and rel_err(lp_sum.cpu(), lp.sum().cpu()) < TOL_VAL
    assert torch.equal(m1.reshape(-1), r1) and torch.equal(m2.reshape(-1), r2)
    pm1, pm2, _, _ = model.predictive_distribution(Xd[:n])
    assert pm1.shape == (1, n) and torch.equal(pm1, m1) and torch.equal(pm2, m2)
    s, _, _ = model.sample_from_predictive_distribution(Xd[:n], S=4)
    assert s.shape == (1, 4, n, 1) and torch.isfinite(s).all()
    q = model.posterior_quantiles(Xd[:n], [0.1, 0.9])          # G(f)'s quantiles go through the unchanged code
    assert q.shape == (1, 2, n) and bool((q[0, 0] < q[0, 1]).all())
    with pytest.raises(NotImplementedError, match="Student-t"):
        model.predictive_quantiles(Xd[:n], [0.5])
    paths = model.posterior_paths(3)
    assert paths(Xd[:n]).shape[-1] == n


def test_linear_mean_takes_the_affine_head_block(outliers):
    """A linear mean goes the route of the other flow likelihoods: a per-row affine block (1, m(x_n)) at the head of the
    program in training, m(X) inside mu in prediction.  The ELBO equals the stand-alone likelihood at mu + m(X)."""
    from tgp.pytorch_amd import ops
    X, Y = outliers
    X, Y = X.to(DEV), Y.to(DEV)
    model = _build_model(X.cpu(), mean="linear")
    with torch.no_grad():
        model.mean_function.a.data.copy_(torch.tensor([0.2, -0.1], dtype=F64).reshape(model.mean_function.a.shape))
        model.mean_function.b.data.fill_(0.3)
    model.set_is_training(True)
    elbo, ell, kld = model.ELBO(X, Y)
    (-elbo).backward()
    ga = model.mean_function.a.grad
    assert ga is not None and torch.isfinite(ga).all() and float(ga.abs().max()) > 0
    lvn = model.likelihood.log_var_noise.detach().reshape(-1)[:1]
    with torch.no_grad():
        mu, v = model.marginal_variational_qf_parameters(X, diagonal=True, is_duvenaud=False)
        comp = ops.ell_student(Y, mu.reshape(-1).contiguous(), v.reshape(-1).contiguous(), lvn, 4.0, _spec([], 0), None,
                               model.quad_points)
    assert rel_err(ell.detach().cpu(), comp["ell"].cpu()) < TOL_VAL
    # dELL/da = X^T dELL/dmu: the adjoint of mu from the same launch
    assert rel_err(-ga.reshape(-1).cpu(), (X.t() @ comp["g_mu"]).cpu()) < TOL_GRAD
    model.set_is_training(False)
    m1, _, mq, _ = model.predictive_distribution(X[:20])
    assert m1.shape == (1, 20) and rel_err(mq.reshape(-1).cpu(), mu.reshape(-1)[:20].cpu()) < TOL_VAL


def test_unwhitened_matches_restatement(outliers):
    """is_whiten=False goes through the unchanged transform: the step's likelihood term equals the CPU restatement at the
    model's own q(f) moments, and the ELBO is that minus the model's KL."""
    X, Y = outliers
    model = _build_model(X, tgp=True, whiten=False)
    _move_qu(model)
    Xd, Yd = X.to(DEV), Y.to(DEV)
    model.set_is_training(True)
    elbo, ell, kld = model.ELBO(Xd, Yd)
    (-elbo).backward()
    assert all(q.grad is not None and torch.isfinite(q.grad).all() for q in model.parameters())
    from tgp.pytorch_amd.flow import compile_flow
    spec, theta_list, _ = compile_flow(model.G_matrix[0])
    theta = torch.stack([q.detach().reshape(()) for q in theta_list]).cpu()
    with torch.no_grad():
        mu, v = model.marginal_variational_qf_parameters(Xd, diagonal=True, is_duvenaud=False)
        kl = model.KLD().sum()
    xs, ws = _hermite(model.quad_points)
    lvn = model.likelihood.log_var_noise.detach().reshape(-1)[:1].cpu()
    ref = SM.ell_torch(Y.reshape(-1), mu.reshape(-1).cpu(), v.reshape(-1).cpu(), lvn, 4.0, list(spec.blocks), theta, xs, ws)
    assert rel_err(ell.detach().cpu(), ref) < TOL_VAL
    assert rel_err(elbo.detach().cpu(), (ell.detach() - kl).cpu()) < TOL_VAL


# ---- 6. the CLI -----------------------------------------------------------------------------------------------------------
def test_cli():
    cmd = [sys.executable, "-m", "tgp.pytorch_amd.main", "--model", "TGP", "--likelihood", "studentt", "--df", "4", "--dataset",
           "synthetic_outliers", "--train_test_seed_split", "1", "--num_inducing", "20", "--epochs", "30"]
    r = subprocess.run(["timeout", "-k", "10", "300"] + cmd, cwd=REPO, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert r.stdout.count("Test Negative LOGL") == 1 and "Test RMSE" in r.stdout
