"""GPU: input gradients of q(f) (tgp_qf_input_grad_f64, csrc/tgp_xgrad.hip) and of the predictive moments
(tgp_predict_moment_grads_f64, k_pred_mgrad of csrc/tgp_quantile.hip), through ops, the autograd Function, the models and the CLI.

The yardstick is the float64 restatement of tests/input_grad_model.py (held to torch autograd through the oracle on the CPU,
tests/test_input_grad_host.py) or oracle autograd itself.  Tolerances: the project's TOL_GRAD = 1e-7 for gradients and
TOL_VAL = 1e-9 for values, through conftest.rel_err, as in tests/test_gpu_parity.py."""
import math
import re
import subprocess
import sys

import pytest
import torch

from conftest import REPO, rel_err
from oracle import tgp_oracle as orc

import flow_shapes_model as fsm
import input_grad_model as IG

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F64 = torch.float64
TOL_VAL = 1e-9
TOL_GRAD = 1e-7
KEYS = ("Z", "raw_lengthscale", "raw_outputscale", "m", "Lam")
RQ_ALPHA = 2.0


@pytest.fixture(scope="module", autouse=True)
def f64():
    from tgp.pytorch_amd import config as cg
    old = torch.get_default_dtype()
    cg.set_maximum_precission()
    cg.device = DEV
    yield
    torch.set_default_dtype(old)


def _dev(p, kernel="scale_rbf"):
    from tgp.pytorch_amd import ops
    t = [p[k].to(DEV) for k in KEYS]
    if kernel == "scale_rq":
        t[2] = ops.rq_scale(t[2], RQ_ALPHA)
    return tuple(t)


# ---- tile edges against the restatement ---------------------------------------------------------------------------
EDGE_N = (1, 63, 65, 130)
EDGE_MD = ((5, 1), (100, 4), (150, 13), (130, 16))     # M < 16, D = 1; the fused-size M; M > 128, odd D; M = 2 steps + 2, D = 16
SAME_ROW = (40, 3)                                      # row 40 of X is row 3 of Z bit for bit
_edge_ref = {}


def _edge(M, D, kernel):
    """One problem of 130 rows per (M, D, kernel), restated once on the CPU: each row's Jacobians depend on that row only, so
    the first N rows of the reference serve every N."""
    key = (M, D, kernel)
    if key not in _edge_ref:
        prob = orc.synthetic_problem(300, D, M, seed=7, flow=None, S=8)      # (Z: M of its 300 rows)
        p, X = prob["params"], prob["X"][:130].clone()
        if D == 1:
            # five N(0, 1) points on a line under length-scale 2: K_ZZ has a condition number near 1e10, and two correct float64
            # routes through its factor differ by about 1e-7 in dv (measured 9e-8, while Matern-3/2 on the same rows gives 1e-13).
            # Length-scale 0.7 keeps the reference itself good to well below TOL_GRAD; the kernel's path is the same.
            p["raw_lengthscale"] = orc.inv_softplus(torch.full((1,), 0.7, dtype=F64))
        X[SAME_ROW[0]] = p["Z"][SAME_ROW[1]]
        alpha = RQ_ALPHA if kernel == "scale_rq" else None
        dmu, dv = IG.qf_input_grad(X, *(p[k] for k in KEYS), kernel=kernel, alpha=alpha)
        _edge_ref[key] = (X, p, dmu, dv)
    return _edge_ref[key]


def _check_edge(N, M, D, kernel):
    from tgp.pytorch_amd import ops
    X, p, dmu_ref, dv_ref = _edge(M, D, kernel)
    Xd = X[:N].contiguous().to(DEV)
    dmu, dv = ops.qf_input_grad(Xd, *_dev(p, kernel), kernel=kernel)
    assert dmu.shape == (N, D) and dv.shape == (N, D) and dmu.is_contiguous() and dv.is_contiguous()
    assert bool(torch.isfinite(dmu).all()) and bool(torch.isfinite(dv).all())
    e = (rel_err(dmu.cpu(), dmu_ref[:N]), rel_err(dv.cpu(), dv_ref[:N]))
    print("N=%d M=%d D=%d %s: dmu %.3e dv %.3e (tol %.1e)" % (N, M, D, kernel, e[0], e[1], TOL_GRAD))
    assert max(e) <= TOL_GRAD
    if N > SAME_ROW[0]:        # the row that coincides with an inducing point, on its own scale
        r = SAME_ROW[0]
        assert rel_err(dmu[r].cpu(), dmu_ref[r]) <= TOL_GRAD and rel_err(dv[r].cpu(), dv_ref[r]) <= TOL_GRAD
    dmu2, dv2 = ops.qf_input_grad(Xd, *_dev(p, kernel), kernel=kernel)
    assert torch.equal(dmu, dmu2) and torch.equal(dv, dv2)


@pytest.mark.parametrize("kernel", ("scale_rbf", "scale_matern32"))
@pytest.mark.parametrize("M,D", EDGE_MD)
@pytest.mark.parametrize("N", EDGE_N)
def test_tile_edges(N, M, D, kernel):
    _check_edge(N, M, D, kernel)


@pytest.mark.parametrize("kernel", ("scale_matern52", "scale_rq"))
def test_other_kernels(kernel):
    _check_edge(65, 100, 4, kernel)


def test_pass_boundary():
    """N = TGP_XGRAD_PASS_ROWS + 1: two passes, the second of one row; every row within tolerance, those beside the boundary too."""
    from tgp.pytorch_amd import lib as L
    from tgp.pytorch_amd import ops
    R = L.XGRAD_PASS_ROWS
    prob = orc.synthetic_problem(R + 1, 2, 5, seed=11, flow=None, S=8)
    p, X = prob["params"], prob["X"]
    dmu_ref, dv_ref = IG.qf_input_grad(X, *(p[k] for k in KEYS))
    dmu, dv = ops.qf_input_grad(X.to(DEV), *_dev(p))
    dmu, dv = dmu.cpu(), dv.cpu()
    assert bool(torch.isfinite(dmu).all()) and bool(torch.isfinite(dv).all())
    e = (rel_err(dmu, dmu_ref), rel_err(dv, dv_ref))
    print("pass boundary: dmu %.3e dv %.3e" % e)
    assert max(e) <= TOL_GRAD
    for r in (R - 1, R):
        assert rel_err(dmu[r], dmu_ref[r]) <= TOL_GRAD and rel_err(dv[r], dv_ref[r]) <= TOL_GRAD, r
    # a row's result does not depend on the pass it falls in: the last row alone
    d1, v1 = ops.qf_input_grad(X[R:].contiguous().to(DEV), *_dev(p))
    assert torch.equal(d1.cpu()[0], dmu[R]) and torch.equal(v1.cpu()[0], dv[R])


def test_refusals_on_the_device():
    from tgp.pytorch_amd import lib as L
    from tgp.pytorch_amd import ops
    prob = orc.synthetic_problem(10, 4, 5, seed=1, flow=None, S=8)
    X = prob["X"].to(DEV)
    need = L.load().tgp_qf_input_grad_workspace_bytes(10, 4, 5)
    with pytest.raises(L.TgpError, match=r"-101 .*tgp_qf_input_grad_f64"):
        ops.qf_input_grad(X, *_dev(prob["params"]), workspace_bytes=need - 8)
    with pytest.raises(L.TgpError, match=r"-100 .*tgp_predict_moment_grads_f64.*lik = %d" % L.LIK_POISSON):
        ops.predict_moment_grads(torch.zeros(4, device=DEV), torch.ones(4, device=DEV), torch.zeros(1, device=DEV),
                                 ops.FlowSpec([], 0, 0, DEV), None, 8, lik=L.LIK_POISSON)


# ---- models --------------------------------------------------------------------------------------------------------
def _build(prob, flow, whiten=True, mean="zero", outputs=1):
    from tgp.pytorch_amd.flow import compile_flow, instance_flow
    from tgp.pytorch_amd.flows import SAL, StepTanhL
    from tgp.pytorch_amd.kernels import instance_kernel
    from tgp.pytorch_amd.likelihoods import GaussianLinearMean, GaussianNonLinearMean
    from tgp.pytorch_amd.models import sparse_MF_GP, sparse_MF_SP
    p = prob["params"]
    N, D = prob["X"].shape
    M = p["m"].numel()
    K = instance_kernel("scale_rbf", ard_num_dim=D, num_multioutput=1, kernel_is_shared=False,
                        init_params={"length_scale": 2.0, "kernel_scale": 2.0, "noisy_variance": 1e-6})
    ip = {"variational_distribution": {"variance_scale": 1e-5, "mean_scale": 0.0}}
    if flow is None:
        model = sparse_MF_GP([mean, K], prob["X"], p["Z"].clone(), N, GaussianLinearMean(1, 0.05, False), 1, whiten, False, False,
                             False, False, 0.0, init_params=ip)
    else:
        lik = GaussianNonLinearMean(1, 0.05, False, quadrature_points=prob["xs"].numel())
        if flow.startswith("sal"):
            specs = SAL(int(flow[3:]))
        else:
            nb, ns = (int(t) for t in flow[4:].split("x"))
            specs = instance_flow(StepTanhL(nb, ns, add_f0=True))
        model = sparse_MF_SP([mean, K], prob["X"], p["Z"].clone(), N, lik, 1, whiten, False, False, False, False, [specs], "single",
                             0.0, init_params=ip)
    with torch.no_grad():
        model.Z.data = p["Z"].reshape(1, M, D).clone()
        model.q_U.variational_mean.data = p["m"].reshape(1, M).clone()
        model.q_U.chol_variational_covar.data = p["Lam"].reshape(1, M, M).clone()
        model.covariance_function.raw_outputscale.data = p["raw_outputscale"].reshape(1).clone()
        model.covariance_function.base_kernel.raw_lengthscale.data = p["raw_lengthscale"].reshape(1, 1, D).clone()
        model.likelihood.log_var_noise.data = p["log_var_noise"].reshape(1, 1).clone()
        if flow is not None:
            for prm, val in zip(compile_flow(model.G_matrix[0])[1], p["theta"]):
                prm.data = val.clone().reshape(())
        if mean == "linear":
            model.mean_function.a.data = p["mean_a"].reshape(1, D, 1).clone()
            model.mean_function.b.data = p["mean_b"].reshape(1, 1, 1).clone()
    return model.to(DEV)


def _problem(flow, whiten, mean, N=65, M=20, D=4, S=32):
    """The problem, and the whitened q(u) the oracle takes: the parameters themselves, or L^-1 (m - m(Z)), L^-1 tril(L_q)."""
    prob = orc.synthetic_problem(N, D, M, seed=5, flow=flow, S=S)
    p = prob["params"]
    g = torch.Generator().manual_seed(17)
    if mean == "linear":
        p["mean_a"] = 0.5 * torch.randn(D, generator=g, dtype=F64)
        p["mean_b"] = torch.tensor([0.3], dtype=F64)
    if not whiten:        # (m, Lam) describe q(u) itself: keep L_q's diagonal away from 0
        p["Lam"] = torch.tril(p["Lam"]) + 0.5 * torch.eye(M, dtype=F64)
    m_w, Lam_w = p["m"], p["Lam"]
    if not whiten:
        Lz = torch.linalg.cholesky(orc.scale_rbf(p["Z"], p["Z"], p["raw_lengthscale"], p["raw_outputscale"]))
        m0 = p["m"] - (p["Z"] @ p["mean_a"] + p["mean_b"] if mean == "linear" else 0.0)
        m_w = torch.linalg.solve_triangular(Lz, m0.reshape(-1, 1), upper=False).reshape(-1)
        Lam_w = torch.linalg.solve_triangular(Lz, torch.tril(p["Lam"]), upper=False)
    return prob, (p["Z"], p["raw_lengthscale"], p["raw_outputscale"], m_w, Lam_w)


def _oracle_qf(Xg, prob, white, mean):
    mu, v = orc.qf_moments(Xg, *white)
    if mean == "linear":
        mu = mu + Xg @ prob["params"]["mean_a"] + prob["params"]["mean_b"]
    return mu, v


@pytest.mark.parametrize("mean", ("zero", "linear"))
@pytest.mark.parametrize("whiten", (True, False), ids=("whitened", "unwhitened"))
@pytest.mark.parametrize("flow", (None, "sal2"), ids=("svgp", "tgp-sal2"))
def test_autograd_in_X(flow, whiten, mean):
    from tgp.pytorch_amd import ops
    prob, white = _problem(flow, whiten, mean)
    model = _build(prob, flow, whiten, mean)
    model.set_is_training(True)
    g = torch.Generator().manual_seed(23)
    N = prob["X"].shape[0]
    c1, c2 = torch.randn(N, generator=g, dtype=F64), torch.randn(N, generator=g, dtype=F64)
    Xg = prob["X"].clone().requires_grad_(True)
    mu_o, v_o = _oracle_qf(Xg, prob, white, mean)
    gX_ref, = torch.autograd.grad((c1 * mu_o + c2 * v_o).sum(), Xg)
    Xd = prob["X"].to(DEV).requires_grad_(True)
    mu, v = model.marginal_variational_qf_parameters(Xd, diagonal=True, is_duvenaud=False)
    assert mu.shape == (1, N, 1) and v.shape == (1, N, 1)
    (c1.to(DEV) * mu.reshape(-1) + c2.to(DEV) * v.reshape(-1)).sum().backward()
    e = (rel_err(mu.detach().cpu(), mu_o.detach()), rel_err(v.detach().cpu(), v_o.detach()), rel_err(Xd.grad.cpu(), gX_ref))
    print("autograd %s whiten=%s mean=%s: mu %.2e v %.2e X.grad %.2e" % ((flow, whiten, mean) + e))
    assert e[0] <= TOL_VAL and e[1] <= TOL_VAL and e[2] <= TOL_GRAD
    assert all(q.grad is not None for q in (model.Z, model.q_U.variational_mean))        # the parameters' gradients still flow
    # X not requiring grad: the bits of ops.qf_moments (plus the mean's launch), and nothing to differentiate in X
    if whiten and mean == "zero":
        with torch.no_grad():
            mu0, v0 = model.marginal_variational_qf_parameters(prob["X"].to(DEV), diagonal=True, is_duvenaud=False)
        mu1, v1 = ops.qf_moments(prob["X"].to(DEV), *(t.to(DEV) for t in white))
        assert torch.equal(mu0.reshape(-1), mu1) and torch.equal(v0.reshape(-1), v1)
        assert torch.equal(mu.detach().reshape(-1), mu1) and torch.equal(v.detach().reshape(-1), v1)
        with pytest.raises(NotImplementedError):
            model.marginal_variational_qf_parameters(Xd, diagonal=False, is_duvenaud=False)


# ---- the partials of the predictive moments ----------------------------------------------------------------------------
def _partials_case(name, S, N=65):
    g = torch.Generator().manual_seed(31)
    mu = torch.randn(N, generator=g, dtype=F64)
    v = 0.05 + torch.rand(N, generator=g, dtype=F64)
    v[9] = 0.0
    xs, ws = orc.hermgauss(S)
    if name == "sinh_r":                         # SinhL's block: an extended kind
        program, theta = fsm.PROGRAMS[name], torch.tensor(fsm.THETA[name], dtype=F64)
        mu = 0.5 * mu                            # (sinh grows exponentially: |f| stays moderate)
    else:
        prob = orc.synthetic_problem(8, 2, 4, seed=5, flow=name, S=S)
        program, theta = prob["program"], prob["params"]["theta"]
    return mu, v, program, theta, xs, ws


@pytest.mark.parametrize("S", (32, 5))
@pytest.mark.parametrize("name", ("sal2", "tanh3x2", "sinh_r"))
def test_moment_partials(name, S):
    from tgp.pytorch_amd import ops
    mu, v, program, theta, xs, ws = _partials_case(name, S)
    lvn = torch.log(torch.tensor([0.05], dtype=F64))
    with fsm.patched():
        r1, r2 = IG.moment_partials(mu, v, program, theta, xs, ws)
        m1_ref, m2_ref = orc.marginal_moments_flow(mu, v.clamp_min(0.0), lvn, program, theta, xs, ws)
    spec = ops.FlowSpec(program, theta.numel(), 0, DEV)
    dm1, dm2 = ops.predict_moment_grads(mu.to(DEV), v.to(DEV), lvn.to(DEV), spec, theta.to(DEV), S)
    assert dm1.shape == (2, 65) and dm2.shape == (2, 65)
    e = [rel_err(dm1[0].cpu(), r1[0]), rel_err(dm1[1].cpu(), r1[1]), rel_err(dm2[0].cpu(), r2[0]), rel_err(dm2[1].cpu(), r2[1])]
    print("partials %s S=%d: %s" % (name, S, " ".join("%.2e" % x for x in e)))
    assert max(e) <= TOL_GRAD
    assert float(dm1[1, 9]) == 0.0 and float(dm2[1, 9]) == 0.0            # v = 0: exact zeros in the v-partials
    assert rel_err(dm1[0, 9].cpu(), r1[0, 9]) <= TOL_GRAD
    m1, m2, _ = ops.predict(mu.to(DEV), v.to(DEV), lvn.to(DEV), spec, theta.to(DEV), S)    # the moments they differentiate
    assert rel_err(m1.cpu(), m1_ref) <= TOL_VAL and rel_err(m2.cpu(), m2_ref) <= TOL_VAL
    dm1b, dm2b = ops.predict_moment_grads(mu.to(DEV), v.to(DEV), lvn.to(DEV), spec, theta.to(DEV), S)
    assert torch.equal(dm1, dm1b) and torch.equal(dm2, dm2b)


def test_moment_partials_of_the_empty_program():
    from tgp.pytorch_amd import ops
    mu = torch.randn(65, dtype=F64, device=DEV)
    v = 0.1 + torch.rand(65, dtype=F64, device=DEV)
    lvn = torch.zeros(1, dtype=F64, device=DEV)
    one, zero = torch.ones(65, dtype=F64, device=DEV), torch.zeros(65, dtype=F64, device=DEV)
    for flow, S in ((None, None), (ops.FlowSpec([], 0, 0, DEV), 8)):
        dm1, dm2 = ops.predict_moment_grads(mu, v, lvn, flow, None, S)
        assert torch.equal(dm1, torch.stack((one, zero))) and torch.equal(dm2, torch.stack((zero, one)))


# ---- the models' methods -------------------------------------------------------------------------------------------------
def test_predictive_input_gradients_match_oracle_autograd():
    prob, white = _problem("sal2", True, "zero")
    p = prob["params"]
    model = _build(prob, "sal2")
    model.set_is_training(False)
    Xg = prob["X"].clone().requires_grad_(True)
    mu, v = orc.qf_moments(Xg, *white)
    m1, m2 = orc.marginal_moments_flow(mu, v, p["log_var_noise"], prob["program"], p["theta"], prob["xs"], prob["ws"])
    g1, = torch.autograd.grad(m1.sum(), Xg, retain_graph=True)
    g2, = torch.autograd.grad(m2.sum(), Xg)
    Xd = prob["X"].to(DEV)
    out = model.predictive_input_gradients(Xd)
    assert set(out) == {"m1", "m2"} and out["m1"].shape == Xd.shape and out["m2"].shape == Xd.shape
    e = (rel_err(out["m1"].cpu(), g1), rel_err(out["m2"].cpu(), g2))
    print("predictive_input_gradients: m1 %.2e m2 %.2e" % e)
    assert max(e) <= TOL_GRAD
    p1, p2, _, _ = model.predictive_distribution(Xd)              # the moments those are the gradients of
    assert rel_err(p1.cpu(), m1.detach()) <= TOL_VAL and rel_err(p2.cpu(), m2.detach()) <= TOL_VAL
    out3 = model.predictive_input_gradients(Xd, Y_std=3.0)
    assert torch.equal(out3["m1"], out["m1"] * 3.0) and torch.equal(out3["m2"], out["m2"] * 9.0)
    assert model.training                                          # train() again, as after every prediction
    # the posterior's own gradients: (Dy, N, D), the restatement's
    dmu, dv = model.posterior_input_gradients(Xd)
    r_mu, r_v = IG.qf_input_grad(prob["X"], *white)
    assert dmu.shape == (1,) + Xd.shape and dv.shape == (1,) + Xd.shape
    assert rel_err(dmu[0].cpu(), r_mu) <= TOL_GRAD and rel_err(dv[0].cpu(), r_v) <= TOL_GRAD
    from tgp.pytorch_amd.utils import input_relevance
    rel = input_relevance(model, Xd, batch_rows=16)                # in pieces: 16 x 4 + 1 rows
    assert rel_err(rel.cpu(), torch.sqrt((g1 * g1).mean(0))) <= TOL_GRAD


def test_svgp_and_linear_mean_slope():
    """The Gaussian likelihood: m1 = mu, m2 = v + noise, so the gradients are dmu (with the mean's slope a) and dv."""
    prob, white = _problem(None, True, "linear")
    model = _build(prob, None, True, "linear")
    model.set_is_training(False)
    Xd = prob["X"].to(DEV)
    r_mu, r_v = IG.qf_input_grad(prob["X"], *white)
    out = model.predictive_input_gradients(Xd)
    assert rel_err(out["m1"].cpu(), r_mu + prob["params"]["mean_a"].reshape(1, -1)) <= TOL_GRAD
    assert rel_err(out["m2"].cpu(), r_v) <= TOL_GRAD


def test_posterior_input_gradients_of_a_heteroscedastic_model():
    from test_gpu_hetero import _build_model, _set_gp_params
    N, D, M = 65, 4, 20
    pa = orc.synthetic_problem(N, D, M, 5, None, 20)
    pb = orc.synthetic_problem(N, D, M, 6, None, 20)
    pf = {k: pa["params"][k].clone() for k in KEYS}
    ph = {k: pb["params"][k].clone() for k in KEYS}
    model = _build_model(pa["X"], M, "sal2", S=20)
    _set_gp_params(model, pf, ph)
    model.set_is_training(False)
    dmu, dv = model.posterior_input_gradients(pa["X"].to(DEV))
    assert dmu.shape == (2, N, D) and dv.shape == (2, N, D)
    for c, p in enumerate((pf, ph)):
        r_mu, r_v = IG.qf_input_grad(pa["X"], *(p[k] for k in KEYS))
        e = (rel_err(dmu[c].cpu(), r_mu), rel_err(dv[c].cpu(), r_v))
        print("hetero GP %d: dmu %.2e dv %.2e" % ((c,) + e))
        assert max(e) <= TOL_GRAD
    with pytest.raises(NotImplementedError, match="heteroscedastic"):
        model.predictive_input_gradients(pa["X"].to(DEV))


# ---- end to end ---------------------------------------------------------------------------------------------------------
def test_relevance_end_to_end():
    """main.py --relevance on synthetic_relevance (y = sin(2 x0) + 0.5 x1 + noise; inputs 2 .. 5 carry nothing), SVGP, M = 20, 300
    epochs at the default optimiser settings, seed 1: the relevance of inputs 0 and 1 each exceeds the largest of inputs 2 .. 5.
    (The six values of the first GPU run are recorded in profiles/input_grad.txt.)"""
    r = subprocess.run([sys.executable, "-m", "tgp.pytorch_amd.main", "--model", "SVGP", "--dataset", "synthetic_relevance",
                        "--train_test_seed_split", "1", "--num_inducing", "20", "--epochs", "300", "--relevance"],
                       cwd=REPO, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    rows = re.findall(r"input (\d) relevance ([0-9.eE+-]+), 1/lengthscale ([0-9.eE+-]+)", r.stdout)
    assert [int(t[0]) for t in rows] == list(range(6)), r.stdout[-2000:]
    rel = [float(t[1]) for t in rows]
    print("relevance %s  1/lengthscale %s" % (" ".join("%.4f" % x for x in rel), " ".join(t[2] for t in rows)))
    assert all(math.isfinite(x) for x in rel)
    assert min(rel[0], rel[1]) > max(rel[2:]), rel
