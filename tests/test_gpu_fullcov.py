"""GPU: full-covariance q(f) (tgp_qf_cov_f64) and joint function draws (tgp_qf_joint_sample_f64) -- csrc/tgp_cov.hip.

Tolerances: mu to 1e-9 and Sigma to 1e-9 max(1, max|Sigma|) (the project's TOL_VAL) against the reference's fixtures and against
the float64 restatement of tests/fullcov_model.py; the draw kernel to 1e-12 against mu + eps Lsig^T formed on the CPU from the
factor the call returns; the draws against the restatement on the reference's Sigma to 10 x SAMPLE_CPU (test_fullcov_host.py:
what the conditioning of chol(Sigma + 1e-6 I) alone puts between two correct implementations; the factor 10 covers another
summation order through the same conditioning), floor 1e-12."""
import pytest
import torch

from conftest import load_golden
from oracle import tgp_oracle as orc

import fullcov_model as fm
from test_fullcov_host import CASES, SAMPLE_CPU, SAMPLE_JITTER

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL_VAL = 1e-9


@pytest.fixture(scope="module", autouse=True)
def f64():
    from tgp.pytorch_amd import config as cg
    old = torch.get_default_dtype()
    cg.set_maximum_precission()
    cg.device = DEV
    yield
    torch.set_default_dtype(old)


def _dev(p):
    return tuple(p[k].to(DEV) for k in ("Z", "raw_lengthscale", "raw_outputscale", "m", "Lam"))


def _check_cov(mu, Sigma, mu_ref, Sigma_ref, what):
    mu, Sigma = mu.cpu(), Sigma.cpu()
    tol = TOL_VAL * max(1.0, float(Sigma_ref.abs().max()))
    e_mu, e_S = float((mu - mu_ref).abs().max()), float((Sigma - Sigma_ref).abs().max())
    print("%s: |mu - ref| %.3e  |Sigma - ref| %.3e (tol %.1e)" % (what, e_mu, e_S, tol))
    assert e_mu <= TOL_VAL, what
    assert e_S <= tol, what
    assert torch.equal(Sigma, Sigma.t()), what
    return tol


# ---- fixture parity ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_fixture_parity(name):
    from tgp.pytorch_amd import ops
    g = load_golden(name)
    X = g["X"].to(DEV)
    mu, Sigma = ops.qf_cov(X, *_dev(g["params"]), kernel=g["kernel"])
    assert Sigma.shape == (X.shape[0], X.shape[0]) and Sigma.is_contiguous()
    tol = _check_cov(mu, Sigma, g["mu"], g["Sigma"], name)
    mu_d, v_d = ops.qf_moments(X, *_dev(g["params"]), kernel=g["kernel"])
    assert float((Sigma.diagonal() - v_d).abs().max()) <= tol
    assert float((mu - mu_d).abs().max()) <= TOL_VAL


# ---- tile edges against the restatement ---------------------------------------------------------------------------
EDGE_N = (1, 15, 64, 65, 129, 300)
EDGE_MD = ((5, 4), (100, 4), (150, 13))       # M < 16; the fused-size M; M > 128 and no multiple of 4
_edge_ref = {}


def _edge(M, D, kernel):
    """One problem of 300 rows per (M, D, kernel), its restatement computed once on the CPU: the q(f) of the first N rows is
    the leading N x N block of the q(f) of all 300."""
    key = (M, D, kernel)
    if key not in _edge_ref:
        prob = orc.synthetic_problem(300, D, M, seed=7, flow=None, S=8)
        p = prob["params"]
        mu, Sigma = fm.qf_cov(prob["X"], p["Z"], p["raw_lengthscale"], p["raw_outputscale"], p["m"], p["Lam"], kernel=kernel)
        _edge_ref[key] = (prob["X"], p, mu, Sigma)
    return _edge_ref[key]


@pytest.mark.parametrize("kernel", ("scale_rbf", "scale_matern32"))
@pytest.mark.parametrize("M,D", EDGE_MD)
@pytest.mark.parametrize("N", EDGE_N)
def test_tile_edges(N, M, D, kernel):
    from tgp.pytorch_amd import ops
    X, p, mu_ref, Sigma_ref = _edge(M, D, kernel)
    Xd = X[:N].contiguous().to(DEV)
    mu, Sigma = ops.qf_cov(Xd, *_dev(p), kernel=kernel)
    assert mu.shape == (N,) and Sigma.shape == (N, N)
    tol = _check_cov(mu, Sigma, mu_ref[:N], Sigma_ref[:N, :N], "N=%d M=%d D=%d %s" % (N, M, D, kernel))
    mu_d, v_d = ops.qf_moments(Xd, *_dev(p), kernel=kernel)
    assert float((Sigma.diagonal() - v_d).abs().max()) <= tol
    mu2, Sigma2 = ops.qf_cov(Xd, *_dev(p), kernel=kernel)
    assert torch.equal(mu, mu2) and torch.equal(Sigma, Sigma2)


# ---- joint samples ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", (1, 4, 65))
@pytest.mark.parametrize("name", CASES)
def test_joint_sample_parity(name, S):
    from tgp.pytorch_amd import ops
    g = load_golden(name)
    mu, Sigma = g["mu"], g["Sigma"]
    N = mu.numel()
    if S <= 4:
        eps = g["eps"][:S].contiguous()
    else:
        eps = torch.randn(S, N, generator=torch.Generator().manual_seed(S), dtype=torch.float64)
    F0, Lsig, status = ops.qf_joint_sample(mu.to(DEV), Sigma.to(DEV), eps.to(DEV), SAMPLE_JITTER, want_L=True)
    assert int(status[0]) == 0
    F0, Lsig = F0.cpu(), Lsig.cpu()
    assert F0.shape == (S, N)
    assert float(Lsig.triu(1).abs().max()) == 0.0 if N > 1 else True
    e_L = float((Lsig @ Lsig.t() - Sigma - SAMPLE_JITTER * torch.eye(N, dtype=torch.float64)).abs().max())
    want = mu.reshape(1, -1) + eps @ Lsig.t()
    e_F = float((F0 - want).abs().max())
    F_cpu, _ = fm.joint_draw(mu, Sigma, eps, SAMPLE_JITTER)
    e_ref = float((F0 - F_cpu).abs().max())
    print("%s S=%d: |L L^T - Sigma_j| %.3e  |F0 - (mu + eps L^T)| %.3e  |F0 - restatement| %.3e (10 x SAMPLE_CPU %.1e)"
          % (name, S, e_L, e_F, e_ref, 10 * SAMPLE_CPU[name]))
    assert e_L <= 1e-12 * max(1.0, float(Sigma.abs().max()))
    assert e_F <= 1e-12 * max(1.0, float(want.abs().max()))
    if S <= 4:          # the fixture's eps: the draws SAMPLE_CPU was computed with
        assert e_ref <= max(10.0 * SAMPLE_CPU[name], 1e-12)
    # the optional factor is optional, and the same input gives the same bits
    F1, none, _ = ops.qf_joint_sample(mu.to(DEV), Sigma.to(DEV), eps.to(DEV), SAMPLE_JITTER)
    assert none is None and torch.equal(F1.cpu(), F0)


# ---- model level ----------------------------------------------------------------------------------------------------
def _build(g, sal):
    from tgp.pytorch_amd.flow import compile_flow
    from tgp.pytorch_amd.flows import SAL
    from tgp.pytorch_amd.kernels import instance_kernel
    from tgp.pytorch_amd.likelihoods import GaussianLinearMean, GaussianNonLinearMean
    from tgp.pytorch_amd.models import sparse_MF_GP, sparse_MF_SP
    p = g["params"]
    N, D = g["X"].shape
    M = p["m"].numel()
    K = instance_kernel(g["kernel"], ard_num_dim=D, num_multioutput=1, kernel_is_shared=False,
                        init_params={"length_scale": 2.0, "kernel_scale": 2.0, "noisy_variance": 1e-6})
    ip = {"variational_distribution": {"variance_scale": 1e-5, "mean_scale": 0.0}}
    if not sal:
        model = sparse_MF_GP(["zero", K], g["X"], p["Z"].clone(), N, GaussianLinearMean(1, 0.05, False), 1, True, False,
                             False, False, False, 0.0, init_params=ip)
    else:
        model = sparse_MF_SP(["zero", K], g["X"], p["Z"].clone(), N, GaussianNonLinearMean(1, 0.05, False, quadrature_points=8),
                             1, True, False, False, False, False, [SAL(2)], "single", 0.0, init_params=ip)
    with torch.no_grad():
        model.Z.data = p["Z"].reshape(1, M, D).clone()
        model.q_U.variational_mean.data = p["m"].reshape(1, M).clone()
        model.q_U.chol_variational_covar.data = p["Lam"].reshape(1, M, M).clone()
        model.covariance_function.raw_outputscale.data = p["raw_outputscale"].reshape(1).clone()
        model.covariance_function.base_kernel.raw_lengthscale.data = p["raw_lengthscale"].reshape(1, 1, D).clone()
        model.likelihood.log_var_noise.data = p["log_var_noise"].reshape(1, 1).clone()
        if sal:
            for prm, val in zip(compile_flow(model.G_matrix[0])[1], p["theta"]):
                prm.data = val.clone().reshape(())
    return model.to(DEV)


@pytest.mark.parametrize("name,sal", (("fullcov_med_sal2", True), ("fullcov_tiny_svgp", False)))
def test_model_full_covariance_and_joint_samples(name, sal):
    from tgp.pytorch_amd import ops
    g = load_golden(name)
    model = _build(g, sal)
    X = g["X"].to(DEV)
    N, S = X.shape[0], 3
    # gradients enabled and parameters that require them: refused, naming the differentiable path
    with pytest.raises(NotImplementedError, match="diagonal=True"):
        model.marginal_variational_qf_parameters(X, diagonal=False, is_duvenaud=False)
    with torch.no_grad():
        mu, cov = model.marginal_variational_qf_parameters(X, diagonal=False, is_duvenaud=False)
        mu_d, v_d = model.marginal_variational_qf_parameters(X, diagonal=True, is_duvenaud=False)
    assert mu.shape == (1, N, 1) and cov.shape == (1, N, N) and not mu.requires_grad and not cov.requires_grad
    _check_cov(mu.reshape(-1), cov[0], g["mu"], g["Sigma"], name + " (model)")
    # the diagonal=True calls are what they were: the untouched operator on the same parameters, bit for bit
    mu_o, v_o = ops.qf_moments(X, *_dev(g["params"]), kernel=g["kernel"])
    assert mu_d.shape == (1, N, 1) and v_d.shape == (1, N, 1)
    assert torch.equal(mu_d.reshape(-1), mu_o) and torch.equal(v_d.reshape(-1), v_o)
    torch.manual_seed(11)
    f_d, m_d, c_d, f0_d = model.sample_from_variational_marginal(X, S, diagonal=True, is_duvenaud=False)
    torch.manual_seed(11)
    e = torch.randn(1, S * N, 1, dtype=torch.float64, device=DEV)
    want_f0 = (e * v_o.repeat(S).reshape(1, -1, 1).sqrt() + mu_o.repeat(S).reshape(1, -1, 1)).squeeze(2)
    assert c_d.shape == (1, S * N, 1) and torch.equal(f0_d, want_f0)
    # joint samples: documented shapes, the draws of a seeded generator through the draw kernel
    torch.manual_seed(5)
    f, mean_q_f0, cov_q_f0, f0 = model.sample_from_variational_marginal(X, S, diagonal=False, is_duvenaud=False)
    assert f.shape == (1, S * N) and f0.shape == (1, S * N)
    assert mean_q_f0.shape == (1, N, 1) and cov_q_f0.shape == (1, N, N)
    assert torch.equal(cov_q_f0, cov) and torch.equal(mean_q_f0, mu)
    torch.manual_seed(5)
    eps = torch.randn(S, N, dtype=torch.float64, device=DEV)
    info = {}
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", ops.NumericalWarning)
        F0 = ops.qf_joint_sample_safe(mu.reshape(-1), cov[0], eps, info=info)
    assert torch.equal(f0.reshape(S, N), F0)
    assert info["jitter"] in (0.0, 1e-8, 1e-7, 1e-6)
    assert bool(torch.isfinite(f).all())
    if sal:
        with torch.no_grad():
            assert torch.equal(f[0], model.G_matrix[0](f0[0], X.repeat(S, 1)))
        assert not torch.equal(f, f0)
    else:
        assert torch.equal(f, f0)
    # predictive samples on joint function draws
    model.set_is_training(False)
    y, f_k, f_0 = model.sample_from_predictive_distribution(X, 2, diagonal=False)
    assert y.shape == (1, 2, N, 1) and f_k.shape == (1, 2 * N) and bool(torch.isfinite(y).all())
    y_d, _, _ = model.sample_from_predictive_distribution(X, 2)
    assert y_d.shape == (1, 2, N, 1)


# ---- refusals -----------------------------------------------------------------------------------------------------
def test_refusals():
    from tgp.pytorch_amd import lib as L
    from tgp.pytorch_amd import ops
    g = load_golden("fullcov_tiny_svgp")
    p = _dev(g["params"])
    X = g["X"].to(DEV)
    big = torch.zeros(4097, X.shape[1], dtype=torch.float64, device=DEV)
    with pytest.raises(L.TgpError, match=r"-100 .*tgp_qf_cov_f64"):
        ops.qf_cov(big, *p)
    assert L.load().tgp_qf_cov_workspace_bytes(4097, 4, 5) == 0
    assert L.load().tgp_qf_joint_sample_workspace_bytes(4097, 4) == 0 and L.load().tgp_qf_joint_sample_workspace_bytes(64, 4097) == 0
    need = L.load().tgp_qf_cov_workspace_bytes(X.shape[0], X.shape[1], 5)
    with pytest.raises(L.TgpError, match=r"-101 .*tgp_qf_cov_f64"):
        ops.qf_cov(X, *p, workspace_bytes=need - 64)
    with pytest.raises(L.TgpError, match=r"-101 .*tgp_qf_joint_sample_f64"):
        ops.qf_joint_sample(g["mu"].to(DEV), g["Sigma"].to(DEV), g["eps"].to(DEV), 1e-6, workspace_bytes=1024)
    torch.cuda.synchronize()


def test_multiclass_model_refuses():
    from tgp.pytorch_amd.kernels import instance_kernel
    from tgp.pytorch_amd.likelihoods import MulticlassCategorical
    from tgp.pytorch_amd.models import sparse_MF_GP
    X = torch.randn(20, 3, generator=torch.Generator().manual_seed(0), dtype=torch.float64)
    K = instance_kernel("scale_rbf", ard_num_dim=3, num_multioutput=3, kernel_is_shared=False)
    model = sparse_MF_GP(["zero", K], X, X[:4].clone(), 20.0, MulticlassCategorical(3), 3, True, False, False, False, False,
                         0.0).to(DEV)
    with torch.no_grad():
        with pytest.raises(NotImplementedError, match="multi-class"):
            model.marginal_variational_qf_parameters(X.to(DEV), diagonal=False, is_duvenaud=False)
        with pytest.raises(NotImplementedError, match="multi-class"):
            model.sample_from_variational_marginal(X.to(DEV), 2, diagonal=False, is_duvenaud=False)
