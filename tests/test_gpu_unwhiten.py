"""Unwhitened q(u) (is_whiten=False) on the GPU: tgp_unwhiten_f64 / tgp_unwhiten_bwd_f64 against tests/unwhiten_model.py, and
the model classes against the reference's fixtures (tools/gen_golden_unwhitened.py)."""
import pytest
import torch

from conftest import load_golden, rel_err

import fullcov_model as fm
import unwhiten_model as um
from test_unwhiten_host import CASES, GRAD_KEYS, TOL_GRAD, TOL_VAL, tolerances

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KEYS = ("Z", "raw_lengthscale", "raw_outputscale", "m", "Lam")


@pytest.fixture(scope="module", autouse=True)
def f64():
    from tgp.pytorch_amd import config as cg
    old = torch.get_default_dtype()
    cg.set_maximum_precission()
    cg.device = DEV
    yield
    torch.set_default_dtype(old)


def _dev(p):
    return tuple(p[k].to(DEV) for k in KEYS)


def _flow_name(name):
    return {"unwh_med_sal2": "sal2", "unwh_adam5_sal2": "sal2", "unwh_bigm_matern": "tanh3x2", "unwh_bern_tiny": "sal1"}.get(name)


def build_model(g, name, is_whiten=False):
    from tgp.pytorch_amd.flow import compile_flow, instance_flow
    from tgp.pytorch_amd.flows import SAL, StepTanhL
    from tgp.pytorch_amd.kernels import instance_kernel
    from tgp.pytorch_amd.likelihoods import Bernoulli, GaussianLinearMean, GaussianNonLinearMean
    from tgp.pytorch_amd.models import sparse_MF_GP, sparse_MF_SP
    p = g["params"]
    N, D = g["X"].shape
    M = p["m"].numel()
    flow = _flow_name(name)
    bern = bool(int(g.get("bernoulli", 0)))
    K = instance_kernel(g["kernel"], ard_num_dim=D, num_multioutput=1, kernel_is_shared=False,
                        init_params={"length_scale": 2.0, "kernel_scale": 2.0, "noisy_variance": 1e-6})
    ip = {"variational_distribution": {"variance_scale": 1e-5, "mean_scale": 0.0}}
    if flow is None:
        model = sparse_MF_GP(["zero", K], g["X"], p["Z"].clone(), N, GaussianLinearMean(1, 0.05, False), 1, is_whiten, False,
                             False, False, False, 0.0, init_params=ip)
    else:
        if bern:
            lik = Bernoulli()
            lik.quad_points = g["xs"].numel()
        else:
            lik = GaussianNonLinearMean(1, 0.05, False, quadrature_points=g["xs"].numel())
        if flow.startswith("sal"):
            specs = SAL(int(flow[3:]))
        else:
            nb, ns = (int(t) for t in flow[4:].split("x"))
            specs = instance_flow(StepTanhL(nb, ns, add_f0=True))
        model = sparse_MF_SP(["zero", K], g["X"], p["Z"].clone(), N, lik, 1, is_whiten, False, False, False, False, [specs],
                             "single", 0.0, init_params=ip)
    with torch.no_grad():
        model.Z.data = p["Z"].reshape(1, M, D).clone()
        model.q_U.variational_mean.data = p["m"].reshape(1, M).clone()
        model.q_U.chol_variational_covar.data = p["Lam"].reshape(1, M, M).clone()
        model.covariance_function.raw_outputscale.data = p["raw_outputscale"].reshape(1).clone()
        model.covariance_function.base_kernel.raw_lengthscale.data = p["raw_lengthscale"].reshape(1, 1, D).clone()
        if not bern:
            model.likelihood.log_var_noise.data = p["log_var_noise"].reshape(1, 1).clone()
        if flow is not None:
            spec, theta_list, _ = compile_flow(model.G_matrix[0])
            assert [tuple(b) for b in spec.blocks] == [tuple(b) for b in g["program"]]
            for prm, val in zip(theta_list, p["theta"]):
                prm.data = val.clone().reshape(())
    return model.to(DEV)


# ---- the transform and its adjoint ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_unwhiten_matches_cpu_model(name):
    from tgp.pytorch_amd import ops
    g = load_golden(name)
    p = g["params"]
    tol, _ = tolerances(name)
    info = {}
    m_w, Lam_w, Lo, Li = ops.unwhiten(*_dev(p), kernel=g["kernel"], info=info)
    assert info["jitter"] == 0.0                                   # the fixtures pin the no-ladder path
    m_c, Lam_c, L_c = um.unwhiten(*(p[k] for k in KEYS), kernel=g["kernel"])
    e = (rel_err(m_w.cpu(), m_c), rel_err(Lam_w.cpu(), Lam_c), rel_err(Lo.cpu(), L_c))
    print("%s: m_w %.2e  Lam_w %.2e  L %.2e (tol %.1e)" % ((name,) + e + (tol,)))
    assert max(e) < tol
    assert float(torch.triu(Lam_w, 1).abs().max()) == 0.0          # exact zeros above the diagonal
    # garbage in the strict upper triangle of L_q changes nothing, bit for bit
    junk = p["Lam"].clone()
    junk += torch.triu(torch.full_like(junk, float("nan")), 1)
    args = _dev(p)[:4] + (junk.to(DEV),)
    m_2, Lam_2, _, _ = ops.unwhiten(*args, kernel=g["kernel"])
    assert torch.equal(m_2, m_w) and torch.equal(Lam_2, Lam_w)


@pytest.mark.parametrize("name", CASES)
def test_unwhiten_backward_matches_autograd(name):
    from tgp.pytorch_amd import ops
    g = load_golden(name)
    p = g["params"]
    _, tol = tolerances(name)
    M = p["m"].numel()
    gen = torch.Generator().manual_seed(11)
    gm, gL = torch.randn(M, generator=gen, dtype=torch.float64), torch.randn(M, M, generator=gen, dtype=torch.float64)
    leaves = [p[k].clone().requires_grad_(True) for k in KEYS]
    m_c, Lam_c, _ = um.unwhiten(*leaves, kernel=g["kernel"])
    ((m_c * gm).sum() + (Lam_c * gL).sum()).backward()
    dl = [p[k].to(DEV).requires_grad_(True) for k in KEYS]
    m_w, Lam_w = ops.UnwhitenFunction.apply(*dl, g["kernel"], 0.0, None, None)
    ((m_w * gm.to(DEV)).sum() + (Lam_w * gL.to(DEV)).sum()).backward()
    first = [t.grad.clone() for t in dl]
    for k, a, b in zip(KEYS, dl, leaves):
        ref = torch.tril(b.grad) if k == "Lam" else b.grad
        e = rel_err(a.grad.cpu(), ref)
        print("%s: d/d%s %.2e (tol %.1e)" % (name, k, e, tol))
        assert e < tol, k
    assert float(torch.triu(dl[4].grad, 1).abs().max()) == 0.0
    # bit-identical repeat of forward and backward
    for t in dl:
        t.grad = None
    m_2, Lam_2 = ops.UnwhitenFunction.apply(*dl, g["kernel"], 0.0, None, None)
    ((m_2 * gm.to(DEV)).sum() + (Lam_2 * gL.to(DEV)).sum()).backward()
    assert torch.equal(m_2, m_w) and torch.equal(Lam_2, Lam_w)
    assert all(torch.equal(t.grad, f) for t, f in zip(dl, first))


@pytest.mark.parametrize("M,D,kernel", ((1, 1, "scale_rbf"), (16, 2, "scale_matern32"), (65, 16, "scale_rbf"), (129, 3, "scale_matern32"),
                                        (200, 5, "scale_rbf")))
def test_tile_edges(M, D, kernel):
    """Sizes around the 16-wide MFMA tile, the 64-wide workgroup tile and the 128 limit of the single-workgroup factorisation,
    well-conditioned (Z spread over several lengthscales): the project's tolerances hold."""
    from tgp.pytorch_amd import ops
    gen = torch.Generator().manual_seed(100 + M)
    p = {"Z": 3.0 * torch.randn(M, D, generator=gen, dtype=torch.float64), "raw_lengthscale": torch.full((D,), 0.3, dtype=torch.float64),
         "raw_outputscale": torch.tensor([0.8], dtype=torch.float64), "m": torch.randn(M, generator=gen, dtype=torch.float64),
         "Lam": torch.eye(M, dtype=torch.float64) + 0.1 * torch.randn(M, M, generator=gen, dtype=torch.float64)}
    gm, gL = torch.randn(M, generator=gen, dtype=torch.float64), torch.randn(M, M, generator=gen, dtype=torch.float64)
    leaves = [p[k].clone().requires_grad_(True) for k in KEYS]
    m_c, Lam_c, _ = um.unwhiten(*leaves, kernel=kernel)
    ((m_c * gm).sum() + (Lam_c * gL).sum()).backward()
    dl = [p[k].to(DEV).requires_grad_(True) for k in KEYS]
    m_w, Lam_w = ops.UnwhitenFunction.apply(*dl, kernel, 0.0, None, None)
    ((m_w * gm.to(DEV)).sum() + (Lam_w * gL.to(DEV)).sum()).backward()
    assert rel_err(m_w.detach().cpu(), m_c.detach()) < TOL_VAL and rel_err(Lam_w.detach().cpu(), Lam_c.detach()) < TOL_VAL
    assert float(torch.triu(Lam_w.detach(), 1).abs().max()) == 0.0
    for k, a, b in zip(KEYS, dl, leaves):
        assert rel_err(a.grad.cpu(), torch.tril(b.grad) if k == "Lam" else b.grad) < TOL_GRAD, k


def test_jitter_reaches_the_prior():
    """A caller's jitter reaches K_ZZ, and a start inside the ladder is kept when the factorisation succeeds there."""
    from tgp.pytorch_amd import ops
    g = load_golden("unwh_bern_tiny")
    p = dict(g["params"])
    info = {}
    m_w, Lam_w, _, _ = ops.unwhiten(*_dev(p), jitter=1e-4, ladder=ops.KL_PRIOR_JITTERS, info=info)
    m_c, Lam_c, _ = um.unwhiten(*(p[k] for k in KEYS), jitter=1e-4)
    m_0, _, _ = um.unwhiten(*(p[k] for k in KEYS))
    assert info["jitter"] == 1e-4 and rel_err(m_w.cpu(), m_c) < TOL_VAL and rel_err(Lam_w.cpu(), Lam_c) < TOL_VAL
    assert rel_err(m_0, m_c) > 1e-4                                  # (the jitter is visible at this tolerance)


def _degenerate():
    """M = 100 inducing points within 0.01 of each other under lengthscales of 5: K_ZZ has rank ~4 in float64, its plain
    factorisation fails, and K_ZZ + 1e-8 I (rounding noise ~ M s2 eps = 2e-14) factorises."""
    gen = torch.Generator().manual_seed(77)
    M, D, N = 100, 4, 64
    p = {"Z": 0.01 * torch.randn(M, D, generator=gen, dtype=torch.float64), "raw_lengthscale": torch.full((D,), 5.0, dtype=torch.float64),
         "raw_outputscale": torch.tensor([1.0], dtype=torch.float64), "m": 0.1 * torch.randn(M, generator=gen, dtype=torch.float64),
         "Lam": 0.1 * torch.eye(M, dtype=torch.float64) + 0.01 * torch.randn(M, M, generator=gen, dtype=torch.float64),
         "log_var_noise": torch.log(torch.tensor([0.05], dtype=torch.float64))}
    X = 0.01 * torch.randn(N, D, generator=gen, dtype=torch.float64)
    Y = torch.randn(N, 1, generator=gen, dtype=torch.float64)
    return {"X": X, "Y": Y, "params": p, "kernel": "scale_rbf", "xs": torch.zeros(8), "program": None, "N_total": float(N)}


def test_ladder_on_a_degenerate_prior():
    """A K_ZZ that fails at jitter 0, through the library: the transform ends on the ladder's first rung with a warning, agrees
    with tests/unwhiten_model.py at that jitter, and the model's ELBO runs the step at the same jitter."""
    from tgp.pytorch_amd import ops
    g = _degenerate()
    p = g["params"]
    K = fm.kernel_matrix(p["Z"], p["Z"], p["raw_lengthscale"], p["raw_outputscale"])
    assert int(torch.linalg.cholesky_ex(K)[1]) != 0                 # (LAPACK agrees that it fails)
    info = {}
    with pytest.warns(ops.NumericalWarning, match="1e-08"):
        m_w, Lam_w, _, _ = ops.unwhiten(*_dev(p), info=info)
    assert info["jitter"] == 1e-8
    m_c, Lam_c, _ = um.unwhiten(*(p[k] for k in KEYS), jitter=1e-8)
    ev = torch.linalg.eigvalsh(K + 1e-8 * torch.eye(100, dtype=torch.float64))
    tol = 100 * 2.2e-16 * float(ev[-1] / ev[0])                     # M eps cond(K_ZZ + j I): both sides solve with this matrix
    e = (rel_err(m_w.cpu(), m_c), rel_err(Lam_w.cpu(), Lam_c))
    print("degenerate prior: m_w %.2e  Lam_w %.2e (tol %.1e)" % (e + (tol,)))
    assert max(e) < tol
    # the KL's ladder starts on its first rung and stays there
    info = {}
    ops.unwhiten(*_dev(p), jitter=ops.KL_PRIOR_JITTERS[0], ladder=ops.KL_PRIOR_JITTERS, info=info)
    assert info["jitter"] == 1e-8
    model = build_model(g, "degenerate")
    model.set_is_training(True)
    with pytest.warns(ops.NumericalWarning):
        elbo, ell, kld = model.ELBO(g["X"].to(DEV), g["Y"].to(DEV))
    assert model._cfg["jitter"] == 1e-8 and int(model._cfg["last_status"][0]) == 0
    (-elbo).backward()
    assert torch.isfinite(elbo) and torch.isfinite(kld) and all(torch.isfinite(q.grad).all() for q in model.parameters())
    kl_c = um.kld(*(p[k] for k in KEYS), jitter=1e-8)
    assert rel_err(kld.detach().cpu(), kl_c) < tol


def test_multiclass_unwhitened_per_class():
    """An unwhitened multi-class model applies the transform per class slice: moments and KLD of every latent GP against
    tests/unwhiten_model.py, and the KLD's gradients against its autograd."""
    from tgp.pytorch_amd.kernels import instance_kernel
    from tgp.pytorch_amd.likelihoods import MulticlassCategorical
    from tgp.pytorch_amd.models import sparse_MF_GP
    gen = torch.Generator().manual_seed(5)
    C, M, D, N = 3, 12, 3, 40
    X = torch.randn(N, D, generator=gen, dtype=torch.float64)
    K = instance_kernel("scale_rbf", ard_num_dim=D, num_multioutput=C, kernel_is_shared=False)
    model = sparse_MF_GP(["zero", K], X, X[:M].clone(), float(N), MulticlassCategorical(C), C, False, False, False, False, False, 0.0)
    p = {"Z": 2.0 * torch.randn(C, M, D, generator=gen, dtype=torch.float64),
         "raw_lengthscale": 0.3 + 0.2 * torch.randn(C, 1, D, generator=gen, dtype=torch.float64),
         "raw_outputscale": 0.5 + 0.2 * torch.randn(C, generator=gen, dtype=torch.float64),
         "m": torch.randn(C, M, generator=gen, dtype=torch.float64),
         "Lam": 0.7 * torch.eye(M, dtype=torch.float64).repeat(C, 1, 1) + 0.1 * torch.randn(C, M, M, generator=gen, dtype=torch.float64)}
    with torch.no_grad():
        model.Z.data = p["Z"].clone()
        model.q_U.variational_mean.data = p["m"].clone()
        model.q_U.chol_variational_covar.data = p["Lam"].clone()
        model.covariance_function.raw_outputscale.data = p["raw_outputscale"].clone()
        model.covariance_function.base_kernel.raw_lengthscale.data = p["raw_lengthscale"].clone()
    model = model.to(DEV)
    assert model.is_whiten is False
    with torch.no_grad():
        mu, v = model.marginal_variational_qf_parameters(X.to(DEV), diagonal=True, is_duvenaud=False)
    kld = model.KLD()
    assert kld.shape == (C,) and mu.shape == (C, N, 1)
    kld.sum().backward()
    k = model.covariance_function
    for c in range(C):
        leaves = [p["Z"][c].clone(), p["raw_lengthscale"][c].reshape(-1).clone(), p["raw_outputscale"][c:c + 1].clone(),
                  p["m"][c].clone(), p["Lam"][c].clone()]
        for t in leaves:
            t.requires_grad_(True)
        mu_c, v_c = um.qf_moments(X, *leaves)
        kl_c = um.kld(*leaves)
        kl_c.backward()
        assert rel_err(mu[c].cpu(), mu_c.detach()) < TOL_VAL and rel_err(v[c].cpu(), v_c.detach()) < TOL_VAL
        assert rel_err(kld[c].detach().cpu(), kl_c.detach()) < TOL_VAL
        got = (model.Z.grad[c], k.base_kernel.raw_lengthscale.grad[c].reshape(-1), k.raw_outputscale.grad[c:c + 1],
               model.q_U.variational_mean.grad[c], model.q_U.chol_variational_covar.grad[c])
        for name, a, b in zip(KEYS, got, leaves):
            assert rel_err(a.cpu(), torch.tril(b.grad) if name == "Lam" else b.grad) < TOL_GRAD, (c, name)


def test_refusals():
    from tgp.pytorch_amd import lib as L
    from tgp.pytorch_amd import ops
    lib = L.load()

    def args(M, D):
        return (torch.zeros(M, D, dtype=torch.float64, device=DEV), torch.zeros(D, dtype=torch.float64, device=DEV),
                torch.zeros(1, dtype=torch.float64, device=DEV), torch.zeros(M, dtype=torch.float64, device=DEV),
                torch.zeros(1, 1, dtype=torch.float64, device=DEV))
    for M, D in ((4097, 4), (8, 17)):
        assert lib.tgp_unwhiten_workspace_bytes(M, D) == 0 and lib.tgp_unwhiten_bwd_workspace_bytes(M, D) == 0
        with pytest.raises(L.TgpError, match=r"-100 tgp_unwhiten_f64"):
            ops.unwhiten(*args(M, D))
    p = load_golden("unwh_tiny_svgp")["params"]
    with pytest.raises(L.TgpError, match=r"-101 tgp_unwhiten_f64"):
        ops.unwhiten(*_dev(p), workspace_bytes=64)
    m_w, Lam_w, Lo, Li = ops.unwhiten(*_dev(p))
    Z, rl, ro = _dev(p)[:3]
    with pytest.raises(L.TgpError, match=r"-101 tgp_unwhiten_bwd_f64"):
        ops.unwhiten_bwd(Z, rl, ro, Lo, Li, m_w, Lam_w, m_w, Lam_w, workspace_bytes=64)
    big = torch.zeros(4097, 4, dtype=torch.float64, device=DEV)
    z1 = torch.zeros(1, dtype=torch.float64, device=DEV)
    rc = lib.tgp_unwhiten_bwd_f64(0, L.ptr(big), L.ptr(rl), L.ptr(ro), 4097, 4, *([L.ptr(z1)] * 11), None, 0, None)
    assert rc == L.E_UNSUPPORTED and b"tgp_unwhiten_bwd_f64" in lib.tgp_last_error()


# ---- the model classes against the reference ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_model_matches_reference(name):
    from tgp.pytorch_amd.flow import compile_flow
    g = load_golden(name)
    tol_v, tol_g = tolerances(name)
    model = build_model(g, name)
    model.set_is_training(True)
    X, Y = g["X"].to(DEV), g["Y"].to(DEV)
    with torch.no_grad():
        mu, v = model.marginal_variational_qf_parameters(X, diagonal=True, is_duvenaud=False)
        kld0 = model.KLD()
    e = (rel_err(mu.cpu(), g["mu"]), rel_err(v.cpu(), g["v"]), rel_err(kld0.cpu(), g["KLD"]))
    print("%s: mu %.2e  v %.2e  KLD %.2e (tol %.1e)" % ((name,) + e + (tol_v,)))
    assert max(e) < tol_v
    elbo, ell, kld = model.ELBO(X, Y)
    (-elbo).backward()
    e = (rel_err(elbo.detach().cpu(), g["ELBO"]), rel_err(ell.detach().cpu(), g["ELL"]), rel_err(kld.detach().cpu(), g["KLD"]))
    print("%s: ELBO %.2e  ELL %.2e  KLD %.2e (tol %.1e)" % ((name,) + e + (tol_v,)))
    assert max(e) < tol_v
    k = model.covariance_function
    got = {"g_Z": model.Z.grad[0], "g_m": model.q_U.variational_mean.grad[0], "g_Lam": model.q_U.chol_variational_covar.grad[0],
           "g_raw_outputscale": k.raw_outputscale.grad, "g_raw_lengthscale": k.base_kernel.raw_lengthscale.grad.reshape(-1)}
    if "g_log_var_noise" in g:
        got["g_log_var_noise"] = model.likelihood.log_var_noise.grad.reshape(-1)
    if "g_theta" in g:
        got["g_theta"] = torch.stack([q.grad.reshape(()) for q in compile_flow(model.G_matrix[0])[1]])
    for _, gk in GRAD_KEYS:
        if gk in g:
            e = rel_err(-got[gk].cpu(), g[gk])
            print("%s: %s %.2e (tol %.1e)" % (name, gk, e, tol_g))
            assert e < tol_g, gk


def test_trainer_first_steps_match_reference():
    from tgp.pytorch_amd.data import DeviceLoader
    from tgp.pytorch_amd.flow import compile_flow
    from tgp.pytorch_amd.trainers import Trainer_SP_regression
    g = load_golden("unwh_adam5_sal2")
    model = build_model(g, "unwh_adam5_sal2")
    loader = DeviceLoader(g["X"], g["Y"], 10000, shuffle=False, device=DEV)
    tr = Trainer_SP_regression(model, [loader, None, None], 1e20, False, False, torch.ones(1, device=DEV), -1, 100, True)
    tr.train(epochs=g["history"].shape[0], lr_ALL=0.01, opt="adam", keep_parameter_groups=True)
    assert tr._engine is None                           # unwhitened trains on the eager path
    hist = torch.tensor([[-l, e, k] for l, e, k in zip(tr.loss_arr, tr.ELL_arr, tr.KLD_arr)], dtype=torch.float64)
    e = (rel_err(hist, g["history"]), rel_err(model.Z.detach()[0].cpu(), g["final_Z"]),
         rel_err(model.q_U.variational_mean.detach()[0].cpu(), g["final_m"]),
         rel_err(torch.tril(model.q_U.chol_variational_covar.detach()[0].cpu()), torch.tril(g["final_Lam"])),
         rel_err(torch.stack([q.detach().reshape(()) for q in compile_flow(model.G_matrix[0])[1]]).cpu(), g["final_theta"]))
    print("unwh_adam5_sal2: history %.2e  Z %.2e  m %.2e  L_q %.2e  theta %.2e" % e)
    # tests/unwhiten_model.py under torch.optim.Adam for the same 5 steps is 3.2e-8 from the reference on the history (cond K_ZZ
    # 1.6e7 enters ELBO, ELL and KLD of every step) and 2.5e-11 / 1.3e-11 / 5.6e-11 / 3.2e-13 on Z / m / L_q / theta: the history is
    # held to 10 x that figure, the parameters to the 1e-8 of the whitened adam5 tests
    assert e[0] < 3.2e-7
    assert max(e[1:]) < 1e-8


@pytest.mark.parametrize("name", ("unwh_tiny_svgp", "unwh_med_sal2", "unwh_bigm_matern"))
def test_full_covariance_of_an_unwhitened_model(name):
    g = load_golden(name)
    p = g["params"]
    model = build_model(g, name)
    with torch.no_grad():
        mu, Sigma = model.marginal_variational_qf_parameters(g["X"].to(DEV), diagonal=False, is_duvenaud=False)
    mu_c, Sig_c = um.qf_cov(g["X"], *(p[k] for k in KEYS), kernel=g["kernel"])
    tol = tolerances(name)[0] * max(1.0, float(Sig_c.abs().max()))
    e = (float((mu.reshape(-1).cpu() - mu_c).abs().max()), float((Sigma[0].cpu() - Sig_c).abs().max()))
    print("%s: |mu - ref| %.2e  |Sigma - ref| %.2e (tol %.1e)" % ((name,) + e + (tol,)))
    assert max(e) <= tol
    assert rel_err(Sigma[0].diagonal().cpu(), g["v"]) < tolerances(name)[0]


def test_engines_refuse():
    from tgp.pytorch_amd.engine import ElboEngine, MinibatchEngine
    g = load_golden("unwh_tiny_svgp")
    with pytest.raises(NotImplementedError, match="is_whiten=True"):
        ElboEngine(g["X"], g["Y"], g["params"], float(g["N_total"]), device=DEV, is_whiten=False)
    with pytest.raises(NotImplementedError, match="is_whiten=True"):
        ElboEngine(g["X"], g["Y"], g["params"], float(g["N_total"]), device=DEV, world_size=2, is_whiten=False)
    with pytest.raises(NotImplementedError, match="is_whiten=True"):
        MinibatchEngine(g["X"], g["Y"], g["params"], float(g["N_total"]), 16, device=DEV, is_whiten=False)


def test_whitened_model_did_not_move():
    """A whitened model's ELBO on med_sal2: the fused step's own output, bit for bit, within the fixture's tolerance."""
    from tgp.pytorch_amd import ops
    from tgp.pytorch_amd.flow import compile_flow
    g = load_golden("med_sal2")
    model = build_model(g, "unwh_med_sal2", is_whiten=True)
    model.set_is_training(True)
    elbo, ell, kld = model.ELBO(g["X"].to(DEV), g["Y"].to(DEV))
    p = {k: v.to(DEV) for k, v in g["params"].items()}
    out, _, _, _ = ops.elbo_step(g["X"].to(DEV), g["Y"].to(DEV), p["Z"], p["raw_lengthscale"], p["raw_outputscale"], p["m"], p["Lam"],
                                 p["log_var_noise"], float(g["N_total"]), flow=compile_flow(model.G_matrix[0])[0], theta=p["theta"],
                                 S=g["xs"].numel())
    assert torch.equal(elbo.detach(), out[0]) and torch.equal(ell, out[1]) and torch.equal(kld, out[2])
    assert rel_err(elbo.detach().cpu(), g["ELBO"]) < TOL_VAL and rel_err(kld.cpu(), g["KLD"]) < TOL_VAL
