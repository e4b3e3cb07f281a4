"""GPU (-m gpu): the Matern-5/2 and rational-quadratic kernels through every layer that serves 'scale_matern32' -- dense K, the
training step on the general-M path, the model classes, q(f), the closed-form q(u) and its weighted pass, greedy selection, the
unwhitened q(u), the full covariance, pathwise draws (RQ) and the step engine -- against tests/kernel_family_model.py.
The kernel settings are kfm.K4 = scale_matern52 and scale_rq at alpha = 0.5, 2, 50."""
import functools
import math

import pytest
import torch

import fullcov_model as fm
import kernel_family_model as kfm
import optqu_model as om
import pathwise_model as pm
import unwhiten_model as um
from conftest import rel_err
from oracle import tgp_oracle as orc
from test_gpu_parity import compare, run_hip

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F64 = torch.float64
TOL = 1e-9            # the project's tolerance for a float64 kernel against its restatement
K4 = kfm.K4


@pytest.fixture(scope="module", autouse=True)
def f64():
    from tgp.pytorch_amd import config as cg
    old = torch.get_default_dtype()
    cg.set_maximum_precission()
    cg.device = DEV
    yield
    torch.set_default_dtype(old)


def _hip(kind, raw_os):
    """(kernel name, raw_os on the device) as the package takes them."""
    name, ro = kfm.hip_args(kind, raw_os)
    return name, ro.to(DEV)


def _kernel_module(kind, D):
    from tgp.pytorch_amd.kernels import instance_kernel
    ip = {"length_scale": 2.0, "kernel_scale": 2.0}
    if kfm.alpha_of(kind) is not None:
        ip["alpha"] = kfm.alpha_of(kind)
    return instance_kernel(kfm.hip_name(kind), ard_num_dim=D, num_multioutput=1, kernel_is_shared=False, init_params=ip)


# ---- 1. dense K ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", K4)
def test_dense_kernel_matrix(kind):
    """ops.kernel_matrix and K(x1, x2).evaluate() at (N1, N2, D) = (1, 1, 1), (65, 17, 3), (130, 129, 16) and the square
    K_ZZ + jitter I form: relative error against the gpytorch-order restatement below 1e-12."""
    from tgp.pytorch_amd import ops
    fn = orc.KERNELS[kind]
    for N1, N2, D in ((1, 1, 1), (65, 17, 3), (130, 129, 16)):
        g = torch.Generator().manual_seed(13 * N1 + D)
        X1, X2 = torch.randn(N1, D, dtype=F64, generator=g), torch.randn(N2, D, dtype=F64, generator=g)
        rl = 0.5 + 0.3 * torch.randn(D, dtype=F64, generator=g) + (0.0 if D < 8 else 1.5)
        ro = torch.tensor([0.4], dtype=F64)
        name, rod = _hip(kind, ro)
        K = ops.kernel_matrix(X1.to(DEV), X2.to(DEV), rl.to(DEV), rod, kernel=name)
        ref = fn(X1, X2, rl, ro)
        print(kind, (N1, N2, D), "K %.3e" % rel_err(K.cpu(), ref))
        assert K.shape == (N1, N2) and rel_err(K.cpu(), ref) < 1e-12
        Ks = ops.kernel_matrix(X1.to(DEV), None, rl.to(DEV), rod, kernel=name, jitter=1e-3)
        refs = fn(X1, X1, rl, ro) + 1e-3 * torch.eye(N1, dtype=F64)
        assert Ks.shape == (N1, N1) and rel_err(Ks.cpu(), refs) < 1e-12
        mod = _kernel_module(kind, D).to(DEV)
        with torch.no_grad():
            mod.raw_outputscale.data = ro.reshape(1).to(DEV)
            mod.base_kernel.raw_lengthscale.data = rl.reshape(1, 1, D).to(DEV)
        assert mod.hip_kernel == name
        assert rel_err(mod(X1.to(DEV), X2.to(DEV)).evaluate().cpu(), ref) < 1e-12


# ---- 2. the training step on the general-M path ------------------------------------------------------------------------------
STEPS = [(300, 3, 33, "sal1", 20), (400, 5, 150, "sal2", 16), (257, 16, 129, None, 8), (300, 1, 20, "tanh3x2", 8)]
# compare's tolerances are stated for cond(K_MM) ~ 1e7 (test_gpu_parity.TOL_GRAD), and the first three problems stay below 2e7 at
# their own length-scales of about 2.  Twenty inducing points on a line do not: at length-scale 2 cond(K_ZZ) is 1e10 (Matern-5/2)
# to 1e18 (RQ), K_ZZ is singular to working precision and the oracle's own ELBO moves by 1e-4 from one machine's BLAS to the
# next.  The D = 1 problem therefore runs at length-scale 0.1, the largest of 0.05, 0.1, 0.2, ... that keeps cond(K_ZZ) below 1e7
# for all four kernel settings (1.6e3 .. 1.4e5 on the CPU; 0.2 gives 2.4e8 at alpha = 50).
STEP_LENGTHSCALE = {(300, 1, 20): 0.1}
STEP_COND_MAX = 2e7


@pytest.mark.parametrize("kind", K4)
@pytest.mark.parametrize("N,D,M,flow,S", STEPS, ids=["sal1-M33", "sal2-M150", "svgp-M129-D16", "tanh3x2-M20-D1"])
def test_step_matches_oracle(N, D, M, flow, S, kind):
    """tgp_elbo_step_f64 against autograd through the restated kernel: M below, across and above the 128 tile, D = 1 and 16;
    test_gpu_parity's tolerances; status words zero; the strict upper triangle of the Lam gradient exactly zero; the slot of
    alpha in the RQ output-scale gradient exactly zero."""
    g, hip = kfm.oracle_case(N, D, M, flow, S, kind, lengthscale=STEP_LENGTHSCALE.get((N, D, M)))
    assert g["cond"] <= STEP_COND_MAX, g["cond"]
    assert all(bool(torch.isfinite(g[k]).all()) for k in ("ELBO", "g_Z", "g_raw_lengthscale", "g_raw_outputscale"))
    out, grads, status, _ = run_hip(hip)
    assert int(status[0]) == 0 and int(status[1]) == 0
    if kfm.alpha_of(kind) is not None:
        assert grads["raw_os"].shape == (2,) and float(grads["raw_os"][1]) == 0.0
        grads["raw_os"] = grads["raw_os"][:1]
    compare(out, grads, g)
    assert float(torch.triu(grads["Lam"], 1).abs().max()) == 0.0


# ---- 3. the model classes ------------------------------------------------------------------------------------------------------
def _build(prob, kind, sal, is_whiten=True):
    from tgp.pytorch_amd.flow import compile_flow
    from tgp.pytorch_amd.flows import SAL
    from tgp.pytorch_amd.likelihoods import GaussianLinearMean, GaussianNonLinearMean
    from tgp.pytorch_amd.models import sparse_MF_GP, sparse_MF_SP
    p = prob["params"]
    N, D = prob["X"].shape
    M = p["m"].numel()
    K = _kernel_module(kind, D)
    qip = {"variational_distribution": {"variance_scale": 1e-5, "mean_scale": 0.0}}
    if not sal:
        model = sparse_MF_GP(["zero", K], prob["X"], p["Z"].clone(), N, GaussianLinearMean(1, 0.05, False), 1, is_whiten, False,
                             False, False, False, 0.0, init_params=qip)
    else:
        lik = GaussianNonLinearMean(1, 0.05, False, quadrature_points=prob["xs"].numel())
        model = sparse_MF_SP(["zero", K], prob["X"], p["Z"].clone(), N, lik, 1, is_whiten, False, False, False, False, [SAL(sal)],
                             "single", 0.0, init_params=qip)
    with torch.no_grad():
        model.Z.data = p["Z"].reshape(1, M, D).clone()
        model.q_U.variational_mean.data = p["m"].reshape(1, M).clone()
        model.q_U.chol_variational_covar.data = p["Lam"].reshape(1, M, M).clone()
        model.covariance_function.raw_outputscale.data = p["raw_outputscale"].reshape(1).clone()
        model.covariance_function.base_kernel.raw_lengthscale.data = p["raw_lengthscale"].reshape(1, 1, D).clone()
        model.likelihood.log_var_noise.data = p["log_var_noise"].reshape(1, 1).clone()
        if sal:
            spec, theta_list, _ = compile_flow(model.G_matrix[0])
            assert [tuple(b) for b in spec.blocks] == [tuple(b) for b in prob["program"]]
            for prm, val in zip(theta_list, p["theta"]):
                prm.data = val.clone().reshape(())
    return model.to(DEV)


@pytest.mark.parametrize("kind", K4)
@pytest.mark.parametrize("sal", (0, 1), ids=["sparse_MF_GP", "sparse_MF_SP-sal1"])
def test_model_class_elbo_and_backward(sal, kind):
    """instance_kernel -> sparse_MF_GP / sparse_MF_SP (SAL x 1) at (200, 4, 30): ELBO + backward against the oracle at the
    1e-9 / 1e-7 of the Matern-3/2 twin (test_gpu_big); alpha is a buffer, not a parameter."""
    prob = orc.synthetic_problem(200, 4, 30, seed=8, flow="sal1" if sal else None, S=8)
    p = prob["params"]
    model = _build(prob, kind, sal)
    K = model.covariance_function
    assert not any("alpha" in n for n, _ in model.named_parameters())
    assert ("covariance_function.base_kernel.alpha" in dict(model.named_buffers())) == (kfm.alpha_of(kind) is not None)
    elbo, ell, kld = model.ELBO(prob["X"].to(DEV), prob["Y"].to(DEV))
    elbo.backward()
    (e_o, l_o, k_o), og = orc.elbo_and_grads(prob["X"], prob["Y"], p, prob["N_total"], prob["program"], prob["xs"], prob["ws"], None,
                                             kernel=kind)
    assert rel_err(elbo.detach().cpu(), e_o) < 1e-9 and rel_err(ell.detach().cpu(), l_o) < 1e-9
    assert rel_err(model.Z.grad[0].cpu(), og["Z"]) < 1e-7
    assert rel_err(K.base_kernel.raw_lengthscale.grad.reshape(-1).cpu(), og["raw_lengthscale"]) < 1e-7
    assert K.raw_outputscale.grad.shape == K.raw_outputscale.shape
    assert rel_err(K.raw_outputscale.grad.reshape(-1).cpu(), og["raw_outputscale"]) < 1e-7
    assert rel_err(model.q_U.variational_mean.grad[0].cpu(), og["m"]) < 1e-7


# ---- 4. moments and prediction -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", K4)
def test_qf_moments_and_prediction(kind):
    """ops.qf_moments at (300, 4, 130) against orc.qf_moments: mu 1e-9, v 1e-6 relative; its autograd Function returns the
    output-scale gradient for element 0 only; the model's test_log_likelihood and exact quantiles run and are finite."""
    from tgp.pytorch_amd import ops
    prob = orc.synthetic_problem(300, 4, 130, seed=4, flow=None, S=8)
    p = prob["params"]
    mu_o, v_o = orc.qf_moments(prob["X"], p["Z"], p["raw_lengthscale"], p["raw_outputscale"], p["m"], p["Lam"], kernel=kind)
    name, ro = _hip(kind, p["raw_outputscale"])
    args = (prob["X"].to(DEV), p["Z"].to(DEV), p["raw_lengthscale"].to(DEV), ro, p["m"].to(DEV), p["Lam"].to(DEV))
    mu, v = ops.qf_moments(*args, kernel=name)
    assert rel_err(mu.cpu(), mu_o.reshape(-1)) < 1e-9
    assert float(((v.cpu() - v_o.reshape(-1)).abs() / v_o.reshape(-1).abs()).max()) < 1e-6
    # autograd: d(sum w mu + u v) against the oracle's
    gen = torch.Generator().manual_seed(2)
    w, u = torch.randn(300, dtype=F64, generator=gen), torch.randn(300, dtype=F64, generator=gen)
    leaves = [t.clone().requires_grad_(True) for t in args[1:]]
    mu_a, v_a = ops.QfMomentsFunction.apply(args[0], *leaves, name)
    ((mu_a * w.to(DEV)).sum() + (v_a * u.to(DEV)).sum()).backward()
    ol = {k: p[k].clone().requires_grad_(True) for k in ("Z", "raw_lengthscale", "raw_outputscale", "m", "Lam")}
    mu_r, v_r = orc.qf_moments(prob["X"], *ol.values(), kernel=kind)
    ((mu_r.reshape(-1) * w).sum() + (v_r.reshape(-1) * u).sum()).backward()
    go = leaves[2].grad.cpu()
    assert go.shape == ro.shape and (go.numel() == 1 or float(go[1]) == 0.0)
    assert rel_err(go[:1], ol["raw_outputscale"].grad.reshape(-1)) < 1e-7
    assert rel_err(leaves[0].grad.cpu(), ol["Z"].grad) < 1e-7 and rel_err(leaves[1].grad.cpu(), ol["raw_lengthscale"].grad) < 1e-7
    # the model's predictive methods
    model = _build(prob, kind, 0)
    model.set_is_training(False)
    ll, _ = model.test_log_likelihood(prob["X"].to(DEV), prob["Y"].to(DEV), False, torch.ones(1, dtype=F64, device=DEV))
    assert bool(torch.isfinite(ll).all())
    model.set_is_training(False)
    q = model.predictive_quantiles(prob["X"].to(DEV), [0.1, 0.5, 0.9])
    assert q.shape[-2:] == (3, 300) and bool(torch.isfinite(q).all()) and bool((q[..., 0, :] < q[..., 2, :]).all())


# ---- 5. the closed-form q(u) and the weighted K_ZX pass ------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _optqu_case(N, D, M, kind):
    """optqu_model.make_case's recipe at this shape (seeded; length-scales that keep cond(K_ZZ) <= 1e5), under `kind`."""
    g = torch.Generator().manual_seed(1000 * N + 10 * M + D)
    X, Z = torch.randn(N, D, dtype=F64, generator=g), torch.randn(M, D, dtype=F64, generator=g)
    Y = torch.sin(X @ torch.randn(D, dtype=F64, generator=g)) + 0.3 * torch.randn(N, dtype=F64, generator=g)
    raw_ls = torch.full((D,), 0.3 if D <= 4 else 0.4 * math.sqrt(D), dtype=F64) + 0.2 * torch.randn(D, dtype=F64, generator=g)
    return dict(name="kf", X=X, Y=Y, Z=Z, raw_ls=raw_ls, raw_os=torch.tensor([0.6], dtype=F64), lvn=torch.tensor([-1.5], dtype=F64),
                c=1.0, N_total=float(N), kernel=kind, jitter=0.0, N=N, D=D, M=M, w=torch.randn(N, dtype=F64, generator=g),
                r=torch.randn(N, dtype=F64, generator=g))


@pytest.mark.parametrize("kind", K4)
@pytest.mark.parametrize("N,D,M", [(300, 4, 63), (260, 8, 129)])
def test_optimal_qu_kxxk_kxwxk(N, D, M, kind):
    """ops.kxxk, ops.kxwxk and ops.optimal_qu against dense float64 torch from the restated K at test_gpu_optqu's 1e-9."""
    from tgp.pytorch_amd import ops
    p = _optqu_case(N, D, M, kind)
    name, ro = _hip(kind, p["raw_os"])
    X, Y, Z, rl, lvn = (p[k].to(DEV) for k in ("X", "Y", "Z", "raw_ls", "lvn"))
    Kzx = kfm.kernel(p["Z"], p["X"], p["raw_ls"], p["raw_os"], kind)
    C, b = ops.kxxk(X, Z, rl, ro, Y, kernel=name)
    assert rel_err(C.cpu(), Kzx @ Kzx.T) < TOL and rel_err(b.cpu(), Kzx @ p["Y"]) < TOL and torch.equal(C, C.T)
    Cw, bw = ops.kxwxk(X, Z, rl, ro, p["w"].to(DEV), p["r"].to(DEV), kernel=name)
    assert rel_err(Cw.cpu(), (Kzx * p["w"]) @ Kzx.T) < TOL and rel_err(bw.cpu(), Kzx @ p["r"]) < TOL and torch.equal(Cw, Cw.T)
    with kfm.patched(om):
        assert om.cond_K(p) <= 1e5
        m0, L0 = om.closed_form_rev(p)
        m1, L1 = om.closed_form_inv(p)
    route = max(om.rel(m0, m1), om.rel(L0, L1))
    info = {}
    m, Lam = ops.optimal_qu(X, Y, Z, rl, ro, lvn, p["N_total"], kernel=name, info=info)
    errs = (rel_err(m.cpu(), m0), rel_err(Lam.cpu(), L0), rel_err((Lam @ Lam.T).cpu(), L0 @ L0.T))
    print(kind, (N, D, M), "m, Lam, S:", errs, "cpu routes", route)
    assert route < 0.1 * TOL and max(errs) < TOL and info["jitter"] == 0.0
    assert float(torch.triu(Lam, 1).abs().max()) == 0.0


@pytest.mark.parametrize("kind", K4)
def test_model_closed_form_and_natural_gradient_steps(kind):
    """set_optimal_qu, collapsed_bound and natgrad_step_qu on a model with the kernel: the collapsed bound is the ELBO at the
    optimum (1e-9), and one natural-gradient step of length 1 from another q(u) lands on the optimum (Gaussian likelihood)."""
    prob = orc.synthetic_problem(300, 4, 63, seed=5, flow=None, S=8)
    model = _build(prob, kind, 0)
    X, Y = prob["X"].to(DEV), prob["Y"].to(DEV)
    model.natgrad_step_qu(X, Y, lr=1.0)                  # from the problem's q(u), not from the optimum
    m_n, L_n = model.q_U.variational_mean.detach().clone(), model.q_U.chol_variational_covar.detach().clone()
    model.set_optimal_qu(X, Y)
    m_s, L_s = model.q_U.variational_mean.detach().clone(), model.q_U.chol_variational_covar.detach().clone()
    with torch.no_grad():
        elbo = model.ELBO(X, Y)[0]
    bound = model.collapsed_bound(X, Y)[0]
    assert rel_err(elbo.cpu().reshape(-1), bound.detach().cpu().reshape(-1)) < TOL
    S_n, S_s = L_n[0].tril() @ L_n[0].tril().T, L_s[0].tril() @ L_s[0].tril().T
    assert rel_err(m_n.cpu(), m_s.cpu()) < 1e-7 and rel_err(S_n.cpu(), S_s.cpu()) < 1e-7


# ---- 6. greedy selection -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", K4)
@pytest.mark.parametrize("N,D,M", kfm.GREEDY_CASES)
def test_greedy_variance(N, D, M, kind):
    """GREEDY_VARIANCE: the trace equals the CPU recurrence's to 1e-10 relative, and the indices are the same (the not-gpu twin
    asserts that every pick of the CPU recurrence leads its runner-up by more than 1e-6)."""
    from tgp.pytorch_amd.utils import GREEDY_VARIANCE
    p = kfm.greedy_case(N, D, M, kind)
    r = kfm.greedy(p)
    assert r["margin"] > kfm.GREEDY_MARGIN
    K = _kernel_module(kind, D)
    with torch.no_grad():
        K.raw_outputscale.data = p["raw_os"].reshape(1).clone()
        K.base_kernel.raw_lengthscale.data = p["raw_ls"].reshape(1, 1, D).clone()
    Z, info = GREEDY_VARIANCE(p["X"].to(DEV), M, K, return_info=True)
    tr = info["trace"].cpu()
    print(kind, (N, D, M), "trace %.3e" % float(((tr - r["trace"]).abs() / r["trace"].abs()).max()), "margin %.2e" % r["margin"])
    assert info["idx"].cpu().tolist() == r["idx"].tolist()
    assert float(((tr - r["trace"]).abs() / r["trace"].abs()).max()) < 1e-10
    assert torch.equal(Z.cpu().to(F64), p["X"][r["idx"]])


# ---- 7. the unwhitened q(u) ----------------------------------------------------------------------------------------------------
UW_KEYS = ("Z", "raw_lengthscale", "raw_outputscale", "m", "Lam")


@pytest.mark.parametrize("kind", K4)
@pytest.mark.parametrize("M,D", [(16, 2), (129, 3)])
def test_unwhiten_and_its_backward(M, D, kind):
    """tgp_unwhiten_f64 / tgp_unwhiten_bwd_f64 against autograd through the restatement (test_gpu_unwhiten's tile-edge case:
    Z spread over several length-scales), 1e-9 on the values and 1e-7 on the gradients."""
    from tgp.pytorch_amd import ops
    gen = torch.Generator().manual_seed(100 + M)
    p = {"Z": 3.0 * torch.randn(M, D, generator=gen, dtype=F64), "raw_lengthscale": torch.full((D,), 0.3, dtype=F64),
         "raw_outputscale": torch.tensor([0.8], dtype=F64), "m": torch.randn(M, generator=gen, dtype=F64),
         "Lam": torch.eye(M, dtype=F64) + 0.1 * torch.randn(M, M, generator=gen, dtype=F64)}
    gm_, gL = torch.randn(M, generator=gen, dtype=F64), torch.randn(M, M, generator=gen, dtype=F64)
    leaves = [p[k].clone().requires_grad_(True) for k in UW_KEYS]
    with kfm.patched(fm):
        m_c, Lam_c, _ = um.unwhiten(*leaves, kernel=kind)
        ((m_c * gm_).sum() + (Lam_c * gL).sum()).backward()
    name, ro = _hip(kind, p["raw_outputscale"])
    dl = [(ro if k == "raw_outputscale" else p[k].to(DEV)).requires_grad_(True) for k in UW_KEYS]
    m_w, Lam_w = ops.UnwhitenFunction.apply(*dl, name, 0.0, None, None)
    ((m_w * gm_.to(DEV)).sum() + (Lam_w * gL.to(DEV)).sum()).backward()
    assert rel_err(m_w.detach().cpu(), m_c.detach()) < 1e-9 and rel_err(Lam_w.detach().cpu(), Lam_c.detach()) < 1e-9
    assert float(torch.triu(Lam_w.detach(), 1).abs().max()) == 0.0
    for k, a, b in zip(UW_KEYS, dl, leaves):
        ga, gb = a.grad.cpu(), torch.tril(b.grad) if k == "Lam" else b.grad
        if k == "raw_outputscale":
            assert ga.numel() == 1 or float(ga[1]) == 0.0
            ga = ga[:1]
        assert rel_err(ga, gb) < 1e-7, k


@pytest.mark.parametrize("kind", K4)
def test_unwhitened_model_elbo(kind):
    """is_whiten=False on the model class: the ELBO and the gradient of the output scale against autograd through the
    restatement (unwhiten_model.elbo), at the tolerances of the whitened twin."""
    prob = orc.synthetic_problem(200, 4, 30, seed=8, flow=None, S=8)
    g = dict(prob, kernel=kind)
    with kfm.patched(fm):
        (e_o, _, _), og = um.elbo_and_grads(g)
    model = _build(prob, kind, 0, is_whiten=False)
    elbo = model.ELBO(prob["X"].to(DEV), prob["Y"].to(DEV))[0]
    elbo.backward()
    assert rel_err(elbo.detach().cpu(), e_o) < 1e-9
    assert rel_err(model.covariance_function.raw_outputscale.grad.reshape(-1).cpu(), og["raw_outputscale"].reshape(-1)) < 1e-7
    assert rel_err(model.Z.grad[0].cpu(), og["Z"]) < 1e-7


# ---- 8. the full covariance of q(f) ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", K4)
def test_full_covariance(kind):
    """ops.qf_cov at N = 130 (three 64-wide tiles, the last ragged), M = 100, D = 4 against fullcov_model.qf_cov under the
    restated kernel, at test_gpu_fullcov's bounds; exactly symmetric; its diagonal is qf_moments' v."""
    from tgp.pytorch_amd import ops
    prob = orc.synthetic_problem(130, 4, 100, seed=7, flow=None, S=8)
    p = prob["params"]
    with kfm.patched(fm):
        mu_ref, S_ref = fm.qf_cov(prob["X"], p["Z"], p["raw_lengthscale"], p["raw_outputscale"], p["m"], p["Lam"], kernel=kind)
    name, ro = _hip(kind, p["raw_outputscale"])
    args = (prob["X"].to(DEV), p["Z"].to(DEV), p["raw_lengthscale"].to(DEV), ro, p["m"].to(DEV), p["Lam"].to(DEV))
    mu, Sigma = ops.qf_cov(*args, kernel=name)
    tol = TOL * max(1.0, float(S_ref.abs().max()))
    assert float((mu.cpu() - mu_ref).abs().max()) <= TOL and float((Sigma.cpu() - S_ref).abs().max()) <= tol
    assert torch.equal(Sigma, Sigma.T)
    _, v = ops.qf_moments(*args, kernel=name)
    assert float((Sigma.diagonal() - v).abs().max()) <= tol


# ---- 9. pathwise draws (RQ: the kernel of this pull request with a spectral sampler) ---------------------------------------------
@pytest.mark.parametrize("kind", [k for k in K4 if kfm.alpha_of(k) is not None])
@pytest.mark.parametrize("N,D,M,R2,S", [(65, 4, 16, 15, 3), (257, 8, 129, 64, 1)])
def test_pathwise_rq(N, D, M, R2, S, kind):
    """ops.pathwise_coeff and ops.pathwise_eval against pathwise_model's restatement under the RQ kernel, with the package's own
    seeded frequencies: coef and F0 within 1e-9 of their largest entries (test_gpu_pathwise's bound), cond(K_ZZ) <= its limit."""
    from tgp.pytorch_amd import ops
    from tgp.pytorch_amd import pathwise as pw
    p = dict(pm.make_case(N, D, M, R2, S, "scale_rbf", seed=3), kernel=kind)
    p["omega"] = pw.spectral_frequencies("scale_rq", R2, D, torch.Generator().manual_seed(R2), alpha=kfm.alpha_of(kind))
    with kfm.patched(pm):
        assert pm.cond_K(p) <= pm.COND_MAX
        cref = pm.coeff(p)
        Fref = pm.evaluate(p, cref)
    name, ro = _hip(kind, p["raw_os"])
    Z, rl, m, Lam, om_, W, eps, X = (p[k].to(DEV) for k in ("Z", "raw_ls", "m", "Lam", "omega", "W", "eps", "X"))
    coef = ops.pathwise_coeff(Z, rl, ro, m, Lam, om_, W, eps, kernel=name)
    F0 = ops.pathwise_eval(X, Z, rl, ro, om_, coef, kernel=name)
    ec = float((coef.cpu() - cref).abs().max() / cref.abs().max())
    ef = float((F0.cpu() - Fref).abs().max() / Fref.abs().max())
    print(kind, (N, D, M, R2, S), "coef %.3g  F0 %.3g" % (ec, ef))
    assert coef.shape == (2 * R2 + M, S) and F0.shape == (S, N) and ec <= TOL and ef <= TOL


def test_posterior_paths_on_the_models():
    """posterior_paths: an RQ model draws functions that are finite and reproducible from a seeded generator; a Matern-5/2 model
    raises the sampler's error."""
    from tgp.pytorch_amd import lib as L
    prob = orc.synthetic_problem(65, 4, 16, seed=3, flow=None, S=8)
    model = _build(prob, "scale_rq@2", 0)
    X = prob["X"].to(DEV)
    a = model.posterior_paths(3, num_frequencies=32, generator=torch.Generator().manual_seed(1))(X)
    b = model.posterior_paths(3, num_frequencies=32, generator=torch.Generator().manual_seed(1))(X)
    assert bool(torch.isfinite(a).all()) and torch.equal(a, b)
    with pytest.raises(L.TgpError, match="spectral"):
        _build(prob, "scale_matern52", 0).posterior_paths(3, num_frequencies=32)


# ---- 10. the step engine ---------------------------------------------------------------------------------------------------------
def test_engine_history_matern52_and_rq_refusal():
    """(300, 3, 33, sal2) with scale_matern52: five Adam steps of the captured engine equal the eager engine loop's and the
    oracle's stepped with torch.optim.Adam on the CPU, at the 1e-8 / 1e-7 of the big-engine history test.  An engine for
    'scale_rq' is refused with engine_refusal's text."""
    from tgp.pytorch_amd.engine import ElboEngine, engine_refusal
    kind = "scale_matern52"
    prob = orc.synthetic_problem(300, 3, 33, seed=9, flow="sal2", S=16)
    leaves = {k: t.clone().requires_grad_(True) for k, t in prob["params"].items()}
    opt = torch.optim.Adam(list(leaves.values()), lr=0.01)
    ref = []
    for _ in range(5):
        elbo, ell, kl = orc.elbo(prob["X"], prob["Y"], leaves["Z"], leaves["raw_lengthscale"], leaves["raw_outputscale"],
                                 leaves["m"], leaves["Lam"], leaves["log_var_noise"], prob["N_total"], prob["program"],
                                 leaves.get("theta"), prob["xs"], prob["ws"], kernel=kind)
        ref.append([float(elbo.detach()), float(ell.detach()), float(kl.detach())])
        opt.zero_grad()
        (-elbo).backward()
        opt.step()
    hists = {}
    for graph in (False, True):
        eng = ElboEngine(prob["X"], prob["Y"], prob["params"], float(prob["N_total"]), flow_blocks=prob["program"], S=16,
                         device=torch.device(DEV), kernel=kind)
        if graph:
            eng.capture()
        hist = []
        for _ in range(5):
            (eng.replay if graph else eng.step)()
            hist.append(list(eng.scalars()))
        eng.check_status()
        hists[graph] = torch.tensor(hist, dtype=F64)
        assert rel_err(hists[graph], torch.tensor(ref, dtype=F64)) < 1e-8
        assert rel_err(eng.fp.view("Z").cpu(), leaves["Z"].detach()) < 1e-7
    assert rel_err(hists[True], hists[False]) < 1e-8
    with pytest.raises(NotImplementedError) as e:
        ElboEngine(prob["X"], prob["Y"], prob["params"], float(prob["N_total"]), flow_blocks=prob["program"], S=16,
                   device=torch.device(DEV), kernel="scale_rq")
    assert str(e.value) == engine_refusal(kernel="scale_rq")


def test_rq_trains_on_the_eager_path():
    """An RQ model under torch.optim.Adam on ELBO + backward (what the trainers run where the engines refuse): the ELBO of the
    last of 5 steps is finite and above the first's, and alpha stays what it was."""
    prob = orc.synthetic_problem(200, 4, 30, seed=8, flow=None, S=8)
    model = _build(prob, "scale_rq@2", 0)
    opt = torch.optim.Adam(model.parameters(), lr=0.01)
    X, Y = prob["X"].to(DEV), prob["Y"].to(DEV)
    hist = []
    for _ in range(5):
        opt.zero_grad()
        elbo = model.ELBO(X, Y)[0]
        (-elbo).backward()
        opt.step()
        hist.append(float(elbo.detach()))
    assert all(math.isfinite(h) for h in hist) and hist[-1] > hist[0]
    assert float(model.covariance_function.base_kernel.alpha) == 2.0
