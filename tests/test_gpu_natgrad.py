"""GPU (-m gpu): the natural-gradient step of q(u) in HIP (tgp_kxwxk_f64, tgp_natgrad_qu_f64) against the float64 CPU restatement
of tests/natgrad_model.py, through the operators, the models and the trainer.  Tolerance rule (the project's): relative error
below 1e-9 where the two CPU routes agree to a tenth of that, else 10 x their discrepancy (natgrad_model.NAT_CPU / tolerance)."""
import functools

import pytest
import torch

import natgrad_model as nm
import optqu_model as om
from conftest import rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F64 = torch.float64


@pytest.fixture(scope="module", autouse=True)
def f64():
    from tgp.pytorch_amd import config as cg
    old = torch.get_default_dtype()
    cg.set_maximum_precission()
    cg.device = DEV
    yield
    torch.set_default_dtype(old)


@functools.lru_cache(maxsize=None)
def _case(name):
    """(inputs on the CPU, the tensors among them on the device): made once per case"""
    p = nm.make_case(name)
    return p, {k: v.to(DEV) for k, v in p.items() if torch.is_tensor(v)}


def _gp(d):
    return d["X"], d["Z"], d["raw_ls"], d["raw_os"]


# ---- 1., 2. the weighted pass ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", nm.OP_CASES)
def test_kxwxk_matches_cpu(name):
    """w normal with exact zeros and both signs, r normal: the error relative to K_ZX diag(|w|) K_XZ (what the sum's terms add up
    to without cancellation); C symmetric bit for bit; two calls bit-identical; without r there is no b."""
    from tgp.pytorch_amd import ops
    p, d = _case(name)
    w, r = nm.weights(p)
    assert bool((w == 0).any()) and bool((w > 0).any()) and bool((w < 0).any())
    C0, b0, Cabs = nm.kxwxk(p, w, r)
    C, b = ops.kxwxk(*_gp(d), w.to(DEV), r.to(DEV), kernel=p["kernel"])
    C2, b2 = ops.kxwxk(*_gp(d), w.to(DEV), r.to(DEV), kernel=p["kernel"])
    tol = nm.tolerance(nm.NAT_CPU[name]["kxwxk"]["route"])
    errs = (float((C.cpu() - C0).abs().max() / Cabs.abs().max()), rel_err(b.cpu(), b0))
    print(name, "C, b:", errs, "tol", tol)
    assert max(errs) < tol
    assert torch.equal(C, C.T) and torch.equal(C, C2) and torch.equal(b, b2)
    C3, b3 = ops.kxwxk(*_gp(d), w.to(DEV), kernel=p["kernel"])
    assert b3 is None and torch.equal(C3, C)


@pytest.mark.parametrize("name", nm.OP_CASES)
def test_kxwxk_with_unit_weights_is_kxxk_bit_for_bit(name):
    """x 1.0 is exact and the sums keep their order: the weighted instantiation returns the unweighted one's bits."""
    from tgp.pytorch_amd import ops
    p, d = _case(name)
    C1, b1 = ops.kxxk(*_gp(d), d["Y"], kernel=p["kernel"])
    C2, b2 = ops.kxwxk(*_gp(d), torch.ones(p["N"], dtype=F64, device=DEV), d["Y"], kernel=p["kernel"])
    assert torch.equal(C1, C2) and torch.equal(b1, b2)


# ---- 3.-6. the step ------------------------------------------------------------------------------------------------------
def _check_step(name, sc, got, want, tol):
    (m, Lam), (m0, L0) = got, want
    errs = (rel_err(m.cpu(), m0), rel_err(Lam.cpu(), L0), rel_err((Lam @ Lam.T).cpu(), L0 @ L0.T))
    print(name, sc, "m, Lam, S:", errs, "tol", tol)
    assert max(errs) < tol
    assert float(torch.triu(Lam, 1).abs().max()) == 0.0 and bool((torch.diagonal(Lam) > 0).all())


def _run(p, d, args, **kw):
    from tgp.pytorch_amd import ops
    m, Lam, mu, mb, vb, rho, floor = args
    info = {}
    out = ops.natgrad_qu(*_gp(d), m.to(DEV), Lam.to(DEV), mu.to(DEV), mb.to(DEV), vb.to(DEV), rho=rho, site_floor=floor,
                         jitter=p["jitter"], kernel=p["kernel"], info=info, **kw)
    assert info["jitter"] == p["jitter"]
    return out


@pytest.mark.parametrize("name", nm.OP_CASES)
def test_gaussian_sites_at_rho_one_give_the_closed_form_optimum(name):
    """lambda = c / sigma^2, r = c y / sigma^2, rho = 1: optqu_model.closed_form_rev's optimum, with NaNs where the model's m and
    Lam are -- at rho = 1 they are not read."""
    p, d = _case(name)
    args = list(nm.scenario(p, "gauss"))
    args[0], args[1] = torch.full_like(args[0], float("nan")), torch.full_like(args[1], float("nan"))
    _check_step(name, "gauss", _run(p, d, args), om.closed_form_rev(p), nm.tolerance(nm.NAT_CPU[name]["gauss"]["route"]))


@pytest.mark.parametrize("rho", nm.RHOS)
@pytest.mark.parametrize("name", nm.OP_CASES)
def test_poisson_sites_match_the_restatement_and_the_step_runs_in_place(name, rho):
    """Poisson sites at a seeded (m, Lam), Lam with one negative diagonal entry (Lam Lam^T decides): m', Lam', Lam' Lam'^T; with the
    outputs aliasing the inputs the same bits."""
    p, d = _case(name)
    sc = "pois_%g" % rho
    args = nm.scenario(p, sc)
    assert args[5] == rho and (p["M"] == 1 or bool((torch.diagonal(args[1]) < 0).any()))
    got = _run(p, d, args)
    _check_step(name, sc, got, nm.update_rev(p, *args), nm.tolerance(nm.NAT_CPU[name][sc]["route"]))
    m, Lam = args[0].to(DEV).clone(), args[1].to(DEV).clone()
    from tgp.pytorch_amd import ops
    out = ops.natgrad_qu(*_gp(d), m, Lam, *(t.to(DEV) for t in args[2:5]), rho=rho, jitter=p["jitter"], kernel=p["kernel"],
                         out=(m, Lam))
    assert out[0] is m and out[1] is Lam and torch.equal(m, got[0]) and torch.equal(Lam, got[1])
    again = _run(p, d, args)
    assert torch.equal(again[0], got[0]) and torch.equal(again[1], got[1])


@pytest.mark.parametrize("name", nm.OP_CASES)
def test_the_floor_clamps_sites_of_mixed_sign(name):
    p, d = _case(name)
    args = nm.scenario(p, "floor")
    lam = -2.0 * args[4]
    assert args[6] == 0.0 and bool((lam < 0).any()) and bool((lam > 0).any())
    _check_step(name, "floor", _run(p, d, args), nm.update_rev(p, *args), nm.tolerance(nm.NAT_CPU[name]["floor"]["route"]))


def test_without_a_floor_an_indefinite_p_prime_is_an_error_and_nothing_is_written():
    """v_bar = +5 on every row (lambda = -10), site_floor=None: the restatement's P' has a negative eigenvalue; the operator raises
    NotPSDError naming P', climbs no jitter, and leaves the outputs as they were."""
    from tgp.pytorch_amd import ops
    name = "m16"
    p, d = _case(name)
    m, Lam = nm.state(p)
    mu, _ = nm.moments(p, m, Lam)
    mb, vb = torch.zeros_like(mu), torch.full_like(mu, 5.0)
    assert float(torch.linalg.eigvalsh(nm.p_prime(p, m, Lam, mu, mb, vb, 1.0, None)).min()) < -1.0
    m_out, Lam_out = torch.full((p["M"],), 7.0, dtype=F64, device=DEV), torch.full((p["M"], p["M"]), 7.0, dtype=F64, device=DEV)
    info = {}
    with pytest.raises(ops.NotPSDError, match="P' ="):
        ops.natgrad_qu(*_gp(d), m.to(DEV), Lam.to(DEV), mu.to(DEV), mb.to(DEV), vb.to(DEV), rho=1.0, site_floor=None,
                       kernel=p["kernel"], info=info, out=(m_out, Lam_out))
    assert info["not_pd"] == "P'" and info["jitter"] == 0.0
    assert bool((m_out == 7.0).all()) and bool((Lam_out == 7.0).all())


# ---- 7.-11. models at the smallest shapes ------------------------------------------------------------------------------
LIKS = ("gauss", "bernoulli", "poisson", "negbin", "student", "tgp")


def _targets(p, lik):
    if lik == "bernoulli":
        return (p["Y"] > 0).to(F64)
    if lik == "student":                 # gross errors in every seventh target: rows whose site is negative
        Y = p["Y"].clone()
        Y[::7] += 4.0
        return Y
    return p["Yc"] if lik in ("poisson", "negbin") else p["Y"]


def build_model(p, lik):
    from tgp.pytorch_amd.flows import SAL
    from tgp.pytorch_amd.kernels import instance_kernel
    from tgp.pytorch_amd.likelihoods import Bernoulli, GaussianLinearMean, GaussianNonLinearMean, NegativeBinomial, Poisson, StudentT
    from tgp.pytorch_amd.models import sparse_MF_GP, sparse_MF_SP
    D, M = p["D"], p["M"]
    K = instance_kernel(p["kernel"], ard_num_dim=D, num_multioutput=1, kernel_is_shared=False)
    tail = (1, True, False, False, False, False)
    if lik == "tgp":
        model = sparse_MF_SP(["zero", K], p["X"], p["Z"].clone(), p["N_total"], GaussianNonLinearMean(1, 0.05, False, 16), *tail,
                             [SAL(1)], "single", 0.0)
    else:
        likelihood = {"gauss": lambda: GaussianLinearMean(1, 0.05, False), "bernoulli": Bernoulli, "poisson": Poisson,
                      "negbin": lambda: NegativeBinomial(2.0), "student": lambda: StudentT(1, 0.05, False, 16, df=4.0)}[lik]()
        model = sparse_MF_GP(["zero", K], p["X"], p["Z"].clone(), p["N_total"], likelihood, *tail, 0.0)
    with torch.no_grad():
        model.Z.data = p["Z"].reshape(1, M, D).clone()
        model.covariance_function.raw_outputscale.data = p["raw_os"].reshape(1).clone()
        model.covariance_function.base_kernel.raw_lengthscale.data = p["raw_ls"].reshape(1, 1, D).clone()
        if hasattr(model.likelihood, "log_var_noise"):
            model.likelihood.log_var_noise.data = p["lvn"].reshape(1, 1).clone()
    return model.to(DEV)


def _set_qu(model, m, Lam):
    with torch.no_grad():
        model.q_U.variational_mean.data[0].copy_(m.to(DEV))
        model.q_U.chol_variational_covar.data[0].copy_(Lam.to(DEV))


def _qu(model):
    return model.q_U.variational_mean.detach()[0].clone(), model.q_U.chol_variational_covar.detach()[0].clone()


def _parent_sites(model, p, d, lik, m, Lam):
    """(mu, mu_bar, v_bar) from the operators the parent has: ops.qf_moments, then the likelihood's own ops.ell_* at scale c"""
    from tgp.pytorch_amd import ops
    Y = _targets(p, lik).to(DEV)
    mu, v = ops.qf_moments(*_gp(d), m.to(DEV), Lam.to(DEV), kernel=p["kernel"])
    c = p["c"]
    if lik == "gauss":
        res = dict(zip(("ell", "g_lvn", "g_mu", "g_v"), ops.ell_gauss(Y, mu, v, d["lvn"], scale=c)))
    else:
        spec, theta, rowp = model._flow_inputs(d["X"], with_grad=False)
        theta = None if theta is None else theta.detach()
        S = model.quad_points
        res = {"bernoulli": lambda: ops.ell_bernoulli(Y, mu, v, spec, theta, S, scale=c),
               "poisson": lambda: ops.ell_poisson(Y, mu, v, spec, theta, S, scale=c),
               "negbin": lambda: ops.ell_negbin(Y, mu, v, model.likelihood.noise().detach().contiguous(), spec, theta, S, scale=c),
               "student": lambda: ops.ell_student(Y, mu, v, d["lvn"], model.likelihood.df, spec, theta, S, scale=c),
               "tgp": lambda: ops.ell_flow(Y, mu, v, d["lvn"], spec, theta, S, scale=c)}[lik]()
    return mu.cpu(), res["g_mu"].cpu(), res["g_v"].cpu()


MODEL_CASES = [(lik, "n60_m8", lr) for lik in LIKS for lr in (0.5,)] + [("poisson", "n60_m8_mat", 1.0), ("student", "n60_m8_mat", 1.0),
                                                                        ("gauss", "n40_m6", 0.25)]


@pytest.mark.parametrize("lik,name,lr", MODEL_CASES)
def test_model_step_is_moments_then_ell_then_the_restatement(lik, name, lr):
    """natgrad_step_qu(lr) from a seeded q(u): q_U afterwards against ops.qf_moments -> the model's ops.ell_* (both as the parent
    has them) -> the CPU update, under the rule with the two CPU routes' discrepancy on these very sites (n40_m6: c = 2.5)."""
    p, d = _case(name)
    model = build_model(p, lik)
    m, Lam = nm.state(p)
    _set_qu(model, m, Lam)
    mu, mb, vb = _parent_sites(model, p, d, lik, m, Lam)
    args = (m, Lam, mu, mb, vb, lr, 0.0)
    print(lik, "rows with a negative site (clamped by the floor):", int((vb > 0).sum()))
    assert lik != "student" or bool((vb > 0).any())      # (the CPU's quadrature of these inputs finds 9 such rows)
    info = model.natgrad_step_qu(d["X"], _targets(p, lik).reshape(-1, 1).to(DEV), lr=lr)
    assert info["jitter"] == 0.0
    _check_step(name, lik, _qu(model), nm.update_rev(p, *args), nm.tolerance(nm.route_discrepancy(p, args)))


@pytest.mark.parametrize("name", ["n60_m8", "n60_m8_mat"])
def test_gaussian_model_at_lr_one_is_set_optimal_qu(name):
    p, d = _case(name)
    model = build_model(p, "gauss")
    X, Y = d["X"], d["Y"].reshape(-1, 1)
    _set_qu(model, *nm.state(p))
    model.natgrad_step_qu(X, Y, lr=1.0)
    got = _qu(model)
    model.set_optimal_qu(X, Y)
    m0, L0 = _qu(model)
    _check_step(name, "optimal", got, (m0.cpu(), L0.cpu()), nm.tolerance(nm.NAT_CPU[name]["gauss"]["route"]))
    _check_step(name, "closed form", got, om.closed_form_rev(p), nm.tolerance(nm.NAT_CPU[name]["gauss"]["route"]))


@pytest.mark.parametrize("lik", ["gauss", "bernoulli", "poisson"])
def test_one_full_step_from_the_constructors_qu_raises_the_elbo(lik):
    p, d = _case("n60_m8")
    M = p["M"]
    m, Lam = torch.zeros(M, dtype=F64), torch.eye(M, dtype=F64)
    cpu = (float(nm.elbo(p, m, Lam, lik)), float(nm.elbo(p, *nm.step(p, m, Lam, lik), lik)))
    assert cpu[1] > cpu[0] + 1.0, cpu                 # the restatement first: the rise is there to be found
    model = build_model(p, lik)
    assert torch.equal(_qu(model)[0].cpu(), m) and torch.equal(_qu(model)[1].cpu(), Lam)
    X, Y = d["X"], _targets(p, lik).reshape(-1, 1).to(DEV)
    before = float(model.ELBO(X, Y)[0].detach())
    model.natgrad_step_qu(X, Y, lr=1.0)
    after = float(model.ELBO(X, Y)[0].detach())
    print(lik, "ELBO", before, "->", after, "cpu", cpu)
    assert after > before + 1.0
    assert abs(before - cpu[0]) < 1e-6 * abs(cpu[0]) and abs(after - cpu[1]) < 1e-6 * abs(cpu[1])


def test_poisson_model_converges_in_twelve_steps():
    """|dELBO/dm| after 12 steps at lr = 1 over its value at the constructor's q(u): the host test's bound x 10."""
    from test_natgrad_host import POISSON_BOUND
    p, d = _case("n60_m8")
    model = build_model(p, "poisson")
    X, Y = d["X"], p["Yc"].reshape(-1, 1).to(DEV)

    def grad_m():
        model.zero_grad()
        model.ELBO(X, Y)[0].backward()
        return float(model.q_U.variational_mean.grad.abs().max())
    g0 = grad_m()
    for _ in range(12):
        model.natgrad_step_qu(X, Y, lr=1.0)
    ratio = grad_m() / g0
    print("ratio", ratio)
    assert ratio < 10.0 * POISSON_BOUND


def test_gpu_models_the_step_is_not_built_for_refuse():
    """On the device as on the host: the reason, before any launch, q_U where it was."""
    from test_natgrad_host import REFUSED, _model
    for kind, whiten, mean, word in REFUSED:
        model = _model(kind, whiten, mean).to(DEV)
        X, Y = torch.zeros(4, 3, dtype=F64, device=DEV), torch.zeros(4, 1, dtype=F64, device=DEV)
        before = model.q_U.variational_mean.detach().clone()
        with pytest.raises(NotImplementedError, match="natgrad_step_qu: .*" + word):
            model.natgrad_step_qu(X, Y)
        assert torch.equal(model.q_U.variational_mean.detach(), before)
    model = _model("tgp").to(DEV)
    model.be_fully_bayesian(True)
    with pytest.raises(NotImplementedError, match="be_fully_bayesian"):
        model.natgrad_step_qu(X, Y)


def test_not_psd_leaves_the_models_qu_as_it_was(monkeypatch):
    """A NotPSDError of the operator reaches the caller of natgrad_step_qu and q_U keeps its bits.  The operator's refusal is
    played by a stub here (the real one: test_without_a_floor_an_indefinite_p_prime_is_an_error_and_nothing_is_written)."""
    from tgp.pytorch_amd import ops
    p, d = _case("n60_m8")
    model = build_model(p, "student")
    _set_qu(model, *nm.state(p))
    before = _qu(model)

    def refuse(*a, **k):
        raise ops.NotPSDError("natgrad_qu: P' = ... not positive definite")
    monkeypatch.setattr(ops, "natgrad_qu", refuse)
    with pytest.raises(ops.NotPSDError, match="P'"):
        model.natgrad_step_qu(d["X"], d["Y"].reshape(-1, 1), site_floor=None)
    after = _qu(model)
    assert torch.equal(before[0], after[0]) and torch.equal(before[1], after[1])


# ---- 12. trainer ---------------------------------------------------------------------------------------------------------
def test_trainer_reproduces_the_hand_written_loop():
    """qu="natgrad", two minibatches, rho = 0.5, 3 epochs, a tiny Bernoulli model: history and parameters of the same calls in the
    same order written out by hand, to 1e-12; no optimiser state exists for q_U.*."""
    from tgp.pytorch_amd.data import DeviceLoader
    from tgp.pytorch_amd.trainers import Trainer_SP_classification
    p, d = _case("n60_m8")
    Y = _targets(p, "bernoulli").reshape(-1, 1)
    model = build_model(p, "bernoulli")
    loader = DeviceLoader(p["X"], Y, 30, shuffle=False, device=DEV)
    assert len(loader) == 2
    tr = Trainer_SP_classification(model, [loader, None, None], 1e20, False, False, torch.ones(1, device=DEV), -1, 100, True,
                                   qu="natgrad", natgrad_lr=0.5)
    tr.train(epochs=3, lr_ALL=0.01, opt="adam", keep_parameter_groups=True)
    assert tr._engine is None
    q_ids = {id(q) for n, q in model.named_parameters() if n.startswith("q_U.")}
    assert q_ids and not any(id(q) in q_ids for g in tr.optimizer.param_groups for q in g["params"])
    assert not any(id(q) in q_ids for q in tr.optimizer.state)
    assert all(q.grad is None for n, q in model.named_parameters() if n.startswith("q_U."))      # q(u) is a constant of the backward
    hist = torch.tensor([[-l, e, k] for l, e, k in zip(tr.loss_arr, tr.ELL_arr, tr.KLD_arr)], dtype=F64)
    assert hist.shape == (6, 3)

    ref = build_model(p, "bernoulli")
    opt = torch.optim.Adam([q for n, q in ref.named_parameters() if not n.startswith("q_U.")], 0.01, amsgrad=False)
    want = []
    Xd, Yd = d["X"], Y.to(DEV)
    for _ in range(3):
        for lo in (0, 30):
            x, y = Xd[lo:lo + 30], Yd[lo:lo + 30]
            info = ref.natgrad_step_qu(x, y, lr=0.5)
            elbo, ell, kld = ref.ELBO(x, y, _qu_jitter=info["jitter"])
            opt.zero_grad()
            (-elbo).backward()
            opt.step()
            want.append([float(elbo.detach()), float(ell), float(kld)])
    want = torch.tensor(want, dtype=F64)
    print("history", rel_err(hist, want))
    assert rel_err(hist, want) < 1e-12
    for (n, a), (_, b) in zip(model.named_parameters(), ref.named_parameters()):
        assert rel_err(a.detach().cpu().reshape(-1), b.detach().cpu().reshape(-1)) < 1e-12, n
    assert float((model.Z.detach().cpu()[0] - p["Z"]).abs().max()) > 1e-3          # the hyper-parameters moved
    assert float(model.q_U.variational_mean.detach().abs().max()) > 1e-2           # and so did q(u), without an optimiser
