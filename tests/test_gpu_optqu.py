"""GPU (-m gpu): the closed-form optimal q(u) in HIP (tgp_kxxk_f64, tgp_optimal_qu_f64) against the float64 CPU restatement of
tests/optqu_model.py, through the operators, the models, the trainer and the collapsed step engine."""
import functools

import pytest
import torch

import optqu_model as om
from conftest import load_golden, rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F64 = torch.float64
TOL = 1e-9            # the project's tolerance for a float64 kernel against its restatement


@pytest.fixture(scope="module", autouse=True)
def f64():
    from tgp.pytorch_amd import config as cg
    old = torch.get_default_dtype()
    cg.set_maximum_precission()
    cg.device = DEV
    yield
    torch.set_default_dtype(old)


# ---- 1. C = K_ZX K_XZ and b = K_ZX y ---------------------------------------------------------------------------------
MS, NS, DS = (1, 16, 63, 64, 65, 100, 128, 129, 200), (1, 15, 17, 257, 1100, 5000), (1, 4, 5, 8, 9, 13, 16)


@functools.lru_cache(maxsize=None)
def _rows(N, D):
    g = torch.Generator().manual_seed(100 * N + D)
    return torch.randn(N, D, dtype=F64, generator=g), torch.randn(N, dtype=F64, generator=g)


@functools.lru_cache(maxsize=None)
def _points(M, D):
    g = torch.Generator().manual_seed(7 + 100 * M + D)
    return (torch.randn(M, D, dtype=F64, generator=g), 0.5 + 0.3 * torch.randn(D, dtype=F64, generator=g),
            torch.tensor([0.4], dtype=F64))


def _kernel_cpu(Z, X, rl, ro, kind):
    """K(Z, X) from exact pairwise differences (no a^2 - 2ab + b^2 expansion), without the N x M x D tensor."""
    ls = torch.nn.functional.softplus(rl)
    d2 = torch.cdist(Z / ls, X / ls, compute_mode="donot_use_mm_for_euclid_dist") ** 2
    s2 = torch.nn.functional.softplus(ro).reshape(())
    if kind == "scale_matern32":
        r = d2.clamp_min(1e-30).sqrt()
        return s2 * (1.0 + om.SQRT3 * r) * torch.exp(-om.SQRT3 * r)
    return s2 * torch.exp(-0.5 * d2)


@pytest.mark.parametrize("kind", ["scale_rbf", "scale_matern32"])
@pytest.mark.parametrize("M", MS)
def test_kxxk_matches_cpu(M, kind):
    """Every N and D of the issue's list at this M: one to three 64-wide tile rows, N below one step, odd, and with several row
    groups.  N * 2^-53 (5000 rows: 6e-13) leaves the 1e-9 ample room."""
    from tgp.pytorch_amd import ops
    for N in NS:
        for D in DS:
            (X, Y), (Z, rl, ro) = _rows(N, D), _points(M, D)
            K = _kernel_cpu(Z, X, rl, ro, kind)
            C, b = ops.kxxk(X.to(DEV), Z.to(DEV), rl.to(DEV), ro.to(DEV), Y.to(DEV), kernel=kind)
            assert rel_err(C.cpu(), K @ K.T) < TOL and rel_err(b.cpu(), K @ Y) < TOL, (N, D)
            assert torch.equal(C, C.T), (N, D)


def test_row_groups_cover_three_with_a_ragged_last_one():
    """The workspace of one tile (M <= 64) is ngroup x (64 x 64 + 64) doubles + 16 bytes: N = 257 (a prime: no equal split) runs in
    at least three row groups, as do 1100 and 5000, and the split does not depend on the device (a host-side query)."""
    from tgp.pytorch_amd import lib as L
    lib = L.load()
    groups = {N: (lib.tgp_kxxk_workspace_bytes(N, 64) - 16) // (8 * (64 * 64 + 64)) for N in NS}
    assert groups[257] >= 3 and groups[1100] >= 3 and groups[5000] >= 3 and groups[1] == groups[15] == groups[17] == 1


# ---- 2.-5. the optimum -------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _case(name):
    """(inputs on the CPU, inputs on the device, the CPU optimum, the device optimum and its info): computed once per case."""
    from tgp.pytorch_amd import ops
    p = om.make_case(name)
    d = {k: v.to(DEV) for k, v in p.items() if torch.is_tensor(v)}
    info = {}
    m, Lam = ops.optimal_qu(d["X"], d["Y"], d["Z"], d["raw_ls"], d["raw_os"], d["lvn"], p["N_total"], jitter=p["jitter"],
                            kernel=p["kernel"], info=info)
    return p, d, om.closed_form_rev(p), (m, Lam), info


def _step(p, d, m, Lam):
    from tgp.pytorch_amd import ops
    out, g, status, _ = ops.elbo_step(d["X"], d["Y"], d["Z"], d["raw_ls"], d["raw_os"], m, Lam, d["lvn"], p["N_total"],
                                      jitter=p["jitter"], kernel=p["kernel"])
    assert int(status[0]) == 0 and int(status[1]) == 0
    return out, g


PLAIN = sorted(k for k in om.CASES if k not in om.VARIANTS)


@pytest.mark.parametrize("name", PLAIN)
def test_optimum_matches_restatement(name):
    """m*, Lam*, Lam* Lam*^T at 1e-9 where the two CPU routes agree to a tenth of it, else 10 x their discrepancy."""
    p, d, (m0, L0), (m, Lam), info = _case(name)
    route = om.OPT_CPU[name]["route"]
    tol = TOL if route < 0.1 * TOL else 10.0 * route
    errs = (rel_err(m.cpu(), m0), rel_err(Lam.cpu(), L0), rel_err((Lam @ Lam.T).cpu(), L0 @ L0.T))
    print(name, "m, Lam, S:", errs, "tol", tol)
    assert max(errs) < tol
    assert info["jitter"] == p["jitter"]
    assert float(torch.triu(Lam, 1).abs().max()) == 0.0 and bool((torch.diagonal(Lam) > 0).all())


# a recorded ratio below 2^-52 is less than the format resolves of a gradient of size 1 (M = 1: 4e-17): no yardstick for a 10 x rule
RATIO_CASES = [k for k in PLAIN if om.OPT_CPU[k]["ratio"] >= 2.0 ** -52]


def _qu_ratio(g, g0):
    num = max(float(g["m"].abs().max()), float(torch.tril(g["Lam"]).abs().max()))
    return num / max(float(g0["m"].abs().max()), float(torch.tril(g0["Lam"]).abs().max()))


@pytest.mark.parametrize("name", RATIO_CASES)
def test_unchanged_step_has_no_gradient_in_qu_at_the_optimum(name):
    """g_m, tril g_Lam of tgp_elbo_step_f64 at (m*, Lam*) relative to their size at m = 0, Lam = I: 10 x the CPU's own ratio.
    c = 2.5 (m64_c, m100_c_mat, m129_c_mat), Matern (m63_mat, m100_c_mat, m129_c_mat), the general-M path (m129*, m200)."""
    assert {"m64_c", "m63_mat", "m129", "m129_c_mat"} <= set(RATIO_CASES)
    p, d, _, (m, Lam), _ = _case(name)
    _, g = _step(p, d, m, Lam)
    _, g0 = _step(p, d, torch.zeros_like(m), torch.eye(p["M"], dtype=F64, device=DEV))
    ratio = _qu_ratio(g, g0)
    print(name, "ratio", ratio, "cpu", om.OPT_CPU[name]["ratio"])
    assert ratio <= 10.0 * om.OPT_CPU[name]["ratio"]


@pytest.mark.parametrize("name", om.DENSE_CASES)
def test_elbo_at_the_optimum_is_the_collapsed_bound(name):
    p, d, _, (m, Lam), _ = _case(name)
    out, _ = _step(p, d, m, Lam)
    err = rel_err(out[0].cpu(), om.dense_bound(p))
    print(name, "bound", err)
    assert err < TOL


@pytest.mark.parametrize("name", ["m16", "m64_c", "m129"])
def test_perturbing_qu_never_raises_the_elbo(name):
    p, d, _, (m, Lam), _ = _case(name)
    best = float(_step(p, d, m, Lam)[0][0])
    g = torch.Generator().manual_seed(11)
    for eps in (1e-3, 1e-1):
        for _ in range(2):
            dm = eps * torch.randn(p["M"], dtype=F64, generator=g).to(DEV)
            dL = eps * torch.tril(torch.randn(p["M"], p["M"], dtype=F64, generator=g)).to(DEV)
            assert float(_step(p, d, m + dm, Lam + dL)[0][0]) < best


@pytest.mark.parametrize("name", ["m64_c", "m100_c_mat", "m200"])
def test_repeats_are_bit_identical_and_c_is_symmetric(name):
    from tgp.pytorch_amd import ops
    p, d, _, (m, Lam), _ = _case(name)
    m2, Lam2 = ops.optimal_qu(d["X"], d["Y"], d["Z"], d["raw_ls"], d["raw_os"], d["lvn"], p["N_total"], jitter=p["jitter"],
                              kernel=p["kernel"])
    assert torch.equal(m, m2) and torch.equal(Lam, Lam2)
    (X, Y), (Z, rl, ro) = _rows(5000, p["D"]), _points(p["M"], p["D"])
    args = (X.to(DEV), Z.to(DEV), rl.to(DEV), ro.to(DEV), Y.to(DEV))
    (C1, b1), (C2, b2) = ops.kxxk(*args, kernel=p["kernel"]), ops.kxxk(*args, kernel=p["kernel"])
    assert torch.equal(C1, C2) and torch.equal(b1, b2) and torch.equal(C1, C1.T)


# ---- models ------------------------------------------------------------------------------------------------------------
def build_model(p, kind="svgp", mean="zero"):
    from tgp.pytorch_amd.flow import compile_flow
    from tgp.pytorch_amd.flows import SAL
    from tgp.pytorch_amd.kernels import instance_kernel
    from tgp.pytorch_amd.likelihoods import GaussianLinearMean, WarpedGaussianLinearMean
    from tgp.pytorch_amd.models import sparse_MF_GP
    D, M = p["D"], p["M"]
    K = instance_kernel(p["kernel"], ard_num_dim=D, num_multioutput=1, kernel_is_shared=False)
    lik = WarpedGaussianLinearMean(1, 0.05, False, SAL(1), 8) if kind == "wgp" else GaussianLinearMean(1, 0.05, False)
    model = sparse_MF_GP([mean, K], p["X"], p["Z"].clone(), p["N_total"], lik, 1, True, False, False, False, False, 0.0)
    with torch.no_grad():
        model.Z.data = p["Z"].reshape(1, M, D).clone()
        model.covariance_function.raw_outputscale.data = p["raw_os"].reshape(1).clone()
        model.covariance_function.base_kernel.raw_lengthscale.data = p["raw_ls"].reshape(1, 1, D).clone()
        lik.log_var_noise.data = p["lvn"].reshape(1, 1).clone()
        if mean == "linear":
            model.mean_function.a.data = p["mean_a"].reshape(model.mean_function.a.shape).clone()
            model.mean_function.b.data = p["mean_b"].reshape(model.mean_function.b.shape).clone()
        if kind == "wgp":
            spec, theta_list, _ = compile_flow(lik.flow[0])
            assert [tuple(b) for b in spec.blocks] == om.WARP_PROGRAM
            for prm, val in zip(theta_list, om.WARP_THETA):
                prm.data = torch.tensor(val, dtype=F64).reshape(prm.shape)
    return model.to(DEV)


HYPER = (("Z", "Z"), ("covariance_function.base_kernel.raw_lengthscale", "raw_ls"), ("covariance_function.raw_outputscale", "raw_os"),
         ("likelihood.log_var_noise", "lvn"))


@pytest.mark.parametrize("name", ["m16", "m63_mat", "m129"])
def test_collapsed_bound_gradients_match_autograd_of_the_dense_bound(name):
    """model.collapsed_bound: the value at 1e-9, the hyper-parameter gradients at 1e-7 against CPU autograd of the dense bound;
    q_U holds the optimum afterwards and receives no gradient."""
    p, d, (m0, L0), _, _ = _case(name)
    model = build_model(p)
    elbo, ell, kld = model.collapsed_bound(d["X"], d["Y"].reshape(-1, 1))
    elbo.backward()
    leaves = [p[k].clone().requires_grad_(True) for k in ("Z", "raw_ls", "raw_os", "lvn")]
    dense = om.dense_bound(p, *leaves)
    want = torch.autograd.grad(dense, leaves)
    assert rel_err(elbo.detach().cpu(), dense.detach()) < TOL
    named = dict(model.named_parameters())
    for (pn, _), w in zip(HYPER, want):
        err = rel_err(named[pn].grad.cpu().reshape(-1), w.reshape(-1))
        print(name, pn, err)
        assert err < 1e-7, pn
    assert model.q_U.variational_mean.grad is None and model.q_U.chol_variational_covar.grad is None
    assert rel_err(model.q_U.variational_mean.detach().cpu()[0], m0) < TOL
    assert rel_err(model.q_U.chol_variational_covar.detach().cpu()[0], L0) < TOL


@pytest.mark.parametrize("name,kind,mean", [("m16_linear", "svgp", "linear"), ("m16_warp", "wgp", "zero")])
def test_set_optimal_qu_on_mean_and_warped_models(name, kind, mean):
    """The optimum for the targets the model's Gaussian step sees (Y - m(X), T(Y)): q_U against the restatement on those
    targets, and the model's own ELBO has no gradient in q_U there (check 3 on the model)."""
    p = om.make_case(name)
    model = build_model(p, kind, mean)
    X, Y = p["X"].to(DEV), p["Y_raw"].reshape(-1, 1).to(DEV)
    M = p["M"]

    def qu_grads():
        model.zero_grad()
        model.ELBO(X, Y)[0].backward()
        return {"m": model.q_U.variational_mean.grad[0].clone(), "Lam": model.q_U.chol_variational_covar.grad[0].clone()}
    with torch.no_grad():
        model.q_U.variational_mean.data.zero_()
        model.q_U.chol_variational_covar.data.copy_(torch.eye(M, dtype=F64, device=DEV).reshape(1, M, M))
    g0 = qu_grads()
    info = model.set_optimal_qu(X, Y)
    assert info["jitter"] == 0.0
    m0, L0 = om.closed_form_rev(p)
    assert rel_err(model.q_U.variational_mean.detach().cpu()[0], m0) < TOL
    assert rel_err(model.q_U.chol_variational_covar.detach().cpu()[0], L0) < TOL
    ratio = _qu_ratio(qu_grads(), g0)
    print(name, "ratio", ratio, "cpu", om.OPT_CPU[name]["ratio"])
    assert ratio <= 10.0 * om.OPT_CPU[name]["ratio"]


def test_gpu_models_without_a_closed_form_refuse():
    """On the device as on the host: the refusal comes before any launch (tests/test_optqu_host.py holds the full list)."""
    from tgp.pytorch_amd.flows import SAL
    from tgp.pytorch_amd.kernels import instance_kernel
    from tgp.pytorch_amd.likelihoods import GaussianLinearMean, GaussianNonLinearMean
    from tgp.pytorch_amd.models import sparse_MF_GP, sparse_MF_SP
    p = om.make_case("m16")
    K = instance_kernel("scale_rbf", ard_num_dim=p["D"], num_multioutput=1, kernel_is_shared=False)
    X, Y = p["X"].to(DEV), p["Y"].reshape(-1, 1).to(DEV)
    tgp = sparse_MF_SP(["zero", K], p["X"], p["Z"].clone(), p["N_total"], GaussianNonLinearMean(1, 0.05, False, 8), 1, True, False,
                       False, False, False, [SAL(1)], "single", 0.0).to(DEV)
    unwh = sparse_MF_GP(["zero", K], p["X"], p["Z"].clone(), p["N_total"], GaussianLinearMean(1, 0.05, False), 1, False, False,
                        False, False, False, 0.0).to(DEV)
    for model, word in ((tgp, "TGP"), (unwh, "is_whiten=False")):
        before = model.q_U.variational_mean.detach().clone()
        with pytest.raises(NotImplementedError, match=word):
            model.set_optimal_qu(X, Y)
        assert torch.equal(model.q_U.variational_mean.detach(), before)


# ---- 6. trainer and engine ---------------------------------------------------------------------------------------------
def _train(p, resident, steps=5):
    from tgp.pytorch_amd import config as cg
    from tgp.pytorch_amd.data import DeviceLoader
    from tgp.pytorch_amd.trainers import Trainer_SP_regression
    model = build_model(p)
    loader = DeviceLoader(p["X"], p["Y"].reshape(-1, 1), 10000, shuffle=False, device=DEV)
    tr = Trainer_SP_regression(model, [loader, None, None], 1e20, False, False, torch.ones(1, device=DEV), -1, 100, True, qu="optimal")
    cg.use_step_engine = resident
    try:
        tr.train(epochs=steps, lr_ALL=0.01, opt="adam", keep_parameter_groups=True)
    finally:
        cg.use_step_engine = True
    assert (tr._engine is not None) == resident and (not resident or tr._engine.collapsed)
    hist = torch.tensor([[-l, e, k] for l, e, k in zip(tr.loss_arr, tr.ELL_arr, tr.KLD_arr)], dtype=F64)
    return model, tr, hist


@pytest.mark.parametrize("name", ["m16", "m129"])
def test_collapsed_engine_reproduces_the_eager_optimal_trainer(name):
    """Five captured collapsed steps (ElboEngine(collapsed=True), alone and as the trainer's resident engine) against five eager
    qu="optimal" steps (collapsed_bound + torch.optim.Adam on the hyper-parameters): history and Z at 1e-9; the step counter
    advances once per step; q_U ends at the optimum of the final hyper-parameters in all three."""
    from tgp.pytorch_amd.engine import ElboEngine
    p = om.make_case(name)
    eager_model, _, eager = _train(p, False)
    res_model, tr, resident = _train(p, True)
    params = {"Z": p["Z"], "raw_lengthscale": p["raw_ls"], "raw_outputscale": p["raw_os"], "m": torch.zeros(p["M"], dtype=F64),
              "Lam": torch.eye(p["M"], dtype=F64), "log_var_noise": p["lvn"]}
    eng = ElboEngine(p["X"], p["Y"], params, p["N_total"], device=DEV, kernel=p["kernel"], lr=0.01, collapsed=True)
    eng.capture()
    hist = []
    for _ in range(5):
        eng.replay()
        hist.append(list(eng.scalars()))
    eng.check_status()
    assert eng.step_dev.cpu().tolist() == [5, 0] and eng.step_tail.cpu().tolist() == [5, 0]
    eng.refresh_qu()
    hist = torch.tensor(hist, dtype=F64)
    print(name, "engine vs eager", rel_err(hist, eager), "trainer engine vs eager", rel_err(resident, eager))
    assert rel_err(hist, eager) < TOL and rel_err(resident, eager) < TOL
    Z = eager_model.Z.detach().cpu()[0]
    assert rel_err(eng.fp.view("Z").cpu(), Z) < TOL and rel_err(res_model.Z.detach().cpu()[0], Z) < TOL
    assert float((Z - p["Z"]).abs().max()) > 1e-3                    # the hyper-parameters moved
    # (m* is a function of the hyper-parameters through K^-1: their 1e-9 times the conditioning of K)
    m, tol_m = eager_model.q_U.variational_mean.detach().cpu()[0], TOL * max(1.0, om.OPT_CPU[name]["cond"])
    assert rel_err(eng.fp.view("m").cpu(), m) < tol_m and rel_err(res_model.q_U.variational_mean.detach().cpu()[0], m) < tol_m
    # and the bound rises over the five steps
    assert float(eager[-1, 0]) > float(eager[0, 0])


def test_qu_adam_leaves_the_adam5_svgp_history_where_it_is():
    """qu="adam", stated explicitly, is the path the trainer had: the reference's five-step SVGP history at the tolerance
    tests/test_gpu_models.py holds it to, through the resident engine and through the eager loop."""
    from test_gpu_models import build_model as build_golden_model
    from tgp.pytorch_amd import config as cg
    from tgp.pytorch_amd.data import DeviceLoader
    from tgp.pytorch_amd.trainers import Trainer_SP_regression
    g = load_golden("adam5_svgp")
    for resident in (True, False):
        model = build_golden_model(g, None)
        loader = DeviceLoader(g["X"], g["Y"], 10000, shuffle=False, device=DEV)
        tr = Trainer_SP_regression(model, [loader, None, None], 1e20, False, False, torch.ones(1, device=DEV), -1, 100, True, qu="adam")
        cg.use_step_engine = resident
        try:
            tr.train(epochs=g["history"].shape[0], lr_ALL=0.01, opt="adam", keep_parameter_groups=True)
        finally:
            cg.use_step_engine = True
        assert (tr._engine is not None) == resident and (not resident or not tr._engine.collapsed)
        hist = torch.tensor([[-l, e, k] for l, e, k in zip(tr.loss_arr, tr.ELL_arr, tr.KLD_arr)], dtype=F64)
        assert rel_err(hist, g["history"]) < 1e-8
        assert rel_err(model.Z.detach().cpu()[0], g["final_Z"]) < 1e-8
