"""GPU (-m gpu): the warped Gaussian likelihood (TGP_LIK_WARPED) through every layer -- tgp_ell_warp_f64 against the
reference's fixtures (tests/golden/warp_*.npz, tools/gen_golden_warped.py) and against the autograd restatement
(tests/warp_model.py) for every kind and flag, the training step on the fused path, the general-M path and Matern, the
empty program against TGP_LIK_GAUSS bit for bit, run-to-run reproducibility, tgp_flow_inverse_f64, tgp_predict_f64, the
resident engine against the reference's Adam history, and a short end-to-end training run.

Values are held to 1e-9 and gradients to 1e-7 (the project's standing bars).  Round trip of the flow inverse: each case is held
to 10x the figures the CPU restatement measures for THAT case (tests/test_warped_host.py ROUNDTRIP_CPU: residual in t and
error in y; the bracketed-Newton cases lie between 2.2e-16 and 1.25e-15, the closed-form affine + SAL chain at 2.15e-14), with
zero non-converged elements."""
import numpy as np
import pytest
import torch

from conftest import load_golden, rel_err
import warp_model as wm
from test_warped_host import (ELL_EXTRA_CASES, EXPECTED, ROUNDTRIP_CASES, ROUNDTRIP_CPU, round_trip_figures,
                              roundtrip_inputs)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL_VAL, TOL_GRAD = 1e-9, 1e-7
F64 = torch.float64


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
    return ops.FlowSpec([tuple(int(v) for v in b) for b in program], P, RP, DEV)


def _theta(z):
    th = z.get("p_theta")
    return th if th is not None and th.numel() else None


# ---- the stand-alone likelihood ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", EXPECTED)
def test_ell_warp_matches_reference(name):
    from tgp.pytorch_amd import ops
    z = load_golden(name)
    th = _theta(z)
    res = ops.ell_warp(z["Y"].to(DEV), z["mu"].to(DEV), z["v"].to(DEV), z["p_log_var_noise"].to(DEV),
                       _spec(z["program"], 0 if th is None else th.numel()), None if th is None else th.to(DEV), want_t=True)
    assert rel_err(res["ell"].cpu(), z["lik_ELL"]) < TOL_VAL
    assert rel_err(res["logdet"].cpu(), z["logdet"]) < TOL_VAL or float(z["logdet"].abs()) == 0.0
    assert rel_err(res["t"].cpu(), z["t"]) < TOL_VAL
    assert rel_err(res["g_mu"].cpu(), z["g_mu"]) < TOL_GRAD and rel_err(res["g_v"].cpu(), z["g_v"]) < TOL_GRAD
    assert rel_err(res["g_lvn"].cpu(), z["lik_g_log_var_noise"]) < TOL_GRAD
    if th is not None:
        assert rel_err(res["g_theta"].cpu(), z["lik_g_theta"]) < TOL_GRAD


@pytest.mark.parametrize("N", [300, 20000])            # 64- and 256-lane workgroups
@pytest.mark.parametrize("case", [c for c in ROUNDTRIP_CASES if c != "per_row_sal"] + list(ELL_EXTRA_CASES))
def test_ell_warp_matches_autograd(case, N):
    from tgp.pytorch_amd import ops
    prog, theta, _, _ = roundtrip_inputs(case)
    g = torch.Generator().manual_seed(N)
    Y = torch.randn(N, generator=g, dtype=F64)
    if "boxcox" in case:
        Y = Y.abs() + 0.3
    mu = 0.8 * torch.randn(N, generator=g, dtype=F64)
    v = 0.3 * torch.rand(N, generator=g, dtype=F64)
    lvn = torch.tensor([-1.3], dtype=F64)
    scale = 2.5
    res = ops.ell_warp(Y.to(DEV), mu.to(DEV), v.to(DEV), lvn.to(DEV), _spec(prog, theta.numel()), theta.to(DEV), scale=scale)
    wrt = [t.clone().requires_grad_(True) for t in (mu, v, lvn, theta)]
    ell, ld, _ = wm.ell_warp_torch(Y, wrt[0], wrt[1], wrt[2], prog, wrt[3], scale)
    gr = torch.autograd.grad(ell, wrt)
    assert rel_err(res["ell"].cpu(), ell.detach()) < TOL_VAL and rel_err(res["logdet"].cpu(), ld.detach()) < TOL_VAL
    assert rel_err(res["g_mu"].cpu(), gr[0]) < TOL_GRAD and rel_err(res["g_v"].cpu(), gr[1]) < TOL_GRAD
    assert rel_err(res["g_lvn"].cpu(), gr[2]) < TOL_GRAD
    assert rel_err(res["g_theta"].cpu(), gr[3]) < TOL_GRAD


# ---- the training step --------------------------------------------------------------------------------------------------
def _step(z, lik, plan=0):
    from tgp.pytorch_amd import ops
    p = {k[2:]: z[k].to(DEV) for k in z if k.startswith("p_")}
    th = _theta(z)
    spec = _spec(z["program"], 0 if th is None else th.numel())
    return ops.elbo_step(z["X"].to(DEV), z["Y"].to(DEV), p["Z"], p["raw_lengthscale"], p["raw_outputscale"], p["m"], p["Lam"],
                         p["log_var_noise"], float(z["N_total"]), flow=spec, theta=None if th is None else th.to(DEV),
                         S=z["xs"].numel(), kernel=z.get("kernel", "scale_rbf"), lik=lik, plan=plan, want_moments=True)


@pytest.mark.parametrize("name", EXPECTED)               # fused path, general-M path (bigm), Matern
def test_elbo_step_matches_reference(name):
    from tgp.pytorch_amd import lib as L
    z = load_golden(name)
    plan = L.plan_chunk_rows(128) if "bigm" in name else 0     # several row chunks on the general-M path
    out, g, status, (mu, v) = _step(z, L.LIK_WARPED, plan)
    assert int(status[0]) == 0 and int(status[1]) == 0
    ref = torch.stack([z["ELBO"].reshape(()), z["ELL"].reshape(()), z["KLD"].reshape(())])
    assert rel_err(out[:3].cpu(), ref) < TOL_VAL
    assert rel_err(mu.cpu(), z["mu"]) < TOL_VAL and rel_err(v.cpu(), z["v"]) < TOL_VAL
    for k, gk in (("Z", "g_Z"), ("raw_ls", "g_raw_lengthscale"), ("raw_os", "g_raw_outputscale"), ("m", "g_m"),
                  ("lvn", "g_log_var_noise")):
        assert rel_err(g[k].cpu(), z[gk]) < TOL_GRAD, k
    assert rel_err(torch.tril(g["Lam"]).cpu(), torch.tril(z["g_Lam"])) < TOL_GRAD
    if "g_theta" in z:
        assert rel_err(g["theta"].cpu(), z["g_theta"]) < TOL_GRAD


@pytest.mark.parametrize("name", ["warp_tiny_empty", "warp_bigm_sal2"])
def test_empty_program_is_the_gaussian_step_bit_for_bit(name):
    from tgp.pytorch_amd import lib as L
    z = dict(load_golden(name))
    z["program"], z["p_theta"] = [], torch.zeros(0, dtype=F64)
    a = _step(z, L.LIK_WARPED)
    b = _step(z, L.LIK_GAUSS)
    assert torch.equal(a[0], b[0])
    for k in b[1]:
        assert torch.equal(a[1][k], b[1][k]), k
    assert torch.equal(a[3][0], b[3][0]) and torch.equal(a[3][1], b[3][1])


def test_two_runs_are_bit_identical():
    from tgp.pytorch_amd import lib as L
    from tgp.pytorch_amd import ops
    z = load_golden("warp_med_tanh3x2")
    a, b = _step(z, L.LIK_WARPED), _step(z, L.LIK_WARPED)
    assert torch.equal(a[0], b[0])
    for k in a[1]:
        assert torch.equal(a[1][k], b[1][k]), k
    prog, theta, _, _ = roundtrip_inputs("sal_al_f0")
    g = torch.Generator().manual_seed(3)
    Y, mu, v = (torch.randn(20000, generator=g, dtype=F64).to(DEV) for _ in range(3))
    lvn = torch.zeros(1, dtype=F64, device=DEV)
    r1 = ops.ell_warp(Y, mu, v.abs(), lvn, _spec(prog, theta.numel()), theta.to(DEV))
    r2 = ops.ell_warp(Y, mu, v.abs(), lvn, _spec(prog, theta.numel()), theta.to(DEV))
    for k in ("ell", "g_lvn", "logdet", "g_theta", "g_mu"):
        assert torch.equal(r1[k], r2[k]), k


def test_unsupported_per_row_program_is_refused():
    from tgp.pytorch_amd import lib as L
    from tgp.pytorch_amd import ops
    Y = torch.zeros(8, dtype=F64, device=DEV)
    with pytest.raises(L.TgpError):
        ops.ell_warp(Y, Y, Y + 1.0, Y[:1], _spec([(1, 0, 0, 4)], 0, 2), None)


# ---- the inverse ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n in EXPECTED if "bcl" not in n and "tanh" not in n and "empty" not in n])
def test_flow_inverse_matches_reference(name):
    from tgp.pytorch_amd import ops
    z = load_golden(name)
    th = _theta(z)
    x, status = ops.flow_inverse(z["inv_grid"].to(DEV), _spec(z["program"], th.numel()), th.to(DEV), check=False)
    assert int(status[0]) == 0
    assert rel_err(x.cpu(), z["inv_x"]) < TOL_VAL


@pytest.mark.parametrize("case", list(ROUNDTRIP_CASES))
def test_flow_inverse_round_trip(case):
    """Every kind, the Newton blocks (tanh steps, ADD_F0) and a PER_ROW program: T(T^-1(t)) and T^-1(T(y)) within 10x the
    figures the CPU restatement measured for the same case."""
    from tgp.pytorch_amd import ops
    prog, theta, y, rowp = roundtrip_inputs(case)
    t, _ = wm.flow_forward(y, prog, theta, rowp)
    spec = _spec(prog, theta.numel(), 0 if rowp is None else rowp.shape[1])
    x, status = ops.flow_inverse(t.to(DEV), spec, theta.to(DEV), None if rowp is None else rowp.to(DEV).contiguous(), check=False)
    assert int(status[0]) == 0
    t2, _ = wm.flow_forward(x.cpu(), prog, theta, rowp)
    r, e = round_trip_figures(t, t2, x.cpu(), y)
    print("round trip %-14s %.3e   |x - y| %.3e   (CPU %.3e, %.3e)" % ((case, r, e) + ROUNDTRIP_CPU[case]))
    assert r <= 10.0 * ROUNDTRIP_CPU[case][0]
    assert e <= 10.0 * ROUNDTRIP_CPU[case][1]


def test_flow_inverse_counts_what_it_cannot_invert():
    from tgp.pytorch_amd import lib as L
    from tgp.pytorch_amd import ops
    prog, theta, _, _ = roundtrip_inputs("tanh3")
    t = torch.tensor([0.0, 50.0, -50.0], dtype=F64, device=DEV)
    x, status = ops.flow_inverse(t, _spec([(2, 3, 0, 0)], theta.numel()), theta.to(DEV), check=False)
    assert int(status[0]) == 2
    with pytest.raises(L.TgpError):
        ops.flow_inverse(t, _spec([(2, 3, 0, 0)], theta.numel()), theta.to(DEV))


# ---- prediction ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n in EXPECTED if "bcl" not in n and "tanh" not in n])
def test_predict_matches_reference_and_restatement(name):
    from tgp.pytorch_amd import lib as L
    from tgp.pytorch_amd import ops
    z = load_golden(name)
    th = _theta(z)
    S = z["xs"].numel()
    spec = _spec(z["program"], 0 if th is None else th.numel())
    thd = None if th is None else th.to(DEV)
    m1, m2, _ = ops.predict(z["pred_mu"].to(DEV), z["pred_v"].to(DEV), z["p_log_var_noise"].to(DEV), spec, thd, S, lik=L.LIK_WARPED)
    assert rel_err(m1.cpu(), z["pred_m1"]) < TOL_VAL and rel_err(m2.cpu(), z["pred_m2"]) < TOL_VAL
    # the exact warped log density on the training rows against the restatement
    _, _, lp = ops.predict(z["mu"].to(DEV), z["v"].to(DEV), z["p_log_var_noise"].to(DEV), spec, thd, S, Y=z["Y"].to(DEV),
                           Y_std=1.7, lik=L.LIK_WARPED)
    wn = z["ws"] / np.sqrt(np.pi)
    theta = th if th is not None else torch.zeros(0, dtype=F64)
    _, _, lp_ref = wm.predict_torch(z["mu"], z["v"], z["p_log_var_noise"], z["program"], theta, z["xs"], wn, Y=z["Y"].reshape(-1),
                                    Y_std=1.7)
    assert rel_err(lp.cpu(), lp_ref) < TOL_VAL


@pytest.mark.parametrize("name", EXPECTED)               # every fixture: the density needs no inverse
def test_predict_logp_matches_restatement(name):
    from tgp.pytorch_amd import lib as L
    from tgp.pytorch_amd import ops
    z = load_golden(name)
    th = _theta(z)
    spec = _spec(z["program"], 0 if th is None else th.numel())
    m1, m2, lp = ops.predict(z["mu"].to(DEV), z["v"].to(DEV), z["p_log_var_noise"].to(DEV), spec, None if th is None else th.to(DEV),
                             z["xs"].numel(), Y=z["Y"].to(DEV), Y_std=1.7, lik=L.LIK_WARPED, want_moments=False)
    assert m1 is None and m2 is None
    theta = th if th is not None else torch.zeros(0, dtype=F64)
    t, ld = wm.flow_forward(z["Y"].reshape(-1), z["program"], theta)
    var = z["v"] + torch.exp(z["p_log_var_noise"].reshape(()))
    ref = -0.5 * (wm.LOG_2PI_REF + torch.log(var) + (t - z["mu"]) ** 2 / var) + ld - np.log(1.7)
    assert rel_err(lp.cpu(), ref) < TOL_VAL


# ---- the resident engine -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["warp_adam5_sal2", "warp_adam5_arcsl2"])
def test_engine_history_graph_equals_eager_equals_reference(name):
    from tgp.pytorch_amd.engine import ElboEngine
    g = load_golden(name)
    hists, finals = [], []
    for graph in (False, True):
        eng = ElboEngine(g["X"], g["Y"], g["params"], float(g["N_total"]), flow_blocks=g["program"], S=g["xs"].numel(),
                         device=DEV, likelihood="warped")
        if graph:
            eng.capture()
        hist = []
        for _ in range(g["history"].shape[0]):
            (eng.replay if graph else eng.step)()
            hist.append(list(eng.scalars()))
        eng.check_status()
        hists.append(torch.tensor(hist, dtype=F64))
        finals.append(eng.fp.data.clone().cpu())
        assert rel_err(hists[-1], g["history"]) < 1e-8
        assert rel_err(eng.fp.view("Z").cpu(), g["final_Z"]) < 1e-8
        assert rel_err(eng.fp.view("theta").cpu(), g["final_theta"]) < 1e-8
        assert rel_err(eng.fp.view("lvn").cpu(), g["final_log_var_noise"]) < 1e-8
    assert torch.equal(hists[0], hists[1]) and torch.equal(finals[0], finals[1])


def test_engines_refuse_minibatch_and_multirank():
    from tgp.pytorch_amd.engine import ElboEngine, MinibatchEngine
    g = load_golden("warp_adam5_sal2")
    with pytest.raises(NotImplementedError):
        MinibatchEngine(g["X"], g["Y"], g["params"], float(g["N_total"]), 32, device=DEV, flow_blocks=g["program"],
                        likelihood="warped")
    with pytest.raises(NotImplementedError):
        ElboEngine(g["X"], g["Y"], g["params"], float(g["N_total"]), flow_blocks=g["program"], device=DEV, world_size=2,
                   likelihood="warped")


# ---- the model classes against the reference ----------------------------------------------------------------------------
def _pkg_specs(name):
    """the specs tools/gen_golden_warped.py built the fixture's flow from (this package's generators, same seeds)"""
    from tgp.pytorch_amd import flows as G

    def steptanh():
        np.random.seed(0)
        return G.StepTanhL(3, 2, add_f0=True)
    gens = {"sal2": (31, lambda: G.SAL(2)), "arcsl2": (32, lambda: G.ArcSL(2)), "sal_al1": (33, lambda: G.build_chain("SAL_AL", 1)),
            "bcl_al1": (34, lambda: G.build_chain("BCL_AL", 1, constraint=None)), "tanh3x2": (35, steptanh)}
    for k, (seed, fn) in gens.items():
        if name.endswith(k):
            np.random.seed(seed)
            return fn()
    raise KeyError(name)


def build_model(g, name):
    from tgp.pytorch_amd.flow import compile_flow
    from tgp.pytorch_amd.kernels import instance_kernel
    from tgp.pytorch_amd.likelihoods import WarpedGaussianLinearMean
    from tgp.pytorch_amd.models import sparse_MF_GP
    p = g["params"]
    N, D = g["X"].shape
    M = p["m"].numel()
    K = instance_kernel(g["kernel"], ard_num_dim=D, num_multioutput=1, kernel_is_shared=False,
                        init_params={"length_scale": 2.0, "kernel_scale": 2.0, "noisy_variance": 1e-6})
    lik = WarpedGaussianLinearMean(1, 0.05, False, _pkg_specs(name), g["xs"].numel())
    model = sparse_MF_GP(["zero", K], g["X"], p["Z"].clone(), N, lik, 1, True, False, False, False, False, 0.0,
                         init_params={"variational_distribution": {"variance_scale": 1e-5, "mean_scale": 0.0}})
    with torch.no_grad():
        model.Z.data = p["Z"].reshape(1, M, D).clone()
        model.q_U.variational_mean.data = p["m"].reshape(1, M).clone()
        model.q_U.chol_variational_covar.data = p["Lam"].reshape(1, M, M).clone()
        model.covariance_function.raw_outputscale.data = p["raw_outputscale"].reshape(1).clone()
        model.covariance_function.base_kernel.raw_lengthscale.data = p["raw_lengthscale"].reshape(1, 1, D).clone()
        lik.log_var_noise.data = p["log_var_noise"].reshape(1, 1).clone()
        spec, theta_list, _ = compile_flow(lik.flow[0])
        assert [tuple(b) for b in spec.blocks] == [tuple(b) for b in g["program"]]
        for prm, val in zip(theta_list, p["theta"]):
            prm.data = val.clone().reshape(prm.shape)
    return model.to(DEV)


def _theta_grad(model):
    from tgp.pytorch_amd.flow import compile_flow
    return torch.stack([q.grad.reshape(()) for q in compile_flow(model.likelihood.flow[0])[1]]).cpu()


MODEL_CASES = ["warp_med_sal2", "warp_med_arcsl2", "warp_med_sal_al1", "warp_med_tanh3x2", "warp_tiny_bcl_al1", "warp_med_matern_sal2",
               "warp_bigm_sal2"]


@pytest.mark.parametrize("name", MODEL_CASES)
def test_model_elbo_matches_reference(name):
    """The eager model path: sparse_MF_GP.ELBO -> ops.ElboFunction with TGP_LIK_WARPED -> .backward()."""
    g = load_golden(name)
    model = build_model(g, name)
    model.set_is_training(True)
    elbo, ell, kld = model.ELBO(g["X"].to(DEV), g["Y"].to(DEV))
    elbo.backward()
    assert rel_err(elbo.detach().cpu(), g["ELBO"]) < TOL_VAL
    assert rel_err(ell.cpu(), g["ELL"]) < TOL_VAL and rel_err(kld.cpu(), g["KLD"]) < TOL_VAL
    k = model.covariance_function
    for got, key in ((model.Z.grad[0], "g_Z"), (model.q_U.variational_mean.grad[0], "g_m"),
                     (k.raw_outputscale.grad, "g_raw_outputscale"), (k.base_kernel.raw_lengthscale.grad.reshape(-1), "g_raw_lengthscale"),
                     (model.likelihood.log_var_noise.grad.reshape(-1), "g_log_var_noise")):
        assert rel_err(got.cpu(), g[key]) < TOL_GRAD, key
    assert rel_err(torch.tril(model.q_U.chol_variational_covar.grad[0]).cpu(), torch.tril(g["g_Lam"])) < TOL_GRAD
    assert rel_err(_theta_grad(model), g["g_theta"]) < TOL_GRAD


@pytest.mark.parametrize("name", ["warp_med_sal2", "warp_med_tanh3x2", "warp_tiny_bcl_al1"])
def test_likelihood_methods_match_reference(name):
    """WarpedGaussianLinearMean.expected_log_prob with autograd (ops.EllWarpFunction), unwarped_marginal_moments, log_marginal."""
    g = load_golden(name)
    model = build_model(g, name)
    lik = model.likelihood
    mu = g["mu"].reshape(1, -1).to(DEV).requires_grad_(True)
    v = g["v"].reshape(1, -1).to(DEV).requires_grad_(True)
    ell = lik.expected_log_prob(g["Y"].t().to(DEV), mu, v)
    ell.sum().backward()
    assert rel_err(ell.detach().cpu(), g["lik_ELL"]) < TOL_VAL
    assert rel_err(mu.grad.cpu(), g["g_mu"]) < TOL_GRAD and rel_err(v.grad.cpu(), g["g_v"]) < TOL_GRAD
    assert rel_err(lik.log_var_noise.grad.cpu(), g["lik_g_log_var_noise"]) < TOL_GRAD
    assert rel_err(_theta_grad(model), g["lik_g_theta"]) < TOL_GRAD
    with torch.no_grad():
        um, uv = lik.unwarped_marginal_moments(mu.detach(), v.detach(), True)
        assert torch.equal(um, mu.detach()) and rel_err(uv.cpu(), g["v"] + torch.exp(g["p_log_var_noise"])) < 1e-15
        # log_marginal with a diagonal "full" covariance: sum_n log N(T(y_n) | mu_n, v_n + s2) + sum_n log T'(y_n)
        n = 48
        lm = lik.log_marginal(g["Y"][:n].t().to(DEV), mu.detach()[:, :n], torch.diag_embed(v.detach()[:, :n]))
        th = g["p_theta"]
        t, ld = wm.flow_forward(g["Y"].reshape(-1)[:n], g["program"], th)
        var = g["v"][:n] + torch.exp(g["p_log_var_noise"].reshape(()))
        ref = (-0.5 * (np.log(2 * np.pi) + torch.log(var) + (t - g["mu"][:n]) ** 2 / var)).sum() + ld.sum()
        assert rel_err(lm.cpu(), ref) < TOL_VAL


@pytest.mark.parametrize("name", ["warp_med_sal2", "warp_med_arcsl2", "warp_med_sal_al1"])
def test_model_prediction_and_inverse_match_reference(name):
    """predictive_distribution (the warped moments), test_log_likelihood (the exact density, summed), flow.inverse and
    sample_from_output on a model built from the fixture."""
    g = load_golden(name)
    model = build_model(g, name)
    lik = model.likelihood
    model.set_is_training(False)
    m1, m2, mq, vq = model.predictive_distribution(g["Xte"].to(DEV))
    assert rel_err(mq.cpu(), g["pred_mu"]) < TOL_VAL and rel_err(vq.cpu(), g["pred_v"]) < TOL_VAL
    assert rel_err(m1.cpu(), g["pred_m1"]) < TOL_VAL and rel_err(m2.cpu(), g["pred_m2"]) < TOL_VAL
    model.set_is_training(False)
    Y_std = torch.tensor([1.7], device=DEV)
    lp, mom = model.test_log_likelihood(g["X"].to(DEV), g["Y"].to(DEV), return_moments=False, Y_std=Y_std)
    wn = g["ws"] / np.sqrt(np.pi)
    _, _, lp_ref = wm.predict_torch(g["mu"], g["v"], g["p_log_var_noise"], g["program"], g["p_theta"], g["xs"], wn,
                                    Y=g["Y"].reshape(-1), Y_std=1.7)
    assert lp.shape == (1,) and rel_err(lp.cpu(), lp_ref.sum()) < TOL_VAL
    grid = g["inv_grid"].reshape(1, -1).to(DEV)
    assert rel_err(lik.flow[0].inverse(grid).cpu(), g["inv_x"]) < TOL_VAL
    # sample_from_output = T^-1(f + s eps): with the noise switched off it is the inverse itself
    with torch.no_grad():
        lik.log_var_noise.fill_(-80.0)
        smp = lik.sample_from_output(grid, 0)
    assert smp.shape == grid.shape and rel_err(smp.cpu(), g["inv_x"]) < TOL_VAL


def test_trainer_eager_loop_matches_reference_history():
    """The trainer without the resident engine (config.use_step_engine = False): model.ELBO -> backward -> torch Adam."""
    from tgp.pytorch_amd import config as cg
    from tgp.pytorch_amd.data import DeviceLoader
    from tgp.pytorch_amd.flow import compile_flow
    from tgp.pytorch_amd.trainers import Trainer_SP_regression
    g = load_golden("warp_adam5_sal2")
    model = build_model(g, "warp_adam5_sal2")
    loader = DeviceLoader(g["X"], g["Y"], 10000, shuffle=False, device=DEV)
    old = getattr(cg, "use_step_engine", True)
    cg.use_step_engine = False
    try:
        tr = Trainer_SP_regression(model, [loader, None, None], 1e20, False, False, torch.ones(1, device=DEV), -1, 100, True)
        tr.train(epochs=g["history"].shape[0], lr_ALL=0.01, opt="adam", keep_parameter_groups=True)
    finally:
        cg.use_step_engine = old
    assert tr._engine is None
    hist = torch.tensor([[-l, e, k] for l, e, k in zip(tr.loss_arr, tr.ELL_arr, tr.KLD_arr)], dtype=F64)
    assert rel_err(hist, g["history"]) < 1e-8
    assert rel_err(model.Z.detach()[0].cpu(), g["final_Z"]) < 1e-8
    th = torch.stack([q.detach().reshape(()) for q in compile_flow(model.likelihood.flow[0])[1]]).cpu()
    assert rel_err(th, g["final_theta"]) < 1e-8
    assert rel_err(model.likelihood.log_var_noise.detach().reshape(-1).cpu(), g["final_log_var_noise"]) < 1e-8


def test_trainer_takes_the_eager_loop_for_minibatches():
    """Several minibatches per epoch: no warped minibatch engine, so the trainer keeps the eager loop (and still trains)."""
    from tgp.pytorch_amd.data import DeviceLoader
    from tgp.pytorch_amd.trainers import Trainer_SP_regression
    g = load_golden("warp_adam5_sal2")
    model = build_model(g, "warp_adam5_sal2")
    loader = DeviceLoader(g["X"], g["Y"], 32, shuffle=False, device=DEV)
    tr = Trainer_SP_regression(model, [loader, None, None], 1e20, False, False, torch.ones(1, device=DEV), -1, 100, True)
    tr.train(epochs=3, lr_ALL=0.01, opt="adam", keep_parameter_groups=True)
    assert tr._engine is None and np.isfinite([float(x) for x in tr.loss_arr]).all()


# ---- the model classes, end to end ----------------------------------------------------------------------------------------
def test_short_training_run_on_synthetic_power():
    """Trainer_SP_regression, WGP with SAL x 2 on synthetic_power: the resident engine takes it, the ELBO rises, the metrics
    (exact warped log density, RMSE of m1) are finite and the status words are clean."""
    from tgp.pytorch_amd import config as cg
    from tgp.pytorch_amd.data import return_dataset
    from tgp.pytorch_amd.flows import SAL
    from tgp.pytorch_amd.kernels import instance_kernel
    from tgp.pytorch_amd.likelihoods import WarpedGaussianLinearMean
    from tgp.pytorch_amd.models import sparse_MF_GP
    from tgp.pytorch_amd.trainers import Trainer_SP_regression
    from tgp.pytorch_amd.utils import KMEANS
    loaders, dc = return_dataset("synthetic_power", 10000, use_validation=None, seed=1, options={"shuffle_train": True})
    Dx, Dy = dc["Dx"], dc["Dy"]
    Z0 = KMEANS(dc["X_tr"], 50, n_init=1, seed=cg.config_seed)
    lik = WarpedGaussianLinearMean(Dy, 0.05, False, SAL(2), cg.quad_points)
    K = instance_kernel("scale_rbf", ard_num_dim=Dx, num_multioutput=Dy, kernel_is_shared=False,
                        init_params={"length_scale": 2.0, "kernel_scale": 2.0, "noisy_variance": 1e-6})
    model = sparse_MF_GP(["zero", K], dc["X_tr"], Z0, dc["N_tr"], lik, Dy, True, False, False, False, False, 0.0,
                         init_params={"variational_distribution": {"variance_scale": 1e-5, "mean_scale": 0.0}})
    model.to(DEV)
    Y_std = (torch.ones((Dy,)) * dc["Y_std"]).to(DEV)
    tr = Trainer_SP_regression(model=model, data_loaders=loaders, validate_each=1000, plot=False, track=False, Y_std=Y_std,
                               plot_each=-1, S_test=100, inference_in_cpu=True)
    tr.train(epochs=300, lr_ALL=0.01, opt="adam", keep_parameter_groups=True, optimisation_schedule=([1.0], [[]]), lr_groups=None)
    assert tr._engine is not None and tr._engine.warped
    tr._engine.check_status()
    loss = [float(x) for x in tr.loss_arr]
    assert np.isfinite(loss).all() and -loss[-1] > -loss[0]
    res = tr.compute_metrics()
    assert np.isfinite([float(r) for r in res]).all()
    # predictive_distribution returns the warped moments (what a caller needs for the reference's log N(y | m1, m2))
    model.set_is_training(False)
    m1, m2, _, _ = model.predictive_distribution(dc["X_te"][:64].to(DEV))
    assert torch.isfinite(m1).all() and (m2 > 0).all()
