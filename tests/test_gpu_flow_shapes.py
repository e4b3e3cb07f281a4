"""GPU (-m gpu): the sinh / normal-CDF / Tukey g-and-h / exp / softplus flow kinds (TGP_FLOW_SINH, _NORMCDF, _TUKEY, _EXP,
_SOFTPLUS) through every layer -- the flow kernels and the quadrature likelihood's gradients against torch autograd of the
restated formulas (flow_shapes_model), the fused ELBO step under every row plan and on the general-M path against the
reference's fixtures (tools/gen_golden_flow_shapes.py), exact quantiles and CDF, the warped likelihood and the flow inverse,
the trainer (eager and resident engine), the flow initialiser and the CLI.  Tolerances: those of test_gpu_flow_kinds.py."""
import subprocess
import sys
import warnings

import numpy as np
import pytest
import torch

from conftest import REPO, load_golden, rel_err

import flow_shapes_model as fm
import test_gpu_flow_kinds as tgk

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F64 = torch.float64
_f64 = tgk._f64          # (autouse: float64 default dtype, cg.device)


def _spec(prog, P):
    from tgp.pytorch_amd import ops
    return ops.FlowSpec(prog, P, 0, DEV)


def _theta(name):
    return torch.tensor(fm.THETA[name], dtype=F64)


# ---- 1. flow evaluation ----
@pytest.mark.parametrize("name", list(fm.PROGRAMS))
def test_flow_eval_and_logdet_match_autograd(name):
    from tgp.pytorch_amd import ops
    prog, th = fm.PROGRAMS[name], _theta(name)
    f = fm.f_values(name)
    fr = f.clone().requires_grad_(True)
    G = fm.flow(fr, prog, th)
    dG, = torch.autograd.grad(G.sum(), fr)
    assert torch.isfinite(G).all() and torch.isfinite(dG).all() and (dG > 0).all()
    thd = th.to(DEV) if th.numel() else None
    res = ops.flow_eval(f.to(DEV), _spec(prog, th.numel()), thd)
    errs = (rel_err(res["G"].cpu(), G.detach()), rel_err(res["dG"].cpu(), dG), rel_err(res["logdG"].cpu(), torch.log(dG)))
    s, _ = ops.flow_logdet(f.to(DEV), _spec(prog, th.numel()), thd)
    errs += (rel_err(s.cpu(), torch.log(dG).sum()),)
    print("flow_eval %s: G %.2e dG %.2e logdG %.2e sum %.2e" % ((name,) + errs))
    assert max(errs) < 1e-12, errs


def test_evaluation_overflow_gives_inf_like_sal():
    from tgp.pytorch_amd import ops
    f = torch.tensor([[-4000.0, -1.0, 0.0, 1.0, 800.0, 4000.0]], dtype=F64, device=DEV)
    G = ops.flow_eval(f, _spec([(fm.EXP, 0, 0, 0)], 0), None, want=("G",))["G"].cpu().reshape(-1)
    assert 0.0 <= G[0] < 1e-300 and G[2] == 1.0 and torch.isinf(G[4:]).all()      # (underflow: exp_fast's smallest value or 0)
    th = torch.tensor([0.0, 1.0, 0.0, 1.0], dtype=F64, device=DEV)
    G = ops.flow_eval(f, _spec([(fm.SINH, 0, 0, 0)], 4), th, want=("G",))["G"].cpu().reshape(-1)
    assert G[0] == -np.inf and G[2] == 0.0 and (G[4:] == np.inf).all()
    G = ops.flow_eval(f, _spec([(fm.SOFTPLUS, 0, 0, 0)], 0), None, want=("G",))["G"].cpu().reshape(-1)
    assert 0.0 <= G[0] < 1e-300 and G[4] == 800.0 and G[5] == 4000.0 and abs(float(G[2]) - np.log(2.0)) < 1e-15


def test_tukey_gamma_zero_is_taken_as_1e_minus_11():
    from tgp.pytorch_amd import ops
    f = torch.linspace(-2.0, 2.0, 64, dtype=F64)
    th = torch.tensor([0.0, -30.0], dtype=F64)                    # h = softplus(-30) ~ 1e-13: g ~ f
    G = ops.flow_eval(f.to(DEV), _spec([(fm.TUKEY, 0, 0, 0)], 2), th.to(DEV), want=("G",))["G"].cpu()
    assert torch.isfinite(G).all() and rel_err(G, f) < 1e-9


# ---- 2. the quadrature likelihood's gradients ----
@pytest.mark.parametrize("name", ["sinh_r", "ncdf_rf0", "tukey_left", "chain"])
# the 32-, 16- and 4-lanes-per-row variants of k_ell_quad; then four nodes in flight per lane
@pytest.mark.parametrize("N,S", [(300, 16), (5000, 16), (20000, 16), (300, 80)], ids=["300", "5000", "20000", "300-S80"])
def test_ell_flow_gradients_match_autograd(name, N, S):
    from tgp.pytorch_amd import ops
    prog, th = fm.PROGRAMS[name], _theta(name)
    g = torch.Generator().manual_seed(N)
    mu = 0.5 * torch.randn(N, generator=g, dtype=F64)
    v = 0.05 + 0.1 * torch.rand(N, generator=g, dtype=F64)
    Y = torch.randn(N, generator=g, dtype=F64)
    lvn = torch.tensor([-1.2], dtype=F64)
    res = ops.ell_flow(Y.to(DEV), mu.to(DEV), v.to(DEV), lvn.to(DEV), _spec(prog, th.numel()), th.to(DEV), S)
    xs, wn = ops.gauss_hermite(S, "cpu")
    mur, vr, thr = mu.clone().requires_grad_(True), v.clone().requires_grad_(True), th.clone().requires_grad_(True)
    f = mur[:, None] + torch.sqrt(2.0 * vr)[:, None] * xs[None, :]
    G = fm.flow(f, prog, thr)
    ell = (wn[None, :] * (-0.5 * lvn - 0.5 * torch.exp(-lvn) * (Y[:, None] - G) ** 2)).sum()
    gm, gv, gt = torch.autograd.grad(ell, (mur, vr, thr))
    assert torch.isfinite(gt).all()
    errs = (rel_err(res["g_mu"].cpu(), gm), rel_err(res["g_v"].cpu(), gv), rel_err(res["g_theta"].cpu(), gt))
    print("ell_flow %s N=%d S=%d: g_mu %.2e g_v %.2e g_theta %.2e" % ((name, N, S) + errs))
    assert max(errs) < 1e-10, errs


# ---- 3. the fused step ----
TINY = ["shapes_tiny_sinh2", "shapes_tiny_ncdf1", "shapes_tiny_tukeyr1", "shapes_tiny_tukeyl1", "shapes_tiny_salexp1"]
MED = ["shapes_med_sinh2", "shapes_med_tukeyr1"]
PLANS = ("auto", "K16", "K", "R4NW4", "R4NW8")
STEP_CASES = [(n, p) for n in TINY + MED for p in PLANS] + [("shapes_bigm_sinh1", "auto")]      # (general-M: no row plans)


def _plan(plan):
    from tgp.pytorch_amd import lib as L
    return {"auto": 0, "K16": L.PLAN_ROWS_K16, "K": L.PLAN_ROWS_K, "R4NW4": L.PLAN_ROWS4_NW4, "R4NW8": L.PLAN_ROWS4_NW8}[plan]


@pytest.mark.parametrize("name,plan", STEP_CASES)
def test_elbo_step_matches_reference_under_every_row_plan(name, plan):
    g = load_golden(name)
    out, grads = tgk._run_step(g, _plan(plan))
    tgk._compare(out, grads, g)


@pytest.fixture(scope="module")
def softplus_case():
    """SALSoftplus(1) at the tiny shape: the reference has no softplus in instance_flow, so the patched oracle is the truth."""
    from oracle import tgp_oracle as orc
    from tgp.pytorch_amd import flows as Gn
    from tgp.pytorch_amd.flow import compile_flow, instance_flow
    prob = orc.synthetic_problem(64, 3, 8, seed=4, flow=None, S=8)
    spec, theta_list, _ = compile_flow(instance_flow(Gn.SALSoftplus(1)))
    gen = torch.Generator().manual_seed(1004)
    theta = torch.stack([p.detach().reshape(()) for p in theta_list]) + 0.3 * torch.randn(len(theta_list), generator=gen, dtype=F64)
    theta[3] += 3.0          # the affine block's offset: softplus(.) well above the noise of the quantile test below
    prob["program"] = [tuple(b) for b in spec.blocks]
    prob["params"]["theta"] = theta
    with fm.patched():
        (elbo, ell, kld), og = orc.elbo_and_grads(prob["X"], prob["Y"], prob["params"], prob["N_total"], prob["program"],
                                                  prob["xs"], prob["ws"])
    g = dict(prob, ELBO=elbo, ELL=ell, KLD=kld, g_Z=og["Z"], g_raw_lengthscale=og["raw_lengthscale"],
             g_raw_outputscale=og["raw_outputscale"], g_m=og["m"], g_Lam=og["Lam"], g_log_var_noise=og["log_var_noise"],
             g_theta=og["theta"])
    return g


@pytest.mark.parametrize("plan", PLANS)
def test_salsoftplus_step_matches_the_patched_oracle(softplus_case, plan):
    assert softplus_case["program"][-1][0] == fm.SOFTPLUS
    out, grads = tgk._run_step(softplus_case, _plan(plan))
    tgk._compare(out, grads, softplus_case)


def test_two_identical_steps_are_bit_identical():
    g = load_golden("shapes_med_tukeyr1")
    a, ga = tgk._run_step(g)
    b, gb = tgk._run_step(g)
    assert torch.equal(a, b) and all(torch.equal(ga[k], gb[k]) for k in ga)


# ---- 4. prediction and quantiles ----
def test_quantiles_and_cdf_are_inverse_to_each_other():
    from tgp.pytorch_amd import ops
    g = load_golden("shapes_med_tukeyr1")
    p = g["params"]
    mu, v, lvn, th = g["mu"].to(DEV), g["v"].to(DEV), p["log_var_noise"].to(DEV), p["theta"].to(DEV)
    spec, S = _spec(g["program"], th.numel()), g["xs"].numel()
    probs = [0.025, 0.5, 0.975]
    t = ops.predict_quantiles(mu, v, lvn, probs, spec, th, S)
    assert t.shape == (3, mu.numel()) and torch.isfinite(t).all() and (t[0] < t[1]).all() and (t[1] < t[2]).all()
    for q, pr in enumerate(probs):
        cdf, sf = ops.predict_cdf(mu, v, lvn, t[q], spec, th, S)
        assert float((cdf - pr).abs().max()) < 1e-10 and float((sf - (1.0 - pr)).abs().max()) < 1e-10


def test_a_softplus_head_gives_positive_quantiles(softplus_case):
    from tgp.pytorch_amd import ops
    p = softplus_case["params"]
    X, th = softplus_case["X"].to(DEV), p["theta"].to(DEV)
    mu, v = ops.qf_moments(X, p["Z"].to(DEV), p["raw_lengthscale"].to(DEV), p["raw_outputscale"].to(DEV), p["m"].to(DEV),
                           p["Lam"].to(DEV))
    lvn = torch.tensor([-9.0], dtype=F64, device=DEV)            # noise sd 0.011 around G(f) > 0
    xs, _ = ops.gauss_hermite(8, DEV)
    Gmin = fm.flow((mu[:, None] + torch.sqrt(2.0 * v)[:, None] * xs[None, :]).cpu(), softplus_case["program"], th.cpu()).min()
    assert float(Gmin) > 0.1                                      # (the set-up: every mixture component 9 noise sds above 0)
    t = ops.predict_quantiles(mu, v, lvn, [0.025, 0.5, 0.975], _spec(softplus_case["program"], th.numel()), th, 8)
    m1, _, _ = ops.predict(mu, v, lvn, _spec(softplus_case["program"], th.numel()), th, 8)
    assert (m1 > 0).all() and (t > 0).all()


# ---- 5. the warped likelihood ----
WARPS = {"sinh": ("sinh", False), "sinh_rf0": ("sinh_rf0", True), "tukey_left": ("tukey_left", True),
         "sinh_tukey": (None, True)}
PROG_ST = [(fm.SINH, 0, 0, fm.RESTRICT), (fm.AFFINE, 0, 4, 0), (fm.TUKEY, 0, 6, fm.RESTRICT)]
THETA_ST = [0.2, 0.8, -0.1, 1.4, 0.9, 0.1, -1.5, -2.5]


def _warp(name):
    if name == "sinh_tukey":
        return PROG_ST, torch.tensor(THETA_ST, dtype=F64)
    return fm.PROGRAMS[name], _theta(name)


@pytest.mark.parametrize("name", list(WARPS))
def test_flow_inverse_returns_the_point(name):
    from tgp.pytorch_amd import ops
    prog, th = _warp(name)
    g = torch.Generator().manual_seed(11)
    y = (1.5 * torch.randn(2, 300, generator=g, dtype=F64)).clamp(-4.0, 4.0)
    t = fm.flow(y, prog, th)
    x, status = ops.flow_inverse(t.to(DEV), _spec(prog, th.numel()), th.to(DEV))
    assert int(status[0]) == 0
    assert float((x.cpu() - y).abs().max()) < 1e-10, float((x.cpu() - y).abs().max())


@pytest.mark.parametrize("name", list(WARPS))
def test_ell_warp_value_and_gradients_match_autograd(name):
    from tgp.pytorch_amd import ops
    prog, th = _warp(name)
    N = 300
    g = torch.Generator().manual_seed(5)
    Y = (1.2 * torch.randn(N, generator=g, dtype=F64)).clamp(-3.5, 3.5)
    mu = 0.5 * torch.randn(N, generator=g, dtype=F64)
    v = 0.05 + 0.1 * torch.rand(N, generator=g, dtype=F64)
    lvn = torch.tensor([-0.7], dtype=F64)
    res = ops.ell_warp(Y.to(DEV), mu.to(DEV), v.to(DEV), lvn.to(DEV), _spec(prog, th.numel()), th.to(DEV))
    from oracle import tgp_oracle as orc
    thr, mur, vr = th.clone().requires_grad_(True), mu.clone().requires_grad_(True), v.clone().requires_grad_(True)
    yr = Y.clone().requires_grad_(True)
    t = fm.flow(yr, prog, thr)
    dt, = torch.autograd.grad(t.sum(), yr, create_graph=True)
    # the Gaussian closed form at t with the reference's float32-rounded pi, plus sum log T'(y)
    ell = (-0.5 * orc.LOG_2PI_REF - 0.5 * lvn - 0.5 * torch.exp(-lvn) * ((t - mur) ** 2 + vr)).sum() + torch.log(dt).sum()
    gm, gv, gt = torch.autograd.grad(ell, (mur, vr, thr))
    assert rel_err(res["ell"].cpu(), ell.detach()) < 1e-12
    assert rel_err(res["logdet"].cpu(), torch.log(dt).sum().detach()) < 1e-12
    assert rel_err(res["g_mu"].cpu(), gm) < 1e-10 and rel_err(res["g_v"].cpu(), gv) < 1e-10
    assert rel_err(res["g_theta"].cpu(), gt) < 1e-10, rel_err(res["g_theta"].cpu(), gt)


def test_a_normal_cdf_warp_is_refused():
    from tgp.pytorch_amd import lib as L
    from tgp.pytorch_amd import ops
    z = torch.zeros(8, dtype=F64, device=DEV)
    th = torch.tensor([0.0, 1.0, 0.0, 1.0], dtype=F64, device=DEV)
    for prog, P in (([(fm.NORMCDF, 0, 0, 0)], 4), ([(fm.EXP, 0, 0, 0)], 0), ([(fm.SOFTPLUS, 0, 0, 0)], 0)):
        with pytest.raises(L.TgpError, match="code %d .*tgp_ell_warp_f64.*real line" % L.E_UNSUPPORTED):
            ops.ell_warp(z, z, z + 1.0, z[:1], _spec(prog, P), th[:P] if P else None)
        with pytest.raises(L.TgpError, match="code %d .*tgp_flow_inverse_f64" % L.E_UNSUPPORTED):
            ops.flow_inverse(z, _spec(prog, P), th[:P] if P else None)
    assert "TGP_FLOW_SOFTPLUS" in L.load().tgp_last_error().decode()


# ---- 6. trainer, initialiser, CLI ----
def _specs_sinh2():
    from tgp.pytorch_amd import flows as Gn
    return Gn.SinhL(2)


@pytest.mark.parametrize("resident", [True, False])
def test_trainer_first_steps_match_reference(resident):
    from tgp.pytorch_amd import config as cg
    from tgp.pytorch_amd.data import DeviceLoader
    from tgp.pytorch_amd.flow import compile_flow
    from tgp.pytorch_amd.trainers import Trainer_SP_regression
    g = load_golden("shapes_adam5_sinh2")
    model = tgk.build_model(g, _specs_sinh2())
    loader = DeviceLoader(g["X"], g["Y"], 10000, shuffle=False, device=DEV)
    tr = Trainer_SP_regression(model, [loader, None, None], 1e20, False, False, torch.ones(1, device=DEV), -1, 100, True)
    cg.use_step_engine = resident
    try:
        tr.train(epochs=g["history"].shape[0], lr_ALL=0.01, opt="adam", keep_parameter_groups=True)
    finally:
        cg.use_step_engine = True
    assert (tr._engine is not None) == resident
    hist = torch.tensor([[-l, e, k] for l, e, k in zip(tr.loss_arr, tr.ELL_arr, tr.KLD_arr)], dtype=F64)
    assert rel_err(hist, g["history"]) < 1e-8
    th = torch.stack([q.detach().reshape(()) for q in compile_flow(model.G_matrix[0])[1]]).cpu()
    assert rel_err(th, g["final_theta"]) < 1e-8


@pytest.mark.parametrize("gen", ["SinhL", "TukeyL"])
def test_flow_initialiser_reduces_the_mse(gen):
    from tgp.pytorch_amd import flows as Gn
    from tgp.pytorch_amd.flow import instance_flow
    from tgp.pytorch_amd.initializers import find_forward_params

    def fn():      # the generators' own near-identity start: a random start of two sinh or Tukey blocks overflows at |x| = 3
        return instance_flow(getattr(Gn, gen)(2))
    x = np.linspace(-3, 3, 500)
    y = np.sinh(0.5 * x) + 0.3 * x
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        fitted, curve = find_forward_params(x.copy(), y, fn, num_restarts=1, num_epochs=200)
    assert np.isfinite(curve[-1]) and curve[-1] < 0.5 * curve[0]


def test_cli_runs_with_a_tukey_flow():
    # (--train_test_seed_split is a required argument of main.py)
    cmd = [sys.executable, "-m", "tgp.pytorch_amd.main", "--model", "TGP", "--dataset", "synthetic_power", "--flow_arch",
           "TukeyL", "--num_blocks", "1", "--num_inducing", "20", "--epochs", "5", "--train_test_seed_split", "1"]
    r = subprocess.run(["timeout", "-k", "10", "300"] + cmd, cwd=REPO, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "Test Negative LOGL" in r.stdout
    nums = [float(x) for line in r.stdout.splitlines() if "Test" in line
            for x in __import__("re").findall(r"[-+]?\d+\.\d+(?:[eE][-+]?\d+)?", line)]
    assert nums and all(np.isfinite(nums))
