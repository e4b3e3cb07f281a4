"""GPU (-m gpu): the arcsinh / Box-Cox / inverse Box-Cox flow kinds (TGP_FLOW_ARCSINH, _BOXCOX, _INV_BOXCOX) through every
layer -- the flow kernels against torch autograd of the formulas restated below, the quadrature likelihood's gradients,
the fused ELBO step under every row plan and on the general-M path against the reference's fixtures
(tools/gen_golden_flows.py), the trainer (eager and resident graph engine), the evaluation path, the flow initialiser,
the refusal of per-row parameters, and the CLI."""
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

from conftest import REPO, load_golden, rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL_VAL, TOL_GRAD = 1e-9, 1e-7


@pytest.fixture(autouse=True)
def _f64():
    from tgp.pytorch_amd import config as cg
    old = torch.get_default_dtype()
    cg.set_maximum_precission()
    cg.device = DEV
    yield
    torch.set_default_dtype(old)


# ---- the formulas (models/flow.py of the reference), differentiated by torch autograd ----
def _asinh_ref(x):
    return torch.log(x + (x ** 2 + 1) ** 0.5)


def ref_flow(f, program, theta):
    for kind, K, poff, flags in program:
        R, A = flags & 1, flags & 2
        t = [theta[poff + j] for j in range(4 if kind == 3 else (1 if kind >= 4 else 2))]
        if kind == 0:
            a = Fn.softplus(t[0]) if R else t[0]
            g = a * f + t[1]
        elif kind == 1:
            b = Fn.softplus(t[1]) if R else t[1]
            g = torch.sinh(b * _asinh_ref(f) - t[0])
        elif kind == 3:
            b, d = (Fn.softplus(t[1]), Fn.softplus(t[3])) if R else (t[1], t[3])
            g = t[0] + b * _asinh_ref((f - t[2]) / d)
        else:
            lam = t[0] + 1e-11 if float(t[0]) == 0.0 else t[0]
            if kind == 4:
                g = (torch.sign(f) * torch.pow(torch.sign(f) * f, lam) - 1) / lam
            else:
                w = lam * f + 1
                g = torch.sign(w) * torch.pow(torch.sign(w) * w, 1. / lam)
        if kind != 0 and A:
            g = g + f
        f = g
    return f


R_, A_ = 1, 2
PROGRAMS = {
    "arcsinh": [(3, 0, 0, 0)],
    "arcsinh_r": [(3, 0, 0, R_)],
    "arcsinh_rf0": [(3, 0, 0, R_ | A_)],
    "boxcox": [(4, 0, 0, 0)],
    "boxcox_f0": [(4, 0, 0, A_)],
    "invboxcox": [(5, 0, 0, 0)],
    "invboxcox_f0": [(5, 0, 0, A_)],
    "chain": [(1, 0, 0, R_), (0, 0, 2, 0), (4, 0, 4, A_), (0, 0, 5, R_), (3, 0, 7, R_ | A_), (5, 0, 11, 0), (0, 0, 12, 0)],
}
THETA = {
    "arcsinh": [0.3, 1.2, -0.4, 0.8], "arcsinh_r": [0.3, 0.2, -0.4, 0.5], "arcsinh_rf0": [-0.2, 0.4, 0.3, -0.1],
    "boxcox": [1.4], "boxcox_f0": [0.7], "invboxcox": [0.6], "invboxcox_f0": [1.8],
    "chain": [0.1, 0.9, 1.1, 0.2, 0.8, 0.5, 0.1, 0.2, 0.6, -0.3, 0.4, 1.3, 0.9, -0.1],
}


def _f_values(name):
    g = torch.Generator().manual_seed(7)
    f = 2.0 * torch.randn(3, 700, generator=g, dtype=torch.float64)
    f = torch.where(f.abs() < 1e-3, f + 0.01, f)                          # away from |f| < 1e-6
    if PROGRAMS[name][0][0] == 5:                                         # and from lam f + 1 = 0
        lam = THETA[name][0]
        f = torch.where((lam * f + 1).abs() < 1e-2, f + 0.05, f)
    return f


def _spec(prog, P):
    from tgp.pytorch_amd import ops
    return ops.FlowSpec(prog, P, 0, DEV)


@pytest.mark.parametrize("name", list(PROGRAMS))
def test_flow_eval_and_logdet_match_autograd(name):
    from tgp.pytorch_amd import ops
    prog, th = PROGRAMS[name], torch.tensor(THETA[name], dtype=torch.float64)
    f = _f_values(name)
    if name == "chain":       # keep every stage's input in the domain where the chain is smooth (no w = 0 crossing)
        f = f.clamp(-1.5, 1.5)
    fr = f.clone().requires_grad_(True)
    G = ref_flow(fr, prog, th)
    dG, = torch.autograd.grad(G.sum(), fr)
    assert torch.isfinite(dG).all()
    res = ops.flow_eval(f.to(DEV), _spec(prog, th.numel()), th.to(DEV))
    assert rel_err(res["G"].cpu(), G.detach()) < 1e-12
    assert rel_err(res["dG"].cpu(), dG) < 1e-12
    assert rel_err(res["logdG"].cpu(), torch.log(dG.abs())) < 1e-12
    s, _ = ops.flow_logdet(f.to(DEV), _spec(prog, th.numel()), th.to(DEV))
    assert rel_err(s.cpu(), torch.log(dG.abs()).sum()) < 1e-12


def test_boxcox_lambda_zero_is_taken_as_1e_minus_11():
    from tgp.pytorch_amd import ops
    f = torch.linspace(0.5, 2.0, 64, dtype=torch.float64)
    th = torch.zeros(1, dtype=torch.float64)
    res = ops.flow_eval(f.to(DEV), _spec([(4, 0, 0, 0)], 1), th.to(DEV), want=("G",))
    assert torch.isfinite(res["G"]).all()
    assert rel_err(res["G"].cpu(), torch.log(f)) < 1e-4          # (|f|^1e-11 - 1) / 1e-11 ~ log f


@pytest.mark.parametrize("name", ["arcsinh_r", "boxcox_f0", "invboxcox", "chain"])
# the 32-, 16- and 4-lanes-per-row variants of k_ell_quad; then four nodes in flight per lane at 32 and at 16 lanes per row
@pytest.mark.parametrize("N,S", [(300, 16), (5000, 16), (20000, 16), (300, 80), (4000, 40)],
                         ids=["300", "5000", "20000", "300-S80", "4000-S40"])
def test_ell_flow_gradients_match_autograd(name, N, S):
    from tgp.pytorch_amd import ops
    prog, th = PROGRAMS[name], torch.tensor(THETA[name], dtype=torch.float64)
    g = torch.Generator().manual_seed(N)
    mu = 0.5 * torch.randn(N, generator=g, dtype=torch.float64)
    v = 0.05 + 0.1 * torch.rand(N, generator=g, dtype=torch.float64)
    Y = torch.randn(N, generator=g, dtype=torch.float64)
    lvn = torch.tensor([-1.2], dtype=torch.float64)
    res = ops.ell_flow(Y.to(DEV), mu.to(DEV), v.to(DEV), lvn.to(DEV), _spec(prog, th.numel()), th.to(DEV), S)
    xs, wn = ops.gauss_hermite(S, "cpu")
    mur, vr, thr = mu.clone().requires_grad_(True), v.clone().requires_grad_(True), th.clone().requires_grad_(True)
    f = mur[:, None] + torch.sqrt(2.0 * vr)[:, None] * xs[None, :]
    G = ref_flow(f, prog, thr)
    ell = (wn[None, :] * (-0.5 * lvn - 0.5 * torch.exp(-lvn) * (Y[:, None] - G) ** 2)).sum()
    gm, gv, gt = torch.autograd.grad(ell, (mur, vr, thr))
    assert rel_err(res["g_mu"].cpu(), gm) < 1e-10
    assert rel_err(res["g_v"].cpu(), gv) < 1e-10
    assert rel_err(res["g_theta"].cpu(), gt) < 1e-10


def test_per_row_arcsinh_is_refused():
    from tgp.pytorch_amd import lib as L
    from tgp.pytorch_amd import ops
    f = torch.zeros(1, 8, dtype=torch.float64, device=DEV)
    rowp = torch.ones(8, 4, dtype=torch.float64, device=DEV)
    spec = ops.FlowSpec([(3, 0, 0, L.FLAG_PER_ROW)], 0, 4, DEV)
    with pytest.raises(L.TgpError):
        ops.flow_eval(f, spec, None, rowp)
    G = torch.full((8,), 123.0, dtype=torch.float64, device=DEV)
    lib = L.load()
    md, keep = ops._flow_model(8, 1, spec, None, torch.zeros(1, dtype=torch.float64, device=DEV), f.device)
    rc = lib.tgp_flow_eval_f64(md, L.ptr(f), 1, 8, L.ptr(rowp), L.ptr(G), None, None, L.stream_ptr())
    torch.cuda.synchronize()
    assert rc < 0 and float(G.min()) == float(G.max()) == 123.0       # refused before any launch


# ---- the fused step against the reference's fixtures ----
STEP_FIXTURES = ["flows_tiny_arcsl2", "flows_tiny_bcl1", "flows_tiny_invbcl1", "flows_tiny_sal_bcl1",
                 "flows_tiny_invbcl_al1", "flows_tiny_sal_al2f0", "flows_med_arcsl2", "flows_med_sal_bcl1",
                 "flows_med_invbcl_al1", "flows_med_bcl1lam5", "flows_bigm_sal_bcl1", "flows_bigm_invbcl_al1",
                 "flows_power_arcsl1", "flows_power_bcl_al1"]


def _run_step(g, plan=0):
    from tgp.pytorch_amd import ops
    p = {k: v.to(DEV) for k, v in g["params"].items()}
    flow = ops.FlowSpec(g["program"], p["theta"].numel(), 0, DEV)
    out, grads, status, _ = ops.elbo_step(g["X"].to(DEV), g["Y"].to(DEV), p["Z"], p["raw_lengthscale"], p["raw_outputscale"],
                                          p["m"], p["Lam"], p["log_var_noise"], float(g["N_total"]), flow=flow,
                                          theta=p["theta"], S=g["xs"].numel(), plan=plan)
    torch.cuda.synchronize()
    assert int(status[0]) == 0 and int(status[1]) == 0
    return out.cpu(), {k: t.cpu() for k, t in grads.items()}


def _compare(out, grads, g):
    assert rel_err(out[0], g["ELBO"]) < TOL_VAL
    assert rel_err(out[1], g["ELL"]) < TOL_VAL
    assert rel_err(out[2], g["KLD"]) < TOL_VAL
    names = {"Z": "g_Z", "raw_ls": "g_raw_lengthscale", "raw_os": "g_raw_outputscale", "m": "g_m", "Lam": "g_Lam",
             "lvn": "g_log_var_noise", "theta": "g_theta"}
    for k, t in grads.items():
        if k in names:
            assert rel_err(t, g[names[k]]) < TOL_GRAD, (k, rel_err(t, g[names[k]]))


# (the general-M fixtures (M > 128) have no row plans; k_rows4 does not take a Power-size launch)
STEP_CASES = [(name, plan) for name in STEP_FIXTURES for plan in ("auto", "K16", "K", "R4NW4", "R4NW8")
              if plan == "auto" or not (name.startswith("flows_bigm") or (name.startswith("flows_power") and plan.startswith("R4")))]


@pytest.mark.parametrize("name,plan", STEP_CASES)
def test_elbo_step_matches_reference_under_every_row_plan(name, plan):
    from tgp.pytorch_amd import lib as L
    g = load_golden(name)
    sel = {"auto": 0, "K16": L.PLAN_ROWS_K16, "K": L.PLAN_ROWS_K, "R4NW4": L.PLAN_ROWS4_NW4, "R4NW8": L.PLAN_ROWS4_NW8}[plan]
    out, grads = _run_step(g, sel)
    _compare(out, grads, g)


def test_two_identical_steps_are_bit_identical():
    g = load_golden("flows_power_bcl_al1")
    a, ga = _run_step(g)
    b, gb = _run_step(g)
    assert torch.equal(a, b) and all(torch.equal(ga[k], gb[k]) for k in ga)


def build_model(g, specs):
    from tgp.pytorch_amd.flow import compile_flow
    from tgp.pytorch_amd.kernels import instance_kernel
    from tgp.pytorch_amd.likelihoods import GaussianNonLinearMean
    from tgp.pytorch_amd.models import sparse_MF_SP
    p = g["params"]
    N, D = g["X"].shape
    M = p["m"].numel()
    K = instance_kernel("scale_rbf", ard_num_dim=D, num_multioutput=1, kernel_is_shared=False,
                        init_params={"length_scale": 2.0, "kernel_scale": 2.0, "noisy_variance": 1e-6})
    ip = {"variational_distribution": {"variance_scale": 1e-5, "mean_scale": 0.0}}
    lik = GaussianNonLinearMean(1, 0.05, False, quadrature_points=g["xs"].numel())
    model = sparse_MF_SP(["zero", K], g["X"], p["Z"].clone(), N, lik, 1, True, False, False, False, False, [specs],
                         "single", 0.0, init_params=ip)
    with torch.no_grad():
        model.Z.data = p["Z"].reshape(1, M, D).clone()
        model.q_U.variational_mean.data = p["m"].reshape(1, M).clone()
        model.q_U.chol_variational_covar.data = p["Lam"].reshape(1, M, M).clone()
        model.covariance_function.raw_outputscale.data = p["raw_outputscale"].reshape(1).clone()
        model.covariance_function.base_kernel.raw_lengthscale.data = p["raw_lengthscale"].reshape(1, 1, D).clone()
        model.likelihood.log_var_noise.data = p["log_var_noise"].reshape(1, 1).clone()
        spec, theta_list, _ = compile_flow(model.G_matrix[0])
        assert [tuple(b) for b in spec.blocks] == [tuple(b) for b in g["program"]]
        for prm, val in zip(theta_list, p["theta"]):
            prm.data = val.clone().reshape(prm.shape)
    return model.to(DEV)


def _specs(name):
    """the specs tools/gen_golden_flows.py built the fixture's model from (this package's generators, same seeds)"""
    from tgp.pytorch_amd import flows as G
    gens = {"arcsl2": (11, lambda: G.ArcSL(2)), "bcl1": (12, lambda: G.BoxCoxL(1)), "invbcl1": (13, lambda: G.InverseBoxCoxL(1)),
            "sal_bcl1": (14, lambda: G.build_chain("SAL_BCL", 1, constraint=None)),
            "invbcl_al1": (15, lambda: G.build_chain("InvBCL_AL", 1, constraint=None)),
            "sal_al2f0": (16, lambda: [s for _ in range(2) for s in G.SAL(1, add_f0=True) + G.ArcSL(1, add_f0=True)]),
            "bcl1lam5": (17, lambda: G.BoxCoxL(1)), "bcl_al1": (18, lambda: G.build_chain("BCL_AL", 1, constraint=None)),
            "arcsl1": (19, lambda: G.ArcSL(1, set_res=True))}
    seed, fn = gens[name]
    np.random.seed(seed)
    return fn()


@pytest.mark.parametrize("name", ["flows_tiny_sal_al2f0", "flows_med_invbcl_al1", "flows_med_bcl1lam5"])
def test_model_classes_match_reference(name):
    g = load_golden(name)
    model = build_model(g, _specs(name.split("_", 2)[2]))
    model.set_is_training(True)
    elbo, ell, kld = model.ELBO(g["X"].to(DEV), g["Y"].to(DEV))
    (-elbo).backward()
    assert rel_err(elbo.detach().cpu(), g["ELBO"]) < TOL_VAL
    from tgp.pytorch_amd.flow import compile_flow
    gt = torch.stack([-q.grad.reshape(()) for q in compile_flow(model.G_matrix[0])[1]]).cpu()
    assert rel_err(gt, g["g_theta"]) < TOL_GRAD


@pytest.mark.parametrize("name", ["flows_tiny_arcsl2", "flows_tiny_invbcl1", "flows_med_sal_bcl1", "flows_power_arcsl1",
                                  "flows_power_bcl_al1"])
def test_evaluation_path_matches_reference(name):
    g = load_golden(name)
    model = build_model(g, _specs(name.split("_", 2)[2]))
    model.set_is_training(False)
    if "X_te" in g:
        X, Y, Y_std = g["X_te"], g["Y_te"], g["Y_std"]
    else:
        X, Y, Y_std = g["X"], g["Y"], g["Y_std"]
    logp, (m1, m2) = model.test_log_likelihood(X.to(DEV), Y.to(DEV), return_moments=True, Y_std=Y_std.to(DEV))
    assert rel_err(logp.cpu(), g["test_logp_sum"]) < 1e-9
    assert rel_err(m1.cpu().reshape(-1), g["pred_m1"]) < 1e-9
    assert rel_err(m2.cpu().reshape(-1), g["pred_m2"]) < 1e-8


@pytest.mark.parametrize("resident", [True, False])
@pytest.mark.parametrize("name", ["flows_adam5_arcsl2", "flows_adam5_sal_bcl1"])
def test_trainer_first_steps_match_reference(name, resident):
    from tgp.pytorch_amd import config as cg
    from tgp.pytorch_amd.data import DeviceLoader
    from tgp.pytorch_amd.trainers import Trainer_SP_regression
    g = load_golden(name)
    model = build_model(g, _specs(name.split("_", 2)[2]))
    loader = DeviceLoader(g["X"], g["Y"], 10000, shuffle=False, device=DEV)
    tr = Trainer_SP_regression(model, [loader, None, None], 1e20, False, False, torch.ones(1, device=DEV), -1, 100, True)
    cg.use_step_engine = resident
    try:
        tr.train(epochs=g["history"].shape[0], lr_ALL=0.01, opt="adam", keep_parameter_groups=True)
    finally:
        cg.use_step_engine = True
    assert (tr._engine is not None) == resident
    hist = torch.tensor([[-l, e, k] for l, e, k in zip(tr.loss_arr, tr.ELL_arr, tr.KLD_arr)], dtype=torch.float64)
    assert rel_err(hist, g["history"]) < 1e-8
    from tgp.pytorch_amd.flow import compile_flow
    th = torch.stack([q.detach().reshape(()) for q in compile_flow(model.G_matrix[0])[1]]).cpu()
    assert rel_err(th, g["final_theta"]) < 1e-8


@pytest.mark.parametrize("graph", [False, True])
def test_engine_adam_history_at_power_size(graph):
    from tgp.pytorch_amd.engine import ElboEngine
    g = load_golden("flows_power_bcl_al1")
    eng = ElboEngine(g["X"], g["Y"], g["params"], float(g["N_total"]), flow_blocks=g["program"], S=g["xs"].numel(),
                     device=DEV)
    if graph:
        eng.capture()
    hist = []
    for _ in range(g["history"].shape[0]):
        (eng.replay if graph else eng.step)()
        hist.append(list(eng.scalars()))
    eng.check_status()
    assert rel_err(torch.tensor(hist, dtype=torch.float64), g["history"]) < 1e-8
    assert rel_err(eng.fp.view("theta").cpu(), g["final_theta"]) < 1e-8


@pytest.mark.parametrize("gen", ["ArcSL", "BoxCoxL"])
def test_flow_initialiser_reduces_the_mse(gen):
    from tgp.pytorch_amd import flows as G
    from tgp.pytorch_amd.flow import instance_flow
    from tgp.pytorch_amd.initializers import find_forward_params

    def fn():
        return instance_flow(getattr(G, gen)(2, init_random=True))
    x = np.linspace(-3, 3, 500)
    y = np.sinh(0.5 * x) + 0.3 * x
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        fitted, curve = find_forward_params(x.copy() + (3.5 if gen == "BoxCoxL" else 0.0), y, fn, num_restarts=1,
                                            num_epochs=200)
    assert np.isfinite(curve[-1]) and curve[-1] < 0.5 * curve[0]


def test_cli_runs_with_a_new_flow_architecture():
    cmd = [sys.executable, "-m", "tgp.pytorch_amd.main", "--model", "TGP", "--dataset", "synthetic_power", "--flow_arch",
           "SAL_AL", "--num_blocks", "2", "--train_test_seed_split", "1", "--num_inducing", "100", "--epochs", "50"]
    r = subprocess.run(["timeout", "-k", "10", "300"] + cmd, cwd=REPO, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "Test Negative LOGL" in r.stdout
