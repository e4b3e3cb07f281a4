"""GPU (-m gpu): the Bernoulli (probit) likelihood (TGP_LIK_BERNOULLI) through every layer -- the stand-alone ELL kernel
and its gradients against torch autograd (tests/test_bernoulli_host.py restates the formula), the saturated tails, the
training step (general-M path at every M) and the model classes against the reference's fixtures
(tests/golden/bern_*.npz, tools/gen_golden_bernoulli.py), the first Adam steps of the trainer, the evaluation path, the
fully Bayesian prediction, a short training run on synthetic_banknote and the CLI."""
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import REPO, load_golden, rel_err
from test_bernoulli_host import ell_torch, pred_torch

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


# ---- the stand-alone ELL kernel against autograd ---------------------------------------------------------------------
CASES = ["empty", "bern_med_sal_invbcl1", "bern_med_bcl_al2", "bern_med_arcsl2", "idsal"]


# 32, 16 and 4 lanes per row; then four nodes in flight per lane at 32 and at 16 lanes per row
@pytest.mark.parametrize("N,S", [(300, 32), (4000, 32), (13000, 32), (300, 80), (4000, 40)],
                         ids=["300", "4000", "13000", "300-S80", "4000-S40"])
@pytest.mark.parametrize("case", CASES)
def test_ell_kernel_matches_autograd(case, N, S):
    from tgp.pytorch_amd import ops
    g = torch.Generator().manual_seed(N)
    mu = 1.2 * torch.randn(N, generator=g, dtype=F64)
    v = 0.3 * torch.rand(N, generator=g, dtype=F64)
    v[:7] = -1e-12                                      # clamped to 0 (Bernoulli.py: gauss_cov[gauss_cov < 0] = 0)
    Y = (torch.rand(N, generator=g, dtype=F64) < 0.5).to(F64)
    Y[-5:] = torch.tensor([0.3, 0.5, 0.9, 0.0, 1.0])      # soft labels behave as in BCELoss
    xs, ws = (torch.tensor(a) for a in np.polynomial.hermite.hermgauss(S))
    theta = rowp = None
    program, P, RP = [], 0, 0
    if case == "idsal":
        program, RP = [(1, 0, 0, 4)], 2
        rowp = torch.stack([0.1 * torch.randn(N, generator=g, dtype=F64), 1.0 + 0.1 * torch.randn(N, generator=g, dtype=F64)], 1)
    elif case != "empty":
        z = load_golden(case)
        program, theta = z["program"], z["p_theta"].clone()
        P = theta.numel()
    scale = 3.5
    res = ops.ell_bernoulli(Y.to(DEV), mu.to(DEV), v.to(DEV), _spec(program, P, RP), None if theta is None else theta.to(DEV),
                            S, None if rowp is None else rowp.to(DEV).contiguous(), scale=scale)
    wrt = [mu.clone().requires_grad_(True), v.clone().requires_grad_(True)]
    th = theta.clone().requires_grad_(True) if theta is not None else None
    rp = rowp.clone().requires_grad_(True) if rowp is not None else None
    ell = ell_torch(Y, wrt[0], wrt[1], program, th, xs, ws, rp, scale)
    extra = [t for t in (th, rp) if t is not None]
    grads = torch.autograd.grad(ell, wrt + extra)
    assert rel_err(res["ell"].cpu(), ell.detach()) < TOL_VAL
    assert rel_err(res["g_mu"].cpu(), grads[0]) < TOL_GRAD
    gv = grads[1].clone()
    gv[:7] = 0.0                                        # v <= 0: the adjoint of v is 0
    assert rel_err(res["g_v"].cpu(), gv) < TOL_GRAD
    assert torch.all(res["g_v"][:7].cpu() == 0)
    if th is not None:
        assert rel_err(res["g_theta"].cpu(), grads[2]) < TOL_GRAD
    if rp is not None:
        assert rel_err(res["g_rowp"].cpu(), grads[-1]) < TOL_GRAD


def test_saturated_tails_are_exact():
    """mu = +-40: log Phi and the Mills ratio stay finite and exact (the reference's BCELoss stops at -100)."""
    from tgp.pytorch_amd import lib as L
    from tgp.pytorch_amd import ops
    mu = torch.tensor([40.0, -40.0, 40.0, -40.0], dtype=F64)
    Y = torch.tensor([0.0, 1.0, 1.0, 0.0], dtype=F64)
    v = torch.tensor([0.0, 0.0, 1e-3, 1e-3], dtype=F64)
    S = 16
    xs, ws = (torch.tensor(a) for a in np.polynomial.hermite.hermgauss(S))
    res = ops.ell_bernoulli(Y.to(DEV), mu.to(DEV), v.to(DEV), _spec([], 0), None, S)
    m, vv = mu.clone().requires_grad_(True), v.clone().requires_grad_(True)
    ell = ell_torch(Y, m, vv, [], None, xs, ws)
    gm, gv = torch.autograd.grad(ell, [m, vv])
    assert torch.isfinite(res["ell"]).item() and float(res["ell"]) < -1600
    assert rel_err(res["ell"].cpu(), ell.detach()) < TOL_VAL
    assert rel_err(res["g_mu"].cpu(), gm) < TOL_GRAD
    # the Mills ratio: d/dmu log Phi(-mu) at mu = 40 is -phi(40)/Phi(-40) ~ -40.025
    assert abs(float(res["g_mu"][0]) + 40.02492) < 1e-4
    assert rel_err(res["g_v"][2:].cpu(), gv[2:]) < TOL_GRAD
    lvn = torch.zeros(1, dtype=F64, device=DEV)
    P, m2, lp = ops.predict(mu.to(DEV), v.to(DEV), lvn, _spec([], 0), None, S, Y=Y.to(DEV), lik=L.LIK_BERNOULLI)
    lp_ref = torch.where(Y > 0.5, torch.special.log_ndtr(mu / torch.sqrt(1 + v)), torch.special.log_ndtr(-mu / torch.sqrt(1 + v)))
    assert torch.isfinite(lp).all() and rel_err(lp.cpu(), lp_ref) < TOL_VAL


# ---- the training step and the model classes against the reference -----------------------------------------------------
def _pkg_specs(name):
    """the specs tools/gen_golden_bernoulli.py built the fixture's model from (this package's generators, same seeds)"""
    from tgp.pytorch_amd import flows as G
    gens = {"sal_invbcl1": (21, lambda: G.build_chain("SAL_InvBCL", 1, constraint=None)),
            "bcl_al2": (22, lambda: G.build_chain("BCL_AL", 2, constraint=None)),
            "arcsl2": (23, lambda: G.ArcSL(2))}
    seed, fn = gens[name]
    np.random.seed(seed)
    return fn()


def _flow_of(name):
    for f in ("sal_invbcl1", "bcl_al2", "arcsl2"):
        if name.endswith(f):
            return f
    return None


def build_model(g, flow):
    from tgp.pytorch_amd.flow import compile_flow
    from tgp.pytorch_amd.kernels import instance_kernel
    from tgp.pytorch_amd.likelihoods import Bernoulli
    from tgp.pytorch_amd.models import sparse_MF_GP, sparse_MF_SP
    p = g["params"]
    N, D = g["X"].shape
    M = p["m"].numel()
    K = instance_kernel("scale_rbf", ard_num_dim=D, num_multioutput=1, kernel_is_shared=False,
                        init_params={"length_scale": 2.0, "kernel_scale": 2.0, "noisy_variance": 1e-6})
    ip = {"variational_distribution": {"variance_scale": 1e-5, "mean_scale": 0.0}}
    lik = Bernoulli()
    lik.quad_points = g["xs"].numel()
    if flow is None:
        model = sparse_MF_GP(["zero", K], g["X"], p["Z"].clone(), N, lik, 1, True, False, False, False, False, 0.0,
                             init_params=ip)
    else:
        model = sparse_MF_SP(["zero", K], g["X"], p["Z"].clone(), N, lik, 1, True, False, False, False, False,
                             [_pkg_specs(flow)], "single", 0.0, init_params=ip)
    with torch.no_grad():
        model.Z.data = p["Z"].reshape(1, M, D).clone()
        model.q_U.variational_mean.data = p["m"].reshape(1, M).clone()
        model.q_U.chol_variational_covar.data = p["Lam"].reshape(1, M, M).clone()
        model.covariance_function.raw_outputscale.data = p["raw_outputscale"].reshape(1).clone()
        model.covariance_function.base_kernel.raw_lengthscale.data = p["raw_lengthscale"].reshape(1, 1, D).clone()
        spec, theta_list, _ = compile_flow(model.G_matrix[0])
        assert [tuple(b) for b in spec.blocks] == [tuple(b) for b in g["program"]]
        for prm, val in zip(theta_list, p.get("theta", [])):
            prm.data = val.clone().reshape(prm.shape)
    return model.to(DEV)


STEP0 = ["bern_tiny_svgp", "bern_med_svgp", "bern_med_sal_invbcl1", "bern_med_bcl_al2", "bern_med_arcsl2",
         "bern_bigm_sal_invbcl1"]


@pytest.mark.parametrize("name", STEP0)
def test_model_elbo_matches_reference(name):
    from tgp.pytorch_amd.flow import compile_flow
    g = load_golden(name)
    model = build_model(g, _flow_of(name))
    assert sorted(n for n, _ in model.named_parameters() if "G_matrix" not in n) == \
        ["Z", "covariance_function.base_kernel.raw_lengthscale", "covariance_function.raw_outputscale",
         "q_U.chol_variational_covar", "q_U.variational_mean"]
    model.set_is_training(True)
    elbo, ell, kld = model.ELBO(g["X"].to(DEV), g["Y"].to(DEV))
    (-elbo).backward()
    assert rel_err(elbo.detach().cpu(), g["ELBO"]) < TOL_VAL
    assert rel_err(ell.cpu(), g["ELL"]) < TOL_VAL and rel_err(kld.cpu(), g["KLD"]) < TOL_VAL
    k = model.covariance_function
    for got, key in ((model.Z.grad[0], "g_Z"), (model.q_U.variational_mean.grad[0], "g_m"),
                     (model.q_U.chol_variational_covar.grad[0], "g_Lam"), (k.raw_outputscale.grad, "g_raw_outputscale"),
                     (k.base_kernel.raw_lengthscale.grad.reshape(-1), "g_raw_lengthscale")):
        assert rel_err(-got.cpu(), g[key]) < TOL_GRAD, key
    if "g_theta" in g:
        gt = torch.stack([-q.grad.reshape(()) for q in compile_flow(model.G_matrix[0])[1]]).cpu()
        assert rel_err(gt, g["g_theta"]) < TOL_GRAD


def _step(g, plan=0, rowp=None):
    from tgp.pytorch_amd import lib as L
    from tgp.pytorch_amd import ops
    p = {k: v.to(DEV) for k, v in g["params"].items()}
    P = p["theta"].numel() if "theta" in p else 0
    RP = rowp.shape[1] if rowp is not None else 0
    lvn = torch.zeros(1, dtype=F64, device=DEV)
    out, grads, status, _ = ops.elbo_step(g["X"].to(DEV), g["Y"].to(DEV), p["Z"], p["raw_lengthscale"], p["raw_outputscale"],
                                          p["m"], p["Lam"], lvn, float(g["N_total"]), flow=_spec(g["program"], P, RP),
                                          theta=p.get("theta"), rowp=None if rowp is None else rowp.to(DEV).contiguous(),
                                          S=g["xs"].numel(), plan=plan, lik=L.LIK_BERNOULLI)
    torch.cuda.synchronize()
    assert int(status[0]) == 0 and int(status[1]) == 0
    return out.cpu(), {k: v.cpu() for k, v in grads.items()}


def _compare(out, grads, g):
    assert rel_err(out[0], g["ELBO"]) < TOL_VAL and rel_err(out[1], g["ELL"]) < TOL_VAL
    for k_hip, k_ref in (("Z", "g_Z"), ("m", "g_m"), ("Lam", "g_Lam"), ("raw_os", "g_raw_outputscale"),
                         ("raw_ls", "g_raw_lengthscale")):
        assert rel_err(grads[k_hip], g[k_ref]) < TOL_GRAD, k_hip
    assert float(grads["lvn"].abs().max()) == 0.0
    if "g_theta" in g:
        assert rel_err(grads["theta"], g["g_theta"]) < TOL_GRAD


@pytest.mark.parametrize("chunk", [0, 128])
def test_general_path_row_chunks(chunk):
    """M = 200 in one chunk and in four 128-row chunks (TGP_PLAN_CHUNK_ROWS)."""
    from tgp.pytorch_amd import lib as L
    g = load_golden("bern_bigm_sal_invbcl1")
    out, grads = _step(g, plan=L.plan_chunk_rows(chunk) if chunk else 0)
    _compare(out, grads, g)


def test_per_row_sal_step_matches_reference():
    g = load_golden("bern_idsal1")
    out, grads = _step(g, rowp=g["rowp"])
    _compare(out, grads, g)
    assert rel_err(grads["rowp"], g["g_rowp"]) < TOL_GRAD


@pytest.mark.parametrize("name", ["bern_adam5_svgp", "bern_adam5_bcl_al2"])
def test_trainer_first_steps_match_reference(name):
    from tgp.pytorch_amd.data import DeviceLoader
    from tgp.pytorch_amd.flow import compile_flow
    from tgp.pytorch_amd.trainers import Trainer_SP_classification
    g = load_golden(name)
    model = build_model(g, _flow_of(name))
    loader = DeviceLoader(g["X"], g["Y"], 10000, shuffle=False, device=DEV)
    tr = Trainer_SP_classification(model, [loader, None, None], 1e20, False, False, torch.ones(1, device=DEV), -1, 100, True)
    tr.train(epochs=g["history"].shape[0], lr_ALL=0.01, opt="adam", keep_parameter_groups=True)
    assert tr._engine is None                           # Bernoulli trains on the eager path
    hist = torch.tensor([[-l, e, k] for l, e, k in zip(tr.loss_arr, tr.ELL_arr, tr.KLD_arr)], dtype=F64)
    assert rel_err(hist, g["history"]) < 1e-8
    assert rel_err(model.Z.detach()[0].cpu(), g["final_Z"]) < 1e-8
    assert rel_err(model.q_U.variational_mean.detach()[0].cpu(), g["final_m"]) < 1e-8
    if "final_theta" in g:
        th = torch.stack([q.detach().reshape(()) for q in compile_flow(model.G_matrix[0])[1]]).cpu()
        assert rel_err(th, g["final_theta"]) < 1e-8


@pytest.mark.parametrize("name", ["bern_tiny_svgp", "bern_med_svgp", "bern_med_sal_invbcl1", "bern_med_bcl_al2",
                                  "bern_med_arcsl2"])
def test_evaluation_path_matches_reference(name):
    from tgp.pytorch_amd import lib as L
    from tgp.pytorch_amd import ops
    from tgp.pytorch_amd.data import DeviceLoader
    from tgp.pytorch_amd.trainers import Trainer_SP_classification
    g = load_golden(name)
    model = build_model(g, _flow_of(name))
    model.set_is_training(False)
    X, Y = g["X"].to(DEV), g["Y"].to(DEV)
    P, m2, _, _ = model.predictive_distribution(X)
    assert m2 is None and P.shape == (X.shape[0], 1)
    assert rel_err(P.cpu().reshape(-1), g["pred_P"]) < TOL_VAL
    model.set_is_training(False)
    logp, (probs,) = model.test_log_likelihood(X, Y, return_moments=True, Y_std=torch.ones(1, device=DEV))
    assert logp.dtype == F64 and rel_err(logp.cpu(), g["test_logp_sum"]) < TOL_VAL
    assert rel_err(probs[:, 1].cpu(), g["pred_P"]) < TOL_VAL
    # the kernel's own log p(y_n) (tgp_predict_f64) sums to the same number
    theta = g["params"].get("theta")
    _, m2k, lp = ops.predict(g["mu"].to(DEV), g["v"].to(DEV), torch.zeros(1, dtype=F64, device=DEV),
                             _spec(g["program"], 0 if theta is None else theta.numel()),
                             None if theta is None else theta.to(DEV), g["xs"].numel(), Y=Y.reshape(-1),
                             lik=L.LIK_BERNOULLI)
    assert rel_err(lp.sum().cpu(), g["test_logp_sum"]) < TOL_VAL
    assert rel_err(m2k.cpu(), g["pred_P"] * (1 - g["pred_P"])) < TOL_VAL
    loader = DeviceLoader(g["X"], g["Y"], 10000, device=DEV)
    tr = Trainer_SP_classification(model, [loader, loader], 1e20, False, False, torch.ones(1, device=DEV), -1, 100, True)
    res = tr.compute_metrics()
    acc_ref = float(((g["pred_P"] > 0.5).to(F64) == g["Y"].reshape(-1)).to(F64).mean())
    assert abs(res[1] - acc_ref) < 1e-12 and abs(res[5] - acc_ref) < 1e-12
    assert abs(res[0] - float(g["test_logp_sum"]) / X.shape[0]) < 1e-9 * abs(res[0])


def test_pred_matches_torch_per_row():
    from tgp.pytorch_amd import lib as L
    from tgp.pytorch_amd import ops
    g = load_golden("bern_med_bcl_al2")
    theta = g["params"]["theta"]
    for S in (32, 1, 5):      # (1: one partly filled group of four nodes; 5: a full group and a one-node tail)
        P, _, _ = ops.predict(g["mu"].to(DEV), g["v"].to(DEV), torch.zeros(1, dtype=F64, device=DEV),
                              _spec(g["program"], theta.numel()), theta.to(DEV), S, lik=L.LIK_BERNOULLI)
        xs, ws = (torch.tensor(a) for a in np.polynomial.hermite.hermgauss(S))
        assert rel_err(P.cpu(), pred_torch(g["mu"], g["v"], g["program"], theta, xs, ws)) < TOL_VAL, S


def test_fully_bayesian_prediction_is_an_mc_average():
    from tgp.pytorch_amd import flows as G
    from tgp.pytorch_amd.flow import instance_flow
    from tgp.pytorch_amd.kernels import instance_kernel
    from tgp.pytorch_amd.likelihoods import Bernoulli
    from tgp.pytorch_amd.models import sparse_MF_SP
    torch.manual_seed(0)
    N, D, M = 80, 4, 10
    X = torch.randn(N, D, dtype=F64)
    specs = instance_flow(G.SAL(1, input_dependent=True, input_dim=D, num_hidden_layers=2, batch_norm=0, dropout=0.25,
                                hidden_dim=50, hidden_activation="relu", inference="MC_dropout"))
    specs.turn_off_initializer_parameters()
    K = instance_kernel("scale_rbf", ard_num_dim=D, num_multioutput=1, kernel_is_shared=False,
                        init_params={"length_scale": 2.0, "kernel_scale": 2.0, "noisy_variance": 1e-6})
    model = sparse_MF_SP(["zero", K], X, X[:M].clone(), N, Bernoulli(), 1, True, False, False, False, False, [specs],
                         "single", 0.0, init_params={"variational_distribution": {"variance_scale": 1e-5, "mean_scale": 0.0}})
    with torch.no_grad():
        model.q_U.variational_mean.data.normal_()
    model = model.to(DEV)
    model.set_is_training(False)
    P_point, _, _, _ = model.predictive_distribution(X.to(DEV))
    model.be_fully_bayesian(True)
    P_mc, m2, _, _ = model.predictive_distribution(X.to(DEV), S_MC_NNet=20)
    assert m2 is None and P_mc.shape == (N, 1)
    assert torch.isfinite(P_mc).all() and bool(((P_mc >= 0) & (P_mc <= 1)).all())
    assert not torch.equal(P_mc, P_point)
    Y = (torch.rand(N, 1, dtype=F64) < 0.5).to(F64).to(DEV)
    lp, (probs,) = model.test_log_likelihood(X.to(DEV), Y, return_moments=True, Y_std=torch.ones(1, device=DEV), S_MC_NNet=20)
    assert torch.isfinite(lp).all() and probs.shape == (N, 2)


def test_training_on_synthetic_banknote_reaches_high_accuracy():
    from tgp.pytorch_amd import config as cg
    from tgp.pytorch_amd.data import return_dataset
    from tgp.pytorch_amd.kernels import instance_kernel
    from tgp.pytorch_amd.likelihoods import Bernoulli
    from tgp.pytorch_amd.models import sparse_MF_GP
    from tgp.pytorch_amd.trainers import Trainer_SP_classification
    from tgp.pytorch_amd.utils import KMEANS
    loaders, dc = return_dataset("synthetic_banknote", 10000, seed=1, options={"shuffle_train": True})
    Z = KMEANS(dc["X_tr"], 50, n_init=2, seed=cg.config_seed)
    K = instance_kernel("scale_rbf", ard_num_dim=4, num_multioutput=1, kernel_is_shared=False,
                        init_params={"length_scale": 2.0, "kernel_scale": 2.0, "noisy_variance": 1e-6})
    model = sparse_MF_GP(["zero", K], dc["X_tr"], Z, dc["N_tr"], Bernoulli(), 1, True, False, False, False, False, 0.0,
                         init_params={"variational_distribution": {"variance_scale": 1e-5, "mean_scale": 0.0}}).to(DEV)
    tr = Trainer_SP_classification(model, loaders, 1e20, False, False, torch.ones(1, device=DEV), -1, 100, True)
    tr.train(epochs=300, lr_ALL=0.05, opt="adam", keep_parameter_groups=True)
    res = tr.compute_metrics()
    assert np.isfinite(res[0]) and np.isfinite(res[4])
    assert res[5] > 0.9, res


def test_cli_classification_run():
    cmd = [sys.executable, "-m", "tgp.pytorch_amd.main", "--model", "TGP", "--likelihood", "bernoulli", "--dataset",
           "synthetic_heart", "--train_test_seed_split", "1", "--num_inducing", "20", "--epochs", "50"]
    r = subprocess.run(["timeout", "-k", "10", "300"] + cmd, cwd=REPO, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "Test Negative LOGL" in r.stdout and "Test Accuracy" in r.stdout
