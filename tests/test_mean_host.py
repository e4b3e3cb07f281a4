"""Linear and identity mean functions, CPU side: tests/mean_model.py against the reference's fixtures
(tools/gen_golden_mean.py), the constructor's parameters, the identity mean's projection, and the CLI."""
import os
import subprocess
import sys

import numpy
import pytest
import torch

from conftest import REPO, load_golden, rel_err

import mean_model as mm

TOL_VAL, TOL_GRAD = 1e-9, 1e-7
# fixture -> (worst value difference, worst gradient difference) of tests/mean_model.py against the reference, relative to the
# largest reference entry, as tools/gen_golden_mean.py printed them; cond(K_ZZ) in the comment.  Every figure is within a tenth
# of the project's 1e-9 / 1e-7, so those hold for the GPU on every case (tolerances() keeps the 10 x rule in one place).
MEAN_CPU = {
    "mean_tiny_svgp_lin": (6.9e-16, 7.7e-15),      # 1.6e1
    "mean_tiny_sal1_lin": (6.9e-16, 1.3e-15),      # 1.6e1
    "mean_med_sal2_lin": (5.1e-14, 1.3e-12),       # 1.6e7
    "mean_edge128_tanh_id": (4.8e-16, 7.1e-15),    # 7.7e1
    "mean_bigm_matern_lin": (5.5e-16, 7.4e-15),    # 4.0e1
    "mean_bern_tiny_lin": (1.7e-15, 1.1e-12),      # 4.6e3
    "mean_unwh_sal2_lin": (9.1e-11, 1.5e-10),      # 1.6e7 (m - m(Z) through K_ZZ^-1: the KL is 1.9e6)
}
CASES = tuple(MEAN_CPU)
REGRESSION = tuple(n for n in CASES if "bern" not in n)
FLOWS = {"mean_tiny_sal1_lin": "sal1", "mean_med_sal2_lin": "sal2", "mean_edge128_tanh_id": "tanh3x2", "mean_bigm_matern_lin": "tanh3x2",
         "mean_bern_tiny_lin": "sal1", "mean_unwh_sal2_lin": "sal2", "mean_adam5_sal2_lin": "sal2"}
GRAD_KEYS = (("Z", "g_Z"), ("m", "g_m"), ("Lam", "g_Lam"), ("raw_outputscale", "g_raw_outputscale"),
             ("raw_lengthscale", "g_raw_lengthscale"), ("log_var_noise", "g_log_var_noise"), ("theta", "g_theta"),
             ("mean_a", "g_mean_a"), ("mean_b", "g_mean_b"))
# mean_adam5_sal2_lin: tests/mean_model.py under torch.optim.Adam(lr = 0.01) for the same 5 steps against the reference's
# history and final parameters (test_cpu_model_adam_steps prints them): history, then Z, m, L_q, theta, a, b
ADAM5_CPU = {"history": 5.1e-14, "params": 5.0e-12}
TOL_ADAM_HISTORY, TOL_ADAM_PARAMS = 1e-9, 1e-8        # the whitened adam5 tests' (tests/test_gpu_models.py)


def tolerances(name):
    """The project's tolerances, or 10 x the CPU restatement's own difference from the reference where it is larger."""
    val, grad = MEAN_CPU[name]
    assert val <= 0.1 * TOL_VAL and grad <= 0.1 * TOL_GRAD
    return max(TOL_VAL, 10.0 * val), max(TOL_GRAD, 10.0 * grad)


def is_identity(g):
    return "mean_W" in g


def build_model(g, name, device=None, mean=None):
    """The product's model at a fixture's values (constructed on the host, moved to `device`)."""
    from tgp.pytorch_amd.flow import compile_flow, instance_flow
    from tgp.pytorch_amd.flows import SAL, StepTanhL
    from tgp.pytorch_amd.kernels import instance_kernel
    from tgp.pytorch_amd.likelihoods import Bernoulli, GaussianLinearMean, GaussianNonLinearMean
    from tgp.pytorch_amd.models import sparse_MF_GP, sparse_MF_SP
    p = g["params"]
    N, D = g["X"].shape
    M = p["m"].numel()
    flow = FLOWS.get(name)
    bern = bool(int(g["bernoulli"]))
    whiten = bool(int(g["whiten"]))
    mean = mean or ("identity" if is_identity(g) else "linear")
    K = instance_kernel(g["kernel"], ard_num_dim=D, num_multioutput=1, kernel_is_shared=False,
                        init_params={"length_scale": 2.0, "kernel_scale": 2.0, "noisy_variance": 1e-6})
    ip = {"variational_distribution": {"variance_scale": 1e-5, "mean_scale": 0.0}}
    if flow is None:
        model = sparse_MF_GP([mean, K], g["X"], p["Z"].clone(), N, GaussianLinearMean(1, 0.05, False), 1, whiten, False,
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
        model = sparse_MF_SP([mean, K], g["X"], p["Z"].clone(), N, lik, 1, whiten, False, False, False, False, [specs],
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
        if mean == "linear":
            model.mean_function.a.data = g["mean_a"].reshape(1, D, 1).clone()
            model.mean_function.b.data = g["mean_b"].reshape(1, 1, 1).clone()
        elif mean == "identity":
            model.mean_function.W.copy_(g["mean_W"].reshape(1, D, 1))
    return model if device is None else model.to(device)


def test_fixture_set():
    for name in CASES + ("mean_adam5_sal2_lin",):
        path = os.path.join(REPO, "tests", "golden", name + ".npz")
        assert os.path.exists(path) and os.path.getsize(path) < 1 << 20, name
    g = load_golden("mean_bern_tiny_lin")
    assert float(g["gmax"]) <= 6.0
    assert set(float(y) for y in g["Y"].reshape(-1)) <= {0.0, 1.0}


@pytest.mark.parametrize("name", CASES)
def test_cpu_model_matches_reference(name):
    g = load_golden(name)
    a, b = mm.mean_params(g)
    mu, v = mm.qf_moments(g, g["X"], g["params"], a, b)
    (elbo, ell, kld), grads = mm.elbo_and_grads(g)
    e = (rel_err(mu, g["mu"]), rel_err(v, g["v"]), rel_err(elbo, g["ELBO"]), rel_err(ell, g["ELL"]), rel_err(kld, g["KLD"]))
    worst = 0.0
    for k, gk in GRAD_KEYS:
        if gk in g:
            worst = max(worst, rel_err(grads[k], g[gk]))
    print("%s: worst value %.2e  worst gradient %.2e" % (name, max(e), worst))
    # (the table's figures with room for another BLAS: a factor 10, which is what the GPU is allowed on top of them)
    assert max(e) <= max(10.0 * MEAN_CPU[name][0], 1e-13) and worst <= max(10.0 * MEAN_CPU[name][1], 1e-12)
    assert tolerances(name) == (TOL_VAL, TOL_GRAD)


@pytest.mark.parametrize("name", REGRESSION)
def test_cpu_model_held_out_moments(name):
    """mu + m(X*) and v on the 16 held-out rows; for the Gaussian likelihood m1 = mu and m2 = v + noise."""
    g = load_golden(name)
    a, b = mm.mean_params(g)
    mu, v = mm.qf_moments(g, g["X_te"], g["params"], a, b)
    assert rel_err(mu, g["mu_te"]) < TOL_VAL and rel_err(v, g["v_te"]) < TOL_VAL
    if g["program"] is None:
        assert rel_err(mu, g["pred_m1"]) < TOL_VAL
        assert rel_err(v + torch.exp(g["params"]["log_var_noise"]), g["pred_m2"]) < TOL_VAL


def test_mean_changes_the_result():
    """The fixtures' means are not negligible: dropping the mean moves mu by more than its own size on some row."""
    for name in ("mean_tiny_svgp_lin", "mean_edge128_tanh_id"):
        g = load_golden(name)
        a, b = mm.mean_params(g)
        assert float(mm.mean(g["X"], a, b).abs().max()) > 0.5


def test_cpu_model_adam_steps():
    g = load_golden("mean_adam5_sal2_lin")
    leaves = {k: v.clone().requires_grad_(True) for k, v in g["params"].items()}
    a, b = g["mean_a"].clone().requires_grad_(True), g["mean_b"].clone().requires_grad_(True)
    opt = torch.optim.Adam(list(leaves.values()) + [a, b], lr=0.01)
    hist = []
    for _ in range(g["history"].shape[0]):
        elbo, ell, kld = mm.elbo(g, leaves, a, b)
        opt.zero_grad()
        (-elbo).backward()
        opt.step()
        hist.append([elbo.item(), ell.item(), kld.item()])
    e_h = rel_err(torch.tensor(hist, dtype=torch.float64), g["history"])
    e_p = max(rel_err(leaves["Z"].detach(), g["final_Z"]), rel_err(leaves["m"].detach(), g["final_m"]),
              rel_err(torch.tril(leaves["Lam"].detach()), torch.tril(g["final_Lam"])), rel_err(leaves["theta"].detach(), g["final_theta"]),
              rel_err(a.detach(), g["final_mean_a"]), rel_err(b.detach(), g["final_mean_b"]),
              rel_err(leaves["raw_lengthscale"].detach(), g["final_raw_lengthscale"]),
              rel_err(leaves["raw_outputscale"].detach(), g["final_raw_outputscale"]),
              rel_err(leaves["log_var_noise"].detach(), g["final_log_var_noise"]))
    print("mean_adam5_sal2_lin: history %.2e  parameters %.2e" % (e_h, e_p))
    assert e_h <= 0.1 * TOL_ADAM_HISTORY and e_p <= 0.1 * TOL_ADAM_PARAMS


# ---- constructor ---------------------------------------------------------------------------------------------------------
def _f64():
    from tgp.pytorch_amd import config as cg
    cg.set_maximum_precission()
    return cg


@pytest.fixture
def f64():
    old = torch.get_default_dtype()
    cg = _f64()
    yield cg
    torch.set_default_dtype(old)


def test_linear_mean_parameters(f64):
    """Names, shapes and initial values: a (1, D, 1) from numpy.random.seed(config_seed) then randn, b (1, 1, 1) zeros."""
    from tgp.pytorch_amd.means import Linear
    g = load_golden("mean_tiny_sal1_lin")
    model = build_model(g, "mean_tiny_sal1_lin")
    D = g["X"].shape[1]
    names = dict(model.named_parameters())
    assert tuple(names["mean_function.a"].shape) == (1, D, 1) and tuple(names["mean_function.b"].shape) == (1, 1, 1)
    fresh = Linear(D, 1)
    numpy.random.seed(f64.config_seed)
    want = numpy.random.randn(1, D, 1)
    assert fresh.a.dtype == torch.float64 and numpy.array_equal(fresh.a.detach().numpy(), want)
    assert float(fresh.b.abs().max()) == 0.0
    # the fixture's a is that draw scaled by 0.3 (tools/gen_golden_mean.py): the reference draws the same numbers
    assert rel_err(0.3 * fresh.a.detach().reshape(-1), g["mean_a"]) < 1e-15
    assert isinstance(model.mean_function, Linear) and model._has_mean


def test_mean_is_shared_with_linear(f64):
    from tgp.pytorch_amd.kernels import instance_kernel
    from tgp.pytorch_amd.likelihoods import GaussianLinearMean
    from tgp.pytorch_amd.models import sparse_MF_GP
    X = torch.randn(20, 3, dtype=torch.float64)
    K = instance_kernel("scale_rbf", ard_num_dim=3, num_multioutput=1, kernel_is_shared=False)
    model = sparse_MF_GP(["linear", K], X, X[:4].clone(), 20.0, GaussianLinearMean(1, 0.05, False), 1, True, False, True, False,
                         False, 0.0)
    assert tuple(model.mean_function.a.shape) == (1, 3, 1) and model.mean_is_shared
    for name in ("zero", "identity"):
        with pytest.raises(AssertionError, match="mean_is_shared"):
            sparse_MF_GP([name, K], X, X[:4].clone(), 20.0, GaussianLinearMean(1, 0.05, False), 1, True, False, True, False, False, 0.0)
    with pytest.raises(AssertionError, match="mean function"):
        sparse_MF_GP(["quadratic", K], X, X[:4].clone(), 20.0, GaussianLinearMean(1, 0.05, False), 1, True, False, False, False,
                     False, 0.0)


def test_identity_projection(f64):
    """W is a buffer (no parameter), the first principal direction of the training inputs: the fixture's up to its sign."""
    from tgp.pytorch_amd.means import Identity, return_projection_matrix
    g = load_golden("mean_edge128_tanh_id")
    D = g["X"].shape[1]
    model = build_model(g, "mean_edge128_tanh_id", mean="zero")      # (built only for its arguments' sake)
    assert not model._has_mean
    W = return_projection_matrix(D, 1, g["X"])
    assert tuple(W.shape) == (D, 1)
    s = 1.0 if float((W.reshape(-1) * g["mean_W"]).sum()) > 0 else -1.0
    assert rel_err(s * W.reshape(-1), g["mean_W"]) < 1e-12
    assert torch.equal(return_projection_matrix(3, 3, g["X"][:, :3]), torch.eye(3, dtype=torch.float64))
    assert tuple(return_projection_matrix(2, 3, g["X"][:, :2]).shape) == (2, 3)
    mean = Identity(W, D, 1)
    assert tuple(mean.W.shape) == (1, D, 1) and not list(mean.parameters()) and "W" not in mean.state_dict()


def test_zero_mean_model_has_no_new_parameters(f64):
    g = load_golden("mean_tiny_svgp_lin")
    model = build_model(g, "mean_tiny_svgp_lin", mean="zero")
    assert not any(n.startswith("mean_function") for n, _ in model.named_parameters())


def test_cli_lists_mean():
    out = subprocess.run([sys.executable, "-m", "tgp.pytorch_amd.main", "--help"], cwd=REPO, capture_output=True, text=True)
    assert out.returncode == 0 and "--mean" in out.stdout and "identity" in out.stdout
