"""CPU: input gradients of q(f) and of the predictive moments above the kernels -- the torch restatement
(tests/input_grad_model.py) against torch autograd through the oracle, the ABI's three symbols, the library's refusals (before any
device is touched), the models' refusals, the synthetic_relevance data set and the CLI."""
import ctypes
import os
import re
import subprocess
import sys

import pytest
import torch

from conftest import REPO

import input_grad_model as IG
from oracle import tgp_oracle as orc
from tgp.pytorch_amd import lib as L

F64 = torch.float64
TOL = 1e-12          # the issue's bound on the restatement against autograd (measured: 4e-16 .. 4e-15)


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


def _problem(flow, N=65, D=4, M=20, S=32):
    prob = orc.synthetic_problem(N, D, M, seed=3, flow=flow, S=S)
    X = prob["X"].clone()
    X[7] = prob["params"]["Z"][11]          # one row of X equal to a row of Z bit for bit
    return prob, X


@pytest.mark.parametrize("kernel", ["scale_rbf", "scale_matern32"])
@pytest.mark.parametrize("flow", ["sal2", "tanh3x2"])
def test_restatement_is_oracle_autograd(kernel, flow):
    prob, X = _problem(flow)
    p = prob["params"]
    args = (p["Z"], p["raw_lengthscale"], p["raw_outputscale"], p["m"], p["Lam"])
    jit = 0.0          # (the oracle's psd_safe_cholesky factorises K_ZZ as it stands where that succeeds, as here)
    Xg = X.clone().requires_grad_(True)
    mu, v = orc.qf_moments(Xg, *args, kernel=kernel)
    g = torch.Generator().manual_seed(9)
    c1, c2 = torch.randn(X.shape[0], generator=g, dtype=F64), torch.randn(X.shape[0], generator=g, dtype=F64)
    dmu_ref, = torch.autograd.grad(mu.sum(), Xg, retain_graph=True)      # (each row's mu depends on that row only)
    dv_ref, = torch.autograd.grad(v.sum(), Xg, retain_graph=True)
    gX_ref, = torch.autograd.grad((c1 * mu + c2 * v).sum(), Xg)
    dmu, dv = IG.qf_input_grad(X, *args, jitter=jit, kernel=kernel)
    assert torch.isfinite(dmu).all() and torch.isfinite(dv).all()
    assert _rel(dmu, dmu_ref) <= TOL and _rel(dv, dv_ref) <= TOL, (_rel(dmu, dmu_ref), _rel(dv, dv_ref))
    assert _rel(c1[:, None] * dmu + c2[:, None] * dv, gX_ref) <= TOL
    mu_r, v_r = IG.qf_moments(X, *args, jitter=jit, kernel=kernel)
    assert _rel(mu_r, mu.detach()) <= TOL and _rel(v_r, v.detach()) <= 1e-9      # (TOL_VAL: two routes through the solves with K_ZZ)
    # the four partials through the flow
    mug, vg = mu.detach().clone().requires_grad_(True), v.detach().clone().requires_grad_(True)
    m1, m2 = orc.marginal_moments_flow(mug, vg, p["log_var_noise"], prob["program"], p["theta"], prob["xs"], prob["ws"])
    r1 = torch.autograd.grad(m1.sum(), [mug, vg], retain_graph=True)
    r2 = torch.autograd.grad(m2.sum(), [mug, vg])
    dm1, dm2 = IG.moment_partials(mu.detach(), v.detach(), prob["program"], p["theta"], prob["xs"], prob["ws"])
    for got, ref in ((dm1[0], r1[0]), (dm1[1], r1[1]), (dm2[0], r2[0]), (dm2[1], r2[1])):
        assert _rel(got, ref) <= TOL, _rel(got, ref)


@pytest.mark.parametrize("kernel,alpha", [("scale_matern52", None), ("scale_rq", 2.0)])
def test_restatement_other_kernels_are_their_own_autograd(kernel, alpha):
    prob, X = _problem("sal2")
    p = prob["params"]
    args = (p["Z"], p["raw_lengthscale"], p["raw_outputscale"], p["m"], p["Lam"])
    Xg = X.clone().requires_grad_(True)
    J_ref = torch.zeros(X.shape[0], p["Z"].shape[0], X.shape[1], dtype=F64)
    K = IG.kernel_matrix(Xg, p["Z"], p["raw_lengthscale"], p["raw_outputscale"], kernel, alpha)
    for m in range(p["Z"].shape[0]):
        J_ref[:, m, :], = torch.autograd.grad(K[:, m].sum(), Xg, retain_graph=True)
    J = IG.kernel_jacobian(X, p["Z"], p["raw_lengthscale"], p["raw_outputscale"], kernel, alpha)
    assert torch.isfinite(J).all() and float(J[7, 11].abs().max()) == 0.0       # the coincident pair: an exact zero
    assert _rel(J, J_ref) <= TOL, _rel(J, J_ref)
    mu, v = IG.qf_moments(Xg, *args, jitter=1e-6, kernel=kernel, alpha=alpha)
    dmu_ref, = torch.autograd.grad(mu.sum(), Xg, retain_graph=True)
    dv_ref, = torch.autograd.grad(v.sum(), Xg)
    dmu, dv = IG.qf_input_grad(X, *args, jitter=1e-6, kernel=kernel, alpha=alpha)
    assert _rel(dmu, dmu_ref) <= TOL and _rel(dv, dv_ref) <= TOL, (_rel(dmu, dmu_ref), _rel(dv, dv_ref))


def test_partials_of_the_empty_program_and_zero_variance():
    mu = torch.tensor([0.3, -1.0, 2.0], dtype=F64)
    v = torch.tensor([0.5, 0.0, 1.5], dtype=F64)
    dm1, dm2 = IG.moment_partials(mu, v, None, None, None, None)
    assert dm1.tolist() == [[1.0, 1.0, 1.0], [0.0, 0.0, 0.0]] and dm2.tolist() == [[0.0, 0.0, 0.0], [1.0, 0.0, 1.0]]
    prob = orc.synthetic_problem(3, 2, 2, seed=1, flow="sal2", S=8)
    dm1, dm2 = IG.moment_partials(mu, v, prob["program"], prob["params"]["theta"], prob["xs"], prob["ws"])
    assert float(dm1[1, 1]) == 0.0 and float(dm2[1, 1]) == 0.0 and torch.isfinite(dm1).all() and torch.isfinite(dm2).all()


def test_abi_declares_the_entries():
    hdr = open(os.path.join(REPO, "include", "tgp_hip.h")).read()
    for name in ("tgp_qf_input_grad_workspace_bytes", "tgp_qf_input_grad_f64", "tgp_predict_moment_grads_f64"):
        assert re.search(r"\b%s\(" % name, hdr), name
        assert name in L.EXPORTS
        assert getattr(L.load(), name).argtypes is not None
    assert re.search(r"#define TGP_VERSION 104\b", hdr) and L.load().tgp_version() == 104
    rows = int(re.search(r"#define TGP_XGRAD_PASS_ROWS (\d+)\b", hdr).group(1))
    assert rows == L.XGRAD_PASS_ROWS and rows % 128 == 0
    assert int(re.search(r"#define TGP_BIG_MAX_M (\d+)\b", hdr).group(1)) == L.BIG_MAX_M
    f = L.load().tgp_qf_input_grad_workspace_bytes
    # sized for min(N, TGP_XGRAD_PASS_ROWS) rows: the same workspace from one pass on, and growing below it
    assert f(rows, 4, 100) == f(rows + 1, 4, 100) == f(100 * rows, 4, 100) > f(rows - 128, 4, 100) > 0


def test_library_refusals_before_any_device():
    """Each refusal comes before a pointer is read: the arrays are host memory."""
    h = L.load()
    buf = torch.zeros(16, dtype=F64)
    st = torch.zeros(8, dtype=torch.int32)
    p, ps = ctypes.c_void_p(buf.data_ptr()), ctypes.c_void_p(st.data_ptr())

    def model(N=10, D=4, M=5, kernel=L.KERNEL_SCALE_RBF):
        md = L.TgpModel()
        md.N, md.D, md.M, md.S, md.kernel = N, D, M, 1, kernel
        md.Z = md.raw_ls = md.raw_os = md.m = md.Lam = md.log_var_noise = p
        return md

    entry = b"tgp_qf_input_grad_f64"
    rc = h.tgp_qf_input_grad_f64(model(kernel=2), p, p, p, ps, p, 1 << 40, None)
    assert rc == -1 and h.tgp_last_error().startswith(entry) and b"kernel = 2" in h.tgp_last_error()
    for kw in ({"D": 17}, {"M": L.BIG_MAX_M + 1}, {"D": 0}, {"M": 0}, {"N": 0}):
        rc = h.tgp_qf_input_grad_f64(model(**kw), p, p, p, ps, p, 1 << 40, None)
        assert rc == L.E_UNSUPPORTED and h.tgp_last_error().startswith(entry), kw
        assert h.tgp_qf_input_grad_workspace_bytes(kw.get("N", 10), kw.get("D", 4), kw.get("M", 5)) == 0
    need = h.tgp_qf_input_grad_workspace_bytes(10, 4, 5)
    rc = h.tgp_qf_input_grad_f64(model(), p, p, p, ps, p, need - 1, None)
    assert rc == L.E_WORKSPACE and h.tgp_last_error().startswith(entry) and str(need).encode() in h.tgp_last_error()
    # null pointers in the house order
    args = [model(), p, p, p, ps, p, need, None]
    for pos, code in ((1, -2), (2, -3), (3, -4), (4, -5), (5, -6)):
        a = list(args)
        a[pos] = None
        assert h.tgp_qf_input_grad_f64(*a) == code, pos
    assert h.tgp_qf_input_grad_f64(None, *args[1:]) == -1
    md = model()
    md.Lam = None
    assert h.tgp_qf_input_grad_f64(md, *args[1:]) == -1

    entry = b"tgp_predict_moment_grads_f64"
    md = L.TgpModel()
    md.N, md.D, md.M, md.S, md.lik = 4, 1, 1, 8, L.LIK_POISSON
    md.log_var_noise = p
    rc = h.tgp_predict_moment_grads_f64(md, p, p, None, p, p, None)
    assert rc == L.E_UNSUPPORTED and h.tgp_last_error().startswith(entry) and b"lik = %d" % L.LIK_POISSON in h.tgp_last_error()
    md.lik, md.S = L.LIK_FLOW, L.QUANTILE_MAX_S + 1
    rc = h.tgp_predict_moment_grads_f64(md, p, p, None, p, p, None)
    assert rc == L.E_UNSUPPORTED and h.tgp_last_error().startswith(entry) and b"S = " in h.tgp_last_error()
    md.lik = L.LIK_GAUSS
    assert h.tgp_predict_moment_grads_f64(md, None, p, None, p, p, None) == -2
    assert h.tgp_predict_moment_grads_f64(md, p, None, None, p, p, None) == -3
    assert h.tgp_predict_moment_grads_f64(md, p, p, None, None, p, None) == -5
    assert h.tgp_predict_moment_grads_f64(md, p, p, None, p, None, None) == -6
    assert h.tgp_predict_moment_grads_f64(None, p, p, None, p, p, None) == -1


def _model(kind, D=3, M=5):
    from tgp.pytorch_amd import config as cg
    from tgp.pytorch_amd.flows import SAL
    from tgp.pytorch_amd.kernels import instance_kernel
    from tgp.pytorch_amd.likelihoods import GaussianNonLinearMean, Poisson
    from tgp.pytorch_amd.models import sparse_MF_SP
    cg.set_maximum_precission()
    X = torch.randn(30, D, dtype=F64)
    K = instance_kernel("scale_rbf", ard_num_dim=D, num_multioutput=1, kernel_is_shared=False,
                        init_params={"length_scale": 2.0, "kernel_scale": 2.0, "noisy_variance": 1e-6})
    if kind == "poisson":
        lik, flow = Poisson(), SAL(1)
    else:
        lik = GaussianNonLinearMean(1, 0.05, False, 20)
        flow = SAL(1, input_dependent=True, input_dim=D, num_hidden_layers=1, batch_norm=0, dropout=0.5, hidden_dim=8,
                   hidden_activation="tanh", inference="MC_dropout")
    return sparse_MF_SP(["zero", K], X, X[:M].clone(), 30, lik, 1, True, False, False, False, False, [flow], "single", 0.0), X


def test_model_refusals_name_the_reason():
    old = torch.get_default_dtype()
    try:
        model, X = _model("poisson")
        model.set_is_training(False)
        with pytest.raises(NotImplementedError, match="Poisson"):
            model.predictive_input_gradients(X)
        from tgp.pytorch_amd.utils import input_relevance
        with pytest.raises(NotImplementedError, match="Poisson"):
            input_relevance(model, X)
        model, X = _model("idtgp")
        model.set_is_training(False)
        with pytest.raises(NotImplementedError, match="input-dependent"):
            model.predictive_input_gradients(X)
        model, X = _model("poisson")
        with pytest.raises(L.TgpError, match="GPU only"):       # (no CPU fall-back behind the new methods either)
            model.posterior_input_gradients(X)
    finally:
        torch.set_default_dtype(old)


def test_synthetic_relevance_is_seeded_and_shaped():
    import numpy as np
    from tgp.pytorch_amd import config as cg
    from tgp.pytorch_amd.data import return_dataset
    from tgp.pytorch_amd.synthetic import RELEVANCE_SHAPE, relevance_dataset
    old = torch.get_default_dtype()
    try:
        cg.set_maximum_precission()
        assert RELEVANCE_SHAPE == (1000, 6, 900)
        X, Y = relevance_dataset()
        X2, Y2 = relevance_dataset()
        assert X.shape == (1000, 6) and Y.shape == (1000, 1) and np.array_equal(X, X2) and np.array_equal(Y, Y2)
        resid = Y[:, 0] - (np.sin(2.0 * X[:, 0]) + 0.5 * X[:, 1])
        assert 0.08 < resid.std() < 0.12                      # 0.1 eps: four inputs carry nothing
        _, dc = return_dataset("synthetic_relevance", 10000, seed=1)
        _, dc2 = return_dataset("synthetic_relevance", 10000, seed=1)
        assert dc["X_tr"].shape == (900, 6) and dc["X_te"].shape == (100, 6) and dc["Y_tr"].shape == (900, 1)
        assert torch.equal(dc["X_tr"], dc2["X_tr"]) and torch.equal(dc["Y_te"], dc2["Y_te"])
    finally:
        torch.set_default_dtype(old)


def test_cli_relevance():
    run = lambda *a: subprocess.run([sys.executable, "-m", "tgp.pytorch_amd.main"] + list(a), cwd=REPO, capture_output=True,
                                    text=True, timeout=120)
    out = run("--help")
    assert out.returncode == 0 and "--relevance" in out.stdout and "synthetic_relevance" in out.stdout
    bad = run("--model", "SVGP", "--likelihood", "poisson", "--relevance", "--dataset", "synthetic_counts",
              "--train_test_seed_split", "1", "--num_inducing", "5")
    assert bad.returncode == 2 and "--relevance: SVGP or TGP with --likelihood gaussian only" in bad.stderr
    bad = run("--model", "ID_TGP", "--relevance", "--dataset", "synthetic_power", "--train_test_seed_split", "1",
              "--num_inducing", "5")
    assert bad.returncode == 2 and "--relevance" in bad.stderr
