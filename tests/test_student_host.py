"""CPU: the Student-t likelihood above the kernels -- the ABI constant, the torch restatement (tests/student_model.py) against
torch.distributions.StudentT, the likelihood class, the synthetic_outliers data set, the refusals of the engines, the models,
the library's quantile entries (before any device is touched) and the CLI."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import REPO

import student_model as SM
from tgp.pytorch_amd import lib as L

F64 = torch.float64


def test_abi_constants():
    hdr = open(os.path.join(REPO, "include", "tgp_hip.h")).read()
    assert re.search(r"#define TGP_LIK_STUDENT 7\b", hdr)
    assert re.search(r"#define TGP_VERSION 104\b", hdr)
    assert "2 < nu <= 1e4" in hdr
    assert L.LIK_STUDENT == 7 and L.STUDENT_MAX_DF == 1e4
    assert L.load().tgp_version() == 104


@pytest.mark.parametrize("nu", [2.5, 4.0, 30.0])
def test_node_term_is_torch_student_t(nu):
    g = torch.Generator().manual_seed(3)
    y = 3.0 * torch.randn(2000, generator=g, dtype=F64)
    loc = torch.randn(2000, generator=g, dtype=F64)
    y[:5] = loc[:5] + torch.tensor([0.0, 1e-9, 50.0, -1e3, 1e6], dtype=F64)
    for sig2 in (0.05, 1.0, 7.0):
        eta = torch.tensor(np.log(sig2), dtype=F64, requires_grad=True)
        locg = loc.clone().requires_grad_(True)
        ours = SM.log_p(y, locg, eta, nu)
        ref = torch.distributions.StudentT(torch.tensor(nu, dtype=F64), locg, torch.exp(0.5 * eta)).log_prob(y)
        err = float(((ours - ref).abs() / ref.abs().clamp(min=1.0)).max().detach())
        assert err <= 1e-12, (nu, sig2, err)
        # the two derivatives the header states, against autograd of torch's own log_prob
        gl, ge = torch.autograd.grad(ref.sum(), [locg, eta])
        r = (y - loc).detach()
        q = nu * sig2 + r * r
        assert float(((nu + 1.0) * r / q - gl).abs().max()) <= 1e-12 * max(1.0, float(gl.abs().max()))
        assert abs(float((-0.5 + 0.5 * (nu + 1.0) * r * r / q).sum() - ge)) <= 1e-12 * max(1.0, abs(float(ge)))


def test_restatement_moments_of_the_empty_program():
    """Gauss-Hermite is exact for the first two moments of the identity flow: m1 = mu, m2 = v + sigma^2 nu / (nu - 2)."""
    g = torch.Generator().manual_seed(1)
    mu = torch.randn(100, generator=g, dtype=F64)
    v = 0.5 * torch.rand(100, generator=g, dtype=F64)
    xs, ws = (torch.tensor(a) for a in np.polynomial.hermite.hermgauss(20))
    eta = torch.tensor(np.log(0.3), dtype=F64)
    m1, m2, lp = SM.pred_torch(mu, v, eta, 4.0, [], None, xs, ws, Y=mu + 0.1, Y_std=2.0)
    assert float((m1 - mu).abs().max()) < 1e-13 and float((m2 - (v + 0.3 * 2.0)).abs().max()) < 1e-13
    assert torch.isfinite(lp).all()
    assert bool(torch.isinf(SM.pred_torch(mu, v, eta, 2.0, [], None, xs, ws)[1]).all())


def test_student_class_api():
    from tgp.pytorch_amd import config as cg
    from tgp.pytorch_amd import likelihoods
    old = torch.get_default_dtype()
    cg.set_maximum_precission()
    try:
        lik = likelihoods.StudentT(1, 0.05, False, 20)
        gauss = likelihoods.GaussianNonLinearMean(1, 0.05, False, 20)
        assert float(lik.df) == 4.0 and lik.quad_points == 20
        names = [n for n, _ in lik.named_parameters()]
        assert names == ["log_var_noise"] == [n for n, _ in gauss.named_parameters()]
        assert lik.log_var_noise.shape == gauss.log_var_noise.shape and torch.equal(lik.log_var_noise, gauss.log_var_noise)
        assert all(p is not lik.df for p in lik.parameters()) and "df" in dict(lik.named_buffers())
        assert "df" in lik.state_dict()
        for bad in (2.0, 1.0, -3.0, 1e4 + 1.0, float("nan")):
            with pytest.raises(ValueError, match="degrees of freedom"):
                likelihoods.StudentT(1, 0.05, False, 20, df=bad)
        assert float(likelihoods.StudentT(1, 0.05, False, 20, df=1e4).df) == 1e4
        for m in ("expected_log_prob", "marginal_moments", "sample_from_output"):
            assert callable(getattr(lik, m))
        # G(f) + sigma t: the draws centre on f and have the Student-t's spread sigma sqrt(nu / (nu - 2)), here 0.5 sqrt(3)
        lik5 = likelihoods.StudentT(1, 0.25, False, 20, df=6.0)
        torch.manual_seed(0)
        f = torch.full((1, 40000), 1.5, dtype=F64)
        s = lik5.sample_from_output(f, 0)
        assert s.shape == f.shape and abs(float(s.mean()) - 1.5) < 0.02
        assert abs(float(s.std()) - 0.5 * np.sqrt(6.0 / 4.0)) < 0.03
    finally:
        torch.set_default_dtype(old)


def test_outliers_dataset(monkeypatch):
    from tgp.pytorch_amd import config as cg
    from tgp.pytorch_amd import data, synthetic
    X, Y = synthetic.outliers_dataset()
    n, d, n_tr = synthetic.OUTLIERS_SHAPE
    assert X.shape == (n, d) and Y.shape == (n, 1) and np.array_equal(Y, synthetic.outliers_dataset(seed=0)[1])
    assert float(np.abs(Y).max()) < 4.0                                  # the clean targets
    Yd, idx = synthetic.gross_errors(Y[:n_tr], seed=1)
    assert idx.size == n_tr // 10 and np.all(np.abs(Yd[idx]) >= 5.0)
    keep = np.setdiff1d(np.arange(n_tr), idx)
    assert np.array_equal(Yd[keep], Y[:n_tr][keep])
    monkeypatch.setattr(cg, "device", "cpu", raising=False)
    loaders, dc = data.return_dataset("synthetic_outliers", 10000, seed=1)
    assert dc["N_tr"] == n_tr and dc["N_te"] == n - n_tr and dc["Dx"] == d and len(loaders) == 2
    # what the loader must hold: the seeded split, 10 % of its TRAINING targets replaced, everything standardised by the
    # (corrupted) training split; the test targets are the clean ones
    tr, te = dc["train_idx"], dc["test_idx"]
    dirty, out = synthetic.gross_errors(Y[tr], seed=1)
    assert np.array_equal(dc["outlier_idx"], out) and out.size == n_tr // 10
    mean, std = dirty.mean(), dirty.std() + 1e-15
    assert np.allclose(dc["Y_tr"].numpy(), (dirty - mean) / std, atol=1e-12)
    assert np.allclose(dc["Y_te"].numpy(), (Y[te] - mean) / std, atol=1e-12)
    assert abs(float(np.asarray(dc["Y_std"]).reshape(-1)[0]) - std) < 1e-12
    _, dc2 = data.return_dataset("synthetic_outliers", 10000, seed=1)
    assert torch.equal(dc["Y_tr"], dc2["Y_tr"]) and np.array_equal(tr, dc2["train_idx"])


def test_engine_refusal_and_surface():
    from tgp.pytorch_amd import models, ops
    from tgp.pytorch_amd.engine import engine_refusal
    assert "Student-t" in engine_refusal(likelihood="studentt")
    assert "Student-t" in engine_refusal(likelihood="studentt", minibatch=True)
    from tgp.pytorch_amd import likelihoods
    assert likelihoods.StudentT.lik_id == L.LIK_STUDENT
    assert callable(ops.ell_student) and callable(ops.EllStudentFunction.apply)
    lvn = torch.zeros(1, dtype=F64)
    assert ops.student_noise(lvn, 4.0).tolist() == [0.0, 4.0]
    assert ops.student_noise(lvn, torch.tensor([30.0])).tolist() == [0.0, 30.0]
    with pytest.raises(ValueError, match="degrees of freedom"):
        ops.student_noise(lvn, 2.0)
    with pytest.raises(L.TgpError, match="Student-t"):
        ops.elbo_step(torch.zeros(4, 1, dtype=F64), torch.zeros(4, dtype=F64), torch.zeros(2, 1, dtype=F64), lvn, lvn,
                      torch.zeros(2, dtype=F64), torch.eye(2, dtype=F64), lvn, 4.0, flow=None, lik=L.LIK_STUDENT, df=4.0)


def _model(kind="svgp", num_outputs=1, D=3, M=5):
    from tgp.pytorch_amd import config as cg
    from tgp.pytorch_amd.flows import SAL
    from tgp.pytorch_amd.kernels import instance_kernel
    from tgp.pytorch_amd.likelihoods import StudentT
    from tgp.pytorch_amd.models import sparse_MF_GP, sparse_MF_SP
    cg.set_maximum_precission()
    X = torch.randn(30, D, dtype=F64)
    K = instance_kernel("scale_rbf", ard_num_dim=D, num_multioutput=num_outputs, kernel_is_shared=False,
                        init_params={"length_scale": 2.0, "kernel_scale": 2.0, "noisy_variance": 1e-6})
    lik = StudentT(num_outputs, 0.05, False, 20, df=4.0)
    if kind == "svgp":
        return sparse_MF_GP(["zero", K], X, X[:M].clone(), 30, lik, num_outputs, True, False, False, False, False, 0.0), X
    flow = SAL(1) if kind == "tgp" else SAL(1, input_dependent=True, input_dim=D, num_hidden_layers=1, batch_norm=0, dropout=0.5,
                                            hidden_dim=8, hidden_activation="tanh", inference="MC_dropout")
    return sparse_MF_SP(["zero", K], X, X[:M].clone(), 30, lik, num_outputs, True, False, False, False, False,
                        [flow] * num_outputs, "single", 0.0), X


def test_model_refusals():
    old = torch.get_default_dtype()
    try:
        with pytest.raises(NotImplementedError, match="Student-t"):
            _model("idtgp")
        with pytest.raises(NotImplementedError, match="Student-t"):
            _model("svgp", num_outputs=2)
        for kind in ("svgp", "tgp"):
            model, X = _model(kind)
            assert model.likelihood.lik_id == L.LIK_STUDENT and model._lik_id == L.LIK_STUDENT
            assert [n for n, _ in model.named_parameters() if "df" in n.split(".")] == []
            assert "likelihood.log_var_noise" in dict(model.named_parameters())
            Y = torch.zeros(30, 1, dtype=F64)
            model.set_is_training(False)
            for call in (lambda: model.set_optimal_qu(X, Y), lambda: model.collapsed_bound(X, Y),
                         lambda: model.predictive_quantiles(X, [0.5]), lambda: model.predictive_cdf(X, Y)):
                with pytest.raises(NotImplementedError, match="Student-t"):
                    call()
    finally:
        torch.set_default_dtype(old)


def test_library_quantile_entries_name_the_likelihood():
    """The two quantile entries refuse TGP_LIK_STUDENT by name before they read a pointer or touch a device."""
    import ctypes
    h = L.load()
    buf = torch.zeros(16, dtype=F64)            # host memory: the refusal comes before any pointer is read
    st = torch.zeros(1, dtype=torch.int32)
    p, ps = ctypes.c_void_p(buf.data_ptr()), ctypes.c_void_p(st.data_ptr())
    md = L.TgpModel()
    md.N, md.D, md.M, md.S, md.lik = 4, 1, 1, 8, L.LIK_STUDENT
    md.log_var_noise = p
    rc = h.tgp_predict_quantile_f64(md, p, p, None, p, p, 1, p, ps, None)
    assert rc == L.E_UNSUPPORTED and b"TGP_LIK_STUDENT" in h.tgp_last_error()
    rc = h.tgp_predict_cdf_f64(md, p, p, None, p, p, None, None)
    assert rc == L.E_UNSUPPORTED and b"TGP_LIK_STUDENT" in h.tgp_last_error()


def test_cli_arguments():
    run = lambda *a: subprocess.run([sys.executable, "-m", "tgp.pytorch_amd.main"] + list(a), cwd=REPO, capture_output=True,
                                    text=True, timeout=120)
    out = run("--help")
    assert out.returncode == 0 and "studentt" in out.stdout and "--df" in out.stdout and "synthetic_outliers" in out.stdout
    tail = ["--dataset", "synthetic_outliers", "--train_test_seed_split", "1", "--num_inducing", "5"]
    bad = run("--model", "ID_TGP", "--likelihood", "studentt", *tail)
    assert bad.returncode == 2 and "--likelihood studentt: SVGP or TGP only" in bad.stderr
    bad = run("--model", "SVGP", "--likelihood", "studentt", "--df", "2", *tail)
    assert bad.returncode == 2 and "--df" in bad.stderr and "(2, 1e4]" in bad.stderr
    bad = run("--model", "SVGP", "--likelihood", "studentt", "--dataset", "synthetic_counts", "--train_test_seed_split", "1",
              "--num_inducing", "5")
    assert bad.returncode == 2 and "count data sets" in bad.stderr     # (the count sets stay Poisson's)
