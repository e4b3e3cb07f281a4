"""CPU: the heteroscedastic Gaussian likelihood above the kernels -- the ABI constant and exports, the closed form of the torch
restatement (tests/hetero_model.py) against an independent two-dimensional Gauss-Hermite product rule, the likelihood class,
the synthetic_hetero data set, every refusal of the models and engines (raised before a device is touched), the library's
single-output entries naming the entry to use, and the CLI's argument errors."""
import ctypes
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import REPO

import hetero_model as HM
from oracle import tgp_oracle as O
from tgp.pytorch_amd import lib as L

F64 = torch.float64


def _hermite(S):
    return tuple(torch.tensor(a) for a in np.polynomial.hermite.hermgauss(S))


def test_abi_constants_and_exports():
    hdr = open(os.path.join(REPO, "include", "tgp_hip.h")).read()
    assert re.search(r"#define TGP_LIK_HETERO 8\b", hdr)
    assert L.LIK_HETERO == 8
    assert "tgp_ell_hetero_f64" in L.EXPORTS and "tgp_predict_hetero_f64" in L.EXPORTS
    h = L.load()
    assert callable(h.tgp_ell_hetero_f64) and callable(h.tgp_predict_hetero_f64)


@pytest.mark.parametrize("flow", ["empty", "sal2"])
def test_closed_form_is_the_two_dimensional_expectation(flow):
    """ell_torch (h integrated out in closed form) against the S x S product rule over (f, h), S = 100, v2 in [0, 1] -- the cap
    is a condition: the product rule in h converges for moderate v2 only.  Bound 1e-12, relative."""
    g = torch.Generator().manual_seed(7)
    N, S = 200, 100
    if flow == "empty":
        program, theta = [], None
    else:
        prob = O.synthetic_problem(64, 4, 8, seed=5, flow="sal2")
        program, theta = [tuple(int(v) for v in b) for b in prob["program"]], prob["params"]["theta"].clone()
    mu = torch.stack([0.5 * torch.randn(N, generator=g, dtype=F64), 0.7 * torch.randn(N, generator=g, dtype=F64)])
    v = torch.stack([0.3 * torch.rand(N, generator=g, dtype=F64), torch.rand(N, generator=g, dtype=F64)])
    v[1, :5] = torch.tensor([0.0, 1.0, 0.5, 1e-8, 0.999], dtype=F64)
    assert float(v[1].max()) <= 1.0 and float(v[1].min()) >= 0.0
    Y = HM.flow_any(mu[0].reshape(1, -1), program, theta).reshape(-1) + 0.3 * torch.randn(N, generator=g, dtype=F64)
    c = torch.tensor([math.log(0.07)], dtype=F64)
    xs, ws = _hermite(S)
    closed = HM.ell_torch(Y, mu, v, c, program, theta, xs, ws, scale=3.5)
    product = HM.ell_product_rule(Y, mu, v, c, program, theta, xs, ws, scale=3.5)
    err = abs(float(closed - product)) / abs(float(product))
    print("closed form %.17g, product rule %.17g, relative difference %.2e" % (float(closed), float(product), err))
    assert err < 1e-12


def test_header_derivatives_are_autograd():
    """d/dmu2 = -1/2 + p A / 2, d/dv2 = -p A / 4, d/dc = sum_n d/dmu2_n, as include/tgp_hip.h states them."""
    g = torch.Generator().manual_seed(2)
    N, S = 50, 20
    mu = torch.randn(2, N, generator=g, dtype=F64).requires_grad_(True)
    v = torch.rand(2, N, generator=g, dtype=F64).requires_grad_(True)
    c = torch.tensor([math.log(0.2)], dtype=F64, requires_grad=True)
    Y = torch.randn(N, generator=g, dtype=F64)
    xs, ws = _hermite(S)
    ell = HM.ell_torch(Y, mu, v, c, [], None, xs, ws)
    gm, gv, gc = torch.autograd.grad(ell, [mu, v, c])
    with torch.no_grad():
        A = (Y - mu[0]) ** 2 + v[0]                       # the empty program: E[(y - f)^2]
        p = torch.exp(-(c + mu[1]) + 0.5 * v[1])
    assert float((gm[1] - (-0.5 + 0.5 * p * A)).abs().max()) < 1e-12 * float(gm[1].abs().max())
    assert float((gv[1] - (-0.25 * p * A)).abs().max()) < 1e-12 * float(gv[1].abs().max())
    assert abs(float(gc) - float(gm[1].sum())) < 1e-12 * abs(float(gc))


def test_restatement_predictive_of_the_empty_program():
    """m1 = mu1, m2 = v1 + exp(a + v2 / 2); with v2 = 0 the S x S mixture is tgp_predict_f64's one-noise mixture, which for the
    empty program is N(y | mu1, v1 + e^a) up to the quadrature of a Gaussian convolution -- which converges like (v1 / e^a)^S,
    so the rows keep v1 <= 0.05 under a noise variance >= 0.5 e^-0.9 = 0.2: a ratio <= 1/4, far below 1e-10 at S = 40."""
    g = torch.Generator().manual_seed(1)
    N = 64
    mu = torch.stack([torch.randn(N, generator=g, dtype=F64), 0.3 * torch.randn(N, generator=g, dtype=F64).clamp(-3.0, 3.0)])
    v = torch.stack([0.05 * torch.rand(N, generator=g, dtype=F64), torch.zeros(N, dtype=F64)])
    c = torch.tensor([math.log(0.5)], dtype=F64)
    xs, ws = _hermite(40)
    Y = mu[0] + 0.2
    m1, m2, lp = HM.pred_torch(mu, v, c, [], None, xs, ws, Y=Y, Y_std=2.0)
    var = v[0] + torch.exp(c + mu[1])
    assert torch.equal(m1, mu[0]) and float((m2 - var).abs().max()) < 1e-13
    exact = -0.5 * (math.log(2 * math.pi) + torch.log(var) + 0.04 / var) - math.log(2.0)
    assert float((lp - exact).abs().max()) < 1e-10
    assert HM.pred_torch(mu, v, c, [], None, xs, ws)[2] is None


def test_likelihood_class():
    from tgp.pytorch_amd import config as cg
    from tgp.pytorch_amd import likelihoods
    old = torch.get_default_dtype()
    cg.set_maximum_precission()
    try:
        lik = likelihoods.HeteroscedasticGaussian(0.05, 20)
        assert [n for n, _ in lik.named_parameters()] == ["log_var_noise"]
        assert lik.log_var_noise.numel() == 1 and abs(float(lik.log_var_noise.detach()) - math.log(0.05)) < 1e-14
        assert lik.quad_points == 20 and lik.out_dim == 2
        for m in ("expected_log_prob", "marginal_moments", "sample_from_output", "noise_std"):
            assert callable(getattr(lik, m))
        # closed-form quantiles of the noise standard deviation: exp((c + mu2 + z_p sqrt(v2)) / 2)
        mu2, v2 = torch.tensor([0.0, 1.0, -2.0], dtype=F64), torch.tensor([0.0, 0.25, 4.0], dtype=F64)
        q = lik.noise_std(mu2, v2, [0.5, 0.975])
        z = 1.959963984540054
        assert q.shape == (2, 3)
        assert float((q[0] - torch.exp(0.5 * (math.log(0.05) + mu2))).abs().max()) < 1e-14
        assert float((q[1] / torch.exp(0.5 * (math.log(0.05) + mu2 + z * torch.sqrt(v2))) - 1.0).abs().max()) < 1e-9
        # G(f) + exp((c + h) / 2) eps: centred on row 0, spread from row 1
        torch.manual_seed(0)
        f = torch.stack([torch.full((40000,), 1.5, dtype=F64), torch.full((40000,), math.log(4.0), dtype=F64)])
        s = lik.sample_from_output(f, 0)
        assert s.shape == (40000,) and abs(float(s.mean()) - 1.5) < 0.02
        assert abs(float(s.std()) - math.sqrt(0.05 * 4.0)) < 0.01
        with pytest.raises(AssertionError, match="two latent GPs"):
            lik.expected_log_prob(torch.zeros(1, 4, dtype=F64), torch.zeros(1, 4, dtype=F64), torch.ones(1, 4, dtype=F64),
                                  flow=[None], X=torch.zeros(1, 4, 1, dtype=F64))
    finally:
        torch.set_default_dtype(old)


def test_hetero_dataset(monkeypatch):
    from tgp.pytorch_amd import config as cg
    from tgp.pytorch_amd import data, synthetic
    n, d, n_tr = synthetic.HETERO_SHAPE
    X, Y, sigma = synthetic.hetero_dataset(1)
    assert (n, d) == (1000, 2) and X.shape == (n, d) and Y.shape == (n, 1) and sigma.shape == (n,)
    X2, Y2, s2 = synthetic.hetero_dataset(1)
    assert np.array_equal(X, X2) and np.array_equal(Y, Y2) and np.array_equal(sigma, s2)
    assert not np.array_equal(Y, synthetic.hetero_dataset(2)[1])
    # the noise level runs log-uniformly over [0.05, 1]: its range, and the two averages behind the 0.6 nats per point
    assert 0.05 <= sigma.min() < 0.052 and 0.96 < sigma.max() <= 1.0
    assert np.array_equal(sigma, synthetic.hetero_noise_std(X))
    assert abs(np.log(sigma).mean() - (-1.50)) < 0.05 and abs(0.5 * np.log((sigma ** 2).mean()) - (-0.90)) < 0.05
    resid = Y[:, 0] - (np.sin(2.0 * X[:, 0]) + 0.5 * X[:, 1])
    assert abs((resid / sigma).std() - 1.0) < 0.1
    monkeypatch.setattr(cg, "device", "cpu", raising=False)
    loaders, dc = data.return_dataset("synthetic_hetero", 10000, seed=1)
    assert dc["N_tr"] == n_tr and dc["N_te"] == n - n_tr and dc["Dx"] == d and dc["Dy"] == 1 and len(loaders) == 2
    assert torch.equal(dc["noise_std_te"], torch.tensor(sigma[dc["test_idx"]], dtype=F64))
    _, dc2 = data.return_dataset("synthetic_hetero", 10000, seed=1)
    assert torch.equal(dc["Y_tr"], dc2["Y_tr"]) and np.array_equal(dc["train_idx"], dc2["train_idx"])


def _model(kind="svgp", D=3, M=5, mean="zero", flow_h=None, num_outputs=2):
    from tgp.pytorch_amd import config as cg
    from tgp.pytorch_amd.flows import SAL
    from tgp.pytorch_amd.kernels import instance_kernel
    from tgp.pytorch_amd.likelihoods import HeteroscedasticGaussian
    from tgp.pytorch_amd.models import sparse_MF_GP, sparse_MF_SP
    cg.set_maximum_precission()
    X = torch.randn(30, D, dtype=F64)
    K = instance_kernel("scale_rbf", ard_num_dim=D, num_multioutput=num_outputs, kernel_is_shared=False,
                        init_params={"length_scale": 2.0, "kernel_scale": 2.0, "noisy_variance": 1e-6})
    lik = HeteroscedasticGaussian(0.05, 20)
    if kind == "svgp":
        return sparse_MF_GP([mean, K], X, X[:M].clone(), 30, lik, num_outputs, True, False, False, False, False, 0.0), X
    flow = SAL(1) if kind == "tgp" else SAL(1, input_dependent=True, input_dim=D, num_hidden_layers=1, batch_norm=0, dropout=0.5,
                                            hidden_dim=8, hidden_activation="tanh", inference="MC_dropout")
    flows = [flow, flow_h if flow_h is not None else [("identity", [])]][:num_outputs]
    return sparse_MF_SP([mean, K], X, X[:M].clone(), 30, lik, num_outputs, True, False, False, False, False, flows, "single",
                        0.0), X


def test_constructor_refusals():
    from tgp.pytorch_amd.flows import SAL
    old = torch.get_default_dtype()
    try:
        with pytest.raises(NotImplementedError, match="no flow on h"):
            _model("tgp", flow_h=SAL(1))
        with pytest.raises(NotImplementedError, match=r"heteroscedastic.*ID_TGP"):
            _model("idtgp")
        for mean in ("linear", "identity"):
            with pytest.raises(NotImplementedError, match="mean function is not built for the heteroscedastic"):
                _model("svgp", mean=mean)
        with pytest.raises(AssertionError, match="num_outputs = 2"):
            _model("svgp", num_outputs=1)
        # every other likelihood keeps its single-output assertion
        from tgp.pytorch_amd.kernels import instance_kernel
        from tgp.pytorch_amd.likelihoods import GaussianLinearMean
        from tgp.pytorch_amd.models import sparse_MF_GP
        X = torch.randn(30, 3, dtype=F64)
        K = instance_kernel("scale_rbf", ard_num_dim=3, num_multioutput=2, kernel_is_shared=False)
        with pytest.raises(AssertionError, match="single-output"):
            sparse_MF_GP(["zero", K], X, X[:5].clone(), 30, GaussianLinearMean(2, 0.05, False), 2, True, False, False, False, False,
                         0.0)
    finally:
        torch.set_default_dtype(old)


def test_method_refusals_name_the_likelihood():
    """Raised on CPU tensors: each refusal comes before the method asks for a device."""
    old = torch.get_default_dtype()
    try:
        for kind in ("svgp", "tgp"):
            model, X = _model(kind)
            assert model.likelihood.num_latent == 2 and model.likelihood.engine_name == "hetero"
            assert model._is_composed and model.out_dim == 2 and model._lik_id is None
            assert "likelihood.log_var_noise" in dict(model.named_parameters())
            assert model.Z.shape == (2, 5, 3) and model.q_U.variational_mean.shape == (2, 5)
            Y = torch.zeros(30, 1, dtype=F64)
            model.set_is_training(False)
            calls = {"predictive_quantiles": lambda: model.predictive_quantiles(X, [0.5]),
                     "predictive_cdf": lambda: model.predictive_cdf(X, Y),
                     "set_optimal_qu": lambda: model.set_optimal_qu(X, Y),
                     "collapsed_bound": lambda: model.collapsed_bound(X, Y),
                     "posterior_paths": lambda: model.posterior_paths(3),
                     "diagonal=False (moments)": lambda: model.marginal_variational_qf_parameters(X, diagonal=False, is_duvenaud=False),
                     "diagonal=False (predictive)": lambda: model.predictive_distribution(X, diagonal=False),
                     "diagonal=False (samples)": lambda: model.sample_from_predictive_distribution(X, 3, diagonal=False)}
            for name, call in calls.items():
                with pytest.raises(NotImplementedError, match="(?i)heteroscedastic"):
                    call()
        # predictive_noise_std belongs to this likelihood alone
        from tgp.pytorch_amd.kernels import instance_kernel
        from tgp.pytorch_amd.likelihoods import GaussianLinearMean
        from tgp.pytorch_amd.models import sparse_MF_GP
        X = torch.randn(30, 3, dtype=F64)
        K = instance_kernel("scale_rbf", ard_num_dim=3, num_multioutput=1, kernel_is_shared=False)
        plain = sparse_MF_GP(["zero", K], X, X[:5].clone(), 30, GaussianLinearMean(1, 0.05, False), 1, True, False, False, False,
                             False, 0.0)
        with pytest.raises(NotImplementedError, match="heteroscedastic likelihood only"):
            plain.predictive_noise_std(X, [0.5])
    finally:
        torch.set_default_dtype(old)


def test_engines_refuse():
    from tgp.pytorch_amd.engine import ElboEngine, MinibatchEngine, engine_refusal
    for kw in ({}, {"minibatch": True}, {"world_size": 2}, {"collective": object()}, {"is_whiten": True, "per_row": True}):
        why = engine_refusal(likelihood="hetero", **kw)
        assert why is not None and "heteroscedastic" in why, kw
    assert engine_refusal(likelihood=None) is None
    z = torch.zeros(4, 1, dtype=F64)
    with pytest.raises(NotImplementedError, match="heteroscedastic"):
        ElboEngine(z, z, {}, 4.0, likelihood="hetero")
    with pytest.raises(NotImplementedError, match="heteroscedastic"):
        ElboEngine(z, z, {}, 4.0, likelihood="hetero", world_size=2)
    with pytest.raises(NotImplementedError, match="heteroscedastic"):
        MinibatchEngine(z, z, {}, 4.0, 2, likelihood="hetero")


def test_single_output_entries_name_the_entry_to_use():
    """TGP_LIK_HETERO into the single-output entries: TGP_E_UNSUPPORTED before a pointer is read or a device touched, and
    tgp_last_error() names tgp_ell_hetero_f64."""
    h = L.load()
    buf = torch.zeros(16, dtype=F64)
    st = torch.zeros(2, dtype=torch.int32)
    p, ps = ctypes.c_void_p(buf.data_ptr()), ctypes.c_void_p(st.data_ptr())
    md = L.TgpModel()
    md.N, md.D, md.M, md.S, md.lik = 4, 1, 1, 8, L.LIK_HETERO
    md.log_var_noise = p
    gr = L.TgpGrads()
    adam = L.TgpAdamArgs()
    calls = {
        "tgp_elbo_step_f64": lambda: h.tgp_elbo_step_f64(md, p, p, None, p, gr, None, None, ps, p, 128, None),
        "tgp_elbo_step_phases_f64": lambda: h.tgp_elbo_step_phases_f64(md, p, p, None, p, gr, None, None, ps, p, 128, 7, None),
        "tgp_elbo_step_adam_f64": lambda: h.tgp_elbo_step_adam_f64(md, p, p, None, p, gr, None, None, ps, p, 128, adam, None),
        "tgp_optimal_qu_f64": lambda: h.tgp_optimal_qu_f64(md, p, p, p, p, ps, p, 128, None),
        "tgp_ell_flow_f64": lambda: h.tgp_ell_flow_f64(md, p, p, p, None, p, None, None, None, None, p, 128, None),
        "tgp_predict_f64": lambda: h.tgp_predict_f64(md, p, p, None, None, 1.0, p, p, None, None),
        "tgp_predict_quantile_f64": lambda: h.tgp_predict_quantile_f64(md, p, p, None, p, p, 1, p, ps, None),
        "tgp_predict_cdf_f64": lambda: h.tgp_predict_cdf_f64(md, p, p, None, p, p, None, None),
    }
    for name, call in calls.items():
        rc = call()
        msg = h.tgp_last_error()
        assert rc == L.E_UNSUPPORTED, (name, rc)
        assert b"tgp_ell_hetero_f64" in msg and b"TGP_LIK_HETERO" in msg, (name, msg)
    # the prediction entry's own limit on S, refused by name before any launch
    for S in (0, 257):
        md.S = S
        rc = h.tgp_predict_hetero_f64(md, p, p, None, None, 1.0, p, p, None, None)
        assert rc == L.E_UNSUPPORTED and b"tgp_predict_hetero_f64: S = %d" % S in h.tgp_last_error(), (S, rc)


def test_cli_arguments():
    run = lambda *a: subprocess.run([sys.executable, "-m", "tgp.pytorch_amd.main"] + list(a), cwd=REPO, capture_output=True,
                                    text=True, timeout=120)
    out = run("--help")
    assert out.returncode == 0 and "hetero" in out.stdout and "synthetic_hetero" in out.stdout
    tail = ["--dataset", "synthetic_hetero", "--train_test_seed_split", "1", "--num_inducing", "5"]
    for model in ("ID_TGP", "WGP"):
        bad = run("--model", model, "--likelihood", "hetero", *tail)
        assert bad.returncode == 2 and "--likelihood hetero: SVGP or TGP only" in bad.stderr, model
    for mean in ("linear", "identity"):
        bad = run("--model", "SVGP", "--likelihood", "hetero", "--mean", mean, *tail)
        assert bad.returncode == 2 and "--mean zero only" in bad.stderr
    bad = run("--model", "SVGP", "--likelihood", "hetero", "--qu", "optimal", *tail)
    assert bad.returncode == 2 and "--qu adam only" in bad.stderr
    bad = run("--model", "TGP", "--likelihood", "hetero", "--coverage", "exact", *tail)
    assert bad.returncode == 2 and "--coverage sampled only" in bad.stderr
