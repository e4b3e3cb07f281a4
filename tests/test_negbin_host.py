"""CPU: the negative-binomial likelihood above the kernels -- the ABI constant, the torch restatement (tests/negbin_model.py)
against torch.distributions.NegativeBinomial and autograd, the trait table and the state names of the likelihood class, the
refusals of the models (before any library call), of the library's quantile, CDF and CRPS entries (before any launch) and of
the CLI, the engines' refusal and the synthetic_overdispersed data set."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import REPO

import negbin_model as NM
from tgp.pytorch_amd import lib as L

F64 = torch.float64


@pytest.fixture(autouse=True)
def _f64():
    from tgp.pytorch_amd import config as cg
    old = torch.get_default_dtype()
    cg.set_maximum_precission()
    yield
    torch.set_default_dtype(old)


def test_abi_constants():
    hdr = open(os.path.join(REPO, "include", "tgp_hip.h")).read()
    assert re.search(r"#define TGP_LIK_NEGBIN 9\b", hdr)
    assert re.search(r"#define TGP_VERSION 104\b", hdr)
    assert "1e-3 <= r <= 1e3" in hdr
    assert L.LIK_NEGBIN == 9
    assert L.load().tgp_version() == 104


def _points(r):
    """Counts and log-means over the range the kernels meet: rates e^-8 .. e^8 around r, zero and large counts."""
    g = torch.Generator().manual_seed(7)
    logm = 3.0 * torch.randn(3000, generator=g, dtype=F64).clamp(-2.7, 2.7)
    y = torch.poisson(torch.exp(logm.clamp(max=6.0)) * torch._standard_gamma(torch.full((3000,), 2.0, dtype=F64), generator=g) / 2.0,
                      generator=g)
    y[:4] = torch.tensor([0.0, 1.0, 1e4, 1e6], dtype=F64)
    return y, logm


@pytest.mark.parametrize("r", [0.05, 0.5, 3.0, 50.0, 1e3])
def test_log_p_is_torch_negative_binomial(r):
    y, logm = _points(r)
    lam = torch.tensor(np.log(r), dtype=F64)
    ours = NM.log_p(y, logm, lam)
    ref = torch.distributions.NegativeBinomial(total_count=torch.tensor(r, dtype=F64), logits=logm - lam).log_prob(y)
    err = float(((ours - ref).abs() / ref.abs().clamp(min=1.0)).max())
    print("r = %g: max relative difference of log p %.3e" % (r, err))
    assert err <= 1e-10


@pytest.mark.parametrize("r", [0.05, 0.5, 3.0, 50.0, 1e3])
def test_derivatives_are_autograd(r):
    """d/dg and d/dlam as the header states them, POINT BY POINT (lam is one autograd leaf per point), against autograd of the
    restatement's own log p at every point and of torch's log_prob at the points with y <= 1e4 (its lgamma differences lose
    digits of d/dlam at y = 1e6 against r = 1e3; its value is compared above).  d/dlam is a sum of terms that cancel, so a
    point's error is measured against the magnitudes of its terms, r psi(y + r), r psi(r), r sp(u) and the two of d/dg, y and
    (y + r) sigmoid(u): each is a few roundings of a library function good to ~1e-15 relative, six of them, and 1e-13 leaves a
    factor of ten."""
    y_all, logm_all = _points(r)
    for which in ("ours", "torch"):
        keep = torch.ones_like(y_all, dtype=torch.bool) if which == "ours" else y_all <= 1e4
        y, logm = y_all[keep], logm_all[keep]
        lam = torch.full_like(y, float(np.log(r))).requires_grad_(True)
        g = logm.clone().requires_grad_(True)
        if which == "ours":
            lp = NM.log_p(y, g, lam)
        else:
            lp = torch.distributions.NegativeBinomial(total_count=torch.exp(lam), logits=g - lam).log_prob(y)
        gg, gl = torch.autograd.grad(lp.sum(), [g, lam])
        lam0 = lam.detach()
        dg = NM.dlog_p_dg(y, logm, lam0)
        dl = NM.dlog_p_dlam(y, logm, lam0)
        scale = r * (torch.digamma(y + r).abs() + abs(float(torch.digamma(torch.tensor(r, dtype=F64))))) \
            + r * NM.softplus(logm - lam0) + y + (y + r) * torch.sigmoid(logm - lam0)
        eg = float(((dg - gg).abs() / (y + r)).max())           # d/dg = y - (y + r) sigmoid(u): against its larger term
        el = float(((dl - gl).abs() / scale).max())
        print("r = %g (%s): per point d/dg %.3e, d/dlam %.3e of its terms' magnitudes" % (r, which, eg, el))
        assert eg <= 1e-13 and el <= 1e-13
    y, logm, lam = y_all, logm_all, torch.tensor(np.log(r), dtype=F64)
    # r (y - mean) / (r + mean), the other form of d/dg
    mean = torch.exp(logm)
    assert float((NM.dlog_p_dg(y, logm, lam.detach()) - r * (y - mean) / (r + mean)).abs().max()) <= 1e-9 * float(y.max())


def test_restatement_poisson_limit_and_moments():
    """r = 1e3 is close to the Poisson restatement, by the next-order term; the moments of the empty program are the log-normal
    closed forms, which the quadrature reproduces."""
    import poisson_model as PM
    g = torch.Generator().manual_seed(2)
    mu = 0.5 * torch.randn(200, generator=g, dtype=F64)
    v = 0.3 * torch.rand(200, generator=g, dtype=F64)
    Y = torch.poisson(torch.exp(mu), generator=g)
    xs, ws = (torch.tensor(a) for a in np.polynomial.hermite.hermgauss(32))
    lam = torch.tensor(np.log(1e3), dtype=F64)
    nb = NM.ell_torch(Y, mu, v, lam, [], None, xs, ws)
    po = PM.ell_torch(Y, mu, v, [], None, xs, ws)
    gq = NM._nodes(mu, v, [], None, xs, None)
    wn = (ws / np.sqrt(np.pi)).reshape(-1, 1)
    bound = 2.0 * float((wn * (((Y.reshape(1, -1) - torch.exp(gq)) ** 2 - Y.reshape(1, -1)).abs() / 2e3)).sum())
    assert abs(float(nb - po)) <= bound
    m1, m2, _ = NM.pred_torch(mu, v, lam, [], None, xs, ws)
    q1, q2 = (wn * torch.exp(gq)).sum(0), (wn * torch.exp(2.0 * gq)).sum(0)
    assert float((m1 - q1).abs().max() / q1.abs().max()) < 1e-12
    assert float((m2 - (q1 + (1.0 + 1e-3) * q2 - q1 * q1)).abs().max() / m2.abs().max()) < 1e-10


def test_trait_table():
    from tgp.pytorch_amd import likelihoods as LK
    base = LK.Likelihood
    lik = LK.NegativeBinomial()
    traits = [n for n in vars(base) if not n.startswith("_") and not callable(getattr(base, n))
              and not isinstance(vars(base)[n], (staticmethod, classmethod))]
    assert "display" in traits and "refuses_cdf" in traits and "num_latent" in traits
    for n in traits:
        getattr(lik, n)                                  # every trait is defined
    assert lik.display == "negative-binomial" and lik.lik_id == L.LIK_NEGBIN == 9 and lik.engine_name == "negbinomial"
    assert lik.kind == "count" and lik.has_noise is True and lik.has_flow is True and lik.one_launch_logp is True
    assert lik.flow_on_targets is False and lik.compiles_flows is False
    assert lik.num_latent == 1 and lik.composed is False
    assert lik.refuses_input_dependent == LK.NO_INPUT_DEPENDENT % lik.display
    assert lik.refuses_optimal_qu == LK.NOT_GAUSSIAN_IN_F % lik.display and lik.refuses_optimal_qu_id is None
    # %s where the base says so: refuses_cdf takes the method asked for; the count likelihoods have a pmf-based CRPS (no refusal)
    assert lik.refuses_cdf.count("%s") == 1 and "predictive_pmf" in lik.refuses_cdf and "negative-binomial" in lik.refuses_cdf
    assert lik.refuses_crps is None and lik.refuses_mean is None and lik.refuses_paths is None and lik.refuses_full_cov is None
    assert "negative-binomial" in lik.outputs_refusal
    assert lik.lik_kwargs() == {"lik": L.LIK_NEGBIN, "df": None}
    # the parameter: one element, log r, what noise() hands to the ABI's noise slot
    assert [n for n, _ in lik.named_parameters()] == ["log_dispersion"] and list(lik.state_dict()) == ["log_dispersion"]
    assert list(dict(lik.named_buffers())) == []
    assert lik.log_dispersion.shape == (1,) and float(lik.log_dispersion.detach()) == 0.0
    assert lik.noise().shape == (1,) and lik.noise().requires_grad
    assert abs(float(LK.NegativeBinomial(dispersion_init=2.5).dispersion) - 2.5) < 1e-15
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="dispersion"):
            LK.NegativeBinomial(dispersion_init=bad)
    with pytest.raises(ValueError, match="counts"):
        lik.check_targets(torch.tensor([[1.0], [2.5]], dtype=F64))
    with pytest.raises(ValueError, match="counts"):
        lik.check_targets(torch.tensor([[1.0], [-1.0]], dtype=F64))
    lik.check_targets(torch.tensor([[0.0], [7.0]], dtype=F64))
    # Gamma-Poisson draws: integers >= 0 with mean e^f and variance mean + mean^2 / r
    lik2 = LK.NegativeBinomial(dispersion_init=2.0)
    torch.manual_seed(0)
    f = torch.full((1, 60000), np.log(4.0), dtype=F64)
    s = lik2.sample_from_output(f, 0)
    assert s.shape == f.shape and bool((s >= 0).all()) and bool((s == torch.round(s)).all())
    assert abs(float(s.mean()) - 4.0) < 0.1 and abs(float(s.var()) - (4.0 + 16.0 / 2.0)) < 0.6


class RecordingLib:
    """Stands where lib.load() stands: every entry that is looked up is recorded and answers with a failure."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def entry(*args):
            self.calls.append(name)
            return -1
        return entry


def _model(kind="svgp", num_outputs=1, D=3, M=5):
    from tgp.pytorch_amd.flows import SAL
    from tgp.pytorch_amd.kernels import instance_kernel
    from tgp.pytorch_amd.likelihoods import NegativeBinomial
    from tgp.pytorch_amd.models import sparse_MF_GP, sparse_MF_SP
    X = torch.randn(30, D, dtype=F64)
    K = instance_kernel("scale_rbf", ard_num_dim=D, num_multioutput=num_outputs, kernel_is_shared=False,
                        init_params={"length_scale": 2.0, "kernel_scale": 2.0, "noisy_variance": 1e-6})
    lik = NegativeBinomial()
    if kind == "svgp":
        return sparse_MF_GP(["zero", K], X, X[:M].clone(), 30, lik, num_outputs, True, False, False, False, False, 0.0), X
    flow = SAL(1) if kind == "tgp" else SAL(1, input_dependent=True, input_dim=D, num_hidden_layers=1, batch_norm=0, dropout=0.5,
                                            hidden_dim=8, hidden_activation="tanh", inference="MC_dropout")
    return sparse_MF_SP(["zero", K], X, X[:M].clone(), 30, lik, num_outputs, True, False, False, False, False,
                        [flow] * num_outputs, "single", 0.0), X


def test_state_names():
    GP = ["Z", "covariance_function.base_kernel.raw_lengthscale", "covariance_function.raw_outputscale",
          "q_U.chol_variational_covar", "q_U.variational_mean"]
    SAL1 = ["G_matrix.0.flow_arr.%d.%s" % (k, ab) for k in range(2) for ab in "ab"]
    for kind, flow in (("svgp", []), ("tgp", SAL1)):
        model, _ = _model(kind)
        want = sorted(flow + GP + ["likelihood.log_dispersion"])
        assert sorted(n for n, _ in model.named_parameters()) == want
        assert sorted(model.state_dict()) == want
        assert [n for n, _ in model.named_buffers()] == []                 # no _bern_lvn: the noise slot is the parameter's
        assert not any("log_var_noise" in n for n in model.state_dict())
        assert model._noise is not None and model._noise.data_ptr() == model.likelihood.log_dispersion.data_ptr()
        assert model._lik_id == L.LIK_NEGBIN


def test_model_refusals(monkeypatch):
    lib = RecordingLib()
    monkeypatch.setattr(L, "load", lambda: lib)
    with pytest.raises(NotImplementedError, match="negative-binomial"):
        _model("idtgp")
    with pytest.raises(NotImplementedError, match="negative-binomial"):
        _model("svgp", num_outputs=2)
    for kind in ("svgp", "tgp"):
        model, X = _model(kind)
        Y = torch.zeros(30, 1, dtype=F64)
        model.set_is_training(False)
        for call in (lambda: model.set_optimal_qu(X, Y), lambda: model.predictive_quantiles(X, [0.5]),
                     lambda: model.predictive_cdf(X, Y)):
            with pytest.raises(NotImplementedError, match="negative-binomial"):
                call()
    assert lib.calls == []


def test_library_refuses_quantile_cdf_and_crps_entries():
    """The quantile, CDF and CRPS entries refuse TGP_LIK_NEGBIN before they read a pointer or touch a device."""
    h = L.load()
    buf = torch.zeros(16, dtype=F64)            # host memory: the refusal comes before any pointer is read
    st = torch.zeros(1, dtype=torch.int32)
    p, ps = ctypes.c_void_p(buf.data_ptr()), ctypes.c_void_p(st.data_ptr())
    md = L.TgpModel()
    md.N, md.D, md.M, md.S, md.lik = 4, 1, 1, 8, L.LIK_NEGBIN
    md.log_var_noise = p
    rc = h.tgp_predict_quantile_f64(md, p, p, None, p, p, 1, p, ps, None)
    assert rc == L.E_UNSUPPORTED and b"TGP_LIK_NEGBIN" in h.tgp_last_error()
    rc = h.tgp_predict_cdf_f64(md, p, p, None, p, p, None, None)
    assert rc == L.E_UNSUPPORTED and b"TGP_LIK_NEGBIN" in h.tgp_last_error()
    rc = h.tgp_predict_crps_f64(md, p, p, None, p, p, None, None)
    assert rc == L.E_UNSUPPORTED and b"lik = 9" in h.tgp_last_error()


def test_engine_refusal_and_surface():
    from tgp.pytorch_amd import ops
    from tgp.pytorch_amd.engine import engine_refusal
    assert "negative-binomial" in engine_refusal(likelihood="negbinomial")
    assert "negative-binomial" in engine_refusal(likelihood="negbinomial", minibatch=True)
    assert "eager path" in engine_refusal(likelihood="negbinomial")
    assert callable(ops.ell_negbin) and callable(ops.EllNegBinFunction.apply)
    lvn = torch.zeros(1, dtype=F64)
    with pytest.raises(L.TgpError, match="negative-binomial"):
        ops.elbo_step(torch.zeros(4, 1, dtype=F64), torch.zeros(4, dtype=F64), torch.zeros(2, 1, dtype=F64), lvn, lvn,
                      torch.zeros(2, dtype=F64), torch.eye(2, dtype=F64), lvn, 4.0, flow=None, lik=L.LIK_NEGBIN)


def test_cli_arguments():
    run = lambda *a: subprocess.run([sys.executable, "-m", "tgp.pytorch_amd.main"] + list(a), cwd=REPO, capture_output=True,
                                    text=True, timeout=120)
    out = run("--help")
    assert out.returncode == 0 and "negbinomial" in out.stdout and "--dispersion_init" in out.stdout
    assert "synthetic_overdispersed" in out.stdout
    tail = ["--train_test_seed_split", "1", "--num_inducing", "5"]
    bad = run("--model", "ID_TGP", "--likelihood", "negbinomial", "--dataset", "synthetic_overdispersed", *tail)
    assert bad.returncode == 2 and "--likelihood negbinomial: SVGP or TGP only" in bad.stderr
    bad = run("--model", "SVGP", "--likelihood", "negbinomial", "--dataset", "synthetic_power", *tail)
    assert bad.returncode == 2 and "count data sets" in bad.stderr and "negbinomial" in bad.stderr
    bad = run("--model", "SVGP", "--likelihood", "negbinomial", "--dispersion_init", "1e4", "--dataset", "synthetic_overdispersed", *tail)
    assert bad.returncode == 2 and "--dispersion_init" in bad.stderr


def test_overdispersed_dataset(monkeypatch):
    from tgp.pytorch_amd import config as cg
    from tgp.pytorch_amd import data, synthetic
    X, Y = synthetic.overdispersed_dataset()
    n, d = synthetic.COUNTS_SHAPE
    assert X.shape == (n, d) and Y.shape == (n, 1) and synthetic.OVERDISPERSED_R == 2.0
    assert np.array_equal(Y, synthetic.overdispersed_dataset(seed=0)[1])                  # seeded
    assert not np.array_equal(Y, synthetic.overdispersed_dataset(seed=1)[1])
    assert np.all(Y >= 0) and np.array_equal(Y, np.round(Y))
    assert np.array_equal(X, synthetic.counts_dataset()[0])                               # the inputs (and log-mean) of synthetic_counts
    # over-dispersed against its own conditional mean: Var[y | x] / E[y | x] = 1 + mean / r, well above 1; also marginally
    mean = np.exp(1.0 + np.sin(2.0 * X[:, 0]) + 0.5 * X[:, 1])
    ratio = float(Y.var() / Y.mean())
    cond = float((((Y[:, 0] - mean) ** 2) / mean).mean())
    print("variance / mean: marginal %.2f, conditional %.2f (Poisson: 1)" % (ratio, cond))
    assert ratio > 1.5 and cond > 1.5
    monkeypatch.setattr(cg, "device", "cpu", raising=False)
    loaders, dc = data.return_dataset("synthetic_overdispersed", 10000, seed=1)
    assert dc["dispersion"] == 2.0 and dc["N_tr"] == 720 and dc["N_te"] == 80 and dc["Dx"] == d and len(loaders) == 2
    assert float(np.asarray(dc["Y_std"]).reshape(-1)[0]) == 1.0
    assert np.array_equal(dc["Y_tr"].numpy(), Y[dc["train_idx"]])                         # raw counts
    from tgp.pytorch_amd import main
    assert "synthetic_overdispersed" in main.COUNT_DATASETS and "synthetic_counts" in main.COUNT_DATASETS
