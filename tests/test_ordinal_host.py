"""CPU: the ordinal (cumulative-probit) likelihood above the kernels -- the ABI constant, the torch restatement
(tests/ordinal_model.py) against the Bernoulli restatement at K = 2 and against its own closed forms, the trait table and the
state names of the likelihood class, what ops.ordinal_noise puts behind the noise pointer and what it refuses, the refusals of
the models (before any library call), of the library's quantile, CDF and CRPS entries (before any launch) and of the CLI, the
engines' refusal and the synthetic_ratings data set."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import REPO

import ordinal_model as OM
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
    assert re.search(r"#define TGP_LIK_ORDINAL 10\b", hdr)
    assert "{eta = log sigma^2, K, b_1, .., b_{K-1}}" in hdr
    assert L.LIK_ORDINAL == 10 and L.ORDINAL_MAX_K == 64
    assert L.LIK_DISPLAY[L.LIK_ORDINAL] == "ordinal"


def test_restatement_at_two_classes_is_bernoulli():
    """K = 2, edge 0, sigma = 1: class 1 has probability Phi(g), class 0 Phi(-g) -- the Bernoulli restatement's log-probabilities."""
    g = torch.Generator().manual_seed(3)
    x = torch.cat((4.0 * torch.randn(2000, generator=g, dtype=F64), torch.tensor([0.0, 37.0, -37.0, 160.0, -160.0], dtype=F64)))
    y = (torch.rand(x.numel(), generator=g) < 0.5).to(F64)
    lp = OM.log_p(x, y, torch.zeros(1, dtype=F64), torch.zeros(1, dtype=F64))
    bern = y * torch.special.log_ndtr(x) + (1.0 - y) * torch.special.log_ndtr(-x)
    err = float(((lp - bern).abs() / bern.abs().clamp(min=1.0)).max())
    print("K = 2 against the Bernoulli log-probabilities: %.3e" % err)
    assert err <= 1e-14


def test_restatement_sums_to_one_and_has_finite_gradients():
    """Over the classes exp(log p) sums to 1; the closed predictive of the empty program is the difference of its CDF; autograd is
    finite at the classes with an infinite edge (no arithmetic on the infinity)."""
    K = 5
    edges = OM.default_edges(K)
    assert edges.tolist() == [-1.5, -0.5, 0.5, 1.5]
    lvn = torch.tensor([np.log(0.07)], dtype=F64)
    assert OM.min_bin_width(lvn, edges) >= OM.MIN_WIDTH
    g = 2.0 * torch.randn(300, generator=torch.Generator().manual_seed(0), dtype=F64)
    tot = sum(torch.exp(OM.log_p(g, torch.full_like(g, float(k)), lvn, edges)) for k in range(K))
    assert float((tot - 1.0).abs().max()) <= 1e-13
    v = 0.3 * torch.rand(300, generator=torch.Generator().manual_seed(1), dtype=F64)
    pmf = OM.pmf_closed(g, v, lvn, edges)
    for k in range(K):
        _, _, lp = OM.pred_torch(g, v, lvn, edges, [], None, None, None, Y=torch.full_like(g, float(k)))
        assert float((torch.exp(lp) - pmf[:, k]).abs().max()) <= 1e-13
    m1, m2, _ = OM.pred_torch(g, v, lvn, edges, [], None, None, None)
    kk = torch.arange(K, dtype=F64)
    assert float((m1 - (pmf * kk).sum(1)).abs().max()) <= 1e-12
    assert float((m2 - ((pmf * kk * kk).sum(1) - m1 * m1)).abs().max()) <= 1e-12
    gg, ll = g.clone().requires_grad_(True), lvn.clone().requires_grad_(True)
    y = torch.randint(0, K, (300,), generator=torch.Generator().manual_seed(2)).to(F64)
    a, b = torch.autograd.grad(OM.log_p(gg, y, ll, edges).sum(), [gg, ll])
    assert torch.isfinite(a).all() and torch.isfinite(b).all()
    # d log p / dg and d log p / d eta as the header states them, at a point of every class
    sig = float(torch.exp(0.5 * lvn))
    for k in range(K):
        g1, l1 = torch.tensor([0.3], dtype=F64, requires_grad=True), lvn.clone().requires_grad_(True)
        dg, de = torch.autograd.grad(OM.log_p(g1, torch.tensor([float(k)]), l1, edges).sum(), [g1, l1])
        lo = -np.inf if k == 0 else (float(edges[k - 1]) - 0.3) / sig
        hi = np.inf if k == K - 1 else (float(edges[k]) - 0.3) / sig
        Phi = lambda z: float(torch.exp(torch.special.log_ndtr(torch.tensor(z, dtype=F64))))   # (ndtr is 1 + erf: no tail)
        phi = lambda z: 0.0 if np.isinf(z) else float(np.exp(-0.5 * z * z) / np.sqrt(2.0 * np.pi))
        zphi = lambda z: 0.0 if np.isinf(z) else z * phi(z)
        p = Phi(hi) - Phi(lo)
        assert abs(float(dg) - (phi(lo) - phi(hi)) / (sig * p)) <= 1e-9 * max(1.0, abs(float(dg)))
        assert abs(float(de) - (zphi(lo) - zphi(hi)) / (2.0 * p)) <= 1e-9 * max(1.0, abs(float(de)))


def test_trait_table():
    from tgp.pytorch_amd import config as cg
    from tgp.pytorch_amd import likelihoods as LK
    base = LK.Likelihood
    lik = LK.Ordinal(5)
    traits = [n for n in vars(base) if not n.startswith("_") and not callable(getattr(base, n))
              and not isinstance(vars(base)[n], (staticmethod, classmethod))]
    assert "display" in traits and "refuses_cdf" in traits and "num_latent" in traits
    names = {n for n, _ in lik.named_parameters()} | {n for n, _ in lik.named_buffers()}
    for n in traits:
        getattr(lik, n)                                  # every trait is defined
        assert n not in names                            # ... and none is a parameter or a buffer
    assert lik.display == "ordinal" and lik.lik_id == L.LIK_ORDINAL == 10 and lik.engine_name == "ordinal"
    assert lik.kind == "count" and lik.has_noise is True and lik.has_flow is True and lik.one_launch_logp is True
    assert lik.flow_on_targets is False and lik.compiles_flows is False
    assert lik.num_latent == 1 and lik.composed is False
    assert lik.refuses_input_dependent == LK.NO_INPUT_DEPENDENT % "ordinal"
    assert lik.refuses_optimal_qu == LK.NOT_GAUSSIAN_IN_F % "ordinal" and lik.refuses_optimal_qu_id is None
    assert lik.refuses_cdf.count("%s") == 1 and "predictive_pmf" in lik.refuses_cdf and "ordinal" in lik.refuses_cdf
    assert lik.refuses_crps is None and lik.refuses_mean is None and lik.refuses_paths is None and lik.refuses_full_cov is None
    assert "ordinal" in lik.outputs_refusal and "one output" in lik.outputs_refusal
    # one parameter under the Gaussian classes' name and shape; the edges are a buffer no optimiser sees
    assert [n for n, _ in lik.named_parameters()] == ["log_var_noise"] and lik.log_var_noise.shape == (1, 1)
    assert [n for n, _ in lik.named_buffers()] == ["bin_edges"] and not lik.bin_edges.requires_grad
    assert sorted(lik.state_dict()) == ["bin_edges", "log_var_noise"]
    assert lik.num_classes == 5 and lik.bin_edges.tolist() == [-1.5, -0.5, 0.5, 1.5] and lik.quad_points == cg.quad_points
    assert float(lik.log_var_noise.detach()) == 0.0 and lik.noise().shape == (1,) and lik.noise().requires_grad
    assert abs(float(LK.Ordinal(3, noise_init=0.07).log_var_noise.detach()) - np.log(0.07)) < 1e-15
    kw = lik.lik_kwargs()
    assert set(kw) == {"lik", "df"} and kw["lik"] == L.LIK_ORDINAL and kw["df"] is lik.bin_edges
    assert LK.Ordinal(4, bin_edges=[-1.0, 0.5, 0.7]).bin_edges.tolist() == [-1.0, 0.5, 0.7]
    assert LK.Ordinal(2).bin_edges.tolist() == [0.0] and LK.Ordinal(64).bin_edges.numel() == 63


def test_constructor_and_ordinal_noise_refuse_bad_edges():
    from tgp.pytorch_amd import likelihoods as LK
    from tgp.pytorch_amd import ops
    lvn = torch.tensor([[np.log(0.5)]], dtype=F64)
    packed = ops.ordinal_noise(lvn, [-1.0, 0.25, 2.0])
    assert packed.dtype == F64 and packed.tolist() == [float(np.log(0.5)), 4.0, -1.0, 0.25, 2.0] and not packed.requires_grad
    assert ops.noise_slot(lvn, L.LIK_ORDINAL, torch.tensor([0.0], dtype=F64)).tolist() == [float(np.log(0.5)), 2.0, 0.0]
    # student_noise keeps its name and behaviour, and is the slot's Student-t case; the other ids carry nothing beside the noise
    assert ops.student_noise(lvn, 4.0).tolist() == ops.noise_slot(lvn, L.LIK_STUDENT, 4.0).tolist() == [float(np.log(0.5)), 4.0]
    assert ops.noise_slot(lvn, L.LIK_NEGBIN, None) is lvn and ops.noise_slot(lvn, None, None) is lvn
    inf, nan = float("inf"), float("nan")
    for bad, what in (([0.0, -1.0], "increasing"), ([0.0, 0.0], "increasing"), ([0.0, inf], "finite"), ([nan, 1.0], "finite"),
                      ([-inf, 0.0], "finite"), ([], "bin edges"), (list(range(64)), "bin edges")):
        with pytest.raises(ValueError, match=what):
            ops.ordinal_noise(lvn, bad)
        with pytest.raises(ValueError):
            LK.Ordinal(len(bad) + 1, bin_edges=bad)
    ops.ordinal_noise(lvn, list(range(63)))              # K = 64: the largest
    for K in (1, 65, 0, 2.5):
        with pytest.raises(ValueError, match="num_classes"):
            LK.Ordinal(K)
    with pytest.raises(ValueError, match="4 bin edges"):      # a count of edges that is not K - 1
        LK.Ordinal(5, bin_edges=[0.0, 1.0, 2.0])
    with pytest.raises(ValueError, match="noise"):
        LK.Ordinal(5, noise_init=0.0)
    with pytest.raises(L.TgpError, match="bin edges"):
        ops.ordinal_noise(lvn, None)


def test_check_targets_and_samples():
    from tgp.pytorch_amd import likelihoods as LK
    lik = LK.Ordinal(5)
    lik.check_targets(torch.tensor([[0.0], [4.0], [2.0]], dtype=F64))
    for bad in (2.5, -1.0, 5.0, float("nan")):
        with pytest.raises(ValueError, match=r"integer in \[0, 4\]"):
            lik.check_targets(torch.tensor([[1.0], [bad]], dtype=F64))
    # draws: the number of edges below f + sigma eps -- classes, with the cumulative-probit frequencies
    torch.manual_seed(0)
    f = torch.full((1, 40000), 0.3, dtype=F64)
    s = lik.sample_from_output(f, 0)
    assert s.shape == f.shape and bool((s >= 0).all()) and bool((s <= 4).all()) and bool((s == torch.round(s)).all())
    pmf = OM.pmf_closed(torch.tensor([0.3], dtype=F64), torch.zeros(1, dtype=F64), torch.zeros(1, dtype=F64), lik.bin_edges)[0]
    freq = torch.bincount(s.reshape(-1).long(), minlength=5).to(F64) / s.numel()
    assert float((freq - pmf).abs().max()) < 0.01


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
    from tgp.pytorch_amd.likelihoods import Ordinal
    from tgp.pytorch_amd.models import sparse_MF_GP, sparse_MF_SP
    X = torch.randn(30, D, dtype=F64)
    K = instance_kernel("scale_rbf", ard_num_dim=D, num_multioutput=num_outputs, kernel_is_shared=False,
                        init_params={"length_scale": 2.0, "kernel_scale": 2.0, "noisy_variance": 1e-6})
    lik = Ordinal(5)
    if kind == "svgp":
        return sparse_MF_GP(["zero", K], X, X[:M].clone(), 30, lik, num_outputs, True, False, False, False, False, 0.0), X
    flow = SAL(1) if kind == "tgp" else SAL(1, input_dependent=True, input_dim=D, num_hidden_layers=1, batch_norm=0, dropout=0.5,
                                            hidden_dim=8, hidden_activation="tanh", inference="MC_dropout")
    return sparse_MF_SP(["zero", K], X, X[:M].clone(), 30, lik, num_outputs, True, False, False, False, False,
                        [flow] * num_outputs, "single", 0.0), X


def test_state_names():
    """The Gaussian models' names plus the buffer of the edges."""
    GP = ["Z", "covariance_function.base_kernel.raw_lengthscale", "covariance_function.raw_outputscale",
          "q_U.chol_variational_covar", "q_U.variational_mean", "likelihood.log_var_noise"]
    SAL1 = ["G_matrix.0.flow_arr.%d.%s" % (k, ab) for k in range(2) for ab in "ab"]
    for kind, flow in (("svgp", []), ("tgp", SAL1)):
        model, _ = _model(kind)
        assert sorted(n for n, _ in model.named_parameters()) == sorted(flow + GP)
        assert sorted(model.state_dict()) == sorted(flow + GP + ["likelihood.bin_edges"])
        assert [n for n, _ in model.named_buffers()] == ["likelihood.bin_edges"]
        assert model._noise is not None and model._noise.data_ptr() == model.likelihood.log_var_noise.data_ptr()
        assert model._lik_id == L.LIK_ORDINAL
        assert set(model.likelihood.lik_kwargs()) == {"lik", "df"}


def test_model_refusals(monkeypatch):
    lib = RecordingLib()
    monkeypatch.setattr(L, "load", lambda: lib)
    with pytest.raises(NotImplementedError, match="ordinal"):
        _model("idtgp")
    with pytest.raises(NotImplementedError, match="ordinal"):
        _model("svgp", num_outputs=2)
    for kind in ("svgp", "tgp"):
        model, X = _model(kind)
        Y = torch.zeros(30, 1, dtype=F64)
        model.set_is_training(False)
        for call in (lambda: model.set_optimal_qu(X, Y), lambda: model.predictive_quantiles(X, [0.5]),
                     lambda: model.predictive_cdf(X, Y)):
            with pytest.raises(NotImplementedError, match="ordinal"):
                call()
    assert lib.calls == []


def test_library_refuses_quantile_cdf_and_crps_entries():
    """The quantile, CDF and CRPS entries refuse TGP_LIK_ORDINAL before they read a pointer or touch a device."""
    h = L.load()
    buf = torch.zeros(16, dtype=F64)            # host memory: the refusal comes before any pointer is read
    st = torch.zeros(1, dtype=torch.int32)
    p, ps = ctypes.c_void_p(buf.data_ptr()), ctypes.c_void_p(st.data_ptr())
    md = L.TgpModel()
    md.N, md.D, md.M, md.S, md.lik = 4, 1, 1, 8, L.LIK_ORDINAL
    md.log_var_noise = p
    rc = h.tgp_predict_quantile_f64(md, p, p, None, p, p, 1, p, ps, None)
    assert rc == L.E_UNSUPPORTED and b"TGP_LIK_ORDINAL" in h.tgp_last_error() and b"discrete" in h.tgp_last_error()
    rc = h.tgp_predict_cdf_f64(md, p, p, None, p, p, None, None)
    assert rc == L.E_UNSUPPORTED and b"TGP_LIK_ORDINAL" in h.tgp_last_error()
    rc = h.tgp_predict_crps_f64(md, p, p, None, p, p, None, None)
    assert rc == L.E_UNSUPPORTED and b"lik = 10" in h.tgp_last_error()


def test_engine_refusal_and_surface():
    from tgp.pytorch_amd import ops
    from tgp.pytorch_amd.engine import engine_refusal
    assert engine_refusal(likelihood="ordinal") == engine_refusal(likelihood="poisson").replace("Poisson", "ordinal")
    assert "ordinal" in engine_refusal(likelihood="ordinal", minibatch=True) and "eager path" in engine_refusal(likelihood="ordinal")
    assert callable(ops.ell_ordinal) and callable(ops.EllOrdinalFunction.apply)
    lvn = torch.zeros(1, dtype=F64)
    with pytest.raises(L.TgpError, match="ordinal"):
        ops.elbo_step(torch.zeros(4, 1, dtype=F64), torch.zeros(4, dtype=F64), torch.zeros(2, 1, dtype=F64), lvn, lvn,
                      torch.zeros(2, dtype=F64), torch.eye(2, dtype=F64), lvn, 4.0, flow=None, lik=L.LIK_ORDINAL, df=[0.0])
    with pytest.raises(L.TgpError, match="ordinal"):
        ops.predict(torch.zeros(4, dtype=F64), torch.ones(4, dtype=F64), lvn, None, lik=L.LIK_ORDINAL, df=[0.0])


def test_cli_arguments():
    run = lambda *a: subprocess.run([sys.executable, "-m", "tgp.pytorch_amd.main"] + list(a), cwd=REPO, capture_output=True,
                                    text=True, timeout=120)
    out = run("--help")
    assert out.returncode == 0 and "ordinal" in out.stdout and "synthetic_ratings" in out.stdout
    tail = ["--train_test_seed_split", "1", "--num_inducing", "5"]
    bad = run("--model", "ID_TGP", "--likelihood", "ordinal", "--dataset", "synthetic_ratings", *tail)
    assert bad.returncode == 2 and "--likelihood ordinal: SVGP or TGP only" in bad.stderr
    bad = run("--model", "WGP", "--likelihood", "ordinal", "--dataset", "synthetic_ratings", *tail)
    assert bad.returncode == 2 and "--likelihood ordinal: SVGP or TGP only" in bad.stderr
    bad = run("--model", "SVGP", "--likelihood", "ordinal", "--dataset", "synthetic_counts", *tail)
    assert bad.returncode == 2 and "ordinal data sets" in bad.stderr and "synthetic_ratings" in bad.stderr
    for other in ("gaussian", "poisson", "multiclass"):     # ... and the other way round
        bad = run("--model", "SVGP", "--likelihood", other, "--dataset", "synthetic_ratings", *tail)
        assert bad.returncode == 2 and "ordinal data sets" in bad.stderr
    bad = run("--model", "SVGP", "--likelihood", "ordinal", "--qu", "optimal", "--dataset", "synthetic_ratings", *tail)
    assert bad.returncode == 2 and "--qu optimal" in bad.stderr


def test_ratings_dataset(monkeypatch):
    from tgp.pytorch_amd import config as cg
    from tgp.pytorch_amd import data, synthetic
    X, Y = synthetic.synthetic_ratings()
    n, d = synthetic.RATINGS_SHAPE
    assert X.shape == (n, d) and Y.shape == (n, 1) and synthetic.RATINGS_CLASSES == 5
    assert synthetic.RATINGS_CUTS == (-1.0, -0.6, 0.3, 1.2)
    assert np.array_equal(Y, synthetic.synthetic_ratings(seed=0)[1])                  # seeded
    assert not np.array_equal(Y, synthetic.synthetic_ratings(seed=1)[1])
    assert np.array_equal(Y, np.round(Y)) and Y.min() == 0 and Y.max() == 4
    # the classes follow the latent: the noiseless cut of h agrees with most of them, and the mean class rises with h
    h = np.sin(2.0 * X[:, 0]) + 0.5 * X[:, 1]
    clean = (h.reshape(-1, 1) > np.asarray(synthetic.RATINGS_CUTS).reshape(1, -1)).sum(1)
    agree = float((clean == Y[:, 0]).mean())
    print("share of the classes that the noiseless latent gives: %.3f" % agree)
    assert agree > 0.5 and np.corrcoef(h, Y[:, 0])[0, 1] > 0.8
    monkeypatch.setattr(cg, "device", "cpu", raising=False)
    loaders, dc = data.return_dataset("synthetic_ratings", 10000, seed=1)
    assert dc["num_classes"] == 5 and dc["N_tr"] == 720 and dc["N_te"] == 80 and dc["Dx"] == d and len(loaders) == 2
    assert float(np.asarray(dc["Y_std"]).reshape(-1)[0]) == 1.0
    assert np.array_equal(dc["Y_tr"].numpy(), Y[dc["train_idx"]])                     # the raw classes, not standardised
    assert sorted(set(dc["Y_tr"].reshape(-1).tolist())) == [0.0, 1.0, 2.0, 3.0, 4.0]  # every class in the training split
    from tgp.pytorch_amd import main
    assert main.ORDINAL_DATASETS == ("synthetic_ratings",) and ("TGP", "ratings") in main.HYPER
