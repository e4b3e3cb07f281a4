"""CPU: the Poisson likelihood above the kernels -- the ABI constants, the torch restatement (tests/poisson_model.py)
against the closed form of the identity link, the likelihood class, the synthetic count data set, the engines' refusal and
the CLI flag."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import REPO, rel_err

import poisson_model as PM
from tgp.pytorch_amd import lib as L

F64 = torch.float64


def test_abi_constants():
    hdr = open(os.path.join(REPO, "include", "tgp_hip.h")).read()
    assert re.search(r"#define TGP_LIK_POISSON 6\b", hdr)
    assert re.search(r"#define TGP_VERSION 104\b", hdr)
    assert L.LIK_POISSON == 6
    assert L.load().tgp_version() == 104


@pytest.mark.parametrize("S", [20, 16])
def test_restatement_matches_closed_form(S):
    """Identity link: E_q[y f - exp(f)] = y mu - exp(mu + v / 2), which Gauss-Hermite reproduces to rounding at these v."""
    g = torch.Generator().manual_seed(1)
    mu = 0.8 * torch.randn(1000, generator=g, dtype=F64)
    v = 0.5 * torch.rand(1000, generator=g, dtype=F64)
    Y = torch.poisson(torch.exp(mu), generator=g)
    xs, ws = (torch.tensor(a) for a in np.polynomial.hermite.hermgauss(S))
    assert PM.max_log_rate(mu, v, [], None, xs, ws) <= PM.GMAX
    ell = PM.ell_torch(Y, mu, v, [], None, xs, ws)
    closed = (Y * mu - torch.exp(mu + 0.5 * v) - torch.lgamma(Y + 1.0)).sum()
    assert rel_err(ell, closed) <= 1e-12
    m1, m2, lp = PM.pred_torch(mu, v, [], None, xs, ws, Y=Y)
    wn = (ws / np.sqrt(np.pi)).reshape(-1, 1)
    gq = mu.reshape(1, -1) + torch.sqrt(2.0 * v).reshape(1, -1) * xs.reshape(-1, 1)
    assert rel_err((wn * torch.exp(gq)).sum(0), m1) <= 1e-12
    assert torch.isfinite(lp).all() and bool((lp < 0).all())


def test_poisson_class_api():
    from tgp.pytorch_amd import config as cg
    from tgp.pytorch_amd import likelihoods
    lik = likelihoods.Poisson()
    assert lik.quad_points == cg.quad_points
    assert list(lik.parameters()) == [] and list(lik.named_parameters()) == []
    for m in ("expected_log_prob", "marginal_moments", "sample_from_output"):
        assert callable(getattr(lik, m))
    s = lik.sample_from_output(torch.tensor([[-50.0], [-50.0]], dtype=F64), 0)
    assert s.reshape(-1).tolist() == [0.0, 0.0]
    s = lik.sample_from_output(torch.full((1, 2000), 1.5, dtype=F64), 0)
    assert bool((s == torch.round(s)).all()) and abs(float(s.mean()) - float(np.exp(1.5))) < 0.3
    mean, cov, X = torch.zeros(1, 3, dtype=F64), torch.ones(1, 3, dtype=F64), torch.zeros(1, 3, 2, dtype=F64)
    for bad in ([[1.0, -1.0, 0.0]], [[0.5, 1.0, 2.0]], [[float("nan"), 1.0, 2.0]]):
        with pytest.raises(ValueError, match="counts"):
            lik.expected_log_prob(torch.tensor(bad, dtype=F64), mean, cov, flow=[None], X=X)


def test_counts_dataset():
    from tgp.pytorch_amd import synthetic
    X, Y = synthetic.counts_dataset()
    X2, Y2 = synthetic.counts_dataset(seed=0)
    assert X.shape == (800, 2) and Y.shape == (800, 1) and X.dtype == np.float64 and Y.dtype == np.float64
    assert np.array_equal(X, X2) and np.array_equal(Y, Y2)
    assert np.all(Y >= 0) and np.array_equal(Y, np.round(Y))
    rng = np.random.default_rng(0)
    Xr = rng.standard_normal((800, 2))
    assert np.array_equal(X, Xr)
    assert np.array_equal(Y[:, 0], rng.poisson(np.exp(1.0 + np.sin(2.0 * Xr[:, 0]) + 0.5 * Xr[:, 1])).astype(np.float64))
    assert not np.array_equal(Y, synthetic.counts_dataset(seed=1)[1])


def test_return_dataset_counts(monkeypatch):
    from tgp.pytorch_amd import config as cg
    from tgp.pytorch_amd import data
    monkeypatch.setattr(cg, "device", "cpu", raising=False)
    loaders, dc = data.return_dataset("synthetic_counts", 10000, seed=1)
    assert dc["N_tr"] + dc["N_te"] == 800 and dc["Dx"] == 2
    assert np.allclose(np.asarray(dc["Y_std"]), 1.0) and np.allclose(np.asarray(dc["Y_mean"]), 0.0)
    Y = torch.cat([dc["Y_tr"].reshape(-1), dc["Y_te"].reshape(-1)])
    assert bool((Y >= 0).all()) and bool((Y == torch.round(Y)).all())
    assert torch.allclose(dc["X_tr"].mean(0), torch.zeros(2, dtype=dc["X_tr"].dtype), atol=1e-5)
    # the seeded split of the binary sets: the same rows for the same seed
    _, dc2 = data.return_dataset("synthetic_counts", 10000, seed=1)
    assert np.array_equal(dc["train_idx"], dc2["train_idx"])


def test_engine_refusal_and_model_surface():
    from tgp.pytorch_amd import models, ops
    from tgp.pytorch_amd.engine import engine_refusal
    assert "Poisson" in engine_refusal(likelihood="poisson")
    assert "Poisson" in engine_refusal(likelihood="poisson", minibatch=True)
    from tgp.pytorch_amd import likelihoods
    assert likelihoods.Poisson.lik_id == L.LIK_POISSON and likelihoods.Poisson.kind == "count"
    assert hasattr(models.sparse_MF_SP, "predictive_pmf")
    assert callable(ops.ell_poisson) and callable(ops.EllPoissonFunction.apply) and callable(ops.EllBernoulliFunction.apply)


def test_cli_lists_poisson():
    out = subprocess.run([sys.executable, "-m", "tgp.pytorch_amd.main", "--help"], cwd=REPO, capture_output=True,
                         text=True, timeout=120)
    assert out.returncode == 0
    assert "poisson" in out.stdout and "synthetic_counts" in out.stdout
    bad = subprocess.run([sys.executable, "-m", "tgp.pytorch_amd.main", "--model", "ID_TGP", "--likelihood", "poisson",
                          "--dataset", "synthetic_counts", "--train_test_seed_split", "1", "--num_inducing", "5"],
                         cwd=REPO, capture_output=True, text=True, timeout=120)
    assert bad.returncode == 2 and "--likelihood poisson: SVGP or TGP only" in bad.stderr
