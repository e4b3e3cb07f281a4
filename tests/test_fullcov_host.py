"""CPU: the torch restatement of the full-covariance kernels (tests/fullcov_model.py) against the reference's fixtures
(tools/gen_golden_fullcov.py), and the table SAMPLE_CPU the GPU test's joint-sample bound is built on."""
import pytest
import torch

from oracle import tgp_oracle as orc

import fullcov_model as fm

CASES = ("fullcov_tiny_svgp", "fullcov_med_sal2", "fullcov_bigm_matern")
TOL = 1e-10          # what test_oracle_golden.py holds the oracle to
SAMPLE_JITTER = 1e-6

# max |F0(Sigma of the reference) - F0(Sigma of the restatement)| at jitter 1e-6 with the fixture's eps: the two Sigma agree to
# 1e-15 .. 7e-14, and chol(Sigma + 1e-6 I) (smallest eigenvalue of Sigma between -1e-15 and 5e-6) carries that difference into the
# draws.  It is the distance the conditioning of the factorisation alone puts between two correct implementations; computed by
# test_sample_cpu_table below (float64, CPU) and committed.
SAMPLE_CPU = {"fullcov_tiny_svgp": 2.4e-13, "fullcov_med_sal2": 2.1e-10, "fullcov_bigm_matern": 4.0e-11}


def _restated(g):
    p = g["params"]
    return fm.qf_cov(g["X"], p["Z"], p["raw_lengthscale"], p["raw_outputscale"], p["m"], p["Lam"], kernel=g["kernel"])


@pytest.mark.parametrize("name", CASES)
def test_restatement_matches_the_reference(golden, name):
    g = golden(name)
    N = g["X"].shape[0]
    assert g["Sigma"].shape == (N, N) and g["mu"].shape == (N,) and g["eps"].shape == (4, N)
    mu, Sigma = _restated(g)
    assert float((mu - g["mu"]).abs().max()) <= TOL
    assert float((Sigma - g["Sigma"]).abs().max()) <= TOL
    assert torch.equal(Sigma, Sigma.t())


@pytest.mark.parametrize("name", CASES)
def test_diagonal_is_the_marginal_variance(golden, name):
    g = golden(name)
    p = g["params"]
    mu_o, v_o = orc.qf_moments(g["X"], p["Z"], p["raw_lengthscale"], p["raw_outputscale"], p["m"], p["Lam"], kernel=g["kernel"])
    mu, Sigma = _restated(g)
    assert float((Sigma.diagonal() - v_o).abs().max()) <= TOL
    assert float((mu - mu_o).abs().max()) <= TOL
    assert float((g["Sigma"].diagonal() - v_o).abs().max()) <= TOL


@pytest.mark.parametrize("name", CASES)
def test_sample_cpu_table(golden, name):
    """The committed figure is what this computes, to the rounding of another host's LAPACK (a factor 10)."""
    g = golden(name)
    mu, Sigma = _restated(g)
    Fa, La = fm.joint_draw(g["mu"], g["Sigma"], g["eps"], SAMPLE_JITTER)
    Fb, _ = fm.joint_draw(mu, Sigma, g["eps"], SAMPLE_JITTER)
    d = float((Fa - Fb).abs().max())
    print("%s: max |F0(reference Sigma) - F0(restated Sigma)| = %.3e (table %.1e)" % (name, d, SAMPLE_CPU[name]))
    assert d <= 10.0 * SAMPLE_CPU[name]
    # the draw itself: L L^T reproduces Sigma + jitter I
    N = Sigma.shape[0]
    assert float((La @ La.t() - g["Sigma"] - SAMPLE_JITTER * torch.eye(N, dtype=torch.float64)).abs().max()) <= 1e-12


def test_jitter_ladder_is_exercised(golden):
    """The smallest eigenvalue of the fixtures' Sigma reaches rounding level: a plain factorisation may fail, the ladder's
    first rungs (1e-8 .. 1e-6) may not."""
    lo = min(float(torch.linalg.eigvalsh(golden(n)["Sigma"]).min()) for n in CASES)
    assert lo < 1e-12
    for n in CASES:
        S = golden(n)["Sigma"]
        _, info = torch.linalg.cholesky_ex(S + 1e-6 * torch.eye(S.shape[0], dtype=torch.float64))
        assert int(info) == 0
