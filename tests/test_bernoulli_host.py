"""CPU: the Bernoulli (probit) likelihood above the kernels -- the formula the kernels implement, restated in torch
(log_ndtr, autograd through the flow formulas) against the reference's own numbers (tests/golden/bern_*.npz, written by
tools/gen_golden_bernoulli.py), the likelihood class, the ABI constants, the binary synthetic data sets and the CLI flag.
`flow_torch` / `ell_torch` / `pred_torch` are also the autograd oracle of tests/test_gpu_bernoulli.py."""
import glob
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, REPO

from tgp.pytorch_amd import lib as L

F64 = torch.float64


def _sp(x):
    return torch.nn.functional.softplus(x)


def flow_torch(f, program, theta, rowp=None):
    """G(f) of a flow program (include/tgp_hip.h), f (S, N); theta raw shared values, rowp (N, RP) raw per-row values."""
    g = f
    for kind, K, poff, flags in (tuple(int(v) for v in b) for b in program):
        res, add0 = flags & L.FLAG_RESTRICT, flags & L.FLAG_ADD_F0
        if flags & L.FLAG_PER_ROW:
            prm = [rowp[:, poff + j] for j in range(2)]
        else:
            prm = [theta[poff + j] for j in range(4 if kind == L.FLOW_ARCSINH else (1 if kind >= L.FLOW_BOXCOX else 2))]
        x = g
        if kind == L.FLOW_AFFINE:
            a, b = prm
            y = (_sp(a) if res else a) * x + b
        elif kind == L.FLOW_SAL:
            a, b = prm
            b = _sp(b) if res else b
            y = torch.sinh(b * torch.log(x + torch.sqrt(x * x + 1.0)) - a)
        elif kind == L.FLOW_ARCSINH:
            a, b, c, d = prm
            if res:
                b, d = _sp(b), _sp(d)
            z = (x - c) / d
            y = a + b * torch.log(z + torch.sqrt(z * z + 1.0))
        elif kind == L.FLOW_BOXCOX:
            lam = prm[0]
            lam = torch.where(lam == 0, torch.full_like(lam, 1e-11), lam)
            y = (torch.sign(x) * torch.abs(x) ** lam - 1.0) / lam
        elif kind == L.FLOW_INV_BOXCOX:
            lam = prm[0]
            w = lam * x + 1.0
            y = torch.sign(w) * torch.abs(w) ** (1.0 / lam)
        else:
            raise ValueError(kind)
        g = y + x if add0 else y
    return g


def ell_torch(Y, mu, v, program, theta, xs, ws, rowp=None, scale=1.0):
    """scale * sum_n sum_s w_s [y log Phi(g) + (1 - y) log Phi(-g)], g = G(mu + sqrt(2 max(v, 0)) x_s)."""
    f0 = mu.reshape(1, -1) + torch.sqrt(2.0 * v.clamp(min=0.0)).reshape(1, -1) * xs.reshape(-1, 1)
    g = flow_torch(f0, program, theta, rowp)
    y = Y.reshape(1, -1)
    t = y * torch.special.log_ndtr(g) + (1.0 - y) * torch.special.log_ndtr(-g)
    return scale * (t * (ws / math.sqrt(math.pi)).reshape(-1, 1)).sum()


def pred_torch(mu, v, program, theta, xs, ws, rowp=None):
    """P(y = 1): Phi(mu / sqrt(1 + v)) for the empty program, else the per-row quadrature clamped to [0, 1]."""
    if len(program) == 0:
        return torch.special.ndtr(mu / torch.sqrt(1.0 + v))
    f0 = mu.reshape(1, -1) + torch.sqrt(2.0 * v.clamp(min=0.0)).reshape(1, -1) * xs.reshape(-1, 1)
    g = flow_torch(f0, program, theta, rowp)
    return (torch.special.ndtr(g) * (ws / math.sqrt(math.pi)).reshape(-1, 1)).sum(0).clamp(0.0, 1.0)


def load(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    return {k: (torch.tensor(z[k]) if z[k].dtype != np.int32 else z[k]) for k in z.files}


def rel(a, b):
    a, b = torch.as_tensor(a, dtype=F64), torch.as_tensor(b, dtype=F64)
    return float((a - b).abs().max() / (b.abs().max() + 1e-300))


STEP0 = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, "bern_*.npz")) if "adam5" not in p)


def test_fixture_set():
    assert len(STEP0) >= 7
    sizes = [os.path.getsize(p) for p in glob.glob(os.path.join(GOLDEN, "bern_*.npz"))]
    assert max(sizes) <= 300 * 1024 and sum(sizes) <= 1536 * 1024


@pytest.mark.parametrize("name", STEP0)
def test_torch_restatement_matches_reference(name):
    """ELL and its flow-parameter gradients from log_ndtr + autograd equal the reference's (BCELoss on Phi) within 1e-10."""
    z = load(name)
    assert float(z["gmax"]) <= 6.0
    theta = z["p_theta"].clone().requires_grad_(True) if "p_theta" in z else None
    rowp = z["rowp"].clone().requires_grad_(True) if "rowp" in z else None
    scale = float(z["N_total"]) / z["X"].shape[0]
    ell = ell_torch(z["Y"], z["mu"], z["v"], z["program"], theta, z["xs"], z["ws"], rowp, scale)
    assert rel(ell.detach(), z["ELL"]) < 1e-10
    wrt = [t for t in (theta, rowp) if t is not None]
    if wrt:
        grads = torch.autograd.grad(ell, wrt)
        if theta is not None:
            assert rel(grads[0], z["g_theta"]) < 1e-10
        if rowp is not None:
            assert rel(grads[-1], z["g_rowp"]) < 1e-10
    if "pred_P" in z:
        P = pred_torch(z["mu"], z["v"], z["program"], z.get("p_theta"), z["xs"], z["ws"])
        assert rel(P, z["pred_P"]) < 1e-12
        y = z["Y"].reshape(-1)
        lp = (y * torch.log(P) + (1 - y) * torch.log1p(-P)).sum()
        assert rel(lp, z["test_logp_sum"]) < 1e-12


def test_saturated_tail_is_exact():
    """|g| = 40: log Phi(-40) is about -804.6 (the reference's BCELoss clamps it at -100); the restatement keeps it."""
    xs, ws = (torch.tensor(a) for a in np.polynomial.hermite.hermgauss(8))
    mu = torch.tensor([40.0, -40.0], dtype=F64)
    v = torch.zeros(2, dtype=F64)
    ell = ell_torch(torch.tensor([0.0, 1.0], dtype=F64), mu, v, [], None, xs, ws)
    assert abs(float(ell) - 2 * float(torch.special.log_ndtr(torch.tensor(-40.0, dtype=F64)))) < 1e-9
    assert float(ell) < -1600


def test_bernoulli_class_api():
    from tgp.pytorch_amd import config as cg
    from tgp.pytorch_amd import likelihoods
    lik = likelihoods.Bernoulli()
    assert lik.C == 2 and lik.quad_points == cg.quad_points
    assert list(lik.parameters()) == [] and list(lik.named_parameters()) == []
    for m in ("expected_log_prob", "marginal_moments", "sample_from_output"):
        assert callable(getattr(lik, m))
    torch.manual_seed(0)
    s = lik.sample_from_output(torch.tensor([[-50.0], [50.0]], dtype=F64), 0)
    assert s.reshape(-1).tolist() == [0.0, 1.0]


def test_abi_constants():
    hdr = open(os.path.join(REPO, "include", "tgp_hip.h")).read()
    assert re.search(r"#define TGP_LIK_BERNOULLI 3\b", hdr)
    assert L.LIK_BERNOULLI == 3
    assert "tgp_workspace_bytes_lik" in L.EXPORTS
    assert re.search(r"size_t tgp_workspace_bytes_lik\(", hdr)


def test_trainer_and_model_surface():
    from tgp.pytorch_amd import trainers
    assert issubclass(trainers.Trainer_SP_classification, trainers.Trainer_SP_regression)
    for m in ("compute_metrics", "performance_metrics"):
        assert m in trainers.Trainer_SP_classification.__dict__
    # the resident engine is kept off Bernoulli models by the engines' one statement of coverage, which the inherited
    # _engine_for consults -- not by an override with a list of its own
    from tgp.pytorch_amd.engine import engine_refusal
    assert trainers.Trainer_SP_classification._engine_for is trainers.Trainer_SP_regression._engine_for
    assert "Bernoulli" in engine_refusal(likelihood="bernoulli") and "multi-class" in engine_refusal(likelihood="multiclass")


@pytest.mark.parametrize("name,shape", [("heart", (299, 12)), ("banknote", (1372, 4))])
def test_synthetic_binary_datasets(name, shape):
    from tgp.pytorch_amd import synthetic
    X, Y = synthetic.binary_dataset(name)
    X2, Y2 = synthetic.binary_dataset(name)
    assert X.shape == shape and Y.shape == (shape[0], 1)
    assert np.array_equal(X, X2) and np.array_equal(Y, Y2)
    assert set(np.unique(Y).tolist()) == {0.0, 1.0}
    assert 0.3 < Y.mean() < 0.7


def test_return_dataset_binary(monkeypatch):
    from tgp.pytorch_amd import config as cg
    from tgp.pytorch_amd import data
    monkeypatch.setattr(cg, "device", "cpu", raising=False)
    loaders, dc = data.return_dataset("synthetic_banknote", 10000, seed=1)
    assert dc["N_tr"] + dc["N_te"] == 1372 and dc["Dx"] == 4
    assert np.allclose(np.asarray(dc["Y_std"]), 1.0)
    Y = torch.cat([dc["Y_tr"].reshape(-1), dc["Y_te"].reshape(-1)])
    assert set(Y.unique().tolist()) <= {0.0, 1.0}
    Xtr = dc["X_tr"]
    assert torch.allclose(Xtr.mean(0), torch.zeros(4, dtype=Xtr.dtype), atol=1e-5)


def test_cli_lists_likelihood():
    out = subprocess.run([sys.executable, "-m", "tgp.pytorch_amd.main", "--help"], cwd=REPO, capture_output=True,
                         text=True, timeout=120)
    assert out.returncode == 0
    assert "--likelihood" in out.stdout and "bernoulli" in out.stdout
    bad = subprocess.run([sys.executable, "-m", "tgp.pytorch_amd.main", "--model", "ID_TGP", "--likelihood", "bernoulli",
                          "--dataset", "synthetic_heart", "--train_test_seed_split", "1", "--num_inducing", "5"],
                         cwd=REPO, capture_output=True, text=True, timeout=120)
    assert bad.returncode == 2 and "SVGP or TGP only" in bad.stderr
