"""Multi-class likelihood, host side (no GPU): the torch restatement of the kernels (tests/softmax_model.py) against the
reference fixtures (tools/gen_golden_multiclass.py), the counter-based normal recipe, and the surface the feature adds to the
header, the ctypes binding and the model classes.

Bars: 1e-10 on values and 1e-9 on gradients -- the restatement is the reference's arithmetic in another summation order over
S * N terms, so it gets a decade more than the 1e-11 / 1e-10 an identical order would."""
import math
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import softmax_model as sm          # noqa: E402

from conftest import load_golden     # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ["mc_id3", "mc_sal2x4", "mc_mixed5", "mc_bigm3"]
TOL_VAL, TOL_GRAD = 1e-10, 1e-9
F64 = torch.float64


def rel_err(a, b):
    a, b = torch.as_tensor(a, dtype=F64), torch.as_tensor(b, dtype=F64)
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300)) if b.numel() else 0.0


def programs_of(g):
    bo = [int(b) for b in g["blk_off"]]
    prog = [tuple(r) for r in g["program"]]
    return [prog[bo[c]:bo[c + 1]] for c in range(len(bo) - 1)]


def theta_of(g):
    return g["params"]["theta"].clone().to(F64)


@pytest.mark.parametrize("name", CASES)
def test_restatement_matches_reference(name):
    g = load_golden(name)
    progs, theta = programs_of(g), theta_of(g).requires_grad_(True)
    mu, v = g["mu"].clone().requires_grad_(True), g["v"].clone().requires_grad_(True)
    assert float(g["v"].min()) > 0.0
    ell = sm.ell_softmax_torch(g["Y"], mu, v, g["eps"], progs, theta, g["theta_off"])
    print(name, "ELL", float(ell), "ref", float(g["lik_ELL"]), "rel", rel_err(ell.detach(), g["lik_ELL"]))
    assert rel_err(ell.detach(), g["lik_ELL"]) < TOL_VAL
    ell.backward()
    for mine, key in ((mu.grad, "g_mu"), (v.grad, "g_v"), (theta.grad, "lik_g_theta")):
        if g[key].numel():
            print(name, key, rel_err(mine, g[key]))
            assert rel_err(mine, g[key]) < TOL_GRAD
    # the scaled ELL of the model-level step
    scale = float(g["N_total"]) / g["X"].shape[0]
    with torch.no_grad():
        assert rel_err(sm.ell_softmax_torch(g["Y"], mu, v, g["eps"], progs, theta, g["theta_off"], scale), g["ELL"]) < TOL_VAL
        P, lp = sm.predict_torch(g["pred_mu"], g["pred_v"], g["eps_te"], progs, theta, g["theta_off"], g["Yte"])
    assert rel_err(P, g["pred_P"]) < TOL_VAL
    assert rel_err(lp.sum(), g["pred_logp"]) < TOL_VAL
    assert abs(float(g["ELBO"]) - (float(g["ELL"]) - float(g["KLD"].sum()))) < 1e-12 * abs(float(g["ELBO"]))


def test_fixture_cases_are_what_the_issue_asks():
    g = load_golden("mc_id3")
    assert g["eps"].shape == (16, 3, 200) and g["X"].shape == (200, 3) and g["params"]["Z"].shape == (3, 20, 3)
    assert len(g["program"]) == 0
    g = load_golden("mc_sal2x4")
    assert [r[0] for r in g["program"]].count(1) == 8 and len(g["blk_off"]) == 5
    g = load_golden("mc_mixed5")
    kinds = {int(r[0]) for r in g["program"]}
    assert kinds == {0, 1, 2, 3, 4} and g["adam_eps"].shape[0] == 5
    assert g["params"]["Z"].shape[1] % 16 != 0
    g = load_golden("mc_bigm3")
    Lam = g["params"]["Lam"]
    assert Lam.shape == (3, 160, 160) and float(torch.triu(Lam, 1).abs().max()) == 0.0 and float(Lam[:, 20, 0].abs().max()) == 0.0


# ---- the counter recipe ----------------------------------------------------------------------------------------
def test_hash_fixed_vectors():
    # splitmix64's published first outputs for state 0: fin(k * GOLD), k = 1, 2, 3
    assert sm._fin(sm.GOLD) == 0xE220A8397B1DCDAF
    assert sm._fin((2 * sm.GOLD) & sm.MASK64) == 0x6E789E6AA1B965F4
    assert sm._fin((3 * sm.GOLD) & sm.MASK64) == 0x06C45D188009454F
    # seed 0, step 1, (s, c, row) = 0: x = GOLD, so h1 is the first vector and h2 = fin(h1 + GOLD)
    h1, h2 = sm.mc_hash(0, 1, 0, 0, 0)
    assert h1 == 0xE220A8397B1DCDAF and h2 == sm._fin((0xE220A8397B1DCDAF + sm.GOLD) & sm.MASK64)
    # the packing: s in bits 56-63, c in bits 48-55, the row below
    assert sm.mc_hash(0, 0, 3, 5, 7)[0] == sm._fin((3 << 56) | (5 << 48) | 7)
    u1 = float((h1 >> 11) + 1) * 2.0 ** -53
    assert sm.mc_normal(0, 1, 0, 0, 0) == math.sqrt(-2.0 * math.log(u1)) * math.cos(6.283185307179586 * float(h2 >> 11) * 2.0 ** -53)


def test_draws_look_standard_normal():
    n = 10 ** 6
    z = sm.mc_normals_np(n, seed=12345, step=3)
    assert abs(float(z[17]) - sm.mc_normal(12345, 3, 0, 0, 17)) < 1e-15      # the vectorised form is the same recipe
    # N(0,1): mean 0 (se 1/sqrt n), variance 1 (se sqrt(2/n)), P(|z| > 3) = erfc(3/sqrt 2) (binomial se)
    p3 = math.erfc(3.0 / math.sqrt(2.0))
    assert abs(z.mean()) < 5.0 / math.sqrt(n)
    assert abs(z.var() - 1.0) < 5.0 * math.sqrt(2.0 / n)
    assert abs((np.abs(z) > 3.0).mean() - p3) < 5.0 * math.sqrt(p3 * (1.0 - p3) / n)


def test_neighbours_do_not_collide():
    seen = set()
    for s in range(4):
        for c in range(5):
            for row in range(200):
                seen.add(sm.mc_hash(99, 7, s, c, row)[0])
    assert len(seen) == 4 * 5 * 200
    assert sm.mc_hash(99, 7, 0, 0, 0) != sm.mc_hash(99, 8, 0, 0, 0) != sm.mc_hash(100, 7, 0, 0, 0)


# ---- the surface -------------------------------------------------------------------------------------------------
NEW_SYMBOLS = ["tgp_ell_softmax_workspace_bytes", "tgp_ell_softmax_f64", "tgp_mc_normals_f64", "tgp_predict_softmax_f64"]


def test_header_declares_the_new_symbols():
    with open(os.path.join(REPO, "include", "tgp_hip.h")) as fh:
        text = fh.read()
    for sym in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % sym, text), sym
    assert re.search(r"#define\s+TGP_LIK_SOFTMAX\s+5\b", text)
    assert re.search(r"#define\s+TGP_VERSION\s+104\b", text)
    assert "typedef struct tgp_softmax" in text


def test_binding_covers_the_new_symbols():
    import ctypes as C
    from tgp.pytorch_amd import lib as L
    for sym in NEW_SYMBOLS:
        assert sym in L.EXPORTS
    assert L.LIK_SOFTMAX == 5
    names = [f[0] for f in L.TgpSoftmax._fields_]
    assert names == ["N", "C", "S", "reserved0", "program", "blk_off", "theta", "theta_off", "scale", "seed", "step_dev", "row0"]
    assert C.sizeof(L.TgpSoftmax) == 80


def _model(lik, C, M=6, D=3, flows=None):
    from tgp.pytorch_amd.kernels import instance_kernel
    from tgp.pytorch_amd.models import sparse_MF_GP, sparse_MF_SP
    K = instance_kernel("scale_rbf", ard_num_dim=D, num_multioutput=C, kernel_is_shared=False)
    X, Z = torch.randn(10, D, dtype=F64), torch.randn(M, D, dtype=F64)
    if flows is None:
        return sparse_MF_GP(["zero", K], X, Z, 10, lik, C, True, False, False, False, False, 0.0)
    return sparse_MF_SP(["zero", K], X, Z, 10, lik, C, True, False, False, False, False, flows, "single", 0.0)


def test_model_takes_c_outputs_only_with_the_multiclass_likelihood():
    from tgp.pytorch_amd import config as cg
    from tgp.pytorch_amd.flows import SAL
    from tgp.pytorch_amd.likelihoods import GaussianLinearMean, MulticlassCategorical
    cg.set_maximum_precission()
    with pytest.raises(AssertionError, match="single-output path"):
        _model(GaussianLinearMean(out_dim=3, noise_init=0.05, noise_is_shared=False), 3)
    with pytest.raises(AssertionError):
        MulticlassCategorical(2)
    with pytest.raises(AssertionError):
        _model(MulticlassCategorical(4), 3)
    C, M, D = 3, 6, 3
    model = _model(MulticlassCategorical(C), C, M, D)
    shapes = {n: tuple(p.shape) for n, p in model.named_parameters()}
    assert shapes == {"Z": (C, M, D), "q_U.variational_mean": (C, M), "q_U.chol_variational_covar": (C, M, M),
                      "covariance_function.raw_outputscale": (C,),
                      "covariance_function.base_kernel.raw_lengthscale": (C, 1, D)}
    assert tuple(model.covariance_function.batch_shape) == (C,) and len(model.G_matrix) == C
    tgp = _model(MulticlassCategorical(C), C, M, D, flows=[SAL(2)] * C)
    per_class = [sorted(n for n, _ in g.named_parameters()) for g in tgp.G_matrix]
    assert len(tgp.G_matrix) == C and all(len(p) == 8 for p in per_class)   # SAL x 2: (sal, affine) x 2
    assert len({id(p) for g in tgp.G_matrix for p in g.parameters()}) == 8 * C       # one flow of its own per class
    with pytest.raises(AssertionError, match="sharing flags"):
        from tgp.pytorch_amd.kernels import instance_kernel
        from tgp.pytorch_amd.models import sparse_MF_GP
        K = instance_kernel("scale_rbf", ard_num_dim=D, num_multioutput=C, kernel_is_shared=False)
        sparse_MF_GP(["zero", K], torch.randn(10, D, dtype=F64), torch.randn(M, D, dtype=F64), 10, MulticlassCategorical(C), C,
                     True, False, False, True, False, 0.0)


def test_blobs_dataset_is_seeded_and_balanced():
    from tgp.pytorch_amd.synthetic import BLOBS_SHAPE, blobs_dataset
    X, Y = blobs_dataset()
    X2, Y2 = blobs_dataset()
    assert X.shape == BLOBS_SHAPE[:2] and Y.shape == (BLOBS_SHAPE[0], 1)
    assert np.array_equal(X, X2) and np.array_equal(Y, Y2)
    assert sorted(np.unique(Y).tolist()) == [0.0, 1.0, 2.0, 3.0]
    assert np.bincount(Y.reshape(-1).astype(int)).tolist() == [300] * 4
