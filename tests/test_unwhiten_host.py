"""Unwhitened q(u) (is_whiten=False), CPU side: tests/unwhiten_model.py against the reference's fixtures
(tools/gen_golden_unwhitened.py), its gradients, the ABI table, and the model's constructor."""
import os

import pytest
import torch

from conftest import REPO, load_golden, rel_err

import unwhiten_model as um

TOL_VAL, TOL_GRAD = 1e-9, 1e-7
# fixture -> (worst value difference, worst gradient difference) of tests/unwhiten_model.py against the reference, relative to
# the largest reference entry, as tools/gen_golden_unwhitened.py printed them; cond(K_ZZ) in the comment
MEASURED = {
    "unwh_tiny_svgp": (7.2e-16, 1.3e-15),      # 1.6e1
    "unwh_med_sal2": (8.5e-11, 3.6e-10),       # 1.6e7
    "unwh_edge128": (1.8e-10, 4.5e-10),        # 6.6e7
    "unwh_bigm_matern": (1.6e-14, 3.7e-12),    # 4.0e1
    "unwh_bern_tiny": (8.5e-14, None),         # 4.6e3 (moments and KL only: the likelihood has no CPU restatement here)
}
CASES = tuple(MEASURED)
GRAD_KEYS = (("Z", "g_Z"), ("m", "g_m"), ("Lam", "g_Lam"), ("raw_outputscale", "g_raw_outputscale"),
             ("raw_lengthscale", "g_raw_lengthscale"), ("log_var_noise", "g_log_var_noise"), ("theta", "g_theta"))


def tolerances(name):
    """The project's tolerances, or 10 x the CPU restatement's own difference from the reference where conditioning alone
    takes a case past them (both implementations round differently at the same condition number)."""
    val, grad = MEASURED[name]
    return max(TOL_VAL, 10.0 * val), max(TOL_GRAD, 10.0 * (grad or 0.0))


@pytest.mark.parametrize("name", CASES)
def test_cpu_model_matches_reference(name):
    g = load_golden(name)
    p = g["params"]
    args = (p["Z"], p["raw_lengthscale"], p["raw_outputscale"], p["m"], p["Lam"])
    mu, v = um.qf_moments(g["X"], *args, kernel=g["kernel"])
    kl = um.kld(*args, kernel=g["kernel"])
    assert rel_err(mu, g["mu"]) < TOL_VAL and rel_err(v, g["v"]) < TOL_VAL and rel_err(kl, g["KLD"]) < TOL_VAL
    if int(g["bernoulli"]):
        return
    (elbo, ell, kld), grads = um.elbo_and_grads(g)
    assert rel_err(elbo, g["ELBO"]) < TOL_VAL and rel_err(ell, g["ELL"]) < TOL_VAL and rel_err(kld, g["KLD"]) < TOL_VAL
    for k, gk in GRAD_KEYS:
        if gk in g:
            assert rel_err(grads[k], g[gk]) < TOL_GRAD, k


def test_upper_triangle_of_L_q_is_ignored():
    g = load_golden("unwh_tiny_svgp")
    p = g["params"]
    assert float(torch.triu(p["Lam"], 1).abs().max()) > 0.0          # the fixture's factor is dense
    a = um.unwhiten(p["Z"], p["raw_lengthscale"], p["raw_outputscale"], p["m"], p["Lam"])
    b = um.unwhiten(p["Z"], p["raw_lengthscale"], p["raw_outputscale"], p["m"], torch.tril(p["Lam"]))
    assert torch.equal(a[1], b[1]) and float(torch.triu(a[1], 1).abs().max()) == 0.0


@pytest.mark.parametrize("kernel", ("scale_rbf", "scale_matern32"))
def test_cpu_model_gradcheck(kernel):
    g = load_golden("unwh_tiny_svgp")
    p = g["params"]
    leaves = [p[k].clone().requires_grad_(True) for k in ("Z", "raw_lengthscale", "raw_outputscale", "m", "Lam")]

    def f(*a):
        m_w, Lam_w, _ = um.unwhiten(*a, kernel=kernel)
        return m_w, Lam_w, um.kld(*a, kernel=kernel)
    assert torch.autograd.gradcheck(f, leaves, eps=1e-6, atol=1e-6, rtol=1e-5)


def test_ladder_values_and_a_singular_prior():
    """Host logic of the two ladders: a K_ZZ with a repeated inducing point is singular to rounding (whether its plain
    factorisation fails is a matter of the last bit) and factorises at the first value of either ladder; the KL's prior
    always carries at least 1e-8 (add_jitter_MultivariateNormal)."""
    from tgp.pytorch_amd import ops
    assert ops.KL_PRIOR_JITTERS == um.KL_PRIOR_JITTERS == (1e-8, 1e-7, 1e-6, 1e-5, 1e-4)
    assert ops.jitter_ladder() == [1e-8, 1e-7, 1e-6]
    g = load_golden("unwh_tiny_svgp")
    p = g["params"]
    Z = p["Z"].clone()
    Z[1] = Z[0]
    K = um.fm.kernel_matrix(Z, Z, p["raw_lengthscale"], p["raw_outputscale"])
    ev = torch.linalg.eigvalsh(K)
    assert float(ev[0]) < 1e-12 * float(ev[-1])
    m_w, Lam_w, L = um.unwhiten(Z, p["raw_lengthscale"], p["raw_outputscale"], p["m"], p["Lam"], jitter=ops.jitter_ladder()[0])
    assert torch.isfinite(m_w).all() and torch.isfinite(Lam_w).all()
    assert torch.isfinite(um.kld(Z, p["raw_lengthscale"], p["raw_outputscale"], p["m"], p["Lam"]))


class _Stub:
    """A factorisation that fails a chosen number of times and records the jitters it was tried at."""

    def __init__(self, failures):
        self.failures, self.seen = failures, []

    def __call__(self, jit):
        self.seen.append(jit)
        return len(self.seen) <= self.failures


@pytest.mark.parametrize("which", ("psd_safe_cholesky", "kl_prior"))
def test_host_ladder_with_a_stub_factorisation(which):
    """ops.run_jitter_ladder, the retry loop of ops.unwhiten, for both ladders: the first try at the starting jitter, then
    the rungs above it in order; info["jitter"], the warning on a success after a failure, NotPSDError on exhaustion."""
    import warnings
    from tgp.pytorch_amd import ops
    if which == "kl_prior":          # KLD(): starts at the first rung (the prior always carries 1e-8), four more above it
        start, ladder, seq = ops.KL_PRIOR_JITTERS[0], ops.KL_PRIOR_JITTERS, [1e-8, 1e-7, 1e-6, 1e-5, 1e-4]
    else:                            # _gp_params(): starts at 0, psd_safe_cholesky's three rungs
        start, ladder, seq = 0.0, None, [0.0, 1e-8, 1e-7, 1e-6]
    for k in range(len(seq)):        # k failures, then success at seq[k]
        stub, info = _Stub(k), {}
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            got = ops.run_jitter_ladder(stub, start, ladder, info)
        assert stub.seen == pytest.approx(seq[:k + 1], rel=1e-12, abs=0.0) and len(stub.seen) == k + 1
        assert got == info["jitter"] == pytest.approx(seq[k], rel=1e-12, abs=0.0)
        hits = [x for x in w if issubclass(x.category, ops.NumericalWarning)]
        assert len(hits) == (1 if k else 0)
        if k:
            assert ("%g" % seq[k]) in str(hits[0].message)
    stub, info = _Stub(len(seq)), {}
    with pytest.raises(ops.NotPSDError, match="%g" % seq[-1]):
        ops.run_jitter_ladder(stub, start, ladder, info)
    assert stub.seen == pytest.approx(seq, rel=1e-12, abs=0.0) and info["jitter"] == start
    # a start inside the ladder skips the rungs at or below it
    stub = _Stub(1)
    with pytest.warns(ops.NumericalWarning):
        assert ops.run_jitter_ladder(stub, 1e-6, ops.KL_PRIOR_JITTERS, None) == pytest.approx(1e-5, rel=1e-12)
    assert stub.seen == pytest.approx([1e-6, 1e-5], rel=1e-12)


def test_abi_lists_the_new_entries():
    from tgp.pytorch_amd import lib
    names = ("tgp_unwhiten_workspace_bytes", "tgp_unwhiten_f64", "tgp_unwhiten_bwd_workspace_bytes", "tgp_unwhiten_bwd_f64")
    header = open(os.path.join(REPO, "include", "tgp_hip.h")).read()
    for n in names:
        assert n in lib.EXPORTS and n + "(" in header
    assert len(lib._SIGS["tgp_unwhiten_f64"][1]) == 17 and len(lib._SIGS["tgp_unwhiten_bwd_f64"][1]) == 20
    assert "#define TGP_VERSION 104" in header


@pytest.mark.parametrize("cls", ("sparse_MF_SP", "sparse_MF_GP"))
def test_unwhitened_model_constructs_with_the_reference_parameters(cls):
    from tgp.pytorch_amd import config as cg
    from tgp.pytorch_amd import models
    from tgp.pytorch_amd.flows import SAL
    from tgp.pytorch_amd.kernels import instance_kernel
    from tgp.pytorch_amd.likelihoods import GaussianLinearMean, GaussianNonLinearMean
    old = torch.get_default_dtype()
    cg.set_maximum_precission()
    try:
        M, D = 7, 3
        X = torch.randn(20, D, dtype=torch.float64)
        K = instance_kernel("scale_rbf", ard_num_dim=D, num_multioutput=1, kernel_is_shared=False,
                            init_params={"length_scale": 2.0, "kernel_scale": 2.0, "noisy_variance": 1e-6})
        ip = {"variational_distribution": {"variance_scale": 4.0, "mean_scale": 0.5}}
        if cls == "sparse_MF_GP":
            model = models.sparse_MF_GP(["zero", K], X, X[:M].clone(), 20, GaussianLinearMean(1, 0.05, False), 1, False, False,
                                        False, False, False, 0.0, init_params=ip)
        else:
            model = models.sparse_MF_SP(["zero", K], X, X[:M].clone(), 20, GaussianNonLinearMean(1, 0.05, False, quadrature_points=8),
                                        1, False, False, False, False, False, [SAL(2)], "single", 0.0, init_params=ip)
    finally:
        torch.set_default_dtype(old)
    assert model.is_whiten is False
    shapes = {n: tuple(q.shape) for n, q in model.named_parameters() if "G_matrix" not in n}
    assert shapes == {"Z": (1, M, D), "q_U.variational_mean": (1, M), "q_U.chol_variational_covar": (1, M, M),
                      "covariance_function.raw_outputscale": (1,), "covariance_function.base_kernel.raw_lengthscale": (1, 1, D),
                      "likelihood.log_var_noise": (1, 1)}
    # initialize_variational_distribution is the same for both modes (sparse_MF_SP.py:158-177)
    assert torch.equal(model.q_U.chol_variational_covar.data[0], 2.0 * torch.eye(M, dtype=torch.float64))
    assert torch.equal(model.q_U.variational_mean.data[0], torch.full((M,), 0.5, dtype=torch.float64))
