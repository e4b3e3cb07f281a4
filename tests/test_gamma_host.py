"""CPU: the Gamma likelihood (TGP_LIK_GAMMA) above the kernels -- the ABI constants, the torch restatement
(tests/gamma_model.py): its incomplete gamma function `pq` (the kernel's series / continued fraction) against mpmath at 50
digits, its quadrature against the closed form of the identity flow, its root rule against plain bisection on every input
tests/test_gpu_gamma.py uses; then the class's traits, the ValueErrors, the engines' refusal, the CLI's argument errors, the
models' CRPS / pmf refusals and the synthetic_claims data set.

RESIDUAL_PQ_CPU is the worst relative error of the SMALLER of (P, Q) from `pq` against mpmath over a in PQ_SHAPES and 221 points
z in [-8, 3] (x = a e^z), measured here (test_pq_against_mpmath prints it): the leading factor exp(a (z - expm1(z)) + c) carries
a rounding of an exponent of magnitude up to a e^3, so the figure grows with a.  This file holds the restatement to 2x the
figure (head room for another libm), as tests/test_quantiles_host.py does with RESIDUAL_CPU.

TORCH_SPECIAL_ERR is the same figure for torch.special.gammainc / gammaincc, the functions gamma_model.tails is made of:
1e-14 for a <= 3.7, but 1.7e-9 at a = 50 and 7.0e-10 at a = 1000, in the middle of the distribution (x within a factor 1.4 of a,
tails between 1e-6 and 0.5: torch's uniform asymptotic expansion for a > 20; scipy's has 8e-14 and 1.3e-12 there).  So at large
shapes the restatement's F, not the kernel's, is what limits the agreement of the two, and the comparisons that go through
`tails` at such a shape allow for it by this measured figure: `eval_noise(a)` in root_tolerance, and the recorded residuals.

RESIDUAL_ROOT_CPU[a] is the worst |F(t) - p| / min(p, 1 - p) of the restated rule's own roots on F through torch.special
(gamma_model.tails) over the quantile inputs below of shape a; tests/test_gpu_gamma.py allows the device 10x the figure of the
case's shape."""
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import REPO

import gamma_model as GM
from oracle import tgp_oracle as orc
from test_quantiles_host import seeded_problem
from tgp.pytorch_amd import lib as L

F64 = torch.float64
TOL_VAL = 1e-9
CPU_HEADROOM = 2.0
PQ_SHAPES = [0.1, 0.5, 1.0, 3.7, 50.0, 1000.0]
RESIDUAL_PQ_CPU = 1.62e-13     # measured by test_pq_against_mpmath: the worst point is a = 50, z = 2.65 (see the docstring)
PQ_ITERS_CPU = 268             # ... and the largest trip count of the series / continued fraction on the same grid
TORCH_SPECIAL_ERR = {0.1: 1e-14, 0.5: 1e-14, 1.0: 1e-14, 3.7: 1e-14, 50.0: 1.7e-9, 1000.0: 7.0e-10}   # measured, as RESIDUAL_PQ_CPU
TORCH_LARGE_SHAPE = 20.0       # torch.special switches to the asymptotic expansion above it
# measured by test_root_rule_on_the_gpu_inputs (it prints the figure per case): by shape, the worst case of that shape.  The
# cases: 1.07e-14, 4.16e-15, 2.78e-15, 6.83e-11, 5.55e-16, 8.19e-15, 7.61e-11 and, the hard ones, 3.39e-14, 5.55e-10, 3.58e-14,
# 3.72e-10 -- at a = 1000 it is torch.special's error that shows (TORCH_SPECIAL_ERR), not the roots'
RESIDUAL_ROOT_CPU = {0.1: 3.58e-14, 1.0: 4.16e-15, 3.7: 1.07e-14, 1000.0: 5.55e-10}


@pytest.fixture(autouse=True)
def _f64():
    from tgp.pytorch_amd import config as cg
    old = torch.get_default_dtype()
    cg.set_maximum_precission()
    yield
    torch.set_default_dtype(old)


# ---------------------------------------------------------------------------------------------------
# shared with tests/test_gpu_gamma.py: the inputs of the CDF and quantile tests
# ---------------------------------------------------------------------------------------------------
Q1, Q3 = [0.975], [0.025, 0.5, 0.975]
Q32 = sorted([0.01, 0.025, 0.975] + [float(x) for x in torch.linspace(0.05, 0.95, 29, dtype=F64)])      # (0.5 among them)
# (kind, N, S, shape a, probabilities): the four programs, the shapes of the range and one inside, Q = 1, 3, 32
QUANT_CASES = [("empty", 5, 16, 3.7, Q3), ("sal2", 9, 17, 1.0, Q3), ("tanh3x2", 5, 33, 0.1, Q3), ("bcl_al", 3, 15, 1000.0, Q3),
               ("sal2", 5, 1, 3.7, Q1), ("empty", 3, 32, 0.1, Q32), ("sal2", 3, 32, 1000.0, Q32)]
HARD_PROBS = [1e-6, 1.0 - 1e-6]
HARD_CASES = [("empty", 0.1), ("empty", 1000.0), ("sal2", 0.1), ("sal2", 1000.0)]


def quant_problem(kind, N, S, a, seed=0):
    """mu, v, the log shape and a flow of `kind` (empty | the kinds of test_quantiles_host.seeded_problem) with seeded
    parameters; the flow's value is the log-mean."""
    if kind == "empty":
        pr = seeded_problem("sal2", N, S, seed=seed)
        pr["program"], pr["theta"] = [], torch.zeros(0, dtype=F64)
    else:
        pr = seeded_problem(kind, N, S, seed=seed)
    pr["lvn"] = torch.tensor([math.log(a)], dtype=F64)
    return pr


def hard_problem(kind, a):
    """Six rows with v in {0, 0, 1e-4, 1e-4, 4, 4} at S = 32, for the probabilities HARD_PROBS; |g| stays below 50 so that
    t = exp(tau) is representable at a = 0.1 (tau reaches g - 140 there)."""
    pr = quant_problem(kind, 6, 32, a, seed=21)
    pr["v"] = torch.tensor([0.0, 0.0, 1e-4, 1e-4, 4.0, 4.0], dtype=F64)
    g = GM.nodes(pr["mu"], pr["v"], pr["xs"], pr["program"], pr["theta"], pr["rowp"])
    assert float(g.abs().max()) < 50.0
    return pr


def solve(pr, probs, count=None):
    return GM.quantiles(pr["mu"], pr["v"], pr["lvn"], probs, pr["xs"], pr["wn"], pr["program"], pr["theta"], pr["rowp"], count)


def bisect(pr, probs):
    return GM.bisect_quantiles(pr["mu"], pr["v"], pr["lvn"], probs, pr["xs"], pr["wn"], pr["program"], pr["theta"], pr["rowp"])


def eval_noise(a):
    """The measured relative error of an evaluation of F: the kernel's algorithm plus torch.special's (the worse of the two
    large shapes above TORCH_LARGE_SHAPE), each with the head room, and never below test_quantiles_host's 2^-46."""
    t = max(TORCH_SPECIAL_ERR[50.0], TORCH_SPECIAL_ERR[1000.0]) if a > TORCH_LARGE_SHAPE else TORCH_SPECIAL_ERR[1.0]
    return max(2.0 ** -46, CPU_HEADROOM * (RESIDUAL_PQ_CPU + t))


def root_tolerance(dens, tau, p, noise):
    """test_quantiles_host.root_tolerance on tau, with the evaluation noise of this F in place of 2^-46: the project's value
    tolerance 1e-9 max(1, |tau|) plus 2 noise min(p, 1 - p) / F'(tau), noise = eval_noise(a)."""
    return TOL_VAL * tau.abs().clamp_min(1.0) + 2.0 * noise * min(p, 1.0 - p) / dens


def roots_agree(pr, probs, tau_a, tau_b, label=""):
    a = GM.shape_of(pr["lvn"])
    g = GM.nodes(pr["mu"], pr["v"], pr["xs"], pr["program"], pr["theta"], pr["rowp"])
    worst = 0.0
    for qi, p in enumerate(probs):
        dens = torch.minimum(GM.tails(g, pr["wn"], a, tau_a[qi])[2], GM.tails(g, pr["wn"], a, tau_b[qi])[2])
        tol = root_tolerance(dens, tau_b[qi], p, eval_noise(a))
        worst = max(worst, float(((tau_a[qi] - tau_b[qi]).abs() / tol).max()))
        assert bool(((tau_a[qi] - tau_b[qi]).abs() <= tol).all()), (label, p, float((tau_a[qi] - tau_b[qi]).abs().max()))
    print("roots agree %-24s worst |dtau| / tolerance %.3e" % (label, worst))


def worst_residual(pr, probs, tau):
    a = GM.shape_of(pr["lvn"])
    g = GM.nodes(pr["mu"], pr["v"], pr["xs"], pr["program"], pr["theta"], pr["rowp"])
    return max(float(GM.residual(g, pr["wn"], a, tau[qi], p).max()) for qi, p in enumerate(probs))


def all_quant_inputs():
    """(label, problem, probabilities) of every quantile input the GPU tests use."""
    for kind, N, S, a, probs in QUANT_CASES:
        yield "%s-N%d-S%d-a%g-Q%d" % (kind, N, S, a, len(probs)), quant_problem(kind, N, S, a, seed=N + S), probs
    for kind, a in HARD_CASES:
        yield "hard-%s-a%g" % (kind, a), hard_problem(kind, a), HARD_PROBS


# ---------------------------------------------------------------------------------------------------
# constants
# ---------------------------------------------------------------------------------------------------
def test_abi_constants():
    hdr = open(os.path.join(REPO, "include", "tgp_hip.h")).read()
    assert re.search(r"#define TGP_LIK_GAMMA 11\b", hdr)
    assert re.search(r"#define TGP_GAMMA_MIN_SHAPE 0\.1\b", hdr) and re.search(r"#define TGP_GAMMA_MAX_SHAPE 1e3\b", hdr)
    assert re.search(r"#define TGP_VERSION 104\b", hdr)          # no struct, signature or version change
    assert L.LIK_GAMMA == 11 and L.GAMMA_MIN_SHAPE == 0.1 and L.GAMMA_MAX_SHAPE == 1e3
    assert (GM.AMIN, GM.AMAX) == (L.GAMMA_MIN_SHAPE, L.GAMMA_MAX_SHAPE)
    cap = int(re.search(r"#define TGP_GAMMA_PQ_MAXIT (\d+)\b", hdr).group(1))
    assert cap == L.GAMMA_PQ_MAXIT
    assert L.LIK_DISPLAY[L.LIK_GAMMA] == "Gamma"
    assert L.load().tgp_version() == 104


# ---------------------------------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------------------------------
def test_log_p_is_torch_gamma():
    g = torch.Generator().manual_seed(7)
    for a in PQ_SHAPES:
        logm = 2.0 * torch.randn(2000, generator=g, dtype=F64)
        y = torch.exp(logm) * torch._standard_gamma(torch.full((2000,), a, dtype=F64), generator=g).clamp_min(1e-300) / a
        lam = torch.tensor(math.log(a), dtype=F64)
        ours = GM.log_p(y, logm, lam)
        ref = torch.distributions.Gamma(torch.tensor(a, dtype=F64), a * torch.exp(-logm)).log_prob(y)
        err = float(((ours - ref).abs() / ref.abs().clamp(min=1.0)).max())
        print("a = %g: max relative difference of log p %.3e" % (a, err))
        assert err <= 1e-10
        # the header's derivatives, point by point, against autograd
        gg = logm.clone().requires_grad_(True)
        ll = torch.full_like(logm, math.log(a)).requires_grad_(True)
        dg, dl = torch.autograd.grad(GM.log_p(y, gg, ll).sum(), [gg, ll])
        z = torch.log(y) - logm
        want_g = a * torch.expm1(z)
        want_l = a * (math.log(a) + 1.0 - float(torch.digamma(torch.tensor(a, dtype=F64)))) + a * (z - torch.exp(z))
        assert float(((dg - want_g).abs() / (a * (1.0 + torch.exp(z)))).max()) <= 1e-13
        assert float(((dl - want_l).abs() / (a * (abs(math.log(a)) + 1.0 + z.abs() + torch.exp(z)) + 1.0)).max()) <= 1e-13


def test_pq_against_mpmath():
    import mpmath
    mpmath.mp.dps = 50
    hdr = open(os.path.join(REPO, "include", "tgp_hip.h")).read()
    cap = int(re.search(r"#define TGP_GAMMA_PQ_MAXIT (\d+)\b", hdr).group(1))
    zs = torch.linspace(-8.0, 3.0, 221, dtype=F64)
    worst, worst_at, most = 0.0, None, 0
    for a in PQ_SHAPES:
        P, Q, h, iters = GM.pq(a, zs)
        most = max(most, iters)
        xt = a * torch.exp(zs)
        Pt, Qt = torch.special.gammainc(torch.full_like(xt, a), xt), torch.special.gammaincc(torch.full_like(xt, a), xt)
        worst_t = 0.0
        for i, z in enumerate(zs.tolist()):
            x = mpmath.mpf(a) * mpmath.exp(mpmath.mpf(z))
            Pm = mpmath.gammainc(a, 0, x, regularized=True)
            Qm = mpmath.gammainc(a, x, mpmath.inf, regularized=True)
            small, ref = (float(P[i]), Pm) if Pm <= Qm else (float(Q[i]), Qm)
            if ref < mpmath.mpf("1e-300"):
                continue                                    # (below the double range: nothing to be relative to)
            err = float(abs(mpmath.mpf(small) - ref) / ref)
            if err > worst:
                worst, worst_at = err, (a, z)
            worst_t = max(worst_t, float(abs(mpmath.mpf(float(Pt[i]) if Pm <= Qm else float(Qt[i])) - ref) / ref))
            assert abs(float(P[i]) + float(Q[i]) - 1.0) <= 4e-16
            hm = mpmath.exp(a * mpmath.log(x) - x - mpmath.loggamma(a))
            assert hm < mpmath.mpf("1e-300") or float(abs(mpmath.mpf(float(h[i])) - hm) / hm) <= CPU_HEADROOM * RESIDUAL_PQ_CPU
        print("a = %g: torch.special worst small-tail relative error %.3e (recorded %.1e)" % (a, worst_t, TORCH_SPECIAL_ERR[a]))
        assert worst_t <= CPU_HEADROOM * TORCH_SPECIAL_ERR[a]
    print("pq: worst small-tail relative error %.3e at (a, z) = %s (recorded %.3e); most iterations %d (recorded %d, cap %d)"
          % (worst, worst_at, RESIDUAL_PQ_CPU, most, PQ_ITERS_CPU, cap))
    assert worst <= CPU_HEADROOM * RESIDUAL_PQ_CPU
    assert most < cap and most <= CPU_HEADROOM * PQ_ITERS_CPU
    # the ends
    P, Q, h, _ = GM.pq(3.7, torch.tensor([-float("inf"), float("inf"), -800.0, 800.0], dtype=F64))
    assert P.tolist() == [0.0, 1.0, 0.0, 1.0] and Q.tolist() == [1.0, 0.0, 1.0, 0.0] and h.tolist() == [0.0] * 4


def test_quadrature_against_the_closed_form():
    """The identity flow: E log p in closed form against the restated quadrature at S = 32, v <= 1."""
    g = torch.Generator().manual_seed(3)
    N = 200
    mu = 0.7 * torch.randn(N, generator=g, dtype=F64)
    v = torch.rand(N, generator=g, dtype=F64)
    v[:5] = torch.tensor([0.0, 1.0, -1e-12, 1e-6, 0.5], dtype=F64)
    xs, ws = orc.hermgauss(32)
    wn = ws / math.sqrt(math.pi)
    for a in (0.1, 1.0, 3.7, 1000.0):
        Y = torch.exp(mu) * torch._standard_gamma(torch.full((N,), 2.0, dtype=F64), generator=g).clamp_min(1e-300) / 2.0
        lam = torch.tensor([math.log(a)], dtype=F64)
        quad = GM.ell_rows(Y, mu, v, lam, [], None, xs, wn)
        closed = GM.ell_closed_rows(Y, mu, v, lam)
        err = float(((quad - closed).abs() / closed.abs().clamp_min(1.0)).max())
        print("a = %g: quadrature against the closed form, worst row %.3e" % (a, err))
        assert err <= TOL_VAL
    # the moments of the empty program: the log-normal closed forms, which the quadrature reproduces
    m1, m2, lp = GM.pred_torch(mu, v, lam, [], None, xs, wn, Y=Y, Y_std=2.5)
    gq = GM.nodes(mu, v, xs, [], None)
    q1, q2 = (wn.reshape(-1, 1) * torch.exp(gq)).sum(0), (wn.reshape(-1, 1) * torch.exp(2.0 * gq)).sum(0)
    assert float(((m1 - q1).abs() / q1).max()) <= TOL_VAL
    assert float(((m2 - ((1.0 + 1e-3) * q2 - q1 * q1)).abs() / m2).max()) <= 1e-7
    lp1 = GM.pred_torch(mu, v, lam, [], None, xs, wn, Y=Y)[2]
    assert float((lp - (lp1 - math.log(2.5))).abs().max()) <= 1e-12


def test_root_rule_on_the_gpu_inputs():
    """Zero failures and agreement with plain bisection on every input tests/test_gpu_gamma.py uses; the evaluations of F a
    root takes stay below the kernel's 2 x 128."""
    most = 0
    for label, pr, probs in all_quant_inputs():
        count = []
        t, failed, tau = solve(pr, probs, count)
        assert failed == 0 and bool(torch.isfinite(tau).all()) and bool(torch.isfinite(t).all()) and bool((t > 0).all()), label
        most = max(most, max(count))
        roots_agree(pr, probs, tau, bisect(pr, probs), label)
        order = sorted(range(len(probs)), key=lambda i: probs[i])
        assert bool((tau[order][1:] > tau[order][:-1]).all()), label
        r = worst_residual(pr, probs, tau)
        a = round(GM.shape_of(pr["lvn"]), 9)
        print("residual %-28s %.3e   (recorded for a = %g: %.3e)" % (label, r, a, RESIDUAL_ROOT_CPU[a]))
        assert r <= CPU_HEADROOM * RESIDUAL_ROOT_CPU[a], label
    print("most evaluations of F for one root %d" % most)
    assert most <= GM.MAXIT


def test_cdf_of_nonpositive_targets():
    pr = quant_problem("sal2", 4, 16, 3.7, seed=1)
    Y = torch.tensor([0.0, -1.0, 1.0, 1e-300], dtype=F64)
    c, s = GM.cdf(pr["mu"], pr["v"], pr["lvn"], Y, pr["xs"], pr["wn"], pr["program"], pr["theta"])
    assert c[:2].tolist() == [0.0, 0.0] and s[:2].tolist() == [float(pr["wn"].sum())] * 2
    assert 0.0 < float(c[2]) < 1.0 and abs(float(c[2] + s[2]) - float(pr["wn"].sum())) <= 1e-15


# ---------------------------------------------------------------------------------------------------
# the class, its traits and its refusals
# ---------------------------------------------------------------------------------------------------
def test_trait_table():
    from tgp.pytorch_amd import likelihoods as LK
    base = LK.Likelihood
    lik = LK.Gamma()
    traits = [n for n in vars(base) if not n.startswith("_") and not callable(getattr(base, n))
              and not isinstance(vars(base)[n], (staticmethod, classmethod))]
    for n in traits:
        getattr(lik, n)                                  # every trait is defined
    assert lik.display == "gamma" and lik.lik_id == L.LIK_GAMMA == 11 and lik.engine_name == "gamma"
    assert lik.kind == "regression" and lik.has_noise is True and lik.has_flow is True and lik.one_launch_logp is True
    assert lik.flow_on_targets is False and lik.compiles_flows is False and lik.num_latent == 1 and lik.composed is False
    assert lik.refuses_cdf is None
    assert lik.refuses_crps.count("%s") == 1 and "no closed pair term" in lik.refuses_crps
    assert lik.refuses_input_dependent == LK.NO_INPUT_DEPENDENT % lik.display
    assert lik.refuses_optimal_qu == LK.NOT_GAUSSIAN_IN_F % lik.display and lik.refuses_optimal_qu_id is None
    assert lik.refuses_mean is None and lik.refuses_paths is None and lik.refuses_full_cov is None
    assert "gamma" in lik.outputs_refusal
    assert lik.lik_kwargs() == {"lik": L.LIK_GAMMA, "df": None}
    assert [n for n, _ in lik.named_parameters()] == ["log_shape"] and list(lik.state_dict()) == ["log_shape"]
    assert lik.log_shape.shape == (1,) and float(lik.log_shape.detach()) == 0.0
    assert lik.noise().shape == (1,) and lik.noise().requires_grad and lik.noise().data_ptr() == lik.log_shape.data_ptr()
    assert abs(float(LK.Gamma(shape_init=2.5).shape) - 2.5) < 1e-15 and not LK.Gamma(2.5).shape.requires_grad
    assert LK.Gamma(quadrature_points=7).quad_points == 7
    for bad in (0.0, 0.05, -1.0, 2e3, float("nan")):
        with pytest.raises(ValueError, match="shape"):
            LK.Gamma(shape_init=bad)
    LK.Gamma(shape_init=0.1), LK.Gamma(shape_init=1e3)
    for bad in ([[1.0], [0.0]], [[1.0], [-2.0]], [[float("nan")]], [[float("inf")]]):
        with pytest.raises(ValueError, match="positive targets"):
            lik.check_targets(torch.tensor(bad, dtype=F64))
    lik.check_targets(torch.tensor([[1e-300], [7.0]], dtype=F64))
    # the shape-range check of the exact CDF / quantiles
    lik.check_shape()
    with torch.no_grad():
        lik.log_shape.fill_(math.log(0.05))
    with pytest.raises(ValueError, match=r"\[0\.1, 1000\]"):
        lik.check_shape()
    # draws: positive, mean e^f, variance e^2f / a
    lik2 = LK.Gamma(shape_init=2.0)
    torch.manual_seed(0)
    f = torch.full((1, 60000), math.log(4.0), dtype=F64)
    s = lik2.sample_from_output(f, 0)
    assert s.shape == f.shape and bool((s > 0).all())
    assert abs(float(s.mean()) - 4.0) < 0.1 and abs(float(s.var()) - 16.0 / 2.0) < 0.5


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
    from tgp.pytorch_amd.likelihoods import Gamma
    from tgp.pytorch_amd.models import sparse_MF_GP, sparse_MF_SP
    X = torch.randn(30, D, dtype=F64)
    K = instance_kernel("scale_rbf", ard_num_dim=D, num_multioutput=num_outputs, kernel_is_shared=False,
                        init_params={"length_scale": 2.0, "kernel_scale": 2.0, "noisy_variance": 1e-6})
    lik = Gamma()
    if kind == "svgp":
        return sparse_MF_GP(["zero", K], X, X[:M].clone(), 30, lik, num_outputs, True, False, False, False, False, 0.0), X
    flow = SAL(1) if kind == "tgp" else SAL(1, input_dependent=True, input_dim=D, num_hidden_layers=1, batch_norm=0, dropout=0.5,
                                            hidden_dim=8, hidden_activation="tanh", inference="MC_dropout")
    return sparse_MF_SP(["zero", K], X, X[:M].clone(), 30, lik, num_outputs, True, False, False, False, False,
                        [flow] * num_outputs, "single", 0.0), X


def test_state_names_and_model_refusals(monkeypatch):
    for kind in ("svgp", "tgp"):
        model, _ = _model(kind)
        assert "likelihood.log_shape" in model.state_dict() and not any("log_var_noise" in n for n in model.state_dict())
        assert model._noise.data_ptr() == model.likelihood.log_shape.data_ptr() and model._lik_id == L.LIK_GAMMA
    lib = RecordingLib()
    monkeypatch.setattr(L, "load", lambda: lib)
    with pytest.raises(NotImplementedError, match="gamma"):
        _model("idtgp")
    with pytest.raises(NotImplementedError, match="gamma"):
        _model("svgp", num_outputs=2)
    for kind in ("svgp", "tgp"):
        model, X = _model(kind)
        Y = torch.ones(30, 1, dtype=F64)
        model.set_is_training(False)
        with pytest.raises(NotImplementedError, match="gamma"):
            model.set_optimal_qu(X, Y)
        # the exact CRPS raises through the trait and points to samples=; the pmf is for count models
        with pytest.raises(NotImplementedError, match="no closed pair term.*samples=S"):
            model.predictive_crps(X, Y)
        with pytest.raises(NotImplementedError, match="predictive_pmf"):
            model.predictive_pmf(X, 5)
        # a shape that has left the range: the exact CDF and quantiles say so before any library call
        with torch.no_grad():
            model.likelihood.log_shape.fill_(math.log(2e3))
        for call in (lambda: model.predictive_quantiles(X, [0.5]), lambda: model.predictive_cdf(X, Y),
                     lambda: model.predictive_interval_score(X, Y)):
            with pytest.raises(ValueError, match=r"\[0\.1, 1000\]"):
                call()
    assert lib.calls == []


def test_library_entries_for_the_id():
    """The CRPS entry refuses TGP_LIK_GAMMA before it reads a pointer; the quantile and CDF entries do not refuse the id (an
    argument error, not TGP_E_UNSUPPORTED, for a model without nodes)."""
    import ctypes
    h = L.load()
    buf = torch.zeros(16, dtype=F64)
    st = torch.zeros(1, dtype=torch.int32)
    p, ps = ctypes.c_void_p(buf.data_ptr()), ctypes.c_void_p(st.data_ptr())
    md = L.TgpModel()
    md.N, md.D, md.M, md.S, md.lik = 4, 1, 1, 8, L.LIK_GAMMA
    md.log_var_noise = p
    rc = h.tgp_predict_crps_f64(md, p, p, None, p, p, None, None)
    assert rc == L.E_UNSUPPORTED and b"lik = 11" in h.tgp_last_error()
    assert h.tgp_predict_quantile_f64(md, p, p, None, p, p, 1, p, ps, None) == -1        # xs, wn missing
    assert h.tgp_predict_cdf_f64(md, p, p, None, p, p, None, None) == -1
    md.S = 257
    assert h.tgp_predict_cdf_f64(md, p, p, None, p, p, None, None) == L.E_UNSUPPORTED and b"S = 257" in h.tgp_last_error()
    shape = (300, 3, 20, 16, 1, 4, 0, L.KERNELS["scale_rbf"], 0)
    assert h.tgp_workspace_bytes_lik(*shape, L.LIK_GAMMA) == h.tgp_workspace_bytes_lik(*shape, L.LIK_POISSON)
    assert h.tgp_workspace_bytes_lik(*shape, L.LIK_GAMMA) != h.tgp_workspace_bytes_lik(*shape, L.LIK_FLOW)


def test_engine_refusal_and_surface():
    from tgp.pytorch_amd import ops
    from tgp.pytorch_amd.engine import engine_refusal
    assert "Gamma" in engine_refusal(likelihood="gamma") and "eager path" in engine_refusal(likelihood="gamma")
    assert "Gamma" in engine_refusal(likelihood="gamma", minibatch=True)
    assert callable(ops.ell_gamma) and callable(ops.EllGammaFunction.apply)
    import inspect
    assert inspect.signature(ops.predict_quantiles).parameters["lik"].default is None
    assert inspect.signature(ops.predict_cdf).parameters["lik"].default is None
    lvn = torch.zeros(1, dtype=F64)
    with pytest.raises(L.TgpError, match="Gamma"):
        ops.predict_quantiles(lvn, lvn, lvn, [0.5], lik=L.LIK_GAMMA)                     # needs a FlowSpec


def test_cli_arguments():
    run = lambda *a: subprocess.run([sys.executable, "-m", "tgp.pytorch_amd.main"] + list(a), cwd=REPO, capture_output=True,
                                    text=True, timeout=120)
    out = run("--help")
    assert out.returncode == 0 and "gamma" in out.stdout and "--shape_init" in out.stdout and "synthetic_claims" in out.stdout
    tail = ["--train_test_seed_split", "1", "--num_inducing", "5"]
    bad = run("--model", "SVGP", "--likelihood", "gamma", "--dataset", "synthetic_power", *tail)
    assert bad.returncode == 2 and "positive data sets" in bad.stderr
    bad = run("--model", "SVGP", "--dataset", "synthetic_claims", *tail)
    assert bad.returncode == 2 and "positive data sets" in bad.stderr
    bad = run("--model", "ID_TGP", "--likelihood", "gamma", "--dataset", "synthetic_claims", *tail)
    assert bad.returncode == 2 and "--likelihood gamma: SVGP or TGP only" in bad.stderr
    bad = run("--model", "SVGP", "--likelihood", "gamma", "--shape_init", "0.01", "--dataset", "synthetic_claims", *tail)
    assert bad.returncode == 2 and "--shape_init" in bad.stderr


def test_claims_dataset(monkeypatch):
    from tgp.pytorch_amd import config as cg
    from tgp.pytorch_amd import data, main, synthetic
    X, Y = synthetic.synthetic_claims()
    n, d = synthetic.CLAIMS_SHAPE
    assert (n, d) == (500, 2) and X.shape == (n, d) and Y.shape == (n, 1) and synthetic.CLAIMS_SHAPE_A == 3.0
    assert np.array_equal(Y, synthetic.synthetic_claims(seed=0)[1]) and not np.array_equal(Y, synthetic.synthetic_claims(seed=1)[1])
    assert np.all(Y > 0) and np.all(np.isfinite(Y))
    # Var[y | x] = mean^2 / 3: the squared coefficient of variation around the true mean
    mean = np.exp(np.sin(2.0 * X[:, 0]) + 0.5 * X[:, 1])
    cv2 = float((((Y[:, 0] - mean) / mean) ** 2).mean())
    print("E[((y - mean) / mean)^2] = %.3f (1 / shape = 0.333)" % cv2)
    assert abs(cv2 - 1.0 / 3.0) < 0.08
    monkeypatch.setattr(cg, "device", "cpu", raising=False)
    loaders, dc = data.return_dataset("synthetic_claims", 10000, seed=1)
    assert dc["shape"] == 3.0 and dc["N_tr"] == 450 and dc["N_te"] == 50 and dc["Dx"] == d and len(loaders) == 2
    assert float(np.asarray(dc["Y_std"]).reshape(-1)[0]) == 1.0 and float(np.asarray(dc["Y_mean"]).reshape(-1)[0]) == 0.0
    assert np.array_equal(dc["Y_tr"].numpy(), Y[dc["train_idx"]])                         # raw targets: not centred, not scaled
    assert main.POSITIVE_DATASETS == ("synthetic_claims",) and ("TGP", "claims") in main.HYPER
