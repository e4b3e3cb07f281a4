"""CPU: the Beta likelihood (TGP_LIK_BETA) above the kernels -- the ABI constants, the torch restatement (tests/beta_model.py):
its log density against torch.distributions.Beta and the header's derivatives against autograd, the numpy port of the device's
incomplete beta function against mpmath at 120 digits, the restated root rule on every input tests/test_gpu_beta.py uses; then
the class's traits, the ValueErrors, the engines' refusal, the CLI's argument errors, the models' refusals and the
synthetic_proportions data set.

RESIDUAL_CF_CPU[phi] is the worst relative error of a tail of one component from the port (`component_port`: the continued
fraction on the side where it converges, the other tail as 1 - that) against mpmath, over the node values g in GRID_G and 61
points x = logit t in [-15, 15], every tail of at least 1e-60, lower and upper alike; measured here (test_port_against_mpmath
prints the figure per phi and |g|).  By |g| the figures are 1.1e-14 (g = 0; 4.8e-13 at phi = 1000), 2.6e-14 (|g| = 4; 1.2e-12 at
phi = 1000), 3.3e-12 (|g| = 8; 1.1e-11 at phi = 1000) and 1.3e-10 (|g| = 12).  The density (the front factor) is within 2.3e-14
everywhere (1.4e-12 at phi = 1000: its exponent is of the size 1e4), so the loss is not there.  Its source: with a shape
parameter of the size 1e-5 nearly all mass of the component sits at one end, the continued fraction runs on the side of the mean,
where it converges, and there it computes the tail that is NEARLY ONE; the other tail, of the size of that shape parameter, is
1 - that and keeps 2^-53 / tail of it.  The side where that tail would be computed directly is the one where the continued
fraction needs thousands of steps (its argument is next to 1), so the loss is stated, not removed: the covered box of
include/tgp_hip.h is this grid, and its tolerance the 2e-10 held here.
CF_STEPS_CPU is the largest number of steps of the continued fraction on that grid and, CF_STEPS_FINE, on a finer one (193 values
of g, 481 of x, seven values of phi): TGP_BETA_CF_MAXIT is twice the latter.

tests/test_gpu_beta.py allows the device 10x RESIDUAL_CF_CPU of the case's phi, on the CDF entry and on every root.  A root is
held to it through `beta_model.residual_within_ulp`: F of the reference at the doubles next to the returned t must bracket p
within that allowance.  At the returned double itself no rule can be held to it near t = 1: the 1 - 1e-6 quantile at phi = 0.5
has 1 - t of the size 1e-14, where one step of 2^-53 in t moves the upper tail by the share b 2^-53 / (1 - t) ~ 5e-3."""
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import REPO

import beta_model as BM
from test_quantiles_host import seeded_problem
from tgp.pytorch_amd import lib as L

F64 = torch.float64
CPU_HEADROOM = 2.0
PHIS = [0.5, 1.0, 10.0, 1000.0]
GRID_G = [0.0, 4.0, -4.0, 8.0, -8.0, 12.0, -12.0]
GRID_X = np.linspace(-15.0, 15.0, 61)
MIN_TAIL = "1e-60"
RESIDUAL_CF_CPU = {0.5: 1.22e-10, 1.0: 7.58e-11, 10.0: 1.29e-10, 1000.0: 1.87e-11}   # measured by test_port_against_mpmath
SCIPY_BIG_SHAPE_ERR = 1.65e-13   # scipy.special.betainc against mpmath where beta_model.tails_ref uses it (test_quick_reference_against_mpmath) ...
REF_ROWS_ERR = 2e-13             # ... and tails_ref as a mixture on the rows of the quantile inputs: far inside every allowance below
CF_BOX_TOL = 2e-10           # what include/tgp_hip.h states for the covered box
CF_STEPS_CPU = 58            # ... and the most steps of the continued fraction on the same grid (phi = 1000, |g| = 12)
CF_STEPS_FINE = 87           # ... on the finer grid of test_cf_steps_on_a_fine_grid (phi = 1000, g = -9.875, x = -6.8125)


@pytest.fixture(autouse=True)
def _f64():
    from tgp.pytorch_amd import config as cg
    old = torch.get_default_dtype()
    cg.set_maximum_precission()
    yield
    torch.set_default_dtype(old)


# ---------------------------------------------------------------------------------------------------
# shared with tests/test_gpu_beta.py: the inputs of the CDF and quantile tests
# ---------------------------------------------------------------------------------------------------
Q1, Q3 = [0.975], [0.025, 0.5, 0.975]
Q32 = sorted([0.01, 0.025, 0.975] + [float(x) for x in torch.linspace(0.05, 0.95, 29, dtype=F64)])      # (0.5 among them)
# (kind, N, S, precision phi, probabilities): the four programs, Q = 1, 3, 32; S = 32, Q = 32 across the four precisions
QUANT_CASES = ([("empty", 5, 16, 0.5, Q3), ("sal2", 9, 17, 1.0, Q3), ("tanh3x2", 5, 33, 1000.0, Q3), ("bcl_al", 3, 15, 10.0, Q3),
                ("sal2", 5, 1, 10.0, Q1)]
               + [(kind, 3, 32, phi, Q32) for kind in ("empty", "sal2") for phi in PHIS])
HARD_PROBS = [1e-6, 1.0 - 1e-6]
HARD_CASES = [("empty", 0.5), ("empty", 1000.0), ("sal2", 0.5), ("sal2", 1000.0)]


def quant_problem(kind, N, S, phi, seed=0):
    """mu, v, the log precision and a flow of `kind` (empty | the kinds of test_quantiles_host.seeded_problem) with seeded
    parameters; the flow's value is the log-odds of the mean.  mu is halved and v is a fifth of that problem's (v in [0.01, 0.11]):
    at phi <= 1 every component is U-shaped, and a q(f) as wide as that problem's puts so much mass next to 0 and 1 that even the
    2.5 % and 97.5 % quantiles leave the doubles strictly inside (0, 1) (1 - t ~ 4e-19 at phi = 0.5)."""
    if kind == "empty":
        pr = seeded_problem("sal2", N, S, seed=seed)
        pr["program"], pr["theta"] = [], torch.zeros(0, dtype=F64)
    else:
        pr = seeded_problem(kind, N, S, seed=seed)
    pr["mu"], pr["v"] = 0.5 * pr["mu"], 0.2 * pr["v"]
    pr["lvn"] = torch.tensor([math.log(phi)], dtype=F64)
    return pr


def hard_problem(kind, phi):
    """Six rows at S = 32 for the probabilities HARD_PROBS.  phi = 1000: v in {0, 0, 1e-4, 1e-4, 1, 1}, which keeps every node
    value inside the covered |g| <= 12.  phi = 0.5: both shape
    parameters of every component are below 0.5, the 1e-6 quantile is of the size (1e-6)^(1 / a) and the 1 - 1e-6 quantile is
    1 - (1e-6)^(1 / b): for both to be doubles strictly inside (0, 1) the flow's value must sit where a >= 0.02 and b >= 0.4, and
    the nodes must stay together -- mu is moved to a flow value near -2.3 and v in {0, 0, 1e-4, 1e-4, 0.02, 0.02}."""
    pr = quant_problem(kind, 6, 32, phi, seed=21)
    if phi < 1.0:
        pr["v"] = torch.tensor([0.0, 0.0, 1e-4, 1e-4, 0.02, 0.02], dtype=F64)
        lo, hi = torch.full((6,), -30.0, dtype=F64), torch.full((6,), 30.0, dtype=F64)
        want = torch.tensor([-2.2, -2.4, -2.3, -2.5, -2.2, -2.4], dtype=F64)
        for _ in range(80):      # the flows are increasing: bisection for G(mu) = want
            mid = 0.5 * (lo + hi)
            below = BM.G(mid.reshape(1, -1), pr["program"], pr["theta"]).reshape(-1) < want
            lo, hi = torch.where(below, mid, lo), torch.where(below, hi, mid)
        pr["mu"] = 0.5 * (lo + hi)
    else:
        pr["v"] = torch.tensor([0.0, 0.0, 1e-4, 1e-4, 1.0, 1.0], dtype=F64)
    assert float(node_values(pr).abs().max()) <= 12.0
    return pr


def solve(pr, probs, count=None):
    return BM.quantiles(pr["mu"], pr["v"], pr["lvn"], probs, pr["xs"], pr["wn"], pr["program"], pr["theta"], pr["rowp"], count)


def node_values(pr):
    return BM.nodes(pr["mu"], pr["v"], pr["xs"], pr["program"], pr["theta"], pr["rowp"])


def worst_root_residual(pr, probs, t, tails=BM.tails_ref):
    """The largest beta_model.residual_within_ulp over the roots t (Q,N), F through `tails`."""
    phi = round(BM.precision_of(pr["lvn"]), 9)
    g = node_values(pr)
    return max(float(BM.residual_within_ulp(g, pr["wn"], phi, t[qi], p, tails).max()) for qi, p in enumerate(probs))


def all_quant_inputs():
    """(label, problem, probabilities) of every quantile input the GPU tests use."""
    for kind, N, S, phi, probs in QUANT_CASES:
        yield "%s-N%d-S%d-phi%g-Q%d" % (kind, N, S, phi, len(probs)), quant_problem(kind, N, S, phi, seed=N + S), probs
    for kind, phi in HARD_CASES:
        yield "hard-%s-phi%g" % (kind, phi), hard_problem(kind, phi), HARD_PROBS


# ---------------------------------------------------------------------------------------------------
# constants
# ---------------------------------------------------------------------------------------------------
def test_abi_constants():
    hdr = open(os.path.join(REPO, "include", "tgp_hip.h")).read()
    assert re.search(r"#define TGP_LIK_BETA 12\b", hdr)
    assert re.search(r"#define TGP_BETA_MIN_PRECISION 0\.5\b", hdr) and re.search(r"#define TGP_BETA_MAX_PRECISION 1e3\b", hdr)
    assert re.search(r"#define TGP_VERSION 104\b", hdr)          # no struct, signature or version change
    assert L.LIK_BETA == 12 and L.BETA_MIN_PRECISION == 0.5 and L.BETA_MAX_PRECISION == 1e3
    assert (BM.PMIN, BM.PMAX) == (L.BETA_MIN_PRECISION, L.BETA_MAX_PRECISION)
    cap = int(re.search(r"#define TGP_BETA_CF_MAXIT (\d+)\b", hdr).group(1))
    assert cap == L.BETA_CF_MAXIT == BM.CF_MAXIT == 2 * CF_STEPS_FINE
    assert L.LIK_DISPLAY[L.LIK_BETA] == "Beta"
    assert L.load().tgp_version() == 104


# ---------------------------------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------------------------------
def test_log_p_is_torch_beta():
    g = torch.Generator().manual_seed(7)
    for phi in PHIS + [3.7]:
        gg = 2.0 * torch.randn(2000, generator=g, dtype=F64)
        y = (0.001 + 0.998 * torch.rand(2000, generator=g, dtype=F64))
        lam = torch.tensor(math.log(phi), dtype=F64)
        ours = BM.log_p(y, gg, lam)
        ref = torch.distributions.Beta(torch.sigmoid(gg) * phi, torch.sigmoid(-gg) * phi).log_prob(y)
        err = float(((ours - ref).abs() / ref.abs().clamp(min=1.0)).max())
        print("phi = %g: max relative difference of log p %.3e" % (phi, err))
        assert err <= 1e-10
        # the header's derivatives, point by point, against autograd
        gr = gg.clone().requires_grad_(True)
        ll = torch.full_like(gg, math.log(phi)).requires_grad_(True)
        dg, dl = torch.autograd.grad(BM.log_p(y, gr, ll).sum(), [gr, ll])
        mu, nu = torch.sigmoid(gg), torch.sigmoid(-gg)
        a, b = mu * phi, nu * phi
        ys, l1 = torch.log(y) - torch.log1p(-y), torch.log1p(-y)
        pa, pb, pp = torch.digamma(a), torch.digamma(b), float(torch.digamma(torch.tensor(phi, dtype=F64)))
        want_g = mu * nu * phi * (ys - pa + pb)
        want_l = phi * (pp - mu * pa - nu * pb + mu * ys + l1)
        size_g = mu * nu * phi * (ys.abs() + pa.abs() + pb.abs())
        size_l = phi * (abs(pp) + mu * pa.abs() + nu * pb.abs() + mu * ys.abs() + l1.abs())
        assert float(((dg - want_g).abs() / size_g).max()) <= 1e-12
        assert float(((dl - want_l).abs() / size_l).max()) <= 1e-12


def test_port_against_mpmath():
    """The numpy port of the device's incomplete beta function against mpmath at 120 digits on the grid of the issue."""
    mp = BM._mp(120)
    floor = mp.mpf(MIN_TAIL)
    most = 0
    for phi in PHIS:
        worst, by_g = 0.0, {}
        for g in GRID_G:
            a, b, nlb = BM.node_table(np.array([g]), phi)
            lo, up, h, steps = BM.component_port(a, b, nlb, GRID_X)
            most = max(most, int(steps.max()))
            wg = 0.0
            for i, x in enumerate(GRID_X):
                rl, ru, rd = BM.mp_component(phi, g, x=x, dps=120)
                for got, ref in ((lo[i], rl), (up[i], ru)):
                    if ref >= floor:
                        wg = max(wg, float(abs(mp.mpf(float(got)) - ref) / ref))
                if rd >= floor:
                    assert float(abs(mp.mpf(float(h[i])) - rd) / rd) <= 3e-12
                assert abs(float(lo[i]) + float(up[i]) - 1.0) <= 4e-16
            by_g[abs(g)] = max(by_g.get(abs(g), 0.0), wg)
            worst = max(worst, wg)
        print("phi = %g: worst relative error of a tail %.3e (recorded %.3e); by |g|: %s"
              % (phi, worst, RESIDUAL_CF_CPU[phi], {k: "%.2e" % e for k, e in by_g.items()}))
        assert worst <= CPU_HEADROOM * RESIDUAL_CF_CPU[phi]
        assert worst <= CF_BOX_TOL
    print("most steps of the continued fraction %d (recorded %d, cap %d)" % (most, CF_STEPS_CPU, BM.CF_MAXIT))
    assert most <= CF_STEPS_CPU < BM.CF_MAXIT
    # the ends: nothing below x = -inf, nothing above x = +inf; a NaN runs to the cap and stays one
    a, b, nlb = BM.node_table(np.array([0.3]), 10.0)
    lo, up, h, steps = BM.component_port(a, b, nlb, np.array([-np.inf, np.inf, np.nan]))
    assert lo[:2].tolist() == [0.0, 1.0] and up[:2].tolist() == [1.0, 0.0] and h[:2].tolist() == [0.0, 0.0]
    assert np.isnan(lo[2]) and np.isnan(up[2]) and int(steps[2]) == BM.CF_MAXIT


def test_quick_reference_against_mpmath():
    """beta_model.tails_ref, the reference of the GPU tests: scipy.special.betainc against mpmath where it is used -- both shape
    parameters at least 1, phi in {2, 10, 100, 1000}, 25 node values in [-12, 12], x on the grid, the same doubles a, b and t on
    both sides -- and the whole of tails_ref, as a mixture, against tails_mp on the rows of the Q <= 3 quantile inputs."""
    from scipy.special import betainc
    mp = BM._mp(60)
    worst = 0.0
    t = 1.0 / (1.0 + np.exp(-GRID_X))
    for phi in (2.0, 10.0, 100.0, 1000.0):
        for g in np.linspace(-12.0, 12.0, 25):
            a, b = phi / (1.0 + np.exp(-g)), phi / (1.0 + np.exp(g))
            if min(a, b) < BM.SCIPY_MIN_SHAPE:
                continue
            lo, up = betainc(a, b, t), betainc(b, a, 1.0 - t)
            for i in range(t.size):
                A, B, T = mp.mpf(float(a)), mp.mpf(float(b)), mp.mpf(float(t[i]))
                for got, ref in ((lo[i], mp.betainc(A, B, 0, T, regularized=True)), (up[i], mp.betainc(B, A, 0, 1 - T, regularized=True))):
                    if ref > mp.mpf("1e-290"):
                        worst = max(worst, float(abs(mp.mpf(float(got)) - ref) / ref))
    print("scipy.special.betainc at shapes >= 1: worst relative error of a tail %.3e (recorded %.3e)" % (worst, SCIPY_BIG_SHAPE_ERR))
    assert worst <= CPU_HEADROOM * SCIPY_BIG_SHAPE_ERR
    worst = 0.0
    for label, pr, probs in all_quant_inputs():
        if len(probs) > 3:
            continue
        phi = round(BM.precision_of(pr["lvn"]), 9)
        g = node_values(pr)
        gen = torch.Generator().manual_seed(5)
        tt = torch.sigmoid(g.mean(0) + 3.0 * (2.0 * torch.rand(g.shape[1], generator=gen, dtype=F64) - 1.0))
        ls, us, _ = BM.tails_ref(g, pr["wn"], phi, t=tt)
        lm, um, _ = BM.tails_mp(g, pr["wn"], phi, t=tt, want="lu")
        worst = max(worst, float(torch.maximum((ls - lm).abs() / lm, (us - um).abs() / um).max()))
    print("tails_ref on the quantile inputs: worst relative error of a tail %.3e (recorded %.3e)" % (worst, REF_ROWS_ERR))
    assert worst <= CPU_HEADROOM * REF_ROWS_ERR


def test_cf_steps_on_a_fine_grid():
    """The trip count that TGP_BETA_CF_MAXIT doubles: 193 node values in [-12, 12] by 481 points x in [-15, 15], seven values of
    phi; and beyond the box, at the probes of a doubling bracket (|x| up to 700), the count stays below the cap as well."""
    gs = np.linspace(-12.0, 12.0, 193)[:, None]
    most = 0
    for xs in (np.linspace(-15.0, 15.0, 481), np.array([-700.0, -200.0, -60.0, -30.0, 30.0, 60.0, 200.0, 700.0])):
        for phi in (0.5, 1.0, 3.0, 10.0, 100.0, 300.0, 1000.0):
            a, b, nlb = BM.node_table(gs, phi)
            lo, up, h, steps = BM.component_port(a, b, nlb, np.broadcast_to(xs[None, :], (gs.shape[0], xs.size)))
            assert np.isfinite(lo).all() and np.isfinite(up).all()
            most = max(most, int(steps.max()))
    print("most steps of the continued fraction on the fine grid %d (recorded %d)" % (most, CF_STEPS_FINE))
    assert most <= CF_STEPS_FINE


def test_quadrature_moments_and_logp():
    """pred_torch on the empty program: the moments are the plain sums over the nodes, Var[y] obeys the law of total variance
    against a Monte-Carlo draw, and logp is the log of the mixture density."""
    from oracle import tgp_oracle as orc
    xs, ws = orc.hermgauss(32)
    wn = ws / math.sqrt(math.pi)
    mu, v = torch.tensor([0.3, -1.0], dtype=F64), torch.tensor([0.5, 0.0], dtype=F64)
    lam = torch.tensor([math.log(10.0)], dtype=F64)
    Y = torch.tensor([0.4, 0.2], dtype=F64)
    m1, m2, lp = BM.pred_torch(mu, v, lam, [], None, xs, wn, Y=Y)
    torch.manual_seed(0)
    f = mu.reshape(1, -1) + torch.sqrt(v).reshape(1, -1) * torch.randn(400000, 2, dtype=F64)
    s = torch.distributions.Beta(torch.sigmoid(f) * 10.0, torch.sigmoid(-f) * 10.0).sample()
    assert float((s.mean(0) - m1).abs().max()) < 2e-3 and float((s.var(0) - m2).abs().max()) < 2e-3
    g = BM.nodes(mu, v, xs, [], None)
    dens = (wn.reshape(-1, 1) * torch.exp(BM.log_p(Y.reshape(1, -1), g, lam.reshape(())))).sum(0)
    assert float((lp - torch.log(dens)).abs().max()) <= 1e-12
    # a row without variance is one Beta
    one = torch.distributions.Beta(torch.sigmoid(mu[1]) * 10.0, torch.sigmoid(-mu[1]) * 10.0)
    assert abs(float(lp[1]) - float(one.log_prob(Y[1]))) <= 1e-12 and abs(float(m2[1]) - float(one.variance)) <= 1e-15


def test_root_rule_on_the_gpu_inputs():
    """Zero failures on every input tests/test_gpu_beta.py uses, roots strictly inside (0, 1) and increasing in p, each within
    the allowance of its phi through the reference CDF; the evaluations of F a root takes stay below the kernel's 128 per phase."""
    most = 0
    for label, pr, probs in all_quant_inputs():
        count = []
        t, failed, x = solve(pr, probs, count)
        assert failed == 0 and bool(torch.isfinite(x).all()) and bool(((t > 0) & (t < 1)).all()), label
        most = max(most, max(count))
        order = sorted(range(len(probs)), key=lambda i: probs[i])
        assert bool((x[order][1:] > x[order][:-1]).all()) and bool((t[order][1:] > t[order][:-1]).all()), label
        phi = round(BM.precision_of(pr["lvn"]), 9)
        r = worst_root_residual(pr, probs, t)
        rm = worst_root_residual(pr, probs, t, BM.tails_mp) if len(probs) <= 3 else float("nan")      # (mpmath where it is quick)
        print("residual %-30s %.3e (mpmath: %.3e)   (allowance of phi = %g: %.3e), most evaluations %d"
              % (label, r, rm, phi, RESIDUAL_CF_CPU[phi], max(count)))
        assert r <= CPU_HEADROOM * RESIDUAL_CF_CPU[phi] and not rm > CPU_HEADROOM * RESIDUAL_CF_CPU[phi], label
    print("most evaluations of F for one root %d" % most)
    assert most <= BM.MAXIT


def test_cdf_outside_the_interval():
    pr = quant_problem("sal2", 5, 16, 10.0, seed=1)
    Y = torch.tensor([0.0, -1.0, 1.0, 2.0, 0.3], dtype=F64)
    c, s = BM.cdf_ref(pr["mu"], pr["v"], pr["lvn"], Y, pr["xs"], pr["wn"], pr["program"], pr["theta"], tails=BM.tails_mp)
    tot = float(pr["wn"].sum())
    assert c[:2].tolist() == [0.0, 0.0] and s[:2].tolist() == [tot] * 2
    assert c[2:4].tolist() == [tot] * 2 and s[2:4].tolist() == [0.0, 0.0]
    assert 0.0 < float(c[4]) < 1.0 and abs(float(c[4] + s[4]) - tot) <= 1e-15


# ---------------------------------------------------------------------------------------------------
# the class, its traits and its refusals
# ---------------------------------------------------------------------------------------------------
def test_trait_table():
    from tgp.pytorch_amd import likelihoods as LK
    base = LK.Likelihood
    lik = LK.Beta()
    traits = [n for n in vars(base) if not n.startswith("_") and not callable(getattr(base, n))
              and not isinstance(vars(base)[n], (staticmethod, classmethod))]
    for n in traits:
        getattr(lik, n)                                  # every trait is defined
    assert lik.display == "beta" and lik.lik_id == L.LIK_BETA == 12 and lik.engine_name == "beta"
    assert lik.kind == "regression" and lik.has_noise is True and lik.has_flow is True and lik.one_launch_logp is True
    assert lik.flow_on_targets is False and lik.compiles_flows is False and lik.num_latent == 1 and lik.composed is False
    assert lik.refuses_cdf is None
    assert lik.refuses_crps.count("%s") == 1 and "no closed pair term" in lik.refuses_crps and "Betas" in lik.refuses_crps
    assert lik.refuses_input_dependent == LK.NO_INPUT_DEPENDENT % lik.display
    assert lik.refuses_optimal_qu == LK.NOT_GAUSSIAN_IN_F % lik.display and lik.refuses_optimal_qu_id is None
    assert lik.refuses_mean is None and lik.refuses_paths is None and lik.refuses_full_cov is None
    assert "beta" in lik.outputs_refusal
    assert lik.lik_kwargs() == {"lik": L.LIK_BETA, "df": None}
    assert [n for n, _ in lik.named_parameters()] == ["log_precision"] and list(lik.state_dict()) == ["log_precision"]
    assert lik.log_precision.shape == (1,) and abs(float(lik.log_precision.detach()) - math.log(10.0)) < 1e-15
    assert lik.noise().shape == (1,) and lik.noise().requires_grad and lik.noise().data_ptr() == lik.log_precision.data_ptr()
    assert abs(float(LK.Beta(precision_init=2.5).precision) - 2.5) < 1e-15 and not LK.Beta(2.5).precision.requires_grad
    assert LK.Beta(quadrature_points=7).quad_points == 7
    for bad in (0.0, 0.1, -1.0, 2e3, float("nan")):
        with pytest.raises(ValueError, match="precision"):
            LK.Beta(precision_init=bad)
    LK.Beta(precision_init=0.5), LK.Beta(precision_init=1e3)
    for bad in ([[0.5], [0.0]], [[0.5], [1.0]], [[-0.2]], [[1.5]], [[float("nan")]], [[float("inf")]]):
        with pytest.raises(ValueError, match="proportions"):
            lik.check_targets(torch.tensor(bad, dtype=F64))
    lik.check_targets(torch.tensor([[1e-300], [1.0 - 1e-16], [0.5]], dtype=F64))
    # the precision-range check of the exact CDF / quantiles
    lik.check_precision()
    with torch.no_grad():
        lik.log_precision.fill_(math.log(0.1))
    with pytest.raises(ValueError, match=r"\[0\.5, 1000\]"):
        lik.check_precision()
    with torch.no_grad():
        lik.log_precision.fill_(math.log(2e3))
    with pytest.raises(ValueError, match=r"\[0\.5, 1000\]"):
        lik.check_precision()
    # draws: inside (0, 1), mean sigmoid(f), variance mu (1 - mu) / (1 + phi)
    lik2 = LK.Beta(precision_init=4.0)
    torch.manual_seed(0)
    f = torch.full((1, 60000), math.log(0.3 / 0.7), dtype=F64)
    s = lik2.sample_from_output(f, 0)
    assert s.shape == f.shape and bool(((s > 0) & (s < 1)).all())
    assert abs(float(s.mean()) - 0.3) < 0.005 and abs(float(s.var()) - 0.3 * 0.7 / 5.0) < 0.002


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
    from tgp.pytorch_amd.likelihoods import Beta
    from tgp.pytorch_amd.models import sparse_MF_GP, sparse_MF_SP
    X = torch.randn(30, D, dtype=F64)
    K = instance_kernel("scale_rbf", ard_num_dim=D, num_multioutput=num_outputs, kernel_is_shared=False,
                        init_params={"length_scale": 2.0, "kernel_scale": 2.0, "noisy_variance": 1e-6})
    lik = Beta()
    if kind == "svgp":
        return sparse_MF_GP(["zero", K], X, X[:M].clone(), 30, lik, num_outputs, True, False, False, False, False, 0.0), X
    flow = SAL(1) if kind == "tgp" else SAL(1, input_dependent=True, input_dim=D, num_hidden_layers=1, batch_norm=0, dropout=0.5,
                                            hidden_dim=8, hidden_activation="tanh", inference="MC_dropout")
    return sparse_MF_SP(["zero", K], X, X[:M].clone(), 30, lik, num_outputs, True, False, False, False, False,
                        [flow] * num_outputs, "single", 0.0), X


def test_state_names_and_model_refusals(monkeypatch):
    for kind in ("svgp", "tgp"):
        model, _ = _model(kind)
        assert "likelihood.log_precision" in model.state_dict() and not any("log_var_noise" in n for n in model.state_dict())
        assert model._noise.data_ptr() == model.likelihood.log_precision.data_ptr() and model._lik_id == L.LIK_BETA
    lib = RecordingLib()
    monkeypatch.setattr(L, "load", lambda: lib)
    with pytest.raises(NotImplementedError, match="beta"):
        _model("idtgp")
    with pytest.raises(NotImplementedError, match="beta"):
        _model("svgp", num_outputs=2)
    for kind in ("svgp", "tgp"):
        model, X = _model(kind)
        Y = torch.full((30, 1), 0.5, dtype=F64)
        model.set_is_training(False)
        with pytest.raises(NotImplementedError, match="beta"):
            model.set_optimal_qu(X, Y)
        # the exact CRPS raises through the trait and points to samples=; the pmf is for count models
        with pytest.raises(NotImplementedError, match="beta.*no closed pair term.*samples=S"):
            model.predictive_crps(X, Y)
        with pytest.raises(NotImplementedError, match="predictive_pmf"):
            model.predictive_pmf(X, 5)
        # targets on or outside the ends of the interval: said before any library call
        model.set_is_training(True)
        for bad in (0.0, 1.0, float("nan")):
            Yb = Y.clone()
            Yb[3] = bad
            with pytest.raises(ValueError, match="proportions"):
                model.likelihood.check_targets(Yb)
        model.set_is_training(False)
        # a precision that has left the range: the exact CDF and quantiles say so before any library call
        with torch.no_grad():
            model.likelihood.log_precision.fill_(math.log(2e3))
        for call in (lambda: model.predictive_quantiles(X, [0.5]), lambda: model.predictive_cdf(X, Y),
                     lambda: model.predictive_interval_score(X, Y)):
            with pytest.raises(ValueError, match=r"\[0\.5, 1000\]"):
                call()
    assert lib.calls == []


def test_library_entries_for_the_id():
    """The CRPS entry refuses TGP_LIK_BETA before it reads a pointer and names the id; the quantile and CDF entries do not
    refuse the id (an argument error, not TGP_E_UNSUPPORTED, for a model without nodes); the step's workspace is the general-M
    path's."""
    import ctypes
    h = L.load()
    buf = torch.zeros(16, dtype=F64)
    st = torch.zeros(1, dtype=torch.int32)
    p, ps = ctypes.c_void_p(buf.data_ptr()), ctypes.c_void_p(st.data_ptr())
    md = L.TgpModel()
    md.N, md.D, md.M, md.S, md.lik = 4, 1, 1, 8, L.LIK_BETA
    md.log_var_noise = p
    rc = h.tgp_predict_crps_f64(md, p, p, None, p, p, None, None)
    assert rc == L.E_UNSUPPORTED and b"lik = 12" in h.tgp_last_error()
    assert h.tgp_predict_quantile_f64(md, p, p, None, p, p, 1, p, ps, None) == -1        # xs, wn missing
    assert h.tgp_predict_cdf_f64(md, p, p, None, p, p, None, None) == -1
    md.S = 257
    assert h.tgp_predict_cdf_f64(md, p, p, None, p, p, None, None) == L.E_UNSUPPORTED and b"S = 257" in h.tgp_last_error()
    shape = (300, 3, 20, 16, 1, 4, 0, L.KERNELS["scale_rbf"], 0)
    assert h.tgp_workspace_bytes_lik(*shape, L.LIK_BETA) == h.tgp_workspace_bytes_lik(*shape, L.LIK_GAMMA)
    assert h.tgp_workspace_bytes_lik(*shape, L.LIK_BETA) != h.tgp_workspace_bytes_lik(*shape, L.LIK_FLOW)
    # the Student-t mixture keeps its refusal
    md.S, md.lik = 8, L.LIK_STUDENT
    assert h.tgp_predict_cdf_f64(md, p, p, None, p, p, None, None) == L.E_UNSUPPORTED and b"incomplete beta" in h.tgp_last_error()


def test_engine_refusal_and_surface():
    from tgp.pytorch_amd import ops
    from tgp.pytorch_amd.engine import engine_refusal
    assert "Beta" in engine_refusal(likelihood="beta") and "eager path" in engine_refusal(likelihood="beta")
    assert "Beta" in engine_refusal(likelihood="beta", minibatch=True)
    assert callable(ops.ell_beta) and callable(ops.EllBetaFunction.apply)
    lvn = torch.zeros(1, dtype=F64)
    with pytest.raises(L.TgpError, match="Beta"):
        ops.predict_quantiles(lvn, lvn, lvn, [0.5], lik=L.LIK_BETA)                     # needs a FlowSpec
    with pytest.raises(L.TgpError, match="Beta"):
        ops.predict_cdf(lvn, lvn, lvn, lvn, lik=L.LIK_BETA)


def test_cli_arguments():
    run = lambda *a: subprocess.run([sys.executable, "-m", "tgp.pytorch_amd.main"] + list(a), cwd=REPO, capture_output=True,
                                    text=True, timeout=120)
    out = run("--help")
    assert out.returncode == 0 and "beta" in out.stdout and "--precision_init" in out.stdout and "synthetic_proportions" in out.stdout
    tail = ["--train_test_seed_split", "1", "--num_inducing", "5"]
    bad = run("--model", "SVGP", "--likelihood", "beta", "--dataset", "synthetic_power", *tail)
    assert bad.returncode == 2 and "proportion data sets" in bad.stderr
    bad = run("--model", "SVGP", "--dataset", "synthetic_proportions", *tail)
    assert bad.returncode == 2 and "proportion data sets" in bad.stderr
    bad = run("--model", "ID_TGP", "--likelihood", "beta", "--dataset", "synthetic_proportions", *tail)
    assert bad.returncode == 2 and "--likelihood beta: SVGP or TGP only" in bad.stderr
    bad = run("--model", "SVGP", "--likelihood", "beta", "--precision_init", "0.1", "--dataset", "synthetic_proportions", *tail)
    assert bad.returncode == 2 and "--precision_init" in bad.stderr


def test_proportions_dataset(monkeypatch):
    from tgp.pytorch_amd import config as cg
    from tgp.pytorch_amd import data, main, synthetic
    X, Y = synthetic.synthetic_proportions()
    n, d = synthetic.PROPORTIONS_SHAPE
    assert (n, d) == (500, 2) and X.shape == (n, d) and Y.shape == (n, 1) and synthetic.PROPORTIONS_PRECISION == 10.0
    assert np.array_equal(Y, synthetic.synthetic_proportions(seed=0)[1])
    assert not np.array_equal(Y, synthetic.synthetic_proportions(seed=1)[1])
    assert np.all(Y >= 1e-6) and np.all(Y <= 1.0 - 1e-6)
    # Var[y | x] = mu (1 - mu) / 11 around the true mean, the probit of the latent function
    eta = 1.5 * np.sin(2.0 * X[:, 0]) + 0.5 * X[:, 1]
    mu = 0.5 * (1.0 + np.array([math.erf(e / math.sqrt(2.0)) for e in eta]))
    ratio = float(((Y[:, 0] - mu) ** 2).mean() / (mu * (1.0 - mu)).mean())
    print("E[(y - mu)^2] / E[mu (1 - mu)] = %.4f (1 / (1 + precision) = 0.0909)" % ratio)
    assert abs(ratio - 1.0 / 11.0) < 0.015
    monkeypatch.setattr(cg, "device", "cpu", raising=False)
    loaders, dc = data.return_dataset("synthetic_proportions", 10000, seed=1)
    assert dc["precision"] == 10.0 and dc["N_tr"] == 450 and dc["N_te"] == 50 and dc["Dx"] == d and len(loaders) == 2
    assert float(np.asarray(dc["Y_std"]).reshape(-1)[0]) == 1.0 and float(np.asarray(dc["Y_mean"]).reshape(-1)[0]) == 0.0
    assert np.array_equal(dc["Y_tr"].numpy(), Y[dc["train_idx"]])                         # raw targets: not centred, not scaled
    assert main.PROPORTION_DATASETS == ("synthetic_proportions",) and ("TGP", "proportions") in main.HYPER
