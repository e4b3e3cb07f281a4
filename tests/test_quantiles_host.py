"""CPU: the exact predictive quantiles / CDF without a GPU -- the torch restatement of csrc/tgp_quantile.hip
(tests/quantile_model.py) on the reference's fixtures (tests/golden/q_*.npz, tools/gen_golden_quantiles.py), against an
independent bisection and against the reference's sampled quantiles; the hard inputs of the root rule; the host side
(probabilities, confidence_intervals on a stub model, the library's refusals, which never reach the device).

Residual of a root t at probability p:  |sum_s wn_s Phi(+-(t - g_s) / sigma) - min(p, 1 - p)| / min(p, 1 - p), the tail that is
small at p, formed from the node values g_s the REFERENCE's flow returned (for the identity: the one Gaussian of variance
v + noise).  RESIDUAL_CPU[case] is that figure for the restatement's roots, worst over the rows and the fixture's three
probabilities, measured here (test_fixture_residuals prints it): between 2.4e-15 (the closed form) and 7.5e-14 -- a few
ulp of the sum divided by 0.025.  This file holds the restatement to 2x each figure (head room for another libm); the GPU
test allows the device 10x each case's own figure.

Roots with no fixture (the seeded problems and the hard inputs below, also used by tests/test_gpu_quantiles.py) are held to
`residual_bound`, which follows from the stopping rule and the number format, not from any result:
    |F(t) - p| <= min(p, 1 - p) 2^-46 + F'(t) max(1, |t|) (2 * 2^-50 + node_tol)
* 2^-46 = 64 ulp: a term's relative error is a few ulp from erfc plus z^2 ulp from the rounding of z, and z^2 < 45 for
  every term that reaches 1e-10 of the sum;
* 2 * 2^-50 max(1, |t|) F'(t): the iteration stops at a step <= 2^-50 max(1, |t|) (after a bisection the root is within two
  such steps), and rounding t - g_s moves F by as much as an error of one ulp of t would;
* node_tol = 0 when F is evaluated by the implementation that found the root, 1e-9 (the project's value tolerance) when the
  other implementation's node values are used.
"""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

from conftest import load_golden
import quantile_model as qm
from oracle import tgp_oracle as orc

F64 = torch.float64
CASES = ["q_bcl_al1", "q_idsal1", "q_med_sal2", "q_med_tanh3x2", "q_s100_sal2", "q_tiny_svgp"]
TOL_VAL = 1e-9
CPU_HEADROOM = 2.0
# measured by test_fixture_residuals (it prints the figure per case), see the docstring
RESIDUAL_CPU = {
    "q_bcl_al1": 7.45e-14,
    "q_idsal1": 1.96e-14,
    "q_med_sal2": 2.41e-14,
    "q_med_tanh3x2": 7.09e-14,
    "q_s100_sal2": 1.01e-14,
    "q_tiny_svgp": 2.36e-15,
}
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


# ---------------------------------------------------------------------------------------------------
# shared with tests/test_gpu_quantiles.py
# ---------------------------------------------------------------------------------------------------
_fix_cache = {}


def fixture(name):
    """Fixture + wn, the restatement's roots and the bisection's, computed once."""
    if name not in _fix_cache:
        g = load_golden(name)
        g["wn"] = g["ws"] / math.sqrt(math.pi)
        g["rowp"] = g.get("rowp")
        g["probs"] = [float(p) for p in g["probs"]]
        g["t"], g["failed"] = qm.quantiles(g["mu"], g["v"], g["p_log_var_noise"], g["probs"], g["xs"], g["wn"], g["program"],
                                           g["p_theta"], g["rowp"])
        _fix_cache[name] = g
    return _fix_cache[name]


def reference_residual(g, t):
    """Worst residual of the roots t (Q,N) over rows and probabilities, on the reference's recorded numbers."""
    sigma = math.sqrt(math.exp(float(g["p_log_var_noise"])))
    worst = 0.0
    for qi, p in enumerate(g["probs"]):
        if len(g["program"]):
            r = qm.residual(g["g_nodes"], g["wn"], sigma, t[qi], p)
        else:
            z = (t[qi] - g["mu"]) / torch.sqrt(g["v"] + sigma * sigma)
            r = qm.residual(torch.zeros(1, z.numel(), dtype=F64), torch.ones(1, dtype=F64), 1.0, z, p)
        worst = max(worst, float(r.max()))
    return worst


def residual_bound(dens, t, p, node_tol=0.0):
    """The docstring's bound on |F(t) - p| / min(p, 1 - p)."""
    q = min(p, 1.0 - p)
    return 2.0 ** -46 + dens * t.abs().clamp_min(1.0) * (2.0 * qm.STEP_TOL + node_tol) / q


def root_tolerance(dens, t, p):
    """How far apart two computed roots of F(t) = p may lie: the project's value tolerance, 1e-9 max(1, |t|), plus what the
    evaluation noise of F leaves undetermined, 2 * 2^-46 min(p, 1 - p) / F'(t).  The second term is ~1e-15 on an ordinary row;
    it takes over only where F is flat to machine precision (nodes much further apart than sigma, with node weights that add up
    to p exactly -- the median of an even S): there every t of the plateau IS a root and only the residual says anything."""
    return TOL_VAL * t.abs().clamp_min(1.0) + 2.0 * 2.0 ** -46 * min(p, 1.0 - p) / dens


def roots_agree(g, t_a, t_b, label=""):
    """t_a, t_b (Q,N) within root_tolerance of each other on fixture g (density from the reference's nodes)."""
    sigma = math.sqrt(math.exp(float(g["p_log_var_noise"])))
    flat = 0
    for qi, p in enumerate(g["probs"]):
        if len(g["program"]):
            dens = torch.minimum(qm.tails(g["g_nodes"], g["wn"], sigma, t_a[qi])[2], qm.tails(g["g_nodes"], g["wn"], sigma, t_b[qi])[2])
        else:
            sd = torch.sqrt(g["v"] + sigma * sigma)
            dens = torch.exp(-0.5 * ((t_b[qi] - g["mu"]) / sd) ** 2) * qm.INV_SQRT_2PI / sd
        tol = root_tolerance(dens, t_b[qi], p)
        flat += int((tol > 2.0 * TOL_VAL * t_b[qi].abs().clamp_min(1.0)).sum())
        assert bool(((t_a[qi] - t_b[qi]).abs() <= tol).all()), (label, p)
    print("roots agree %-14s (%d of %d on a plateau of F)" % (label, flat, t_b.numel()))
    return flat


def seeded_problem(kind, N, S, seed=0, lvn=math.log(0.05)):
    """mu, v, noise and a flow of `kind` with seeded parameters: sal2 | tanh3x2 | bcl_al | idsal1."""
    g = torch.Generator().manual_seed(4000 + seed)
    mu = torch.randn(N, generator=g, dtype=F64)
    v = 0.05 + 0.5 * torch.rand(N, generator=g, dtype=F64)
    rowp = None
    if kind == "sal2":
        prog, theta = orc.sal_program(2)
        theta = theta + 0.2 * torch.randn(theta.shape, generator=g, dtype=F64)
        theta[1], theta[5] = theta[1].abs(), theta[5].abs()          # SAL b > 0, and the affine slopes
        theta[2], theta[6] = theta[2].abs(), theta[6].abs()
    elif kind == "tanh3x2":
        prog, theta = orc.steptanh_program(3, 2, np.random.default_rng(seed))
    elif kind == "bcl_al":
        prog = [(4, 0, 0, 0), (0, 0, 1, 0)]                           # BOXCOX lam, then AFFINE a, b
        theta = torch.tensor([1.3, 0.8, 0.1], dtype=F64)
    elif kind == "idsal1":
        prog, theta = orc.sal_program(1, per_row=True)
        theta = theta + torch.tensor([-0.1, 0.2], dtype=F64)
        rowp = torch.tensor([0.0, 1.0], dtype=F64).reshape(1, 2) + 0.2 * torch.randn(N, 2, generator=g, dtype=F64)
    else:
        raise ValueError(kind)
    xs, ws = orc.hermgauss(S)
    return {"mu": mu, "v": v, "lvn": torch.tensor([lvn], dtype=F64), "program": prog, "theta": theta, "rowp": rowp, "xs": xs,
            "wn": ws / math.sqrt(math.pi), "S": S}


def hard_problem(name):
    """The three hard inputs of the root rule and their probabilities."""
    if name == "staircase":          # sigma^2 = 1e-8 against v = 4: F is close to a staircase over the nodes
        pr = seeded_problem("sal2", 5, 32, seed=11, lvn=math.log(1e-8))
        pr["v"] = torch.full((5,), 4.0, dtype=F64)
        return pr, [0.025, 0.31, 0.5, 0.77, 0.975]
    if name == "far_tails":
        return seeded_problem("sal2", 9, 32, seed=12), [1e-6, 1.0 - 1e-6]
    if name == "bimodal":            # G(f) = f + 3 tanh(f / 0.05): q(f) straddles the step, two modes near -3 and +3
        pr = seeded_problem("tanh3x2", 6, 50, seed=13)
        pr["program"] = [(2, 1, 0, 2)]
        pr["theta"] = torch.cat([torch.tensor([0.0]), orc.inv_softplus(3.0).reshape(1), torch.tensor([0.0]),
                                 orc.inv_softplus(0.05).reshape(1)]).to(F64)
        pr["mu"] = torch.linspace(-0.3, 0.3, 6, dtype=F64)
        pr["v"] = torch.full((6,), 1.0, dtype=F64)
        return pr, [0.025, 0.25, 0.5, 0.75, 0.975]
    raise ValueError(name)


HARD = ["staircase", "far_tails", "bimodal"]


def solve(pr, probs):
    return qm.quantiles(pr["mu"], pr["v"], pr["lvn"], probs, pr["xs"], pr["wn"], pr["program"], pr["theta"], pr["rowp"])


def check_residuals(pr, probs, t, node_tol=0.0, label=""):
    """Every root of t (Q,N) within residual_bound on the restatement's F; returns the worst residual / bound."""
    sigma = math.sqrt(math.exp(float(pr["lvn"])))
    g = qm.nodes(pr["mu"], pr["v"], pr["xs"], pr["program"], pr["theta"], pr["rowp"])
    worst = 0.0
    for qi, p in enumerate(probs):
        _, _, dens = qm.tails(g, pr["wn"], sigma, t[qi])
        ratio = qm.residual(g, pr["wn"], sigma, t[qi], p) / residual_bound(dens, t[qi], p, node_tol)
        worst = max(worst, float(ratio.max()))
    print("residual / bound %-28s %.3f" % (label, worst))
    assert worst <= 1.0, label
    return worst


# ---------------------------------------------------------------------------------------------------
# fixtures
# ---------------------------------------------------------------------------------------------------
def test_fixture_set():
    import glob
    files = glob.glob(os.path.join(GOLDEN, "q_*.npz"))
    assert sorted(os.path.basename(p)[:-4] for p in files) == CASES == sorted(RESIDUAL_CPU)
    assert max(os.path.getsize(p) for p in files) < 256 * 1024       # data only, far below the committed-file limit
    shapes = {"q_tiny_svgp": (7, 16), "q_med_sal2": (65, 32), "q_med_tanh3x2": (257, 50), "q_bcl_al1": (65, 32),
              "q_idsal1": (65, 32), "q_s100_sal2": (33, 100)}
    for name, (N, S) in shapes.items():
        g = fixture(name)
        assert g["mu"].numel() == N and g["xs"].numel() == S and tuple(g["g_nodes"].shape) == (S, N), name
        assert g["probs"] == [0.025, 0.5, 0.975] and int(g["samp_S"]) == 200000 and g["samp_rows"].numel() == min(8, N)
    assert len(fixture("q_tiny_svgp")["program"]) == 0
    assert any(b[0] >= 3 for b in fixture("q_bcl_al1")["program"])            # an extended kind
    assert any(b[3] & 4 for b in fixture("q_idsal1")["program"]) and fixture("q_idsal1")["rowp"] is not None


def test_restated_nodes_are_the_references():
    """The restatement's flow reproduces the node values the reference recorded (what F is made of)."""
    for name in CASES:
        g = fixture(name)
        mine = qm.nodes(g["mu"], g["v"], g["xs"], g["program"], g["p_theta"], g["rowp"])
        err = float(((mine - g["g_nodes"]).abs() / g["g_nodes"].abs().clamp_min(1.0)).max())
        assert err <= TOL_VAL, (name, err)


def test_fixture_residuals():
    for name in CASES:
        g = fixture(name)
        assert g["failed"] == 0, name
        r = reference_residual(g, g["t"])
        print("residual %-14s %.3e   (recorded %.3e)" % (name, r, RESIDUAL_CPU[name]))
        assert r <= CPU_HEADROOM * RESIDUAL_CPU[name], name


def test_roots_agree_with_plain_bisection():
    for name in CASES:
        g = fixture(name)
        tb = qm.bisect_quantiles(g["mu"], g["v"], g["p_log_var_noise"], g["probs"], g["xs"], g["wn"], g["program"], g["p_theta"],
                                 g["rowp"])
        flat = roots_agree(g, g["t"], tb, name)
        assert flat <= g["t"].numel() // 10, name          # the plateau rule must stay the exception


def test_roots_against_the_references_sampled_quantiles():
    """|t_exact - t_sampled| <= 6 sqrt(p (1 - p) / S) / F'(t_exact): six standard errors of a sample quantile at
    S = 200 000, on the 8 rows the reference sampled (the median included)."""
    for name in CASES:
        g = fixture(name)
        rows = g["samp_rows"].long()
        sigma = math.sqrt(math.exp(float(g["p_log_var_noise"])))
        for qi, p in enumerate(g["probs"]):
            t = g["t"][qi, rows]
            if len(g["program"]):
                _, _, dens = qm.tails(g["g_nodes"][:, rows], g["wn"], sigma, t)
            else:
                sd = torch.sqrt(g["v"][rows] + sigma * sigma)
                dens = torch.exp(-0.5 * ((t - g["mu"][rows]) / sd) ** 2) * qm.INV_SQRT_2PI / sd
            bound = 6.0 * math.sqrt(p * (1.0 - p) / float(g["samp_S"])) / dens
            assert bool(((t - g["samp_q"][qi]).abs() <= bound).all()), (name, p)


def test_symmetric_median_is_the_mean():
    """The identity's predictive is symmetric about mu: the exact median is mu itself."""
    g = fixture("q_tiny_svgp")
    assert torch.equal(g["t"][1], g["mu"])


# ---------------------------------------------------------------------------------------------------
# the root rule on inputs with no fixture
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", HARD)
def test_rule_converges_on_the_hard_inputs(name):
    pr, probs = hard_problem(name)
    t, failed = solve(pr, probs)
    assert failed == 0 and bool(torch.isfinite(t).all())
    check_residuals(pr, probs, t, label=name)
    assert bool((t[1:] > t[:-1]).all())                 # increasing in p


def test_far_tails_are_resolved_relatively():
    """p = 1e-6 and 1 - 1e-6: the residual is relative to 1e-6, so an absolute accuracy of 1e-16 would not do."""
    pr, probs = hard_problem("far_tails")
    t, _ = solve(pr, probs)
    sigma = math.sqrt(math.exp(float(pr["lvn"])))
    g = qm.nodes(pr["mu"], pr["v"], pr["xs"], pr["program"], pr["theta"], pr["rowp"])
    lower, _, _ = qm.tails(g, pr["wn"], sigma, t[0])
    _, upper, _ = qm.tails(g, pr["wn"], sigma, t[1])
    assert float((lower / 1e-6 - 1.0).abs().max()) < 1e-12 and float((upper / 1e-6 - 1.0).abs().max()) < 1e-9
    # (the upper target is 1 - p as float64 holds it, 1.0000000000287557e-06; the lower one is 1e-6 itself)
    assert float((upper / (1.0 - probs[1]) - 1.0).abs().max()) < 1e-12


def test_zero_variance_row_takes_its_closed_form():
    pr = seeded_problem("sal2", 5, 8, seed=3)
    pr["v"][2] = 0.0
    probs = [0.9, 0.1]
    t, failed = solve(pr, probs)
    assert failed == 0
    sigma = math.sqrt(math.exp(float(pr["lvn"])))
    zq = torch.special.ndtri(torch.tensor(probs, dtype=F64))
    want = qm.G(pr["mu"][2:3], pr["program"], pr["theta"]) + zq * sigma
    assert torch.equal(t[:, 2], want)


def test_out_of_evaluations_is_counted_not_looped_on():
    """A flow that overflows to +inf at the start leaves nothing to bracket: NaN and a count, after a bounded number of steps."""
    pr = seeded_problem("sal2", 3, 8, seed=5)
    pr["mu"] = torch.tensor([0.0, 1e200, 0.0], dtype=F64)
    t, failed = solve(pr, [0.3])
    assert failed == 1 and bool(torch.isnan(t[0, 1])) and bool(torch.isfinite(t[0, [0, 2]]).all())


# ---------------------------------------------------------------------------------------------------
# host side
# ---------------------------------------------------------------------------------------------------
def test_probabilities_unsorted_single_and_rejected():
    from tgp.pytorch_amd import ops
    p, zq = ops.quantile_probs([0.975, 0.025, 0.5])
    assert p.tolist() == [0.975, 0.025, 0.5] and zq.dtype == F64
    assert abs(float(zq[0]) - 1.959963984540054) < 1e-14 and abs(float(zq[1]) + float(zq[0])) < 1e-14 and float(zq[2]) == 0.0
    p1, z1 = ops.quantile_probs(0.5)
    assert p1.shape == (1,) and z1.shape == (1,)
    for bad in ([0.0], [1.0], [float("nan")], [0.5, -0.1], [0.5, 1.5]):
        with pytest.raises(ValueError):
            ops.quantile_probs(bad)
    # the restatement keeps the caller's order too
    pr = seeded_problem("sal2", 4, 8, seed=1)
    a, _ = solve(pr, [0.975, 0.025, 0.5])
    b, _ = solve(pr, [0.025, 0.5, 0.975])
    assert torch.equal(a[0], b[2]) and torch.equal(a[1], b[0]) and torch.equal(a[2], b[1])
    c, _ = solve(pr, [0.5])
    assert c.shape == (1, 4) and torch.equal(c[0], b[1])


class _StubModel:
    """What confidence_intervals(exact=False) asks of a model: the two samplers, with this package's return values."""
    out_dim = 1

    def sample_from_predictive_distribution(self, X, S):
        N = X.shape[0]
        s = torch.arange(S, dtype=F64).reshape(1, S, 1, 1) + 100.0 * torch.arange(N, dtype=F64).reshape(1, 1, N, 1)
        return s, None, None

    def sample_from_variational_marginal(self, X, S, diagonal, is_duvenaud, init_Z=None):
        assert diagonal and not is_duvenaud
        N = X.shape[0]
        s = torch.arange(S, dtype=F64).reshape(S, 1) - 100.0 * torch.arange(N, dtype=F64).reshape(1, N)
        return s.reshape(1, S * N), None, None, None


def test_confidence_intervals_sampled_structure():
    from tgp.pytorch_amd import utils
    X = torch.zeros(5, 3, dtype=F64)
    for dist, sign in (("predictive", 1.0), ("posterior", -1.0)):
        ci = utils.compute_95_and_median_confidence_intervals(_StubModel(), X, 101, dist, False)
        assert isinstance(ci, list) and len(ci) == 1 and isinstance(ci[0], list) and len(ci[0]) == 3
        for arr, q in zip(ci[0], (2.5, 50.0, 97.5)):           # numpy.quantile of 0..100 per row
            assert isinstance(arr, np.ndarray) and arr.shape == (5, 1)
            assert np.allclose(arr[:, 0], q + sign * 100.0 * np.arange(5), rtol=0, atol=1e-12)
    ci = utils.confidence_intervals(_StubModel(), X, [0.1], 11, "predictive", False)
    assert len(ci[0]) == 1 and ci[0][0].shape == (5, 1) and np.allclose(ci[0][0][:, 0], 1.0 + 100.0 * np.arange(5))
    with pytest.raises(NotImplementedError):
        utils.confidence_intervals(_StubModel(), X, [0.5], 11, "predictive", True)
    with pytest.raises(ValueError):
        utils.confidence_intervals(_StubModel(), X, [0.5], 11, "prior", False)
    with pytest.raises(AssertionError):
        utils.compute_95_and_median_confidence_intervals(_StubModel(), X, 11, "prior", False)


def test_trainer_and_cli_take_the_coverage_keyword():
    import inspect
    from tgp.pytorch_amd import main, trainers
    assert inspect.signature(trainers.Trainer_SP_regression.__init__).parameters["coverage"].default == "sampled"
    with pytest.raises(ValueError):
        trainers.Trainer_SP_regression(model=type("M", (), {"out_dim": 1})(), data_loaders=[None], validate_each=1, plot=False,
                                       track=False, Y_std=torch.ones(1), plot_each=-1, S_test=10, coverage="approximate")
    with pytest.raises(SystemExit):
        main.main(["--model", "TGP", "--dataset", "synthetic_power", "--train_test_seed_split", "1", "--num_inducing", "10",
                   "--coverage", "approximate"])


def test_library_refuses_before_any_launch():
    """S = 257, Q = 33, Q = 0 and the likelihoods without quantiles: TGP_E_UNSUPPORTED with the entry named, decided on the
    host (the pointers below are never followed).  The header's constants are the binding's."""
    from tgp.pytorch_amd import lib as L
    h = L.load()
    text = open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "tgp_hip.h")).read()
    assert "#define TGP_QUANTILE_MAX_S %d" % L.QUANTILE_MAX_S in text and "#define TGP_QUANTILE_MAX_Q %d" % L.QUANTILE_MAX_Q in text
    assert "#define TGP_VERSION 104" in text and h.tgp_version() == 104
    buf = (C.c_double * 8)()
    p = C.cast(buf, C.c_void_p)
    prog = (C.c_int32 * 4)(1, 0, 0, 0)

    def model(S, lik):
        md = L.TgpModel()
        md.N, md.D, md.M, md.S, md.nblk, md.P, md.RP, md.lik = 4, 1, 1, S, 1, 2, 0, lik
        md.log_var_noise, md.theta, md.xs, md.wn = p, p, p, p
        md.program = C.cast(prog, C.c_void_p)
        return md

    def quant(md, Q):
        return h.tgp_predict_quantile_f64(md, p, p, None, p, p, Q, p, p, None)

    for md, Q, what in ((model(257, L.LIK_FLOW), 3, b"S = 257"), (model(0, L.LIK_FLOW), 3, b"S = 0"),
                        (model(32, L.LIK_FLOW), 33, b"Q = 33"), (model(32, L.LIK_FLOW), 0, b"Q = 0"),
                        (model(32, L.LIK_BERNOULLI), 3, b"lik = 3"), (model(32, L.LIK_WARPED), 3, b"lik = 4"),
                        (model(32, L.LIK_SOFTMAX), 3, b"lik = 5")):
        assert quant(md, Q) == L.E_UNSUPPORTED
        msg = h.tgp_last_error()
        assert msg.startswith(b"tgp_predict_quantile_f64") and what in msg, msg
    for md, what in ((model(257, L.LIK_FLOW), b"S = 257"), (model(32, L.LIK_BERNOULLI), b"lik = 3")):
        assert h.tgp_predict_cdf_f64(md, p, p, None, p, p, p, None) == L.E_UNSUPPORTED
        msg = h.tgp_last_error()
        assert msg.startswith(b"tgp_predict_cdf_f64") and what in msg, msg
    # argument errors are codes too
    assert quant(None, 3) == -1
    assert h.tgp_predict_quantile_f64(model(32, L.LIK_FLOW), None, p, None, p, p, 3, p, p, None) == -2
    assert h.tgp_predict_quantile_f64(model(32, L.LIK_FLOW), p, p, None, p, p, 3, p, None, None) == -9
    assert h.tgp_predict_cdf_f64(model(32, L.LIK_FLOW), p, p, None, None, p, p, None) == -5
