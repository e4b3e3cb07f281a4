"""CPU: the exact CRPS of the Gauss-Hermite predictive without a GPU -- the torch restatement of k_pred_crps / k_crps_gauss
(tests/crps_model.py) on the reference's fixtures (tests/golden/q_*.npz) against an independent quadrature of
int (F - 1{t >= y})^2 dt, its properties, the sampled estimator and the interval score, and the host side (the library's
refusals, which never reach the device, and the models').

QUAD_CPU[case]: the worst relative difference |restatement - quadrature| / quadrature over the rows of the fixture, with seeded
targets within 3 sigma of the predictive mean and a 16-point Gauss-Legendre rule over 400 panels a side, measured here
(test_restatement_against_quadrature prints it).  This file holds the restatement to 2x each figure (head room for another
libm), as tests/test_quantiles_host.py does.  Everything else is held to crps_model.bound, which follows from the formula and
the number format (see that module)."""
import ctypes as C
import math
import os

import pytest
import torch

import crps_model as cm
import quantile_model as qm
from test_quantiles_host import CASES, GOLDEN, TOL_VAL, fixture, hard_problem, seeded_problem

F64 = torch.float64
FLOW_CASES = [c for c in CASES if c != "q_tiny_svgp"]
CPU_HEADROOM = 2.0
# measured by test_restatement_against_quadrature (it prints the figure per case), see the docstring
QUAD_CPU = {
    "q_bcl_al1": 1.56e-15,
    "q_idsal1": 3.34e-15,
    "q_med_sal2": 3.02e-15,
    "q_med_tanh3x2": 3.40e-15,
    "q_s100_sal2": 2.86e-15,
}


# ---------------------------------------------------------------------------------------------------
# shared with tests/test_gpu_crps.py
# ---------------------------------------------------------------------------------------------------
def sigma_of(lvn):
    return math.sqrt(math.exp(float(lvn)))


def targets(mu_pred, sigma, seed, spread=3.0):
    """Seeded targets within `spread` sigma of the predictive mean."""
    g = torch.Generator().manual_seed(7000 + seed)
    return mu_pred + spread * sigma * (2.0 * torch.rand(mu_pred.numel(), generator=g, dtype=F64) - 1.0)


_fix_cache = {}


def crps_fixture(name):
    """The q_* fixture with targets `y`, the restated nodes `g_mine` and the restatement's (crps, T1, T2) on them, once."""
    if name not in _fix_cache:
        g = dict(fixture(name))
        sigma = sigma_of(g["p_log_var_noise"])
        if len(g["program"]):
            g["g_mine"] = qm.nodes(g["mu"], g["v"], g["xs"], g["program"], g["p_theta"], g["rowp"])
            mean = (g["wn"].unsqueeze(1) * g["g_nodes"]).sum(0)
        else:
            g["g_mine"], mean = None, g["mu"]
        g["y"] = targets(mean, sigma, CASES.index(name))
        g["crps"] = cm.crps(g["mu"], g["v"], g["p_log_var_noise"], g["y"], g["xs"], g["wn"], g["program"], g["p_theta"], g["rowp"])
        _fix_cache[name] = g
    return _fix_cache[name]


def problem_nodes(pr):
    return qm.nodes(pr["mu"], pr["v"], pr["xs"], pr["program"], pr["theta"], pr["rowp"])


def problem_targets(pr, seed, spread=3.0):
    g = problem_nodes(pr)
    return targets((pr["wn"].unsqueeze(1) * g).sum(0), sigma_of(pr["lvn"]), seed, spread)


def restated(pr, y):
    return cm.crps(pr["mu"], pr["v"], pr["lvn"], y, pr["xs"], pr["wn"], pr["program"], pr["theta"], pr["rowp"])


def within_bound(got, want, T1, T2, S, gmax=None, node_tol=0.0, label=""):
    """|got - want| <= crps_model.bound on every row; prints the worst ratio before it asserts."""
    b = cm.bound(S, T1, T2, gmax, node_tol)
    ratio = float(((got - want).abs() / b).max())
    print("crps |delta| / bound %-32s %.3e" % (label, ratio))
    assert ratio <= 1.0, (label, ratio)
    return ratio


def closed_form(mu, v, lvn, y):
    """sd (a(z) - 1 / sqrt pi) with a(z) = z (2 Phi(z) - 1) + 2 phi(z), through ndtr: not the restatement's erf form."""
    sd = torch.sqrt(v.clamp_min(0.0) + math.exp(float(lvn)))
    z = (y - mu) / sd
    az = z * (2.0 * torch.special.ndtr(z) - 1.0) + 2.0 * torch.exp(-0.5 * z * z) * qm.INV_SQRT_2PI
    return sd * (az - 1.0 / math.sqrt(math.pi))


# ---------------------------------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FLOW_CASES)
def test_restatement_against_quadrature(name):
    assert sorted(QUAD_CPU) == sorted(FLOW_CASES)
    g = crps_fixture(name)
    sigma = sigma_of(g["p_log_var_noise"])
    c, T1, T2 = cm.crps_parts(g["g_nodes"], g["wn"], sigma, g["y"])
    quad = cm.crps_quadrature(g["g_nodes"], g["wn"], sigma, g["y"])
    rel = float(((c - quad).abs() / quad).max())
    print("crps restatement vs quadrature %-14s %.3e   (recorded %.3e)   (T1 + T2) / crps <= %.2f"
          % (name, rel, QUAD_CPU[name], float(((T1 + T2) / c).max())))
    assert rel <= CPU_HEADROOM * QUAD_CPU[name], name


def test_restated_nodes_against_the_references():
    for name in FLOW_CASES:
        g = crps_fixture(name)
        sigma = sigma_of(g["p_log_var_noise"])
        ref, T1, T2 = cm.crps_parts(g["g_nodes"], g["wn"], sigma, g["y"])
        within_bound(g["crps"][0], ref, T1, T2, g["xs"].numel(), g["g_nodes"].abs().max(0).values, TOL_VAL, name)


def test_pair_numbering_takes_every_pair_once():
    for S in (1, 2, 3, 15, 16, 17, 33, 100, 256):
        s, t = cm.pair_indices(S)
        assert s.numel() == S * (S - 1) // 2
        if S > 1:
            assert bool((s != t).all()) and int(t.max()) < S
            key = torch.minimum(s, t) * S + torch.maximum(s, t)
            assert key.unique().numel() == key.numel(), S


def test_closed_form():
    g = crps_fixture("q_tiny_svgp")
    assert len(g["program"]) == 0
    c, T1, T2 = g["crps"]
    want = closed_form(g["mu"], g["v"], g["p_log_var_noise"], g["y"])
    assert float(((c - want).abs() / want).max()) <= 16 * 2.0 ** -52
    assert torch.equal(c, T1 - T2)
    # an empty program on a flow problem: the same rule
    pr = seeded_problem("sal2", 9, 8, seed=2)
    pr["program"], pr["theta"] = [], torch.zeros(0, dtype=F64)
    y = targets(pr["mu"], 1.0, 3)
    c, _, _ = restated(pr, y)
    assert float(((c - closed_form(pr["mu"], pr["v"], pr["lvn"], y)).abs() / c).max()) <= 16 * 2.0 ** -52
    # a single-node mixture is the closed form with v = 0, exactly
    one = cm.crps_parts(pr["mu"].unsqueeze(0), torch.ones(1, dtype=F64), sigma_of(pr["lvn"]), y)
    cf = cm.gauss_parts(pr["mu"], torch.zeros(9, dtype=F64), pr["lvn"], y)
    for a_, b_ in zip(one, cf):
        assert torch.equal(a_, b_)


@pytest.mark.parametrize("kind,S", [("sal2", 32), ("tanh3x2", 50), ("bcl_al", 17), ("idsal1", 16)])
def test_properties(kind, S):
    pr = seeded_problem(kind, 13, S, seed=S)
    y = problem_targets(pr, S)
    c, T1, T2 = restated(pr, y)
    assert bool((c >= 0.0).all()) and bool((T1 >= T2).all())
    # CRPS(y) is minimal at the row's exact median (d CRPS / dy = 2 F(y) - 1)
    med, failed = qm.quantiles(pr["mu"], pr["v"], pr["lvn"], [0.5], pr["xs"], pr["wn"], pr["program"], pr["theta"], pr["rowp"])
    assert failed == 0
    sigma = sigma_of(pr["lvn"])
    c0, T10, T20 = restated(pr, med[0])
    for k in [x for x in range(-20, 21) if x != 0]:
        ck, T1k, T2k = restated(pr, med[0] + 0.25 * k * sigma)
        assert bool((c0 <= ck + cm.bound(S, T10, T20) + cm.bound(S, T1k, T2k)).all()), k


def test_symmetric_program_gives_a_symmetric_score():
    pr = seeded_problem("sal2", 11, 16, seed=21)
    pr["program"], pr["theta"] = [(0, 0, 0, 0)], torch.tensor([0.3, 0.9], dtype=F64)          # one affine block
    m = qm.G(pr["mu"], pr["program"], pr["theta"])
    for d in (0.01, 0.4, 3.0):
        up, T1u, T2u = restated(pr, m + d)
        dn, T1d, T2d = restated(pr, m - d)
        # (the nodes mirror about m to an ulp of |g|: 2 wn_s each)
        slack = cm.bound(16, T1u, T2u) + cm.bound(16, T1d, T2d) + 4.0 * 2.0 ** -52 * (m.abs() + d + 3.0)
        assert bool(((up - dn).abs() <= slack).all()), d


@pytest.mark.parametrize("name", ["staircase", "bimodal"])
def test_hard_inputs(name):
    pr, _ = hard_problem(name)
    sigma = sigma_of(pr["lvn"])
    g = problem_nodes(pr)
    y = problem_targets(pr, 5)
    c, T1, T2 = restated(pr, y)
    assert bool(torch.isfinite(c).all()) and bool((c >= 0.0).all())
    # far targets: a(z) = |z|, so T1 = E|Y - y| = |y - mean| and the score stays finite
    mean = (pr["wn"].unsqueeze(1) * g).sum(0)
    for sgn in (-1.0, 1.0):
        far, T1f, T2f = restated(pr, mean + sgn * 1e8 * sigma)
        assert bool(torch.isfinite(far).all())
        assert float(((far - (1e8 * sigma - T2f)).abs() / far).max()) <= 1e-12


def test_zero_variance_rows_take_the_closed_form():
    pr = seeded_problem("sal2", 6, 8, seed=3)
    pr["v"][2], pr["v"][4] = 0.0, -1e-9
    y = problem_targets(pr, 1)
    c, T1, T2 = restated(pr, y)
    gm = qm.G(pr["mu"], pr["program"], pr["theta"])
    want, _, _ = cm.gauss_parts(gm, torch.zeros(6, dtype=F64), pr["lvn"], y)
    for n in (2, 4):
        assert abs(float(c[n] - want[n])) <= float(cm.bound(8, T1, T2)[n])


# ---------------------------------------------------------------------------------------------------
# the sampled estimator and the scores
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [1, 2, 7, 100])
def test_crps_from_samples_is_the_double_sum(S):
    from tgp.pytorch_amd import ops
    g = torch.Generator().manual_seed(S)
    x = torch.randn(S, 6, generator=g, dtype=F64) * 3.0 + 1.0
    if S > 2:
        x[1], x[S - 1, 2] = x[0], x[2, 2]                       # ties
    y = torch.randn(6, generator=g, dtype=F64)
    brute = (x - y).abs().mean(0) - (x.unsqueeze(0) - x.unsqueeze(1)).abs().sum((0, 1)) / (2.0 * S * S)
    got = ops.crps_from_samples(x, y)
    assert got.shape == (6,)
    assert float(((got - brute).abs() / brute.abs().clamp_min(1e-300)).max()) <= 1e-13
    assert torch.equal(ops.crps_from_samples(x.unsqueeze(2), y.unsqueeze(1)), got)             # (S,N,1) draws


def test_interval_score_by_hand():
    from tgp.pytorch_amd import ops
    lo, hi = torch.tensor([1.0, 1.0, 1.0], dtype=F64), torch.tensor([3.0, 3.0, 3.0], dtype=F64)
    y = torch.tensor([2.0, 0.5, 4.0], dtype=F64)                # inside, below, above
    got = ops.interval_score(lo, hi, y, 0.05)
    assert got.tolist() == [2.0, 2.0 + 40.0 * 0.5, 2.0 + 40.0 * 1.0]
    assert ops.interval_score(lo, hi, y, 0.5).tolist() == [2.0, 4.0, 6.0]
    with pytest.raises(ValueError):
        ops.interval_score(lo, hi, y, 0.0)


def test_poisson_crps_by_hand():
    pmf = torch.tensor([[0.1, 0.2, 0.3, 0.4], [0.7, 0.3, 0.0, 0.0]], dtype=F64)
    y = torch.tensor([2.0, 0.0], dtype=F64)
    want = []
    for n in range(2):
        tot, cdf = 0.0, 0.0
        for k in range(4):
            cdf += float(pmf[n, k])
            tot += (cdf - (1.0 if k >= float(y[n]) else 0.0)) ** 2
        want.append(tot)
    got = cm.poisson_crps(pmf, y)
    assert float((got - torch.tensor(want, dtype=F64)).abs().max()) <= 1e-15
    assert abs(float(got[0]) - (0.01 + 0.09 + 0.16)) <= 1e-15


# ---------------------------------------------------------------------------------------------------
# host side
# ---------------------------------------------------------------------------------------------------
def test_library_refuses_before_any_launch():
    """S = 257, S = 0 and every likelihood but GAUSS and FLOW: TGP_E_UNSUPPORTED with the entry named, decided on the host (the
    pointers below are never followed)."""
    from tgp.pytorch_amd import lib as L
    h = L.load()
    text = open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "tgp_hip.h")).read()
    assert "int tgp_predict_crps_f64(const tgp_model* model" in text and "tgp_predict_crps_f64" in L.EXPORTS
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

    cases = [(model(257, L.LIK_FLOW), b"S = 257"), (model(0, L.LIK_FLOW), b"S = 0")]
    cases += [(model(32, k), b"lik = %d" % k) for k in range(3, 9)]
    assert (L.LIK_BERNOULLI, L.LIK_HETERO) == (3, 8)
    for md, what in cases:
        assert h.tgp_predict_crps_f64(md, p, p, None, p, p, p, None) == L.E_UNSUPPORTED
        msg = h.tgp_last_error()
        assert msg.startswith(b"tgp_predict_crps_f64") and what in msg, msg
    ok = model(32, L.LIK_FLOW)
    assert h.tgp_predict_crps_f64(None, p, p, None, p, p, p, None) == -1
    assert h.tgp_predict_crps_f64(ok, None, p, None, p, p, p, None) == -2
    assert h.tgp_predict_crps_f64(ok, p, None, None, p, p, p, None) == -3
    assert h.tgp_predict_crps_f64(ok, p, p, None, None, p, p, None) == -5
    assert h.tgp_predict_crps_f64(ok, p, p, None, p, None, p, None) == -6


def test_ops_checks_the_length_of_Y():
    from tgp.pytorch_amd import ops
    z = torch.zeros(4, dtype=F64)
    with pytest.raises(ValueError, match="one value per row"):
        ops.predict_crps(z, z, torch.zeros(1, dtype=F64), torch.zeros(3, dtype=F64))


def _plain_model(kind):
    from tgp.pytorch_amd import config as cg
    from tgp.pytorch_amd.flows import SAL
    from tgp.pytorch_amd.kernels import instance_kernel
    from tgp.pytorch_amd.likelihoods import Bernoulli, GaussianNonLinearMean, WarpedGaussianLinearMean
    from tgp.pytorch_amd.models import sparse_MF_GP, sparse_MF_SP
    cg.set_maximum_precission()
    X = torch.randn(30, 3, dtype=F64)
    K = instance_kernel("scale_rbf", ard_num_dim=3, num_multioutput=1, kernel_is_shared=False,
                        init_params={"length_scale": 2.0, "kernel_scale": 2.0, "noisy_variance": 1e-6})
    args = (["zero", K], X, X[:5].clone(), 30)
    if kind == "warped":
        lik = WarpedGaussianLinearMean(1, 0.05, False, SAL(2), 20)
        return sparse_MF_GP(*args, lik, 1, True, False, False, False, False, 0.0), X
    if kind == "bernoulli":
        return sparse_MF_GP(*args, Bernoulli(), 1, True, False, False, False, False, 0.0), X
    flow = SAL(1, input_dependent=True, input_dim=3, num_hidden_layers=1, batch_norm=0, dropout=0.5, hidden_dim=8,
               hidden_activation="tanh", inference="MC_dropout")
    model = sparse_MF_SP(*args, GaussianNonLinearMean(1, 0.05, False, 20), 1, True, False, False, False, False, [flow], "single",
                         0.0, be_fully_bayesian=True)
    return model, X


def test_model_refusals():
    """Without samples=, the models with no closed pair term name themselves and point to samples=; classifiers always raise."""
    from test_hetero_host import _model as hetero_model
    from test_student_host import _model as student_model
    old = torch.get_default_dtype()
    try:
        Y = torch.zeros(30, 1, dtype=F64)
        for build, names in ((lambda: student_model("svgp"), ("StudentT", "Student-t")),
                             (lambda: hetero_model("svgp"), ("HeteroscedasticGaussian", "heteroscedastic")),
                             (lambda: _plain_model("warped"), ("WarpedGaussianLinearMean", "warped")),
                             (lambda: _plain_model("bayes"), ("fully Bayesian",))):
            model, X = build()
            model.set_is_training(False)
            with pytest.raises(NotImplementedError) as e:
                model.predictive_crps(X, Y)
            msg = str(e.value)
            assert all(n in msg for n in names) and "samples=" in msg, msg
        model, X = _plain_model("bernoulli")
        for kw in ({}, {"samples": 10}):
            with pytest.raises(NotImplementedError, match="Bernoulli"):
                model.predictive_crps(X, Y, **kw)
        with pytest.raises(NotImplementedError, match="Bernoulli"):
            model.predictive_interval_score(X, Y)
    finally:
        torch.set_default_dtype(old)


def test_cli_flag_and_trainer_keep_their_shape(capsys):
    from tgp.pytorch_amd import main, trainers
    with pytest.raises(SystemExit) as e:
        main.main(["--help"])
    assert e.value.code == 0 and "--scores" in capsys.readouterr().out
    with pytest.raises(SystemExit) as e:
        main.main(["--model", "SVGP", "--dataset", "synthetic_heart", "--train_test_seed_split", "1", "--num_inducing", "10",
                   "--likelihood", "bernoulli", "--scores"])
    assert e.value.code == 2 and "--scores: regression only" in capsys.readouterr().err
    tr = trainers.Trainer_SP_regression(model=type("M", (), {"out_dim": 1})(), data_loaders=["train", "test"], validate_each=1, plot=False,
                                        track=False, Y_std=torch.ones(1), plot_each=-1, S_test=10)
    tr._loader_metrics = lambda loader: (1.0, 2.0, 3.0)
    res = tr.compute_metrics()
    assert len(res) == 9 and all(isinstance(x, float) for x in res)
    tr._loader_scores = lambda loader, samples: {"crps": 0.5, "interval_score": 2.0}
    sc = tr.compute_scores()
    assert set(sc) == {"train", "valid", "test"} and sc["valid"] is None and set(sc["test"]) == {"crps", "interval_score"}
