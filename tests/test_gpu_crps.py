"""The exact CRPS on the GPU: tgp_predict_crps_f64 against the CPU restatement (tests/crps_model.py) on the reference's
fixtures (tests/golden/q_*.npz), the lane layout's edge shapes, the closed form, the hard inputs, an integration of the
EXISTING CDF entry that shares nothing with the restatement, bit-identical repeats, and the model / trainer layer.

Every comparison with the restatement is held to crps_model.bound (the formula and the number format, see that module) with
node_tol = 1e-9 where the two sides ran different flow code; the closed form to 16 ulp relative; the integration of
ops.predict_cdf to the figure tests/test_crps_host.py recorded for that quadrature (QUAD_CPU) plus the bound."""
import math

import pytest
import torch

import crps_model as cm
import quantile_model as qm
from test_crps_host import QUAD_CPU, closed_form, crps_fixture, problem_nodes, problem_targets, restated, sigma_of, within_bound
from test_quantiles_host import CASES, TOL_VAL, hard_problem, seeded_problem

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F64 = torch.float64


@pytest.fixture(scope="module", autouse=True)
def f64():
    from tgp.pytorch_amd import config as cg
    old = torch.get_default_dtype()
    cg.set_maximum_precission()
    cg.device = DEV
    yield
    torch.set_default_dtype(old)


def _spec(program, P, RP):
    from tgp.pytorch_amd import ops
    return ops.FlowSpec(program, P, RP, DEV)


def _d(t):
    return None if t is None else t.to(DEV).contiguous()


def gpu_crps(pr, y):
    """ops.predict_crps on a problem dict of test_quantiles_host: (crps, parts) on the CPU."""
    from tgp.pytorch_amd import ops
    rp = pr["rowp"]
    spec = _spec(pr["program"], pr["theta"].numel(), 0 if rp is None else rp.shape[1])
    c, parts = ops.predict_crps(_d(pr["mu"]), _d(pr["v"]), _d(pr["lvn"]), _d(y), spec, _d(pr["theta"]), pr["S"], _d(rp),
                                want_parts=True)
    return c.cpu(), parts.cpu()


def check(pr, y, label):
    c, parts = gpu_crps(pr, y)
    want, T1, T2 = restated(pr, y)
    assert bool(torch.isfinite(want).all()) and bool(torch.isfinite(c).all()), label
    assert torch.equal(c, parts[0] - parts[1]), label
    gmax = problem_nodes(pr).abs().max(0).values if len(pr["program"]) else pr["mu"].abs()
    within_bound(c, want, T1, T2, pr["S"], gmax, TOL_VAL, label)
    return c


# ---- parity with the restatement on the reference's fixtures ---------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_fixture_parity(name):
    g = crps_fixture(name)
    pr = {"mu": g["mu"], "v": g["v"], "lvn": g["p_log_var_noise"], "program": g["program"], "theta": g["p_theta"],
          "rowp": g["rowp"], "xs": g["xs"], "wn": g["wn"], "S": g["xs"].numel()}
    c, parts = gpu_crps(pr, g["y"])
    want, T1, T2 = g["crps"]
    assert torch.equal(c, parts[0] - parts[1])
    gmax = g["g_mine"].abs().max(0).values if g["g_mine"] is not None else g["mu"].abs()
    within_bound(c, want, T1, T2, pr["S"], gmax, TOL_VAL, name)
    within_bound(parts[0], T1, T1, T2, pr["S"], gmax, TOL_VAL, name + " T1")
    within_bound(parts[1], T2, T1, T2, pr["S"], gmax, TOL_VAL, name + " T2")


# ---- shapes where the lane layout can go wrong -----------------------------------------------------------------------------
SHAPES = [("sal2", 1, 1), ("sal2", 3, 2), ("tanh3x2", 4, 15), ("bcl_al", 5, 16), ("idsal1", 63, 17), ("sal2", 64, 33),
          ("tanh3x2", 65, 100), ("bcl_al", 3, 256), ("idsal1", 257, 33), ("idsal1", 5, 100), ("tanh3x2", 257, 2),
          ("bcl_al", 64, 1)]


def test_shapes_cover_every_edge():
    assert {s[1] for s in SHAPES} == {1, 3, 4, 5, 63, 64, 65, 257} and {s[2] for s in SHAPES} == {1, 2, 15, 16, 17, 33, 100, 256}
    assert {s[0] for s in SHAPES} == {"sal2", "tanh3x2", "bcl_al", "idsal1"}


@pytest.mark.parametrize("kind,N,S", SHAPES)
def test_lane_layout_shapes(kind, N, S):
    pr = seeded_problem(kind, N, S, seed=N + S)
    check(pr, problem_targets(pr, N + S), "%s N=%d S=%d" % (kind, N, S))


# ---- closed form -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 64, 257])
def test_gaussian_and_identity_closed_form(N):
    from tgp.pytorch_amd import ops
    g = torch.Generator().manual_seed(N)
    mu, v = torch.randn(N, generator=g, dtype=F64), 0.01 + torch.rand(N, generator=g, dtype=F64)
    lvn = torch.tensor([math.log(0.07)], dtype=F64)
    y = mu + 3.0 * torch.sqrt(v + 0.07) * (2.0 * torch.rand(N, generator=g, dtype=F64) - 1.0)
    want = closed_form(mu, v, lvn, y)
    c_gauss, p_gauss = ops.predict_crps(_d(mu), _d(v), _d(lvn), _d(y), want_parts=True)                   # TGP_LIK_GAUSS
    c_ident = ops.predict_crps(_d(mu), _d(v), _d(lvn), _d(y), _spec([], 0, 0), None, 16)                   # the empty program
    assert c_gauss.shape == (N,) and torch.equal(c_gauss, c_ident) and torch.equal(c_gauss, p_gauss[0] - p_gauss[1])
    rel = float(((c_gauss.cpu() - want).abs() / want).max())
    print("closed form N=%d: worst relative difference %.3e (16 ulp = %.3e)" % (N, rel, 16 * 2.0 ** -52))
    assert rel <= 16 * 2.0 ** -52


# ---- hard inputs -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["staircase", "bimodal"])
def test_hard_inputs(name):
    pr, _ = hard_problem(name)
    check(pr, problem_targets(pr, 5), name)
    mean = (pr["wn"].unsqueeze(1) * problem_nodes(pr)).sum(0)
    for sgn in (-1.0, 1.0):
        c = check(pr, mean + sgn * 1e8 * sigma_of(pr["lvn"]), "%s %+.0e sigma" % (name, sgn * 1e8))
        assert bool(torch.isfinite(c).all()) and bool((c > 0.0).all())


def test_rows_without_variance_inside_a_batch():
    pr = seeded_problem("sal2", 70, 8, seed=3)
    pr["v"][[2, 69]] = 0.0
    pr["v"][17] = -1e-9                       # counts as 0 too
    y = problem_targets(pr, 2)
    c = check(pr, y, "v <= 0 rows")
    rows = torch.tensor([2, 17, 69])
    gm = qm.G(pr["mu"][rows], pr["program"], pr["theta"])
    want, T1, T2 = cm.gauss_parts(gm, torch.zeros(3, dtype=F64), pr["lvn"], y[rows])
    within_bound(c[rows], want, T1, T2, 8, gm.abs(), TOL_VAL, "v = 0 closed form")


# ---- independence from the restatement: the existing CDF entry, integrated ---------------------------------------------------
def test_integral_of_the_existing_cdf_entry():
    from tgp.pytorch_amd import ops
    pr = seeded_problem("sal2", 5, 32, seed=9)
    y = problem_targets(pr, 9)
    c, parts = gpu_crps(pr, y)
    t_lo, w_lo, t_hi, w_hi = cm.quadrature_rule(problem_nodes(pr), sigma_of(pr["lvn"]), y)
    spec = _spec(pr["program"], pr["theta"].numel(), 0)
    quad = torch.zeros(5, dtype=F64)
    for t, w, which in ((t_lo, w_lo, 0), (t_hi, w_hi, 1)):
        K = t.shape[0]
        tails = ops.predict_cdf(_d(pr["mu"].repeat(K)), _d(pr["v"].repeat(K)), _d(pr["lvn"]), _d(t.reshape(-1)), spec,
                                _d(pr["theta"]), pr["S"])
        tail = tails[which].cpu().reshape(K, 5)
        quad = quad + (w * tail * tail).sum(0)
    tol = QUAD_CPU["q_med_sal2"] * quad + cm.bound(32, parts[0], parts[1])
    print("crps vs integrated predict_cdf: worst |delta| / tolerance %.3e, relative %.3e"
          % (float(((c - quad).abs() / tol).max()), float(((c - quad).abs() / quad).max())))
    assert bool(((c - quad).abs() <= tol).all())


# ---- same input, same bits; a row's value is its own --------------------------------------------------------------------------
@pytest.mark.parametrize("kind,S", [("sal2", 33), ("idsal1", 100)])
def test_bit_identical_repeats_and_rows(kind, S):
    pr = seeded_problem(kind, 257, S, seed=41)
    y = problem_targets(pr, 41)
    c, parts = gpu_crps(pr, y)
    c2, parts2 = gpu_crps(pr, y)
    assert torch.equal(c, c2) and torch.equal(parts, parts2)
    for k in (0, 130, 255, 256):
        one = dict(pr, mu=pr["mu"][k:k + 1], v=pr["v"][k:k + 1], rowp=None if pr["rowp"] is None else pr["rowp"][k:k + 1])
        ck, pk = gpu_crps(one, y[k:k + 1])
        assert torch.equal(ck, c[k:k + 1]) and torch.equal(pk, parts[:, k:k + 1]), k


# ---- models and trainer ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["svgp", "tgp", "id_tgp", "unwhitened"])
def test_model_scores(which):
    from test_gpu_quantiles import _models
    from tgp.pytorch_amd import ops
    model, X = _models(which)
    model.set_is_training(False)
    N = X.shape[0]
    q = model.predictive_quantiles(X, [0.025, 0.975, 0.4])[0]
    Y = q[2].clone().reshape(-1, 1)                                         # the 40 % quantile: inside the 95 % interval
    Y[0], Y[N - 1] = q[0, 0] - 0.5, q[1, N - 1] + 0.5                      # one below, one above it
    c = model.predictive_crps(X, Y)
    mu, v, lvn, spec, theta, rowp = model._quantile_inputs(X, "predictive_cdf")
    model.train()
    want = ops.predict_crps(mu, v, lvn, Y.reshape(-1), spec, theta, model.quad_points, rowp)
    assert c.shape == (1, N) and c.is_cuda and torch.equal(c[0], want) and bool((c > 0.0).all())
    assert torch.equal(model.predictive_crps(X, Y, Y_std=torch.tensor([2.5], dtype=F64)), c * 2.5)
    isc = model.predictive_interval_score(X, Y, alpha=0.05)
    assert isc.shape == (1, N) and torch.equal(isc[0], ops.interval_score(q[0], q[1], Y.reshape(-1), 0.05))
    width = q[1] - q[0]
    assert abs(float(isc[0, 0]) - float(width[0] + 20.0)) <= 1e-12 * float(isc[0, 0]) and float(isc[0, 1]) == float(width[1])
    assert abs(float(isc[0, N - 1]) - float(width[N - 1] + 20.0)) <= 1e-12 * float(isc[0, N - 1])
    assert torch.equal(model.predictive_interval_score(X, Y, Y_std=torch.tensor([2.5], dtype=F64)), isc * 2.5)
    # the sampled estimator of the same predictive: eight standard errors of a 2000-draw mean of |x - y| - |x - x'| / 2
    torch.manual_seed(3)
    cs = model.predictive_crps(X, Y, samples=2000)
    assert cs.shape == (1, N) and float(((cs - c).abs() / c).median()) < 0.1


def test_student_and_poisson_models():
    from test_gpu_poisson import _build_model as build_poisson
    from test_gpu_student import _build_model as build_student
    from tgp.pytorch_amd import synthetic
    g = torch.Generator().manual_seed(1)
    X = torch.randn(40, 3, generator=g, dtype=F64)
    model = build_student(X, tgp=True)
    Xd, Yd = X.to(DEV), torch.randn(40, 1, generator=g, dtype=F64).to(DEV)
    with pytest.raises(NotImplementedError, match="Student-t"):
        model.predictive_crps(Xd, Yd)
    c = model.predictive_crps(Xd, Yd, samples=50)
    assert c.shape == (1, 40) and bool(torch.isfinite(c).all()) and bool((c > 0.0).all())
    Xc, Yc = synthetic.counts_dataset()
    Xc, Yc = torch.tensor(Xc[:60], dtype=F64), torch.tensor(Yc[:60], dtype=F64)
    pois = build_poisson(Xc, Yc)
    pois.set_is_training(False)
    cp = pois.predictive_crps(Xc.to(DEV), Yc.to(DEV), kmax=60)
    want = cm.poisson_crps(pois.predictive_pmf(Xc.to(DEV), 60), Yc.to(DEV).reshape(-1))
    assert cp.shape == (1, 60) and float((cp[0] - want).abs().max()) <= 1e-14 and bool((cp >= 0.0).all())
    with pytest.raises(ValueError, match="kmax"):
        pois.predictive_crps(Xc.to(DEV), Yc.to(DEV))


def test_trainer_compute_scores():
    from oracle import tgp_oracle as orc
    from conftest import load_golden
    from test_gpu_models import build_model
    from tgp.pytorch_amd.data import DeviceLoader
    from tgp.pytorch_amd.trainers import Trainer_SP_regression
    prob = orc.synthetic_problem(120, 4, 20, seed=0, flow="sal2", S=32)
    prob["params"]["theta"] = load_golden("med_sal2")["params"]["theta"]
    model = build_model(prob, "sal2")
    X, Y = prob["X"].to(DEV), prob["Y"].to(DEV)
    Y_std = torch.full((1,), 3.0, dtype=F64, device=DEV)
    loaders = [DeviceLoader(X, Y, 120, shuffle=False, device=DEV), DeviceLoader(X[:50], Y[:50], 50, shuffle=False, device=DEV)]
    tr = Trainer_SP_regression(model, loaders, 0, False, False, Y_std, -1, S_test=100)
    sc = tr.compute_scores()
    assert set(sc) == {"train", "valid", "test"} and sc["valid"] is None
    assert set(sc["train"]) == set(sc["test"]) == {"crps", "interval_score"}
    model.set_is_training(False)
    assert abs(sc["train"]["crps"] - 3.0 * float(model.predictive_crps(X, Y).mean())) <= 1e-12 * sc["train"]["crps"]
    assert abs(sc["test"]["interval_score"] - 3.0 * float(model.predictive_interval_score(X[:50], Y[:50]).mean())) \
        <= 1e-12 * sc["test"]["interval_score"]
    torch.manual_seed(2)
    ss = tr.compute_scores(samples=200)
    assert ss["train"]["interval_score"] is None and abs(ss["train"]["crps"] / sc["train"]["crps"] - 1.0) < 0.2
    assert len(tr.compute_metrics()) == 9
