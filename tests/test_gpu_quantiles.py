"""Exact predictive quantiles and CDF on the GPU: tgp_predict_quantile_f64 / tgp_predict_cdf_f64 against the CPU restatement
(tests/quantile_model.py) on the reference's fixtures (tests/golden/q_*.npz), the closed forms, properties on seeded problems
without a fixture, the hard inputs of the root rule, the limits, bit-identical repeats, and the model / utils / trainer layer.

Bars (tests/test_quantiles_host.py holds the definitions and the reasoning): roots against the restatement at 1e-9 relative to
max(1, |t|) (`root_tolerance`: plus what a plateau of F leaves undetermined); the residual of every fixture root on the
reference's node values within 10x the figure the restatement measured for THAT case (RESIDUAL_CPU); roots without a fixture
within `residual_bound`, with node_tol = 0 through the GPU's own CDF entry and 1e-9 through the restatement's nodes."""
import math

import numpy as np
import pytest
import torch

from conftest import load_golden
import quantile_model as qm
from test_quantiles_host import (CASES, HARD, RESIDUAL_CPU, TOL_VAL, check_residuals, fixture, hard_problem, reference_residual,
                                 residual_bound, roots_agree, seeded_problem, solve)

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


def gpu_quantiles(pr, probs, check=False):
    """ops.predict_quantiles on a problem dict of test_quantiles_host: (t on the CPU, failed count)."""
    from tgp.pytorch_amd import ops
    rp = pr["rowp"]
    spec = _spec(pr["program"], pr["theta"].numel(), 0 if rp is None else rp.shape[1])
    t, status = ops.predict_quantiles(_d(pr["mu"]), _d(pr["v"]), _d(pr["lvn"]), probs, spec, _d(pr["theta"]), pr["S"], _d(rp),
                                      check=False)
    return t.cpu(), int(status[0])


def gpu_cdf(pr, Y):
    from tgp.pytorch_amd import ops
    rp = pr["rowp"]
    spec = _spec(pr["program"], pr["theta"].numel(), 0 if rp is None else rp.shape[1])
    cdf, sf = ops.predict_cdf(_d(pr["mu"]), _d(pr["v"]), _d(pr["lvn"]), _d(Y), spec, _d(pr["theta"]), pr["S"], _d(rp))
    return cdf.cpu(), sf.cpu()


def as_problem(g):
    return {"mu": g["mu"], "v": g["v"], "lvn": g["p_log_var_noise"], "program": g["program"], "theta": g["p_theta"],
            "rowp": g["rowp"], "xs": g["xs"], "wn": g["wn"], "S": g["xs"].numel()}


# ---- parity with the restatement on the reference's fixtures ---------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_fixture_parity_and_residuals(name):
    g = fixture(name)
    t, failed = gpu_quantiles(as_problem(g), g["probs"])
    assert failed == 0 and bool(torch.isfinite(t).all())
    roots_agree(g, t, g["t"], name)
    r = reference_residual(g, t)
    print("residual %-14s %.3e   (CPU %.3e)" % (name, r, RESIDUAL_CPU[name]))
    assert r <= 10.0 * RESIDUAL_CPU[name]


# ---- closed forms -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 63, 64, 65, 257])
def test_gaussian_and_identity_closed_form(N):
    from tgp.pytorch_amd import ops
    g = torch.Generator().manual_seed(N)
    mu, v = torch.randn(N, generator=g, dtype=F64), 0.01 + torch.rand(N, generator=g, dtype=F64)
    lvn = torch.tensor([math.log(0.07)], dtype=F64)
    probs = [0.975, 0.5, 0.025, 1e-6]
    zq = torch.special.ndtri(torch.tensor(probs, dtype=F64))
    want = mu.unsqueeze(0) + zq.unsqueeze(1) * torch.sqrt(v + math.exp(float(lvn))).unsqueeze(0)
    t_gauss = ops.predict_quantiles(_d(mu), _d(v), _d(lvn), probs).cpu()                               # TGP_LIK_GAUSS
    t_ident = ops.predict_quantiles(_d(mu), _d(v), _d(lvn), probs, _spec([], 0, 0), None, 16).cpu()   # the empty program
    for t in (t_gauss, t_ident):
        assert t.shape == (4, N)
        assert float(((t - want).abs() / want.abs().clamp_min(1e-300)).max()) <= 1e-13
    assert torch.equal(t_gauss, t_ident)
    # the one-term CDF: back to p, and the two tails add up
    cdf, sf = ops.predict_cdf(_d(mu), _d(v), _d(lvn), _d(want[0]))
    assert float((cdf.cpu() - 0.975).abs().max()) <= 1e-14 and float((cdf + sf - 1.0).abs().max()) <= 1e-15
    cdf, sf = ops.predict_cdf(_d(mu), _d(v), _d(lvn), _d(want[3]), _spec([], 0, 0), None, 16)
    assert float((cdf.cpu() / 1e-6 - 1.0).abs().max()) <= 1e-9


def test_zero_variance_row_inside_a_batch():
    pr = seeded_problem("sal2", 70, 8, seed=3)
    pr["v"][[2, 69]] = 0.0
    pr["v"][17] = -1e-9                       # counts as 0 too
    probs = [0.9, 0.1, 0.5]
    t, failed = gpu_quantiles(pr, probs)
    assert failed == 0
    sigma = math.sqrt(math.exp(float(pr["lvn"])))
    zq = torch.special.ndtri(torch.tensor(probs, dtype=F64))
    for n in (2, 17, 69):
        want = qm.G(pr["mu"][n:n + 1], pr["program"], pr["theta"]) + zq * sigma
        assert float(((t[:, n] - want).abs() / want.abs().clamp_min(1.0)).max()) <= TOL_VAL
    pr["v"] = pr["v"].clamp_min(0.0)
    tc, _ = solve(pr, probs)
    assert float(((t - tc).abs() / tc.abs().clamp_min(1.0)).max()) <= TOL_VAL


# ---- properties on seeded problems with no fixture ----------------------------------------------------------------------------
Q32 = [float(x) for x in torch.linspace(0.01, 0.99, 32, dtype=F64)]
Q5 = [0.975, 0.025, 0.5, 0.2, 0.8]            # unsorted on purpose
PROPS = [("sal2", 1, 32, [0.3]), ("sal2", 65, 1, Q5), ("sal2", 257, 100, [0.5]), ("tanh3x2", 65, 8, Q32),
         ("tanh3x2", 257, 32, Q5), ("bcl_al", 65, 32, Q5), ("bcl_al", 1, 100, Q32), ("idsal1", 65, 100, Q5),
         ("idsal1", 257, 8, [0.9]), ("idsal1", 1, 1, Q5)]


@pytest.mark.parametrize("kind,N,S,probs", PROPS, ids=["%s-N%d-S%d-Q%d" % (k, n, s, len(q)) for k, n, s, q in PROPS])
def test_properties_without_a_fixture(kind, N, S, probs):
    from tgp.pytorch_amd import ops
    pr = seeded_problem(kind, N, S, seed=N + S)
    t, failed = gpu_quantiles(pr, probs)
    assert failed == 0 and t.shape == (len(probs), N) and bool(torch.isfinite(t).all())
    # strictly increasing in p, row by row
    order = sorted(range(len(probs)), key=lambda i: probs[i])
    ts = t[order]
    assert bool((ts[1:] > ts[:-1]).all())
    # the residual rule through the restatement's F (its own node values) ...
    check_residuals(pr, probs, t, node_tol=TOL_VAL, label="%s restated F" % kind)
    # ... and through the GPU's own CDF entry
    sigma = math.sqrt(math.exp(float(pr["lvn"])))
    g = qm.nodes(pr["mu"], pr["v"], pr["xs"], pr["program"], pr["theta"], pr["rowp"])
    for qi, p in enumerate(probs):
        cdf, sf = gpu_cdf(pr, t[qi])
        assert float((cdf + sf - 1.0).abs().max()) <= 1e-15
        res = ((sf - (1.0 - p)).abs() / (1.0 - p)) if p > 0.5 else ((cdf - p).abs() / p)
        _, _, dens = qm.tails(g, pr["wn"], sigma, t[qi])
        assert bool((res <= residual_bound(dens, t[qi], p)).all()), (kind, p, float(res.max()))
        # the CDF entry against the restatement, value tolerance on both tails
        lo, up = qm.cdf(pr["mu"], pr["v"], pr["lvn"], t[qi], pr["xs"], pr["wn"], pr["program"], pr["theta"], pr["rowp"])
        assert float((cdf - lo).abs().max()) <= TOL_VAL and float((sf - up).abs().max()) <= TOL_VAL
    # d cdf / dY is the density tgp_predict_f64 ships (Y_std = 1; its float32-pi constant put back to log 2 pi).  Central
    # difference, h = 1e-5: truncation <= h^2/6 max|F'''| <= h^2/6 * 0.4 / sigma^3, rounding <= 4e-15 / h
    h = 1e-5
    Y = t[0]
    cp, _ = gpu_cdf(pr, Y + h)
    cm, _ = gpu_cdf(pr, Y - h)
    rp = pr["rowp"]
    spec = _spec(pr["program"], pr["theta"].numel(), 0 if rp is None else rp.shape[1])
    _, _, logp = ops.predict(_d(pr["mu"]), _d(pr["v"]), _d(pr["lvn"]), spec, _d(pr["theta"]), S, _d(rp), Y=_d(Y), Y_std=1.0)
    dens = torch.exp(logp.cpu() + 0.5 * 1.8378770942368803 - 0.5 * math.log(2.0 * math.pi))
    tol = h * h / 6.0 * 0.4 / sigma ** 3 + 4e-15 / h
    assert float(((cp - cm) / ((Y + h) - (Y - h)) - dens).abs().max()) <= tol


# ---- hard inputs of the root rule -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", HARD)
def test_hard_inputs_converge(name):
    pr, probs = hard_problem(name)
    tc, failed_c = solve(pr, probs)                     # the rule itself converges on them (test_quantiles_host.py)
    assert failed_c == 0
    t, failed = gpu_quantiles(pr, probs)
    assert failed == 0 and bool(torch.isfinite(t).all())
    assert bool((t[1:] > t[:-1]).all())
    check_residuals(pr, probs, t, node_tol=TOL_VAL, label=name + " restated F")
    sigma = math.sqrt(math.exp(float(pr["lvn"])))
    g = qm.nodes(pr["mu"], pr["v"], pr["xs"], pr["program"], pr["theta"], pr["rowp"])
    for qi, p in enumerate(probs):
        cdf, sf = gpu_cdf(pr, t[qi])
        res = ((sf - (1.0 - p)).abs() / (1.0 - p)) if p > 0.5 else ((cdf - p).abs() / p)
        _, _, dens = qm.tails(g, pr["wn"], sigma, t[qi])
        assert bool((res <= residual_bound(dens, t[qi], p)).all()), (name, p, float(res.max()))


def test_out_of_evaluations_is_counted_and_nan():
    from tgp.pytorch_amd import lib as L
    from tgp.pytorch_amd import ops
    pr = seeded_problem("sal2", 70, 8, seed=5)
    pr["mu"][[1, 68]] = 1e200                        # the flow overflows: nothing to bracket
    t, failed = gpu_quantiles(pr, [0.3, 0.6])
    assert failed == 4 and bool(torch.isnan(t[:, [1, 68]]).all())
    keep = [n for n in range(70) if n not in (1, 68)]
    assert bool(torch.isfinite(t[:, keep]).all())
    with pytest.raises(L.TgpError):
        ops.predict_quantiles(_d(pr["mu"]), _d(pr["v"]), _d(pr["lvn"]), [0.3], _spec(pr["program"], 8, 0), _d(pr["theta"]), 8)


# ---- limits, refusals, repeats ----------------------------------------------------------------------------------------------------
def test_limits_and_refusals():
    from tgp.pytorch_amd import lib as L
    from tgp.pytorch_amd import ops
    pr = seeded_problem("sal2", 9, 8, seed=1)
    mu, v, lvn, th = _d(pr["mu"]), _d(pr["v"]), _d(pr["lvn"]), _d(pr["theta"])
    spec = _spec(pr["program"], 8, 0)
    h = L.load()

    def refused(fn, what):
        with pytest.raises(L.TgpError) as e:
            fn()
        assert "-100" in str(e.value) and "tgp_predict_quantile_f64" in str(e.value) and what in str(e.value), str(e.value)

    refused(lambda: ops.predict_quantiles(mu, v, lvn, [0.5], spec, th, 257), "S = 257")
    refused(lambda: ops.predict_quantiles(mu, v, lvn, [0.5 + 0.01 * i for i in range(33)], spec, th, 8), "Q = 33")
    refused(lambda: ops.predict_quantiles(mu, v, lvn, [], spec, th, 8), "Q = 0")
    md, keep = ops._flow_model(9, 8, spec, th, lvn, mu.device, lik=L.LIK_BERNOULLI)
    p, zq = ops.quantile_probs([0.5], DEV)
    t = torch.empty(1, 9, dtype=F64, device=DEV)
    st = torch.zeros(1, dtype=torch.int32, device=DEV)
    rc = h.tgp_predict_quantile_f64(md, L.ptr(mu), L.ptr(v), None, L.ptr(p), L.ptr(zq), 1, L.ptr(t), L.ptr(st), L.stream_ptr())
    assert rc == L.E_UNSUPPORTED and b"tgp_predict_quantile_f64" in h.tgp_last_error() and b"lik = 3" in h.tgp_last_error()
    rc = h.tgp_predict_cdf_f64(md, L.ptr(mu), L.ptr(v), None, L.ptr(mu), L.ptr(t), None, L.stream_ptr())
    assert rc == L.E_UNSUPPORTED and b"tgp_predict_cdf_f64" in h.tgp_last_error()
    # out-of-range probabilities never reach a launch
    for bad in ([0.0], [1.0], [float("nan")], [0.5, 1.0]):
        with pytest.raises(ValueError):
            ops.predict_quantiles(mu, v, lvn, bad, spec, th, 8)
    # the limits themselves are inside: S = 256 (Q = 32 runs in the property tests)
    pr = seeded_problem("sal2", 5, 256, seed=2)
    t, failed = gpu_quantiles(pr, [0.025, 0.975])
    assert failed == 0
    check_residuals(pr, [0.025, 0.975], t, node_tol=TOL_VAL, label="S = 256")


def test_repeats_are_bit_identical():
    pr = seeded_problem("tanh3x2", 257, 50, seed=9)
    a, _ = gpu_quantiles(pr, Q5)
    b, _ = gpu_quantiles(pr, Q5)
    assert torch.equal(a, b)
    ca, sa = gpu_cdf(pr, a[0])
    cb, sb = gpu_cdf(pr, a[0])
    assert torch.equal(ca, cb) and torch.equal(sa, sb)


# ---- model, utils, trainer ------------------------------------------------------------------------------------------------------
def _id_tgp(prob):
    from tgp.pytorch_amd.flow import compile_flow, instance_flow
    from tgp.pytorch_amd.flows import SAL
    from tgp.pytorch_amd.kernels import instance_kernel
    from tgp.pytorch_amd.likelihoods import GaussianNonLinearMean
    from tgp.pytorch_amd.models import sparse_MF_SP
    torch.manual_seed(0)
    p = prob["params"]
    idf = instance_flow(SAL(1, input_dependent=True, input_dim=4, num_hidden_layers=2, batch_norm=0, dropout=0.25,
                            hidden_dim=50, hidden_activation="relu", inference="MC_dropout"))
    idf.turn_off_initializer_parameters()
    K = instance_kernel("scale_rbf", ard_num_dim=4, num_multioutput=1, kernel_is_shared=False,
                        init_params={"length_scale": 2.0, "kernel_scale": 2.0})
    model = sparse_MF_SP(["zero", K], prob["X"], p["Z"].clone(), prob["X"].shape[0], GaussianNonLinearMean(1, 0.05, False, 16), 1,
                         True, False, False, False, False, [idf], "single", 0.0,
                         init_params={"variational_distribution": {"variance_scale": 1e-5, "mean_scale": 0.0}}).to(DEV)
    with torch.no_grad():
        model.q_U.variational_mean.data = p["m"].reshape(1, -1).to(DEV)
        model.q_U.chol_variational_covar.data = p["Lam"].reshape(1, 20, 20).to(DEV)
        for prm, val in zip(compile_flow(model.G_matrix[0])[1], p["theta"]):
            prm.data = val.clone().reshape(()).to(DEV)
        # output layers shrunk around the identity flow (a_n ~ 0, b_n ~ 1), the state the flow initialiser leaves the networks
        # in: every row's G is increasing
        for i, net in enumerate(compile_flow(model.G_matrix[0])[2]):
            ps = list(net.parameters())
            ps[-2].mul_(0.3)
            ps[-1].fill_(float(i % 2))
    return model


def _models(which):
    """(model, X on the device): SVGP, TGP, ID_TGP (point estimate) and an unwhitened TGP, built as the other GPU tests do."""
    if which == "svgp":
        from test_gpu_models import build_model
        g = load_golden("tiny_svgp")
        return build_model(g, None), g["X"].to(DEV)
    if which == "tgp":
        from test_gpu_models import build_model
        g = load_golden("med_sal2")
        return build_model(g, "sal2"), g["X"][:130].to(DEV)
    if which == "unwhitened":
        from test_gpu_unwhiten import build_model
        g = load_golden("unwh_med_sal2")
        return build_model(g, "unwh_med_sal2"), g["X"][:65].to(DEV)
    from oracle import tgp_oracle as orc
    prob = orc.synthetic_problem(200, 4, 20, seed=2, flow="idsal1", S=16)
    return _id_tgp(prob), prob["X"][:77].to(DEV)


@pytest.mark.parametrize("which", ["svgp", "tgp", "id_tgp", "unwhitened"])
def test_model_quantiles(which):
    model, X = _models(which)
    model.set_is_training(False)
    probs = [0.975, 0.025, 0.5]
    qp = model.predictive_quantiles(X, probs)
    qf = model.posterior_quantiles(X, probs)
    N = X.shape[0]
    assert qp.shape == (1, 3, N) and qf.shape == (1, 3, N) and qp.is_cuda
    # the restatement on the model's own moments and flow inputs
    model.eval()
    with torch.no_grad():
        mu, v = model.marginal_variational_qf_parameters(X.repeat(1, 1, 1), diagonal=True, is_duvenaud=False)
        spec, theta, rowp = model._flow_inputs(X, with_grad=False)
    model.train()
    mu, v = mu.reshape(-1).cpu(), v.reshape(-1).cpu()
    lvn = model.likelihood.log_var_noise.detach().reshape(-1)[:1].cpu()
    prog = [] if spec is None else spec.blocks
    theta = torch.zeros(0, dtype=F64) if theta is None else theta.detach().cpu()
    rowp = None if rowp is None else rowp.detach().cpu()
    S = model.quad_points
    xs, ws = np.polynomial.hermite.hermgauss(S)
    xs, wn = torch.tensor(xs, dtype=F64), torch.tensor(ws / math.sqrt(math.pi), dtype=F64)
    tc, failed = qm.quantiles(mu, v, lvn, probs, xs, wn, prog, theta, rowp)
    assert failed == 0
    g = {"probs": probs, "program": prog, "p_log_var_noise": lvn, "wn": wn, "mu": mu, "v": v,
         "g_nodes": qm.nodes(mu, v, xs, prog, theta, rowp) if prog else None}
    roots_agree(g, qp[0].cpu(), tc, which)
    zq = torch.special.ndtri(torch.tensor(probs, dtype=F64))
    want = qm.G(mu.unsqueeze(0) + zq.unsqueeze(1) * torch.sqrt(v).unsqueeze(0), prog, theta, rowp)
    assert float(((qf[0].cpu() - want).abs() / want.abs().clamp_min(1.0)).max()) <= TOL_VAL
    # PIT values: the CDF at the predictive quantile is the probability
    pit = model.predictive_cdf(X, qp[0, 2].reshape(-1, 1))
    assert pit.shape == (1, N) and float((pit.cpu() - 0.5).abs().max()) <= 1e-9
    # exact intervals through utils: structure of the reference, values of the two methods
    from tgp.pytorch_amd import utils
    for dist, q in (("predictive", qp), ("posterior", qf)):
        ci = utils.compute_95_and_median_confidence_intervals(model, X, 0, dist, False, exact=True)
        assert len(ci) == 1 and len(ci[0]) == 3 and all(a.shape == (N, 1) and isinstance(a, np.ndarray) for a in ci[0])
        assert bool((ci[0][0] < ci[0][1]).all() and (ci[0][1] < ci[0][2]).all())
        for i, j in ((0, 1), (1, 2), (2, 0)):            # [0.025, 0.5, 0.975] against probs = [0.975, 0.025, 0.5]
            assert np.array_equal(ci[0][i][:, 0], q[0, j].cpu().numpy())


def test_models_without_quantiles_say_so():
    from tgp.pytorch_amd import utils
    model, X = _models("id_tgp")
    model.set_is_training(False)
    model.be_fully_bayesian(True)
    for fn in (model.predictive_quantiles, model.posterior_quantiles):
        with pytest.raises(NotImplementedError, match="fully Bayesian"):
            fn(X, [0.5])
    model.be_fully_bayesian(False)
    with pytest.raises(NotImplementedError):
        utils.confidence_intervals(model, X, [0.5], 10, "predictive", True, exact=True)
    from test_gpu_bernoulli import build_model as build_bern
    g = load_golden("bern_tiny_svgp")
    bern = build_bern(g, None)
    bern.set_is_training(False)
    with pytest.raises(NotImplementedError, match="Bernoulli"):
        bern.predictive_quantiles(g["X"].to(DEV), [0.5])


def test_exact_intervals_bracket_the_sampled_ones():
    """compute_95_and_median_confidence_intervals(exact=True) against exact=False at S = 20 000 samples: six standard errors of
    a sample quantile, 6 sqrt(p (1 - p) / S) / F'(t_exact), on rows near the inducing inputs -- where the S-node quadrature the
    exact quantiles belong to and the continuous predictive the samples come from are the same distribution to well below
    that."""
    from tgp.pytorch_amd import utils
    model, _ = _models("tgp")
    model.set_is_training(False)
    g = torch.Generator().manual_seed(3)
    Z = model.Z.detach()[0].cpu()
    X = (Z[torch.arange(24) % Z.shape[0]] + 0.05 * torch.randn(24, Z.shape[1], generator=g, dtype=F64)).to(DEV)
    S = 20000
    torch.manual_seed(11)
    exact = utils.compute_95_and_median_confidence_intervals(model, X, S, "predictive", False, exact=True)
    sampled = utils.compute_95_and_median_confidence_intervals(model, X, S, "predictive", False)
    assert len(sampled) == 1 and len(sampled[0]) == 3 and sampled[0][0].shape == (24, 1)
    t = torch.tensor(np.stack([a[:, 0] for a in exact[0]]))
    h = 1e-6
    for qi, p in enumerate((0.025, 0.5, 0.975)):         # F' from the package's own CDF entry
        Y = t[qi].to(DEV)
        d = (model.predictive_cdf(X, (Y + h).reshape(-1, 1)) - model.predictive_cdf(X, (Y - h).reshape(-1, 1)))[0].cpu() / (2 * h)
        bound = 6.0 * math.sqrt(p * (1.0 - p) / S) / d
        diff = (t[qi] - torch.tensor(sampled[0][qi][:, 0])).abs()
        print("exact vs sampled p=%.3f: worst |diff| / bound %.3f" % (p, float((diff / bound).max())))
        assert bool((diff <= bound).all()), p


def test_wgp_closed_form():
    """A warped model's quantiles: T(t_p) = mu + zq sqrt(v + noise), held to 10x the round trip the host test records for the
    closed-form affine + SAL chain (tests/test_warped_host.py ROUNDTRIP_CPU['affine_sal'], residual in t)."""
    from test_gpu_warped import build_model as build_wgp
    from test_warped_host import ROUNDTRIP_CPU
    from tgp.pytorch_amd import ops
    g = load_golden("warp_med_sal2")
    model = build_wgp(g, "warp_med_sal2")
    model.set_is_training(False)
    X = g["X"][:97].to(DEV)
    probs = [0.1, 0.5, 0.975]
    q = model.predictive_quantiles(X, probs)
    assert q.shape == (1, 3, 97)
    with torch.no_grad():
        mu, v = model.marginal_variational_qf_parameters(X.repeat(1, 1, 1), diagonal=True, is_duvenaud=False)
        spec, theta, _ = model._flow_inputs(X, with_grad=False)
        Tq = ops.flow_eval(q[0].contiguous(), spec, theta, want=("G",))["G"]
    zq = torch.special.ndtri(torch.tensor(probs, dtype=F64)).to(DEV)
    noise = torch.exp(model.likelihood.log_var_noise.detach().reshape(-1)[:1])
    want = mu.reshape(1, -1) + zq.unsqueeze(1) * torch.sqrt(v.reshape(1, -1) + noise)
    r = float(((Tq - want).abs() / want.abs().clamp_min(1.0)).max())
    print("WGP T(t_p) residual %.3e" % r)
    assert r <= 10.0 * ROUNDTRIP_CPU["affine_sal"][0]
    # the latent function of a warped model carries no flow
    qf = model.posterior_quantiles(X, probs)
    want = mu.reshape(1, -1) + zq.unsqueeze(1) * torch.sqrt(v.reshape(1, -1))
    assert qf.shape == (1, 3, 97) and float((qf[0] - want).abs().max()) <= 1e-13


def test_trainer_exact_coverage():
    """coverage='exact' = the count computed on the host from predictive_quantiles, and within the binomial six-standard-error
    band of coverage='sampled' at S_test = 5000 (300 rows)."""
    from oracle import tgp_oracle as orc
    from test_gpu_models import build_model
    from tgp.pytorch_amd.data import DeviceLoader
    from tgp.pytorch_amd.trainers import Trainer_SP_regression
    prob = orc.synthetic_problem(300, 4, 20, seed=0, flow="sal2", S=32)
    prob["params"]["theta"] = load_golden("med_sal2")["params"]["theta"]
    model = build_model(prob, "sal2")
    X, Y = prob["X"].to(DEV), prob["Y"].to(DEV)
    Y_std = torch.ones(1, dtype=F64, device=DEV)

    def trainer(**kw):
        loader = DeviceLoader(X, Y, 300, shuffle=False, device=DEV)
        return Trainer_SP_regression(model, [loader], 0, False, False, Y_std, -1, **kw)

    ex = trainer(S_test=100, coverage="exact").compute_metrics()
    model.set_is_training(False)
    q = model.predictive_quantiles(X, [0.025, 0.975])[0].cpu()
    y = prob["Y"][:, 0]
    want = float(((y >= q[0]) & (y <= q[1])).sum()) / 300.0
    assert ex[2] == want and 0.0 < want <= 1.0
    torch.manual_seed(5)
    sa = trainer(S_test=5000, coverage="sampled").compute_metrics()
    assert ex[0] == sa[0] and ex[1] == sa[1]                    # log-likelihood and RMSE do not depend on the keyword
    band = 6.0 * math.sqrt(max(want * (1.0 - want), 1.0 / 300.0) / 300.0)
    print("coverage exact %.4f sampled %.4f band %.4f" % (ex[2], sa[2], band))
    assert abs(ex[2] - sa[2]) <= band
