"""GPU: the acquisition functions (tgp_predict_acquisition_f64, k_pred_acq / k_acq_gauss of csrc/tgp_quantile.hip) through ops,
the models, utils.suggest_candidates and the CLI.

The yardstick is the float64 restatement of tests/acquisition_model.py (held to an independent integral, its own central
differences and mpmath on the CPU, tests/test_acquisition_host.py).  Tolerances: those tests/test_gpu_input_grad.py applies to
ops.predict_moment_grads against its restatement -- TOL_GRAD = 1e-7 for the partials, TOL_VAL = 1e-9 for the values, through
conftest.rel_err: the sums and the flows are the same."""
import math
import re
import subprocess
import sys

import pytest
import torch

from conftest import REPO, rel_err
from oracle import tgp_oracle as orc

import acquisition_model as AM
import flow_shapes_model as fsm
from test_acquisition_host import LOGH_RECORDED

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F64 = torch.float64
TOL_VAL = 1e-9
TOL_GRAD = 1e-7
TOL_FD = 1e-6        # a central difference with h = 1e-5 in float64: h^2 |f'''| / 6 + eps |f| / h (tests/test_gpu_derivative.py)
NS = (1, 3, 7, 13)                      # not multiples of the 4 rows of a wave: its last rows are idle
SS = (1, 15, 16, 17, 63, 65)            # around the 16-lane stride and the 64-node batch of the sweep
DS = (1, 3, 17)                         # the fused chain below, at and beyond 16 inputs
NMAX = max(NS)
PROGRAMS = ("sal2", "tanh3x2", "sinh_r", "empty", "gauss")
NOISE = 0.3


@pytest.fixture(scope="module", autouse=True)
def f64():
    from tgp.pytorch_amd import config as cg
    old = torch.get_default_dtype()
    cg.set_maximum_precission()
    yield
    torch.set_default_dtype(old)


def _rows(name, S):
    """NMAX rows: row 2 has v = 0, row 5 has v < 0.  The flows' programs are those of tests/test_gpu_input_grad.py."""
    g = torch.Generator().manual_seed(31)
    mu = torch.randn(NMAX, generator=g, dtype=F64)
    v = 0.05 + torch.rand(NMAX, generator=g, dtype=F64)
    v[2], v[5] = 0.0, -0.25
    xs, ws = orc.hermgauss(S)
    program, theta = [], torch.zeros(0, dtype=F64)
    if name == "sinh_r":                         # SinhL's block: an extended kind
        program, theta = fsm.PROGRAMS[name], torch.tensor(fsm.THETA[name], dtype=F64)
        mu = 0.5 * mu
    elif name in ("sal2", "tanh3x2"):
        prob = orc.synthetic_problem(8, 2, 4, seed=5, flow=name, S=8)
        program, theta = prob["program"], prob["params"]["theta"]
    return mu, v, program, theta, xs, ws / math.sqrt(math.pi)


_ref = {}


def _reference(name, S, kind, c, best):
    """The restatement at NMAX rows, computed once per case: a row's outputs depend on that row only, so the first N rows serve
    every N."""
    key = (name, S, kind, c, best)
    if key not in _ref:
        mu, v, program, theta, xs, wn = _rows(name, S)
        lvn = torch.log(torch.tensor([NOISE], dtype=F64))
        with fsm.patched():
            _ref[key] = AM.acquisition(mu, v, lvn, kind, best, c, xs, wn, program, theta, want_partials=True)
    return _ref[key]


def _call(name, S, kind, c, best, N=NMAX, jac=None, want_partials=True):
    from tgp.pytorch_amd import ops
    mu, v, program, theta, xs, wn = _rows(name, S)
    lvn = torch.log(torch.tensor([NOISE], dtype=F64)).to(DEV)
    spec = None if name == "gauss" else ops.FlowSpec(program, theta.numel(), 0, DEV)
    return ops.predict_acquisition(mu[:N].to(DEV), v[:N].to(DEV), lvn, kind, best, spec, theta.to(DEV) if theta.numel() else None,
                                   None if name == "gauss" else S, maximize=c > 0, want_partials=want_partials, jac=jac)


# (one Gaussian has no nodes: S does not enter, one case each)
CASES = tuple((name, S) for name in PROGRAMS[:3] for S in SS) + (("empty", 8), ("gauss", 1))


@pytest.mark.parametrize("name,S", CASES)
def test_against_the_restatement(name, S):
    """Every kind, both signs of c and every N against the restatement; rows with v = 0 and v < 0 have exact zeros in the
    v-partial and the values of a row at v = 0."""
    worst = [0.0, 0.0]
    for kind in AM.KINDS:
        for c in (1.0, -1.0):
            best = 0.2 * c
            val_ref, part_ref = _reference(name, S, kind, c, best)
            for N in NS:
                val, part = _call(name, S, kind, c, best, N)
                assert val.shape == (N,) and part.shape == (2, N)
                assert bool(torch.isfinite(val).all()) and bool(torch.isfinite(part).all())
                e = (rel_err(val.cpu(), val_ref[:N]), rel_err(part[0].cpu(), part_ref[0, :N]),
                     rel_err(part[1].cpu(), part_ref[1, :N]) if N > 1 else 0.0)
                worst = [max(worst[0], e[0]), max(worst[1], e[1], e[2])]
                assert e[0] <= TOL_VAL and e[1] <= TOL_GRAD and e[2] <= TOL_GRAD, (kind, c, N, e)
                for r in (2, 5):
                    if r < N:
                        assert float(part[1, r]) == 0.0
    print("%s S=%d: values %.2e partials %.2e" % (name, S, worst[0], worst[1]))


def test_per_row_parameters():
    """An input-dependent program (SAL x 2 with per-row parameters, rowp (N, 4)): values and partials at fixed rowp."""
    from tgp.pytorch_amd import ops
    S, N = 17, NMAX
    prob = orc.synthetic_problem(N, 2, 4, seed=6, flow="idsal2", S=S)
    program, theta, rowp = prob["program"], prob["params"]["theta"], prob["rowp"]
    mu, v, _, _, xs, wn = _rows("empty", S)
    lvn = torch.log(torch.tensor([NOISE], dtype=F64))
    spec = ops.FlowSpec(program, theta.numel(), rowp.shape[1], DEV)
    for kind in AM.KINDS:
        val_ref, part_ref = AM.acquisition(mu, v, lvn, kind, -0.1, -1.0, xs, wn, program, theta, rowp, want_partials=True)
        val, part = ops.predict_acquisition(mu.to(DEV), v.to(DEV), lvn.to(DEV), kind, -0.1, spec, theta.to(DEV), S, rowp.to(DEV),
                                            maximize=False, want_partials=True)
        e = (rel_err(val.cpu(), val_ref), rel_err(part.cpu(), part_ref))
        print("per-row parameters %s: value %.2e partials %.2e" % ((kind,) + e))
        assert e[0] <= TOL_VAL and e[1] <= TOL_GRAD
        few = ops.predict_acquisition(mu[:3].to(DEV), v[:3].to(DEV), lvn.to(DEV), kind, -0.1, spec, theta.to(DEV), S,
                                      rowp[:3].contiguous().to(DEV), maximize=False)
        assert torch.equal(few, val[:3])


def test_gauss_and_the_empty_program_agree():
    """TGP_LIK_GAUSS and an empty program under TGP_LIK_FLOW take the same kernel: the same bits."""
    for kind in AM.KINDS:
        a, b = _call("gauss", 1, kind, 1.0, 0.2), _call("empty", 8, kind, 1.0, 0.2)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.mark.parametrize("name", ("sal2", "tanh3x2", "gauss"))
def test_far_tail(name):
    """The incumbent 40 sigma beyond every node: EI is 0 (or denormal), log EI is finite and within the host test's bound of the
    restatement (10 x the recorded error of log h, relative), its partials finite and not zero."""
    S = 17
    mu, v, program, theta, xs, wn = _rows(name, S)
    sigma = math.sqrt(NOISE)
    for c in (1.0, -1.0):
        if name == "gauss":
            edge = float((c * mu + 40.0 * torch.sqrt(v.clamp_min(0.0) + NOISE)).max())
        else:
            edge = float((c * AM.nodes(mu, v, xs, program, theta)).max()) + 40.0 * sigma
        best = c * edge
        ei, _ = _call(name, S, "ei", c, best)
        assert bool((ei.abs() < 2.3e-308).all()), ei
        val, part = _call(name, S, "log_ei", c, best)
        val_ref, part_ref = _reference(name, S, "log_ei", c, best)
        assert bool(torch.isfinite(val).all()) and bool(torch.isfinite(part).all())
        e = float(((val.cpu() - val_ref) / val_ref).abs().max())
        print("far tail %s c=%+d: log EI in [%.1f, %.1f], rel %.2e (bound %.1e); partials %.2e"
              % (name, c, float(val.min()), float(val.max()), e, 10.0 * LOGH_RECORDED, rel_err(part.cpu(), part_ref)))
        assert e <= 10.0 * LOGH_RECORDED
        assert bool((part[0] != 0.0).all()) and bool((part[1][v.to(DEV) > 0.0] != 0.0).all())
        assert bool((c * part[0] > 0.0).all())                  # towards the incumbent
        assert rel_err(part.cpu(), part_ref) <= TOL_GRAD
        pi, _ = _call(name, S, "pi", c, best)
        assert bool((pi >= 0.0).all()) and bool((pi < 1e-300).all())


@pytest.mark.parametrize("name", ("tanh3x2", "sinh_r", "gauss"))
def test_same_input_same_bits(name):
    """Two calls give the same bits, and a row's outputs do not change when other rows are appended."""
    S = 65
    for kind in AM.KINDS:
        a, b = _call(name, S, kind, -1.0, 0.1), _call(name, S, kind, -1.0, 0.1)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        for N in (1, 5):
            few = _call(name, S, kind, -1.0, 0.1, N)
            assert torch.equal(few[0], a[0][:N]) and torch.equal(few[1], a[1][:, :N]), (kind, N)


@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("name", ("sal2", "gauss"))
def test_fused_chain(name, D):
    """grad_x of the launch against partials[0][:, None] * dmu_dx + partials[1][:, None] * dv_dx from torch: 2 ulp per element (a
    fused multiply-add may differ from the two-step product); value and partials are the bits of the call without it."""
    g = torch.Generator().manual_seed(7 + D)
    for N in NS:
        dmu, dv = (torch.randn(N, D, generator=g, dtype=F64).to(DEV) for _ in range(2))
        for kind in AM.KINDS:
            val, part, gx = _call(name, 17, kind, 1.0, 0.2, N, jac=(dmu, dv))
            val0, part0 = _call(name, 17, kind, 1.0, 0.2, N)
            assert torch.equal(val, val0) and torch.equal(part, part0)
            want = part[0][:, None] * dmu + part[1][:, None] * dv
            assert gx.shape == (N, D)
            ulp = torch.nextafter(want.abs(), torch.full_like(want, float("inf"))) - want.abs()
            assert bool(((gx - want).abs() <= 2.0 * ulp).all()), (kind, N, float((gx - want).abs().max()))
            val1, gx1 = _call(name, 17, kind, 1.0, 0.2, N, jac=(dmu, dv), want_partials=False)       # partials = NULL
            assert torch.equal(val1, val) and torch.equal(gx1, gx)


# ---- the models -------------------------------------------------------------------------------------------------------------
def _relevance_model(flow):
    """A small SVGP (flow None) or TGP (SAL x 1) on rows of synthetic_relevance, M = 20, five Adam steps."""
    from test_gpu_input_grad import _build
    from tgp.pytorch_amd.synthetic import relevance_dataset
    N, M = 120, 20
    Xn, Yn = relevance_dataset(seed=1)
    X = torch.tensor(Xn[:N], dtype=F64)
    Y = torch.tensor(Yn[:N], dtype=F64)
    Y = (Y - Y.mean()) / Y.std()
    prob = orc.synthetic_problem(N, X.shape[1], M, seed=5, flow=flow, S=16)
    prob["X"], prob["Y"] = X, Y
    prob["params"]["Z"] = X[:M].clone()
    model = _build(prob, flow)
    opt = torch.optim.Adam(model.parameters(), lr=0.01)
    Xd, Yd = X.to(DEV), Y.to(DEV)
    for _ in range(5):
        opt.zero_grad()
        (-model.ELBO(Xd, Yd)[0]).backward()
        opt.step()
    return model, Xd, Yd


_models = {}


def _model(flow):
    if flow not in _models:
        _models[flow] = _relevance_model(flow)
    return _models[flow]


@pytest.mark.parametrize("flow", (None, "sal1"), ids=("svgp", "tgp-sal1"))
def test_model_acquisition_gradient_is_the_slope_of_its_value(flow):
    """model.acquisition(X, kind, best, return_grad=True) on 5 rows against central differences in x of its own value, h = 1e-5,
    for the four kinds; bound TOL_FD as derived in tests/test_gpu_derivative.py.  PI is predictive_cdf's upper tail at Y = best."""
    model, X, Y = _model(flow)
    Xr = X[:5].contiguous()
    best = float(Y.median())
    h = 1e-5
    for kind in ("ei", "log_ei", "pi", "ucb"):
        for maximize in (True, False):
            kw = dict(kind=kind, best=best, maximize=maximize, beta=1.5)
            val, grad = model.acquisition(Xr, return_grad=True, **kw)
            assert val.shape == (5,) and grad.shape == Xr.shape and model.training
            assert torch.equal(val, model.acquisition(Xr, **kw))
            fd = torch.empty_like(grad)
            for d in range(Xr.shape[1]):
                Xp, Xm = Xr.clone(), Xr.clone()
                Xp[:, d] += h
                Xm[:, d] -= h
                fd[:, d] = (model.acquisition(Xp, **kw) - model.acquisition(Xm, **kw)) / (Xp[:, d] - Xm[:, d])
            e = rel_err(grad.cpu(), fd.cpu())
            print("%s %s maximize=%s against the central difference: %.3e (bound %.0e)" % (flow, kind, maximize, e, TOL_FD))
            assert e <= TOL_FD
    cdf = model.predictive_cdf(Xr, torch.full((5, 1), best, dtype=F64, device=DEV))[0]
    pi_up = model.acquisition(Xr, kind="pi", best=best, maximize=True)
    pi_dn = model.acquisition(Xr, kind="pi", best=best, maximize=False)
    print("PI against predictive_cdf: upper %.2e lower %.2e" % (rel_err(pi_up.cpu(), (1.0 - cdf).cpu()), rel_err(pi_dn.cpu(), cdf.cpu())))
    assert rel_err(pi_dn.cpu(), cdf.cpu()) <= TOL_VAL and rel_err(pi_up.cpu(), (1.0 - cdf).cpu()) <= TOL_VAL
    from tgp.pytorch_amd import ops
    mu, v, lvn, spec, theta, rowp = model._quantile_inputs(Xr, "predictive_cdf")
    model.train()
    _, sf = ops.predict_cdf(mu, v, lvn, torch.full((5,), best, dtype=F64, device=DEV), spec, theta, model.quad_points, rowp)
    assert rel_err(pi_up.cpu(), sf.cpu()) <= TOL_VAL             # the upper tail from its own sum


def test_suggest_candidates_on_a_grid():
    """suggest_candidates from a 257-point grid of starts on a 1-D toy: never below the grid's best point (the best-seen rule),
    and strictly above it for log EI."""
    from test_gpu_input_grad import _build
    from tgp.pytorch_amd import utils
    N, M = 60, 12
    g = torch.Generator().manual_seed(3)
    X = (4.0 * torch.rand(N, 1, generator=g, dtype=F64) - 2.0)
    Y = torch.sin(3.0 * X) + 0.3 * X + 0.05 * torch.randn(N, 1, generator=g, dtype=F64)
    Y = (Y - Y.mean()) / Y.std()
    prob = orc.synthetic_problem(N, 1, M, seed=5, flow=None, S=8)
    prob["X"], prob["Y"] = X, Y
    prob["params"]["Z"] = torch.linspace(-2.0, 2.0, M, dtype=F64).reshape(M, 1)
    prob["params"]["raw_lengthscale"] = orc.inv_softplus(torch.full((1,), 0.5, dtype=F64))
    model = _build(prob, None)
    opt = torch.optim.Adam(model.parameters(), lr=0.05)
    Xd, Yd = X.to(DEV), Y.to(DEV)
    for _ in range(30):
        opt.zero_grad()
        (-model.ELBO(Xd, Yd)[0]).backward()
        opt.step()
    best = float(Y.max())
    bounds = torch.tensor([[-2.0], [2.0]], dtype=F64, device=DEV)
    grid = torch.linspace(-2.0, 2.0, 257, dtype=F64, device=DEV).reshape(-1, 1)
    for kind in ("log_ei", "ei", "pi", "ucb"):
        on_grid = float(model.acquisition(grid, kind=kind, best=best).max())
        x, val, finals = utils.suggest_candidates(model, bounds, kind=kind, best=best, starts=grid, steps=50)
        print("suggest %s: grid maximum %.12g, result %.12g at x = %.6f" % (kind, on_grid, float(val), float(x)))
        assert x.shape == (1,) and -2.0 <= float(x) <= 2.0 and finals["X"].shape == (257, 1)
        assert float(val) >= on_grid
        if kind == "log_ei":
            assert float(val) > on_grid
            assert float(val) == float(model.acquisition(x.reshape(1, 1), kind=kind, best=best)[0])
    a = utils.suggest_candidates(model, bounds, best=best, num_starts=16, steps=5, generator=torch.Generator().manual_seed(1))
    b = utils.suggest_candidates(model, bounds, best=best, num_starts=16, steps=5, generator=torch.Generator().manual_seed(1))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


# ---- refusals -----------------------------------------------------------------------------------------------------------------
def test_refusals():
    from tgp.pytorch_amd import lib as L
    from tgp.pytorch_amd import ops
    mu, v, lvn = torch.zeros(4, device=DEV, dtype=F64), torch.ones(4, device=DEV, dtype=F64), torch.zeros(1, device=DEV, dtype=F64)
    with pytest.raises(ValueError, match="kind must be one of"):
        ops.predict_acquisition(mu, v, lvn, "ucb", 0.0)
    with pytest.raises(L.TgpError, match=r"-100 .*tgp_predict_acquisition_f64.*best"):
        ops.predict_acquisition(mu, v, lvn, "ei", float("nan"))
    with pytest.raises(L.TgpError, match=r"-100 .*tgp_predict_acquisition_f64.*S = %d" % (L.QUANTILE_MAX_S + 1)):
        ops.predict_acquisition(mu, v, lvn, "ei", 0.0, ops.FlowSpec([], 0, 0, DEV), None, L.QUANTILE_MAX_S + 1)
    with pytest.raises(ValueError, match="jac must be"):
        ops.predict_acquisition(mu, v, lvn, "ei", 0.0, jac=(torch.zeros(3, 2, device=DEV, dtype=F64),) * 2)
    model, X, Y = _model("sal1")
    with pytest.raises(ValueError, match="needs best="):
        model.acquisition(X[:3], kind="ei")
    with pytest.raises(ValueError, match="kind must be one of"):
        model.acquisition(X[:3], kind="kg", best=0.0)
    assert model.acquisition(X[:3], kind="ucb").shape == (3,)               # the bound needs no incumbent
    model.fully_bayesian = True
    try:
        with pytest.raises(NotImplementedError, match="acquisition: the fully Bayesian model"):
            model.acquisition(X[:3], best=0.0, return_grad=True)
    finally:
        model.fully_bayesian = False


def _small(lik, outputs=1, flows=None, D=4, N=40, M=10):
    from tgp.pytorch_amd.kernels import instance_kernel
    from tgp.pytorch_amd.models import sparse_MF_GP, sparse_MF_SP
    X = torch.randn(N, D, generator=torch.Generator().manual_seed(4), dtype=F64)
    K = instance_kernel("scale_rbf", ard_num_dim=D, num_multioutput=outputs, kernel_is_shared=False,
                        init_params={"length_scale": 2.0, "kernel_scale": 2.0, "noisy_variance": 1e-6})
    ip = {"variational_distribution": {"variance_scale": 1e-5, "mean_scale": 0.0}}
    args = (["zero", K], X, X[:M].clone(), N, lik, outputs, True, False, False, False, False)
    model = sparse_MF_GP(*args, 0.0, init_params=ip) if flows is None else sparse_MF_SP(*args, flows, "single", 0.0, init_params=ip)
    return model.to(DEV), X.to(DEV)


def test_model_refusals_by_likelihood():
    """Every likelihood but the Gaussian and flow regression ones -- a Student-t model, a warped one, a heteroscedastic (composed,
    two-output) one -- refuses the value and the gradient alike, naming the reason."""
    from tgp.pytorch_amd.flows import SAL
    from tgp.pytorch_amd.likelihoods import HeteroscedasticGaussian, StudentT, WarpedGaussianLinearMean
    cases = ((StudentT(1, 0.05, False, 8, df=4.0), 1, "Student-t"),
             (WarpedGaussianLinearMean(1, 0.05, False, SAL(1), 8), 1, None),
             (HeteroscedasticGaussian(0.07, 8), 2, None))
    for lik, outputs, display in cases:
        model, X = _small(lik, outputs)
        for grad in (False, True):
            with pytest.raises(NotImplementedError, match="acquisition: the Gaussian and flow regression likelihoods only") as e:
                model.acquisition(X[:3], kind="ei", best=0.0, return_grad=grad)
            assert "tgp_predict_acquisition_f64" in str(e.value)
            assert (display or lik.display or type(lik).__name__) in str(e.value)
            with pytest.raises(NotImplementedError, match="acquisition:"):
                model.acquisition(X[:3], kind="ucb", return_grad=grad)


def test_input_dependent_flows_give_values_and_refuse_the_gradient():
    """An ID_TGP (SAL x 1 whose parameters come from a network on x): values through the per-row parameters, equal to the
    restatement on the model's own moments and rowp and, for PI, to predictive_cdf; return_grad raises with the reason."""
    from tgp.pytorch_amd.flow import instance_flow
    from tgp.pytorch_amd.flows import SAL
    from tgp.pytorch_amd.likelihoods import GaussianNonLinearMean
    torch.manual_seed(0)
    idf = instance_flow(SAL(1, input_dependent=True, input_dim=4, num_hidden_layers=2, batch_norm=0, dropout=0.25, hidden_dim=50,
                            hidden_activation="relu", inference="MC_dropout"))
    idf.turn_off_initializer_parameters()
    model, X = _small(GaussianNonLinearMean(1, 0.05, False, 16), 1, [idf])
    assert model._input_dependent
    Xr = X[:7].contiguous()
    for kind in ("ei", "log_ei", "pi", "ucb"):
        with pytest.raises(NotImplementedError, match="acquisition: the model has input-dependent flows"):
            model.acquisition(Xr, kind=kind, best=0.1, return_grad=True)
    mu, v, lvn, spec, theta, rowp = model._quantile_inputs(Xr, "acquisition")
    model.train()
    assert rowp is not None and rowp.shape[0] == 7
    xs, ws = orc.hermgauss(model.quad_points)
    for kind in AM.KINDS:
        for maximize in (True, False):
            val = model.acquisition(Xr, kind=kind, best=0.1, maximize=maximize)
            assert val.shape == (7,) and bool(torch.isfinite(val).all()) and model.training
            ref = AM.acquisition(mu.cpu(), v.cpu(), lvn.cpu(), kind, 0.1, 1.0 if maximize else -1.0, xs, ws / math.sqrt(math.pi),
                                 spec.blocks, theta.cpu(), rowp.cpu())
            assert rel_err(val.cpu(), ref) <= TOL_VAL, (kind, maximize)
    cdf = model.predictive_cdf(Xr, torch.full((7, 1), 0.1, dtype=F64, device=DEV))[0]
    assert rel_err(model.acquisition(Xr, kind="pi", best=0.1, maximize=False).cpu(), cdf.cpu()) <= TOL_VAL
    assert model.acquisition(Xr, kind="ucb").shape == (7,)


def test_cli_suggest():
    """main.py --suggest 3 on synthetic_power, M = 20, 5 epochs: three candidate rows after every other line, inside the
    bounding box of the training inputs."""
    from tgp.pytorch_amd.data import return_dataset
    r = subprocess.run([sys.executable, "-m", "tgp.pytorch_amd.main", "--model", "TGP", "--dataset", "synthetic_power",
                        "--train_test_seed_split", "1", "--num_inducing", "20", "--epochs", "5", "--suggest", "3"],
                       cwd=REPO, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    rows = [re.search(r"candidate (\d) log_ei ([0-9.eE+-]+) at x = \[(.*)\]", ln) for ln in lines[-3:]]
    assert all(rows), r.stdout[-2000:]
    assert [int(m.group(1)) for m in rows] == [0, 1, 2]
    vals = [float(m.group(2)) for m in rows]
    assert all(math.isfinite(t) for t in vals) and vals == sorted(vals, reverse=True)
    xs = torch.tensor([[float(t) for t in m.group(3).split(",")] for m in rows], dtype=F64)
    _, dc = return_dataset("synthetic_power", 10000, seed=1)
    Xtr = dc["X_tr"].to(F64)
    assert xs.shape == (3, Xtr.shape[1])
    assert bool((xs >= Xtr.min(0).values - 1e-6).all()) and bool((xs <= Xtr.max(0).values + 1e-6).all())
    assert len({tuple(t.tolist()) for t in xs}) == 3                        # distinct
