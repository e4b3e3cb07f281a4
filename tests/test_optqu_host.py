"""CPU: the closed-form optimal q(u) (Titsias' collapsed bound) -- the algebra restated in float64 torch (tests/optqu_model.py),
what the models, the trainer and the engine refuse, and the host plumbing with the library stubbed."""
import ctypes as C
import warnings

import pytest
import torch

import optqu_model as om
from tgp.pytorch_amd import lib as L
from tgp.pytorch_amd import ops

F64 = torch.float64


@pytest.fixture(scope="module", autouse=True)
def f64():
    from tgp.pytorch_amd import config as cg
    old = torch.get_default_dtype()
    cg.set_maximum_precission()
    cg.device = "cpu"
    yield
    torch.set_default_dtype(old)


# ---- the algebra ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(om.CASES))
def test_every_input_is_well_conditioned(name):
    """cond(K_ZZ + j I) <= 1e5: the conditioning of K_ZZ, not the closed form, sets the accuracy of every check below."""
    assert set(om.OPT_CPU) == set(om.CASES)
    c = om.cond_K(om.make_case(name))
    assert c <= 1e5, c
    assert 0.5 * om.OPT_CPU[name]["cond"] <= c <= 2.0 * om.OPT_CPU[name]["cond"]


@pytest.mark.parametrize("name", sorted(om.CASES))
def test_two_routes_agree_and_the_gradient_vanishes(name):
    """The reversed Cholesky and inv / solve give the same (m*, Lam*); the ELBO's gradient in q(u) vanishes there; at c = 1 the
    ELBO there is the dense collapsed bound.  The figures stay where OPT_CPU recorded them (4 x: another BLAS may round
    differently; 1e-15: figures of a few ulp)."""
    r, rec = om.measure(name), om.OPT_CPU[name]
    print(name, r)
    assert r["route"] < 1e-12 and r["route"] <= 4.0 * rec["route"] + 1e-15
    assert r["ratio"] < 1e-11 and r["ratio"] <= 4.0 * rec["ratio"] + 1e-15
    assert (r["bound"] is None) == (rec["bound"] is None) == (name not in om.DENSE_CASES)
    if r["bound"] is not None:
        assert r["bound"] < 1e-12


@pytest.mark.parametrize("name", sorted(om.CASES))
def test_factor_is_lower_with_positive_diagonal(name):
    p = om.make_case(name)
    for m, Lam in (om.closed_form_rev(p), om.closed_form_inv(p)):
        assert torch.equal(Lam, torch.tril(Lam)) and bool((torch.diagonal(Lam) > 0).all())
        assert m.shape == (p["M"],)


@pytest.mark.parametrize("name", ["m1_d1", "m16", "m63_mat", "m129"])
def test_hyper_gradients_at_the_optimum_are_the_collapsed_bounds(name):
    """Envelope theorem: d ELBO / d (Z, length-scales, output scale, noise) with q(u) held at its optimum equals autograd of the
    dense bound."""
    p = om.make_case(name)
    m, Lam = om.closed_form_rev(p)
    leaves = [p[k].clone().requires_grad_(True) for k in ("Z", "raw_ls", "raw_os", "lvn")]
    g_step = torch.autograd.grad(om.elbo(p, m, Lam, *leaves)[0], leaves)
    leaves2 = [p[k].clone().requires_grad_(True) for k in ("Z", "raw_ls", "raw_os", "lvn")]
    g_dense = torch.autograd.grad(om.dense_bound(p, *leaves2), leaves2)
    for a, b in zip(g_step, g_dense):
        assert om.rel(a, b) < 1e-8


@pytest.mark.parametrize("name", ["m16", "m64_c", "m100_c_mat"])
def test_perturbing_q_u_never_raises_the_elbo(name):
    p = om.make_case(name)
    m, Lam = om.closed_form_rev(p)
    best = float(om.elbo(p, m, Lam)[0])
    g = torch.Generator().manual_seed(7)
    for eps in (1e-3, 1e-2, 1e-1):
        for _ in range(3):
            dm = eps * torch.randn(p["M"], dtype=F64, generator=g)
            dL = eps * torch.tril(torch.randn(p["M"], p["M"], dtype=F64, generator=g))
            assert float(om.elbo(p, m + dm, Lam + dL)[0]) < best


# ---- refusals --------------------------------------------------------------------------------------------------------
def _model(kind, whiten=True, mean="zero"):
    from tgp.pytorch_amd.flows import SAL
    from tgp.pytorch_amd.kernels import instance_kernel
    from tgp.pytorch_amd.likelihoods import (Bernoulli, GaussianLinearMean, GaussianNonLinearMean, MulticlassCategorical,
                                             WarpedGaussianLinearMean)
    from tgp.pytorch_amd.models import sparse_MF_GP, sparse_MF_SP
    torch.manual_seed(0)
    D, M, N = 3, 5, 20
    X = torch.randn(N, D, dtype=F64)
    nout = 3 if kind == "multiclass" else 1
    K = instance_kernel("scale_rbf", ard_num_dim=D, num_multioutput=nout, kernel_is_shared=False)
    tail = (nout, whiten, False, False, False, False)
    if kind == "svgp":
        return sparse_MF_GP([mean, K], X, X[:M].clone(), float(N), GaussianLinearMean(1, 0.05, False), *tail, 0.0)
    if kind == "wgp":
        lik = WarpedGaussianLinearMean(out_dim=1, noise_init=0.05, noise_is_shared=False, flow=SAL(1), quad_points=8)
        return sparse_MF_GP([mean, K], X, X[:M].clone(), float(N), lik, *tail, 0.0)
    if kind == "bernoulli":
        return sparse_MF_GP([mean, K], X, X[:M].clone(), float(N), Bernoulli(), *tail, 0.0)
    if kind == "multiclass":
        return sparse_MF_GP([mean, K], X, X[:M].clone(), float(N), MulticlassCategorical(3), *tail, 0.0)
    flow = SAL(1) if kind == "tgp" else SAL(1, input_dependent=True, input_dim=D, num_hidden_layers=1, batch_norm=0, dropout=0.5,
                                            hidden_dim=8, hidden_activation="tanh", inference="MC_dropout")
    return sparse_MF_SP([mean, K], X, X[:M].clone(), float(N), GaussianNonLinearMean(1, 0.05, False, quadrature_points=8), *tail,
                        [flow], "single", 0.0)


REFUSED = [("tgp", True, r"flow on f \(TGP\)"), ("id_tgp", True, "input-dependent"), ("bernoulli", True, "Bernoulli"),
           ("multiclass", True, "multi-class"), ("svgp", False, "is_whiten=False"), ("wgp", False, "is_whiten=False")]


@pytest.mark.parametrize("kind,whiten,word", REFUSED)
def test_models_without_a_closed_form_refuse_with_the_reason(kind, whiten, word):
    from tgp.pytorch_amd.trainers import Trainer_SP_regression
    model = _model(kind, whiten)
    X, Y = torch.zeros(4, 3, dtype=F64), torch.zeros(4, 1, dtype=F64)
    for call in (model.set_optimal_qu, model.collapsed_bound):
        with pytest.raises(NotImplementedError, match=word):
            call(X, Y)
    with pytest.raises(NotImplementedError, match=word):
        Trainer_SP_regression(model, [[(X, Y)]], 1e20, False, False, torch.ones(1), -1, 100, qu="optimal")


@pytest.mark.parametrize("kind,mean", [("svgp", "zero"), ("svgp", "linear"), ("svgp", "identity"), ("wgp", "zero")])
def test_models_with_a_closed_form_are_not_refused(kind, mean):
    assert _model(kind, True, mean)._qu_refusal() is None


def test_trainer_qu_option():
    """qu="adam" is the default and changes nothing; "optimal" leaves q(u) out of every optimiser group, wants one full batch
    per epoch and takes the step the model's collapsed_bound gives."""
    from tgp.pytorch_amd.trainers import Trainer_SP_regression
    model = _model("svgp")
    X, Y = torch.zeros(4, 3, dtype=F64), torch.zeros(4, 1, dtype=F64)
    args = (1e20, False, False, torch.ones(1), -1, 100)
    with pytest.raises(ValueError, match="qu must be"):
        Trainer_SP_regression(model, [[(X, Y)]], *args, qu="natural")
    with pytest.raises(NotImplementedError, match="one full batch"):
        Trainer_SP_regression(model, [[(X, Y), (X, Y)]], *args, qu="optimal")
    adam = Trainer_SP_regression(model, [[(X, Y)]], *args)
    assert adam.qu == "adam"
    groups, placed = adam._param_groups(None, 0.01)
    assert {id(q) for g in groups for q in g["params"]} == {id(q) for q in model.parameters()}
    opt = Trainer_SP_regression(model, [[(X, Y)]], *args, qu="optimal")
    groups, placed = opt._param_groups(None, 0.01)
    assert not any(n.startswith("q_U.") for n in placed)
    assert {id(q) for g in groups for q in g["params"]} == {id(q) for n, q in model.named_parameters() if not n.startswith("q_U.")}
    groups, placed = opt._param_groups([[0.02, "variational_mean"], [0.03, "Z"]], 0.01)       # naming q(u) places nothing
    assert "Z" in placed and not any(n.startswith("q_U.") for n in placed)
    calls = []
    model.collapsed_bound = lambda x, y: calls.append("collapsed") or (torch.zeros(()), torch.zeros(()), torch.zeros(()))
    model.ELBO = lambda x, y: calls.append("elbo") or (torch.zeros(()), torch.zeros(()), torch.zeros(()))
    opt.ELBO_call(X, Y)
    adam.ELBO_call(X, Y)
    assert calls == ["collapsed", "elbo"]
    adam.refresh_qu()                                   # nothing to refresh: no call reaches the model
    model.set_optimal_qu = lambda x, y: calls.append("refresh")
    opt.refresh_qu()
    assert calls == ["collapsed", "elbo", "refresh"]


COLLAPSED_REFUSES = [(dict(flow_blocks=[(1, 0, 0, 0)]), "no flow"), (dict(rowp=torch.zeros(8, 1)), "no flow"),
                     (dict(likelihood="warped"), "Gaussian likelihood only"),
                     (dict(mean=("linear", torch.zeros(2), torch.zeros(1))), "zero mean only"),
                     (dict(world_size=2), "single-rank"), (dict(collective="abi"), "single-rank"),
                     (dict(mb_global=16), "full batch")]


@pytest.mark.parametrize("kw,word", COLLAPSED_REFUSES)
def test_collapsed_engine_refuses_before_the_library_is_loaded(monkeypatch, kw, word):
    from tgp.pytorch_amd import engine

    def no_library(*a, **k):
        raise AssertionError("the library was loaded before the refusal")
    monkeypatch.setattr(L, "load", no_library)
    with pytest.raises(NotImplementedError, match=word):
        engine.ElboEngine(torch.zeros(8, 2), torch.zeros(8), {}, 8.0, collapsed=True, **kw)
    with pytest.raises(NotImplementedError, match="is_whiten=True"):          # engine_refusal's own message comes first
        engine.ElboEngine(torch.zeros(8, 2), torch.zeros(8), {}, 8.0, collapsed=True, is_whiten=False)
    assert engine.collapsed_refusal() is None


# ---- host plumbing, the library stubbed ------------------------------------------------------------------------------
PIVOT = 2


class StubLib:
    """tgp_optimal_qu_f64 / tgp_kxxk_f64 on host tensors: records what it was handed, fails a scripted number of times, writes a
    recognisable optimum through the output pointers."""

    def __init__(self, failures=0):
        self.failures, self.seen, self.calls = failures, [], []

    def tgp_optimal_qu_workspace_bytes(self, N, D, M):
        self.calls.append(("ws", N, D, M))
        return 4096

    def tgp_optimal_qu_f64(self, md, X, Y, m, Lam, status, ws, nbytes, stream):
        self.seen.append(dict(jitter=float(md.jitter), scale=float(md.scale), N=md.N, D=md.D, M=md.M, kernel=md.kernel, nbytes=nbytes))
        bad = len(self.seen) <= self.failures
        (C.c_int32 * 8).from_address(status.value)[0] = PIVOT if bad else 0
        M = md.M
        mv = (C.c_double * M).from_address(m.value)
        Lv = (C.c_double * (M * M)).from_address(Lam.value)
        y = (C.c_double * md.N).from_address(Y.value)
        for i in range(M):
            mv[i] = y[0] + i
            for j in range(M):
                Lv[i * M + j] = 1.0 + i if j == i else 0.0
        return 0

    def tgp_kxxk_workspace_bytes(self, N, M):
        return 256

    def tgp_kxxk_f64(self, kernel, X, N, Z, M, D, rl, ro, Y, Cp, b, ws, nbytes, stream):
        self.calls.append(("kxxk", kernel, N, M, D, Y is not None and Y.value is not None, b is not None and b.value is not None, nbytes))
        return 0


@pytest.fixture
def stub(monkeypatch):
    monkeypatch.setattr(L, "ptr", lambda t: None if t is None else C.c_void_p(t.data_ptr()))
    monkeypatch.setattr(L, "stream_ptr", lambda: None)

    def make(failures=0):
        lib = StubLib(failures)
        monkeypatch.setattr(L, "load", lambda: lib)
        return lib
    return make


def _inputs(N=6, D=2, M=3):
    g = torch.Generator().manual_seed(0)
    r = lambda *s: torch.randn(*s, dtype=F64, generator=g)      # noqa: E731
    return r(N, D), r(N, 1), r(M, D), r(D), r(1), r(1)          # X, Y, Z, raw_ls, raw_os, lvn


@pytest.mark.parametrize("failures", (0, 1, 3, 4))
def test_optimal_qu_runs_the_jitter_ladder(stub, failures):
    lib, info = stub(failures), {}
    X, Y, Z, rl, ro, lvn = _inputs()
    ladder = [0.0, 1e-8, 1e-7, 1e-6]
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        if failures >= len(ladder):
            with pytest.raises(ops.NotPSDError, match=r"K_MM.*\(pivot %d\)" % PIVOT):
                ops.optimal_qu(X, Y, Z, rl, ro, lvn, 15.0, info=info)
        else:
            m, Lam = ops.optimal_qu(X, Y, Z, rl, ro, lvn, 15.0, kernel="scale_matern32", info=info)
            assert m.tolist() == [float(Y[0]) + i for i in range(3)] and torch.equal(Lam, torch.diag(torch.tensor([1.0, 2.0, 3.0], dtype=F64)))
            assert info["jitter"] == pytest.approx(ladder[failures], rel=1e-12, abs=0.0)
            assert lib.seen[0]["kernel"] == L.KERNEL_SCALE_MATERN32
    assert [s["jitter"] for s in lib.seen] == pytest.approx(ladder[:failures + 1] if failures < len(ladder) else ladder, rel=1e-12, abs=0.0)
    assert len([x for x in w if issubclass(x.category, ops.NumericalWarning)]) == (1 if 0 < failures < len(ladder) else 0)
    first = lib.seen[0]
    assert (first["N"], first["D"], first["M"]) == (6, 2, 3) and first["scale"] == 15.0 / 6 and first["nbytes"] == 4096
    assert ("ws", 6, 2, 3) in lib.calls


def test_optimal_qu_writes_in_place_and_checks_shapes(stub):
    lib = stub()
    X, Y, Z, rl, ro, lvn = _inputs()
    m, Lam = torch.zeros(3, dtype=F64), torch.zeros(3, 3, dtype=F64)
    out = ops.optimal_qu(X, Y, Z, rl, ro, lvn, 6.0, jitter=1e-7, out=(m, Lam), check=False)
    assert out[0] is m and out[1] is Lam and float(Lam[2, 2]) == 3.0 and lib.seen == [dict(lib.seen[0], jitter=1e-7, scale=1.0)]
    with pytest.raises(ValueError):
        ops.optimal_qu(X, Y[:-1], Z, rl, ro, lvn, 6.0)
    with pytest.raises(ValueError):
        ops.optimal_qu(X, Y, Z[:, :1], rl, ro, lvn, 6.0)
    with pytest.raises(L.TgpError, match="float64"):
        ops.optimal_qu(X.float(), Y, Z, rl, ro, lvn, 6.0)
    C_, b = ops.kxxk(X, Z, rl, ro)
    assert b is None and C_.shape == (3, 3) and lib.calls[-1] == ("kxxk", L.KERNEL_SCALE_RBF, 6, 3, 2, False, False, 256)
    C_, b = ops.kxxk(X, Z, rl, ro, Y, kernel="scale_matern32")
    assert b.shape == (3,) and lib.calls[-1] == ("kxxk", L.KERNEL_SCALE_MATERN32, 6, 3, 2, True, True, 256)


def test_set_optimal_qu_hands_over_the_models_targets(monkeypatch):
    """Gaussian: Y; linear / identity mean: Y - m(X); warped: T(Y) from ops.flow_eval.  q_U receives the optimum under no_grad,
    collapsed_bound then runs ELBO with q(u) detached at the optimum's jitter."""
    seen = {}

    def fake_optimal_qu(X, Y, Z, rl, ro, lvn, N_total, jitter=0.0, kernel="scale_rbf", info=None, **kw):
        assert not torch.is_grad_enabled() and not any(t.requires_grad for t in (X, Y, Z, rl, ro, lvn))
        seen.update(Y=Y.clone(), N_total=N_total, kernel=kernel, ladder=kw.get("ladder"))
        info["jitter"] = 1e-7
        M = Z.shape[0]
        return torch.arange(M, dtype=F64), torch.eye(M, dtype=F64) * 2.0
    monkeypatch.setattr(ops, "optimal_qu", fake_optimal_qu)
    X, Y = torch.randn(4, 3, dtype=F64), torch.randn(4, 1, dtype=F64)
    for kind, mean in (("svgp", "zero"), ("svgp", "linear"), ("wgp", "zero")):
        model = _model(kind, True, mean)
        monkeypatch.setattr(model, "_require_gpu", lambda t: None)
        want = Y.reshape(-1)
        if mean == "linear":
            monkeypatch.setattr(model.mean_function, "vector", lambda X2, alpha=1.0, inp=None: inp + alpha * 0.5)
            want = want - 0.5
        if kind == "wgp":
            monkeypatch.setattr(ops, "flow_eval", lambda f, spec, theta, want=None: {"G": 3.0 * f})
            want = 3.0 * want
        info = model.set_optimal_qu(X, Y)
        assert info == {"jitter": 1e-7} and torch.equal(seen["Y"], want) and seen["N_total"] == 20.0
        assert seen["kernel"] == "scale_rbf" and seen["ladder"] == ops.jitter_ladder()
        assert model.q_U.variational_mean.detach()[0].tolist() == [0.0, 1.0, 2.0, 3.0, 4.0]
        assert torch.equal(model.q_U.chol_variational_covar.detach()[0], 2.0 * torch.eye(5, dtype=F64))
        assert model.q_U.variational_mean.grad is None
    model = _model("svgp")
    got = {}

    def fake_elbo(X, Y, _qu_jitter=None):
        got["jitter"] = _qu_jitter
        return "bound"
    monkeypatch.setattr(model, "_require_gpu", lambda t: None)
    monkeypatch.setattr(model, "ELBO", fake_elbo)
    assert model.collapsed_bound(X, Y) == "bound" and got["jitter"] == 1e-7


# ---- the C ABI's own refusals (the real library; every one comes back before a launch) -----------------------------------
def test_abi_limits_and_workspace_refusals():
    lib = L.load()
    assert lib.tgp_version() == 104
    assert lib.tgp_optimal_qu_workspace_bytes(8611, 4, 100) > 0 and lib.tgp_kxxk_workspace_bytes(8611, 100) > 0
    for N, D, M in ((0, 4, 100), (100, 0, 10), (100, 17, 10), (100, 4, 0), (100, 4, 4097)):
        assert lib.tgp_optimal_qu_workspace_bytes(N, D, M) == 0
    assert lib.tgp_kxxk_workspace_bytes(0, 10) == 0 and lib.tgp_kxxk_workspace_bytes(10, 4097) == 0
    # the row split is a function of N and M alone: the same on every call, monotone in N
    assert lib.tgp_kxxk_workspace_bytes(5000, 64) == lib.tgp_kxxk_workspace_bytes(5000, 64) > lib.tgp_kxxk_workspace_bytes(257, 64)
    fake = C.c_void_p(4096)                  # a non-null address: every refusal below comes before anything reads it
    md = L.TgpModel()
    md.N, md.D, md.M, md.kernel, md.scale = 100, 4, 4097, 0, 1.0
    md.Z = md.raw_ls = md.raw_os = md.log_var_noise = fake
    assert lib.tgp_optimal_qu_f64(md, fake, fake, fake, fake, fake, fake, 1 << 40, None) == L.E_UNSUPPORTED
    assert b"tgp_optimal_qu_f64" in lib.tgp_last_error() and b"4097" in lib.tgp_last_error()
    md.M, md.D = 10, 17
    assert lib.tgp_optimal_qu_f64(md, fake, fake, fake, fake, fake, fake, 1 << 40, None) == L.E_UNSUPPORTED
    md.D = 4
    need = lib.tgp_optimal_qu_workspace_bytes(100, 4, 10)
    assert lib.tgp_optimal_qu_f64(md, fake, fake, fake, fake, fake, fake, need - 24, None) == L.E_WORKSPACE   # (16 bytes are alignment slack)
    assert b"tgp_optimal_qu_f64" in lib.tgp_last_error() and str(need).encode() in lib.tgp_last_error()
    assert lib.tgp_optimal_qu_f64(None, fake, fake, fake, fake, fake, fake, need, None) == -1
    for k, code in enumerate((-2, -3, -4, -5, -6, -7)):
        args = [fake] * 6
        args[k] = None
        assert lib.tgp_optimal_qu_f64(md, *args, need, None) == code
    md.kernel = 7
    assert lib.tgp_optimal_qu_f64(md, fake, fake, fake, fake, fake, fake, need, None) == -1
    assert lib.tgp_kxxk_f64(0, fake, 100, fake, 4097, 4, fake, fake, fake, fake, fake, fake, 1 << 40, None) == L.E_UNSUPPORTED
    assert b"tgp_kxxk_f64" in lib.tgp_last_error()
    assert lib.tgp_kxxk_f64(0, fake, 100, fake, 10, 4, fake, fake, fake, fake, fake, fake, 64, None) == L.E_WORKSPACE
    assert b"tgp_kxxk_f64" in lib.tgp_last_error()
