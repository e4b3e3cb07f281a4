"""CPU: the natural-gradient step of q(u) -- the exported surface, the library's argument refusals (no device is touched), the
restatement's own checks (tests/natgrad_model.py), what the models, the trainer and main.py refuse, and the trainer's loop."""
import ctypes as C
import math
import os
import re

import pytest
import torch

import natgrad_model as nm
import optqu_model as om
from tgp.pytorch_amd import lib as L

F64 = torch.float64
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("tgp_kxwxk_workspace_bytes", "tgp_kxwxk_f64", "tgp_natgrad_qu_workspace_bytes", "tgp_natgrad_qu_f64")


@pytest.fixture(scope="module", autouse=True)
def f64():
    from tgp.pytorch_amd import config as cg
    old = torch.get_default_dtype()
    cg.set_maximum_precission()
    cg.device = "cpu"
    yield
    torch.set_default_dtype(old)


# ---- the surface ------------------------------------------------------------------------------------------------------
def test_header_and_binding_carry_the_four_symbols():
    text = open(os.path.join(REPO, "include", "tgp_hip.h")).read()
    decl = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = L.load()
    for s in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, decl), s
        assert s in L.EXPORTS and hasattr(lib, s)
    assert lib.tgp_version() == 104 and "#define TGP_VERSION 104" in text


def _md(N=100, D=4, M=10, kernel=0):
    md = L.TgpModel()
    md.N, md.D, md.M, md.kernel = N, D, M, kernel
    fake = C.c_void_p(64)          # never dereferenced: every call below is refused, or returns, before a launch
    md.Z = md.raw_ls = md.raw_os = md.m = md.Lam = md.log_var_noise = fake
    return md, fake


def test_natgrad_qu_refuses_its_arguments_without_a_device():
    lib = L.load()
    md, fake = _md()
    need = lib.tgp_natgrad_qu_workspace_bytes(100, 4, 10)
    assert need > lib.tgp_optimal_qu_workspace_bytes(100, 4, 10) > 0

    def call(md, rho, nbytes=1 << 40, floor=0.0):
        return lib.tgp_natgrad_qu_f64(md, fake, fake, fake, fake, rho, floor, fake, fake, fake, fake, nbytes, None)
    for rho in (0.0, 1.5, float("nan"), -0.25):
        assert call(md, rho) == L.E_UNSUPPORTED, rho
        assert b"tgp_natgrad_qu_f64" in lib.tgp_last_error() and b"rho" in lib.tgp_last_error()
    for kw in (dict(M=4097), dict(D=17), dict(kernel=7), dict(M=0), dict(N=0)):
        bad, _ = _md(**kw)
        assert call(bad, 1.0) == L.E_UNSUPPORTED, kw
        assert b"tgp_natgrad_qu_f64" in lib.tgp_last_error()
    assert lib.tgp_natgrad_qu_workspace_bytes(100, 4, 4097) == 0 and lib.tgp_natgrad_qu_workspace_bytes(100, 17, 10) == 0
    assert call(md, 0.5, need - 24) == L.E_WORKSPACE            # (16 bytes are alignment slack)
    assert b"tgp_natgrad_qu_f64" in lib.tgp_last_error() and str(need).encode() in lib.tgp_last_error()
    assert lib.tgp_natgrad_qu_f64(None, fake, fake, fake, fake, 1.0, 0.0, fake, fake, fake, fake, need, None) == -1
    for i, code in ((1, -2), (2, -3), (3, -4), (4, -5), (7, -8), (8, -9), (9, -10), (10, -11)):   # a null pointer: its own code
        args = [md, fake, fake, fake, fake, 1.0, 0.0, fake, fake, fake, fake]
        args[i] = None
        assert lib.tgp_natgrad_qu_f64(*args, need, None) == code, i
    md.m = None                                                   # rho = 1 reads neither m nor Lam; rho < 1 needs both
    assert call(md, 0.5, need) == -1


def test_kxwxk_refuses_its_arguments_without_a_device():
    lib = L.load()
    fake = C.c_void_p(64)
    assert lib.tgp_kxwxk_workspace_bytes(5000, 64) == lib.tgp_kxxk_workspace_bytes(5000, 64) > 0      # the same row split
    assert lib.tgp_kxwxk_workspace_bytes(10, 4097) == 0 and lib.tgp_kxwxk_workspace_bytes(0, 10) == 0

    def call(kernel=0, N=100, M=10, D=4, nbytes=1 << 40):
        return lib.tgp_kxwxk_f64(kernel, fake, N, fake, M, D, fake, fake, fake, fake, fake, fake, fake, nbytes, None)
    assert call(M=4097) == L.E_UNSUPPORTED and b"tgp_kxwxk_f64" in lib.tgp_last_error()
    assert call(D=17) == L.E_UNSUPPORTED and call(kernel=7) == -1       # (tgp_kxxk_f64's codes)
    assert call(nbytes=64) == L.E_WORKSPACE and b"tgp_kxwxk_f64" in lib.tgp_last_error()
    assert lib.tgp_kxwxk_f64(0, fake, 100, fake, 10, 4, fake, fake, None, fake, fake, fake, fake, 1 << 40, None) == -9


# ---- the restatement ---------------------------------------------------------------------------------------------------
ALL_CASES = nm.OP_CASES + tuple(nm.SMALL)


@pytest.mark.parametrize("name", ALL_CASES)
def test_two_routes_agree_where_the_table_says(name):
    """Both routes of the update agree to a few ulp times cond(P') on every scenario the GPU tests use, and the figures stay where
    NAT_CPU recorded them (4 x: another BLAS may round differently; 1e-15: figures of a few ulp)."""
    assert set(nm.NAT_CPU) == set(ALL_CASES)
    got, rec = nm.measure(name), nm.NAT_CPU[name]
    print(name, got)
    assert set(got) == set(rec) == {"kxwxk"} | set(nm.SCENARIOS)
    for sc in got:
        assert got[sc]["route"] < 1e-12 and got[sc]["route"] <= 4.0 * rec[sc]["route"] + 1e-15, sc
        if sc != "kxwxk":
            assert 0.5 * rec[sc]["cond"] <= got[sc]["cond"] <= 2.0 * rec[sc]["cond"], sc


@pytest.mark.parametrize("name", ALL_CASES)
def test_gaussian_sites_at_rho_one_give_the_closed_form_optimum(name):
    """lambda = c / sigma^2, r = c y / sigma^2: the step is optqu_model.closed_form_rev's (m*, Lam*), from any q(u)."""
    p = nm.make_case(name)
    m0, L0 = om.closed_form_rev(p)
    args = nm.scenario(p, "gauss")
    garbage = nm.state(p)
    for upd in (nm.update_rev, nm.update_inv):
        for q in (args[:2], garbage):
            m, Lam = upd(p, *q, *args[2:])
            errs = (om.rel(m, m0), om.rel(Lam, L0))
            print(name, upd.__name__, errs)
            assert max(errs) < nm.TOL
            assert torch.equal(Lam, torch.tril(Lam)) and bool((torch.diagonal(Lam) > 0).all())


POISSON_BOUND = 1e-6      # |dELBO/dm| after 12 steps at rho = 1 over its value at the start


@pytest.mark.parametrize("name", ["n40_m6", "n60_m8"])
def test_poisson_steps_are_monotone_and_converge(name):
    p = nm.make_case(name)
    M = p["M"]
    m, Lam = torch.zeros(M, dtype=F64), torch.eye(M, dtype=F64)
    g0 = float(nm.grad_m(p, m, Lam, "poisson").abs().max())
    hist = [float(nm.elbo(p, m, Lam, "poisson"))]
    for _ in range(12):
        m, Lam = nm.step(p, m, Lam, "poisson")
        hist.append(float(nm.elbo(p, m, Lam, "poisson")))
    ratio = float(nm.grad_m(p, m, Lam, "poisson").abs().max()) / g0
    print(name, hist, ratio)
    assert all(b >= a - 1e-9 * abs(a) for a, b in zip(hist, hist[1:])) and hist[1] > hist[0] + 1.0
    assert ratio < POISSON_BOUND


@pytest.mark.parametrize("rho", [0.1, 0.5])
def test_damped_poisson_steps_are_monotone(rho):
    p = nm.make_case("n40_m6")
    m, Lam = torch.zeros(p["M"], dtype=F64), torch.eye(p["M"], dtype=F64)
    hist = [float(nm.elbo(p, m, Lam, "poisson"))]
    for _ in range(4):
        m, Lam = nm.step(p, m, Lam, "poisson", rho=rho)
        hist.append(float(nm.elbo(p, m, Lam, "poisson")))
    assert all(b > a for a, b in zip(hist, hist[1:])), hist


def test_a_fixed_point_of_m_is_a_stationary_point_whatever_the_floor():
    """m' = m <=> dELBO/dm = 0: after convergence with one floor, a step with another leaves m where it is."""
    p = nm.make_case("n40_m6")
    m, Lam = torch.zeros(p["M"], dtype=F64), torch.eye(p["M"], dtype=F64)
    for _ in range(14):
        m, Lam = nm.step(p, m, Lam, "poisson")
    for floor in (0.0, 0.7, None):
        m2, _ = nm.step(p, m, Lam, "poisson", floor=floor)
        assert om.rel(m2, m) < 1e-8, floor


def test_sites_without_a_floor_can_make_p_prime_indefinite():
    """v_bar = +5 (lambda = -10 on every row): lambda_min(P') < 0 without a floor, P' = I with the floor at 0."""
    for name in ("n40_m6", "n60_m8"):
        p = nm.make_case(name)
        m, Lam = nm.state(p)
        mu, _ = nm.moments(p, m, Lam)
        vb = torch.full_like(mu, 5.0)
        lmin = float(torch.linalg.eigvalsh(nm.p_prime(p, m, Lam, mu, torch.zeros_like(mu), vb, 1.0, None)).min())
        print(name, "lambda_min", lmin)
        assert lmin < -1.0
        assert torch.equal(nm.p_prime(p, m, Lam, mu, torch.zeros_like(mu), vb, 1.0, 0.0), torch.eye(p["M"], dtype=F64))


def test_closed_form_sites_are_the_autograd_of_their_ell():
    p = nm.make_case("n60_m8")
    mu, v = nm.moments(p, *nm.state(p))
    for closed, ell in ((nm.gauss_sites, nm.gauss_ell), (nm.poisson_sites, nm.poisson_ell)):
        (a, b), (c, d) = closed(p, mu, v), nm.autograd_sites(ell, p, mu, v)
        assert om.rel(a, c) < 1e-13 and om.rel(b, d) < 1e-13


# ---- the operator's reading of the status words, the library stubbed ------------------------------------------------------
class StubLib:
    """tgp_natgrad_qu_f64 on host tensors: writes a scripted (status[0], status[1]) per call and records the jitter it was handed."""

    def __init__(self, script):
        self.script, self.jitters = list(script), []

    def tgp_natgrad_qu_workspace_bytes(self, N, D, M):
        return 4096

    def tgp_natgrad_qu_f64(self, md, X, mu, mb, vb, rho, floor, m, Lam, status, ws, nbytes, stream):
        self.jitters.append(float(md.jitter))
        st = (C.c_int32 * 8).from_address(status.value)
        st[0], st[1] = self.script[min(len(self.jitters), len(self.script)) - 1]
        return 0


@pytest.mark.parametrize("script,error,word,calls", [
    ([(0, 0)], None, None, 1),
    ([(2, 0), (0, 0)], None, None, 2),                                   # K's pivot: the ladder climbs
    ([(0, 1)], "NanError", "NaN", 1),                                    # K's NaN flag is not a pivot of P'
    ([(3, 1)], "NanError", "NaN", 1),
    ([(0, 4)], "NotPSDError", r"P' = .*\(pivot 3\)", 1),                  # 1 + pivot of P': no jitter tried
    ([(0, -2)], "NotPSDError", r"Lam Lam\^T not positive definite \(pivot 2\)", 1),
    ([(0, 5)], "NotPSDError", "it holds NaNs", 1),                       # M = 3: pivot M + 1 stands for NaNs without a pivot
    ([(2, 0), (0, 3)], "NotPSDError", r"P' = .*\(pivot 2\)", 2),
])
def test_natgrad_qu_tells_the_status_words_apart(monkeypatch, script, error, word, calls):
    import warnings
    from tgp.pytorch_amd import ops
    monkeypatch.setattr(L, "ptr", lambda t: None if t is None else C.c_void_p(t.data_ptr()))
    monkeypatch.setattr(L, "stream_ptr", lambda: None)
    lib = StubLib(script)
    monkeypatch.setattr(L, "load", lambda: lib)
    g = torch.Generator().manual_seed(0)
    r = lambda *s: torch.randn(*s, dtype=F64, generator=g)      # noqa: E731
    args = (r(6, 2), r(3, 2), r(2), r(1), r(3), r(3, 3), r(6), r(6), r(6))
    info = {}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", ops.NumericalWarning)
        if error is None:
            ops.natgrad_qu(*args, rho=0.5, info=info)
            assert "not_pd" not in info
        else:
            with pytest.raises(getattr(ops, error), match=word):
                ops.natgrad_qu(*args, rho=0.5, info=info)
    assert len(lib.jitters) == calls and lib.jitters[0] == 0.0 and (calls == 1 or lib.jitters[1] == 1e-8)
    assert info["jitter"] == lib.jitters[-1]


# ---- refusals ----------------------------------------------------------------------------------------------------------
def _model(kind, whiten=True, mean="zero"):
    from tgp.pytorch_amd.flows import SAL
    from tgp.pytorch_amd.kernels import instance_kernel
    from tgp.pytorch_amd.likelihoods import (Bernoulli, GaussianLinearMean, GaussianNonLinearMean, HeteroscedasticGaussian,
                                             MulticlassCategorical, NegativeBinomial, Poisson, StudentT, WarpedGaussianLinearMean)
    from tgp.pytorch_amd.models import sparse_MF_GP, sparse_MF_SP
    torch.manual_seed(0)
    D, M, N = 3, 5, 20
    X = torch.randn(N, D, dtype=F64)
    nout = {"multiclass": 3, "hetero": 2}.get(kind, 1)
    K = instance_kernel("scale_rbf", ard_num_dim=D, num_multioutput=nout, kernel_is_shared=False)
    tail = (nout, whiten, False, False, False, False)
    liks = {"svgp": lambda: GaussianLinearMean(1, 0.05, False), "bernoulli": Bernoulli, "poisson": Poisson,
            "negbin": NegativeBinomial, "student": lambda: StudentT(1, 0.05, False, 8),
            "multiclass": lambda: MulticlassCategorical(3),
            "wgp": lambda: WarpedGaussianLinearMean(out_dim=1, noise_init=0.05, noise_is_shared=False, flow=SAL(1), quad_points=8)}
    if kind in liks:
        return sparse_MF_GP([mean, K], X, X[:M].clone(), float(N), liks[kind](), *tail, 0.0)
    if kind == "hetero":
        return sparse_MF_SP([mean, K], X, X[:M].clone(), float(N), HeteroscedasticGaussian(noise_init=0.05, quadrature_points=8),
                            *tail, [[("identity", [])], [("identity", [])]], "single", 0.0)
    flow = SAL(1) if kind == "tgp" else SAL(1, input_dependent=True, input_dim=D, num_hidden_layers=1, batch_norm=0, dropout=0.5,
                                            hidden_dim=8, hidden_activation="tanh", inference="MC_dropout")
    return sparse_MF_SP([mean, K], X, X[:M].clone(), float(N), GaussianNonLinearMean(1, 0.05, False, quadrature_points=8), *tail,
                        [flow], "single", 0.0)


REFUSED = [("multiclass", True, "zero", "3 coupled latent GPs"), ("hetero", True, "zero", "2 coupled latent GPs"),
           ("svgp", False, "zero", "is_whiten=False"), ("id_tgp", True, "zero", r"input-dependent flows \(ID_TGP\)"),
           ("svgp", True, "linear", "non-zero mean function"), ("bernoulli", True, "identity", "non-zero mean function"),
           ("wgp", True, "zero", "set_optimal_qu gives the exact optimum")]
COVERED = ["svgp", "bernoulli", "poisson", "negbin", "student", "tgp"]


@pytest.mark.parametrize("kind,whiten,mean,word", REFUSED)
def test_models_the_step_is_not_built_for_refuse_with_the_reason(kind, whiten, mean, word):
    from tgp.pytorch_amd.trainers import Trainer_SP_regression
    model = _model(kind, whiten, mean)
    X, Y = torch.zeros(4, 3, dtype=F64), torch.zeros(4, 1, dtype=F64)
    before = model.q_U.variational_mean.detach().clone()
    with pytest.raises(NotImplementedError, match="natgrad_step_qu: .*" + word):
        model.natgrad_step_qu(X, Y)
    with pytest.raises(NotImplementedError, match="qu='natgrad': .*" + word):
        Trainer_SP_regression(model, [[(X, Y)]], 1e20, False, False, torch.ones(model.out_dim), -1, 100, qu="natgrad")
    assert torch.equal(model.q_U.variational_mean.detach(), before)


def test_fully_bayesian_mode_refuses():
    model = _model("tgp")
    model.be_fully_bayesian(True)
    with pytest.raises(NotImplementedError, match="natgrad_step_qu: be_fully_bayesian"):
        model.natgrad_step_qu(torch.zeros(4, 3, dtype=F64), torch.zeros(4, 1, dtype=F64))


@pytest.mark.parametrize("kind", COVERED)
def test_covered_models_are_not_refused(kind):
    assert _model(kind)._natgrad_refusal() is None


# ---- trainer -----------------------------------------------------------------------------------------------------------
class StubModel(torch.nn.Module):
    """Records the calls of the trainer's loop; ELBO is a quadratic in its one hyper-parameter."""

    out_dim = 1
    fully_bayesian = False

    def __init__(self, refusal=None):
        super().__init__()
        self.w = torch.nn.Parameter(torch.ones(1, dtype=F64))
        self.q_U = torch.nn.Module()
        self.q_U.variational_mean = torch.nn.Parameter(torch.zeros(1, 2, dtype=F64))
        self.calls, self.refusal = [], refusal

    def _natgrad_refusal(self):
        return self.refusal

    def set_is_training(self, mode):
        pass

    def natgrad_step_qu(self, x, y, lr=1.0, site_floor=0.0):
        self.calls.append(("natgrad", x.shape[0], lr, site_floor))
        return {"jitter": 0.25}

    def ELBO(self, x, y, _qu_jitter=None):
        self.calls.append(("elbo", x.shape[0]) if _qu_jitter is None else ("elbo", x.shape[0], _qu_jitter))
        e = -(self.w ** 2).sum()
        return e, e.detach(), torch.zeros(())


def test_trainer_natgrad_option():
    from tgp.pytorch_amd.trainers import Trainer_SP_classification, Trainer_SP_regression
    X, Y = torch.zeros(4, 3, dtype=F64), torch.zeros(4, 1, dtype=F64)
    args = (1e20, False, False, torch.ones(1), -1, 100)
    with pytest.raises(ValueError, match="qu must be 'adam', 'optimal' or 'natgrad', got 'natural'"):
        Trainer_SP_regression(StubModel(), [[(X, Y)]], *args, qu="natural")
    with pytest.raises(NotImplementedError, match="qu='natgrad': because"):
        Trainer_SP_regression(StubModel("because"), [[(X, Y)]], *args, qu="natgrad")
    for bad in (0.0, 1.5, float("nan")):
        with pytest.raises(ValueError, match="natgrad_lr must be in"):
            Trainer_SP_regression(StubModel(), [[(X, Y)]], *args, qu="natgrad", natgrad_lr=bad)
    for cls in (Trainer_SP_regression, Trainer_SP_classification):
        model = StubModel()
        tr = cls(model, [[(X, Y), (X[:3], Y[:3])]], *args, qu="natgrad", natgrad_lr=0.5)      # any number of minibatches
        assert tr.qu == "natgrad" and tr.natgrad_lr == 0.5
        groups, placed = tr._param_groups([[0.02, "variational_mean"]], 0.01)                  # naming q(u) places nothing
        assert placed == ["w"] and [id(q) for g in groups for q in g["params"]] == [id(model.w)]
        tr.train(epochs=2, lr_ALL=0.1, opt="adam", keep_parameter_groups=True)
        assert tr._engine is None
        # (the ELBO takes q(u) as a constant, at the jitter the step reported)
        assert model.calls == [("natgrad", 4, 0.5, 0.0), ("elbo", 4, 0.25), ("natgrad", 3, 0.5, 0.0), ("elbo", 3, 0.25)] * 2
        held = {id(q) for g in tr.optimizer.param_groups for q in g["params"]}
        assert held == {id(model.w)} and all(id(q) in held for q in tr.optimizer.state)
        assert float(model.w.detach()) < 1.0 and len(tr.loss_arr) == 4
        tr.refresh_qu()                                                                        # nothing to refresh
        assert len(model.calls) == 8
    plain = StubModel()
    Trainer_SP_regression(plain, [[(X, Y)]], *args).train(epochs=1, lr_ALL=0.1, opt="adam", keep_parameter_groups=True)
    assert plain.calls == [("elbo", 4)]


# ---- main.py -----------------------------------------------------------------------------------------------------------
BASE = ["--train_test_seed_split", "1", "--num_inducing", "5", "--qu", "natgrad"]
MAIN_REFUSED = [
    (["--model", "SVGP", "--dataset", "synthetic_hetero", "--likelihood", "hetero"], "--qu natgrad: not --likelihood hetero (two coupled latent GPs"),
    (["--model", "SVGP", "--dataset", "synthetic_blobs", "--likelihood", "multiclass"], "--qu natgrad: not --likelihood multiclass (C coupled latent GPs"),
    (["--model", "WGP", "--dataset", "synthetic_power"], "--qu natgrad: not --model WGP (Gaussian in f on the warped targets: --qu optimal"),
    (["--model", "ID_TGP", "--dataset", "synthetic_power"], "--qu natgrad: not --model ID_TGP (input-dependent flows"),
    (["--model", "SVGP", "--dataset", "synthetic_power", "--whiten", "0"], "--qu natgrad: --whiten 1 only"),
    (["--model", "SVGP", "--dataset", "synthetic_power", "--mean", "linear"], "--qu natgrad: --mean zero only"),
    (["--model", "TGP", "--dataset", "synthetic_counts", "--likelihood", "poisson", "--mean", "identity"], "--qu natgrad: --mean zero only"),
    (["--model", "SVGP", "--dataset", "synthetic_power", "--natgrad_lr", "0"], "--natgrad_lr: the step size must be in (0, 1], got 0"),
    (["--model", "SVGP", "--dataset", "synthetic_power", "--natgrad_lr", "1.5"], "--natgrad_lr: the step size must be in (0, 1], got 1.5"),
]


@pytest.mark.parametrize("argv,text", MAIN_REFUSED)
def test_main_refuses_with_the_reason(capsys, argv, text):
    from tgp.pytorch_amd import main as M
    with pytest.raises(SystemExit) as e:
        M.main(argv + BASE)
    assert e.value.code == 2 and text in capsys.readouterr().err


def test_main_keeps_the_optimal_errors_word_for_word(capsys):
    from tgp.pytorch_amd import main as M
    for argv, text in (
            (["--model", "TGP", "--dataset", "synthetic_power"],
             "--qu optimal: SVGP or WGP with the gaussian likelihood and --whiten 1 (the likelihood must be Gaussian in f)"),
            (["--model", "SVGP", "--dataset", "synthetic_hetero", "--likelihood", "hetero"],
             "--likelihood hetero: --qu adam only (two coupled latent GPs: no closed-form optimal q(u))")):
        with pytest.raises(SystemExit):
            M.main(argv + ["--train_test_seed_split", "1", "--num_inducing", "5", "--qu", "optimal"])
        assert text in capsys.readouterr().err


class _TrainerReached(Exception):
    pass


def test_main_hands_the_option_to_the_trainer(monkeypatch):
    """main([... --qu natgrad --natgrad_lr 0.5]) up to the trainer's construction, data set, initialiser and model stubbed."""
    from tgp.pytorch_amd import config as cg
    from tgp.pytorch_amd import main as M
    monkeypatch.setattr(cg, "device", "cpu")

    class HostConfig:
        """config with a device that stays where it is: main() names the GPU, this test has none"""

        def __getattr__(self, k):
            return getattr(cg, k)

        def __setattr__(self, k, v):
            if k != "device":
                setattr(cg, k, v)
    monkeypatch.setattr(M, "cg", HostConfig())
    X = torch.randn(20, 3, dtype=F64, generator=torch.Generator().manual_seed(4))
    dc = {"X_tr": X, "Y_tr": X[:, :1].abs().round(), "Dx": 3, "Dy": 1, "N_tr": 20, "Y_std": 1.0}
    monkeypatch.setattr(M, "return_dataset", lambda *a, **k: ([None, None, None], dc))
    monkeypatch.setattr(M, "KMEANS", lambda Xa, num_Z, **kw: Xa[:num_Z])
    monkeypatch.setattr(M, "sparse_MF_GP", lambda **kw: StubModel())

    def trainer(**kw):
        raise _TrainerReached(kw)
    monkeypatch.setattr(M, "Trainer_SP_regression", trainer)
    with pytest.raises(_TrainerReached) as e:
        M.main(["--model", "SVGP", "--dataset", "synthetic_counts", "--likelihood", "poisson", "--natgrad_lr", "0.5"] + BASE)
    kw = e.value.args[0]
    assert kw["qu"] == "natgrad" and kw["natgrad_lr"] == 0.5 and math.isfinite(kw["natgrad_lr"])
