"""CPU: pathwise posterior function draws -- the covariance of the restated draws (tests/pathwise_model.py) against the exact q(f)
covariance, the spectral sampler of the package, the library's host-side refusals, and ops.pathwise_coeff / ops.pathwise_eval /
PosteriorPaths / model.posterior_paths with the library stubbed."""
import ctypes as C

import pytest
import torch

import pathwise_model as pm
from tgp.pytorch_amd import lib as L
from tgp.pytorch_amd import ops
from tgp.pytorch_amd import pathwise as pw

F64 = torch.float64


@pytest.fixture(scope="module", autouse=True)
def f64():
    from tgp.pytorch_amd import config as cg
    old = torch.get_default_dtype()
    cg.set_maximum_precission()
    cg.device = "cpu"
    yield
    torch.set_default_dtype(old)


# ---- the restatement ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", pm.CASES, ids=lambda c: "%d-%d-%d-%d-%d-%s" % c)
def test_case_table_and_interpolation(case):
    """Every case keeps cond(K_ZZ) <= 1e5 where PATHWISE_CPU recorded it, and the restated draws interpolate u_s = L (m + Lam eps_s)
    at X = Z below 1e-12 (cond x 2^-52 = 2e-11 would be the bound of a solve at the limit; the cases stay far inside)."""
    assert set(pm.PATHWISE_CPU) == set(pm.CASES)
    p = pm.make_case(*case)
    rec = pm.PATHWISE_CPU[case]
    cond = pm.cond_K(p)
    assert cond <= pm.COND_MAX and 0.5 * rec["cond"] <= cond <= 2.0 * rec["cond"]
    cf = pm.coeff(p)
    u = pm.inducing_values(p)
    err = float((pm.evaluate(p, cf, p["Z"]).T - u).abs().max() / u.abs().max())
    print(case, "cond %.1e interp %.1e" % (cond, err))
    assert err < 1e-12
    assert cf.shape == (2 * p["R2"] + p["M"], p["S"])
    # the prior variance of the features is s2 at every row
    Phi = pm.features(p["X"], p["raw_ls"], p["raw_os"], p["omega"])
    assert float(((Phi ** 2).sum(1) - p["s2"]).abs().max()) < 1e-13 * p["s2"] * max(1, p["R2"]) ** 0.5 + 1e-14


@pytest.mark.parametrize("kind", pm.KINDS)
def test_draw_covariance_approaches_the_exact_one(kind):
    """J_w J_w^T + J_e J_e^T of the restated draws against K_XX + A^T (Lam Lam^T - I) A at R2 = 256 and 2048 (N = 300, D = 4,
    M = 40): the error shrinks with R2 and each stays within 2 x what DRAW_COV_CPU recorded (seeded inputs: the margin covers
    library differences only)."""
    err = {}
    for R2 in (256, 2048):
        p = pm.cov_case(kind, R2)
        assert pm.cond_K(p) <= pm.COND_MAX
        err[R2] = float((pm.draw_cov(p) - pm.exact_cov(p)).abs().max() / p["s2"])
        print(kind, R2, "draw covariance error / s2 = %.3e" % err[R2])
        assert err[R2] <= 2.0 * pm.DRAW_COV_CPU[(kind, R2)]
    assert err[2048] < err[256]


@pytest.mark.parametrize("kind", pm.KINDS)
def test_spectral_frequencies_give_the_kernel(kind):
    """Phi_X Phi_X^T with the PACKAGE's frequencies approaches K_XX for both kernels (a wrong Student-t scaling of the Matern
    frequencies leaves an error of order s2 that does not shrink), within 2 x what SPECTRAL_CPU recorded."""
    err = {}
    for R2 in (256, 2048):
        om = pw.spectral_frequencies(kind, R2, 4, torch.Generator().manual_seed(0))
        assert om.shape == (R2, 4) and om.dtype == F64
        err[R2] = pm.spectral_error(pm.cov_case(kind, R2, omega=om))
        print(kind, R2, "spectral error / s2 = %.3e" % err[R2])
        assert err[R2] <= 2.0 * pm.SPECTRAL_CPU[(kind, R2)]
    assert err[2048] < err[256]
    # seeded: the same generator state gives the same frequencies, and they are the restatement's own
    a = pw.spectral_frequencies(kind, 7, 3, torch.Generator().manual_seed(5))
    assert torch.equal(a, pw.spectral_frequencies(kind, 7, 3, torch.Generator().manual_seed(5)))
    assert torch.equal(a, pm.spectral_frequencies(kind, 7, 3, torch.Generator().manual_seed(5)))
    with pytest.raises(L.TgpError, match="spectral"):
        pw.spectral_frequencies("scale_matern52", 7, 3)


# ---- the library's refusals: host-only, nothing touches a device ----------------------------------------------------------
def test_library_refuses_outside_its_limits():
    lib = L.load()
    f = lib.tgp_pathwise_workspace_bytes
    need = f(1, 4, 40, 64, 5)
    assert need > 0 and (need - 16) % 512 == 0 and need == f(250000, 4, 40, 64, 5)
    assert f(250000, 8, 1000, 2048, 64) < 1024 ** 3 and f(1, 16, 4096, 8192, 256) > 0
    fake = C.c_void_p(64)
    md = L.TgpModel()
    md.Z = md.raw_ls = md.raw_os = md.m = md.Lam = fake
    for D, M, R2, S, kern in ((0, 40, 64, 5, 0), (17, 40, 64, 5, 0), (4, 0, 64, 5, 0), (4, 4097, 64, 5, 0), (4, 40, 0, 5, 0),
                              (4, 40, 8193, 5, 1), (4, 40, 64, 0, 1), (4, 40, 64, 257, 0), (4, 40, 64, 5, 2), (4, 40, 64, 5, -1)):
        md.D, md.M, md.kernel = D, M, kern
        if kern in (0, 1):
            assert f(1, D, M, R2, S) == 0
        rc = lib.tgp_pathwise_coeff_f64(md, fake, R2, fake, fake, S, fake, fake, fake, 1 << 40, None)
        assert rc == L.E_UNSUPPORTED and b"tgp_pathwise_coeff_f64" in lib.tgp_last_error(), (D, M, R2, S, kern)
        rc = lib.tgp_pathwise_eval_f64(kern, fake, 10, D, fake, M, fake, fake, fake, R2, fake, S, fake, None)
        assert rc == L.E_UNSUPPORTED and b"tgp_pathwise_eval_f64" in lib.tgp_last_error(), (D, M, R2, S, kern)
    assert lib.tgp_pathwise_eval_f64(0, fake, 0, 4, fake, 40, fake, fake, fake, 64, fake, 5, fake, None) == L.E_UNSUPPORTED
    assert f(0, 4, 40, 64, 5) == 0
    md.D, md.M, md.kernel = 4, 40, 0
    rc = lib.tgp_pathwise_coeff_f64(md, fake, 64, fake, fake, 5, fake, fake, fake, need - 24, None)
    assert rc == L.E_WORKSPACE and b"tgp_pathwise_coeff_f64" in lib.tgp_last_error() and str(need).encode() in lib.tgp_last_error()
    args = [md, fake, 64, fake, fake, 5, fake, fake, fake, need, None]
    for pos, code in ((1, -2), (3, -4), (4, -5), (6, -7), (7, -8), (8, -9)):
        a = list(args)
        a[pos] = None
        assert lib.tgp_pathwise_coeff_f64(*a) == code, pos
    assert lib.tgp_pathwise_coeff_f64(None, *args[1:]) == -1
    md.m = None
    assert lib.tgp_pathwise_coeff_f64(*args) == -1
    args = [0, fake, 10, 4, fake, 40, fake, fake, fake, 64, fake, 5, fake, None]
    for pos, code in ((1, -2), (4, -5), (6, -7), (7, -8), (8, -9), (10, -11), (12, -13)):
        a = list(args)
        a[pos] = None
        assert lib.tgp_pathwise_eval_f64(*a) == code, pos
    assert lib.tgp_version() == 104


# ---- host plumbing, the library stubbed -----------------------------------------------------------------------------------
def _vec(ptr, n):
    return list((C.c_double * n).from_address(ptr.value))


class StubLib:
    """The two entries on host tensors: records what it was handed.  coeff fails its factorisation (pivot 3) below `ok_from`;
    coef[r][s] = 100 r + s; F0[s][n] = 1000 s + X[n][0]."""

    def __init__(self, ok_from=0.0):
        self.ok_from, self.calls = ok_from, []

    def tgp_pathwise_workspace_bytes(self, N, D, M, R2, S):
        self.calls.append(dict(entry="bytes", N=N, D=D, M=M, R2=R2, S=S))
        return 4096 + 16

    def tgp_pathwise_coeff_f64(self, md, omega, R2, W, eps, S, coef, status, ws, nbytes, stream):
        md = md if isinstance(md, L.TgpModel) else md.contents
        M, D = md.M, md.D
        self.calls.append(dict(entry="coeff", D=D, M=M, kernel=md.kernel, jitter=md.jitter, R2=R2, S=S, nbytes=nbytes,
                               omega=_vec(omega, R2 * D), W=_vec(W, S * 2 * R2), eps=_vec(eps, S * M),
                               Z=_vec(C.c_void_p(md.Z), M * D), m=_vec(C.c_void_p(md.m), M), Lam=_vec(C.c_void_p(md.Lam), M * M),
                               raw_ls=_vec(C.c_void_p(md.raw_ls), D), raw_os=_vec(C.c_void_p(md.raw_os), 1)))
        st = (C.c_int32 * 8).from_address(status.value)
        st[0] = 0 if md.jitter >= self.ok_from else 3
        cv = (C.c_double * ((2 * R2 + M) * S)).from_address(coef.value)
        for r in range(2 * R2 + M):
            for s in range(S):
                cv[r * S + s] = 100.0 * r + s
        return 0

    def tgp_pathwise_eval_f64(self, kernel, X, N, D, Z, M, rl, ro, omega, R2, coef, S, F0, stream):
        x = _vec(X, N * D)
        self.calls.append(dict(entry="eval", kernel=kernel, N=N, D=D, M=M, R2=R2, S=S, x0=x[0], Z=_vec(Z, M * D), raw_ls=_vec(rl, D),
                               raw_os=_vec(ro, 1), omega=_vec(omega, R2 * D), coef=_vec(coef, (2 * R2 + M) * S)))
        fv = (C.c_double * (S * N)).from_address(F0.value)
        for s in range(S):
            for n in range(N):
                fv[s * N + n] = 1000.0 * s + x[n * D]
        return 0

    def of(self, entry):
        return [c for c in self.calls if c["entry"] == entry]


@pytest.fixture
def stub(monkeypatch):
    monkeypatch.setattr(L, "ptr", lambda t: None if t is None else C.c_void_p(t.data_ptr()))
    monkeypatch.setattr(L, "stream_ptr", lambda: None)

    def make(ok_from=0.0):
        lib = StubLib(ok_from)
        monkeypatch.setattr(L, "load", lambda: lib)
        return lib
    return make


def _inputs(M=5, D=3, R2=4, S=2, seed=0):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, dtype=F64, generator=g)          # noqa: E731
    return dict(Z=r(M, D), raw_ls=r(D), raw_os=r(1), m=r(M), Lam=r(M, M), omega=r(R2, D), W=r(S, 2 * R2), eps=r(S, M))


def test_ops_pathwise_coeff_hands_over_its_arguments_in_order(stub):
    lib = stub()
    q = _inputs()
    info = {}
    coef = ops.pathwise_coeff(q["Z"], q["raw_ls"], q["raw_os"], q["m"], q["Lam"], q["omega"], q["W"], q["eps"], jitter=1e-7,
                              kernel="scale_matern32", info=info)
    assert lib.of("bytes")[-1] == dict(entry="bytes", N=1, D=3, M=5, R2=4, S=2)
    c = lib.of("coeff")[-1]
    assert (c["D"], c["M"], c["R2"], c["S"], c["kernel"], c["jitter"], c["nbytes"]) == (3, 5, 4, 2, L.KERNEL_SCALE_MATERN32, 1e-7, 4112)
    for k in ("Z", "raw_ls", "raw_os", "m", "Lam", "omega", "W", "eps"):
        assert c[k] == q[k].reshape(-1).tolist(), k
    assert coef.shape == (13, 2) and coef[12, 1] == 1201.0 and info["jitter"] == 1e-7
    with pytest.raises(ValueError, match="pathwise_coeff"):
        ops.pathwise_coeff(q["Z"], q["raw_ls"], q["raw_os"], q["m"], q["Lam"], q["omega"], q["W"][:, :-1], q["eps"])
    with pytest.raises(ValueError, match="pathwise_coeff"):
        ops.pathwise_coeff(q["Z"], q["raw_ls"], q["raw_os"], q["m"], q["Lam"], q["omega"], q["W"], q["eps"][:1])
    with pytest.raises(L.TgpError, match="float64"):
        ops.pathwise_coeff(q["Z"].float(), q["raw_ls"], q["raw_os"], q["m"], q["Lam"], q["omega"], q["W"], q["eps"])
    assert len(lib.of("coeff")) == 1


def test_ops_pathwise_coeff_runs_the_one_jitter_ladder(stub):
    lib = stub(ok_from=1e-7)
    q = _inputs()
    info = {}
    with pytest.warns(ops.NumericalWarning):
        ops.pathwise_coeff(q["Z"], q["raw_ls"], q["raw_os"], q["m"], q["Lam"], q["omega"], q["W"], q["eps"], info=info)
    assert [c["jitter"] for c in lib.of("coeff")] == [0.0, 1e-8, 1e-7] and info["jitter"] == 1e-7
    lib = stub(ok_from=1.0)
    with pytest.raises(ops.NotPSDError, match="K_MM"):
        ops.pathwise_coeff(q["Z"], q["raw_ls"], q["raw_os"], q["m"], q["Lam"], q["omega"], q["W"], q["eps"])
    assert [c["jitter"] for c in lib.of("coeff")] == [0.0, 1e-8, 1e-7, 1e-6]
    lib = stub(ok_from=1.0)                     # check=False: one launch, the status is not read
    ops.pathwise_coeff(q["Z"], q["raw_ls"], q["raw_os"], q["m"], q["Lam"], q["omega"], q["W"], q["eps"], check=False)
    assert len(lib.of("coeff")) == 1


def test_ops_pathwise_eval_splits_the_rows(stub):
    lib = stub()
    q = _inputs()
    coef = torch.arange(13 * 2, dtype=F64).reshape(13, 2)
    X = torch.arange(10 * 3, dtype=F64).reshape(10, 3)
    F = ops.pathwise_eval(X, q["Z"], q["raw_ls"], q["raw_os"], q["omega"], coef, kernel="scale_rbf")
    want = torch.stack([X[:, 0], 1000.0 + X[:, 0]])
    c = lib.of("eval")[-1]
    assert torch.equal(F, want) and len(lib.of("eval")) == 1
    assert (c["kernel"], c["N"], c["D"], c["M"], c["R2"], c["S"]) == (L.KERNEL_SCALE_RBF, 10, 3, 5, 4, 2)
    for k in ("Z", "raw_ls", "raw_os", "omega"):
        assert c[k] == q[k].reshape(-1).tolist(), k
    assert c["coef"] == coef.reshape(-1).tolist()
    for step, sizes in ((4, [4, 4, 2]), (1, [1] * 10), (10, [10]), (99, [10])):
        lib.calls.clear()
        assert torch.equal(ops.pathwise_eval(X, q["Z"], q["raw_ls"], q["raw_os"], q["omega"], coef, batch_rows=step), want)
        assert [c["N"] for c in lib.of("eval")] == sizes
        starts = [0] + [sum(sizes[:i]) for i in range(1, len(sizes))]
        assert [c["x0"] for c in lib.of("eval")] == [float(X[a, 0]) for a in starts]
    with pytest.raises(ValueError, match="batch_rows"):
        ops.pathwise_eval(X, q["Z"], q["raw_ls"], q["raw_os"], q["omega"], coef, batch_rows=0)
    with pytest.raises(ValueError, match="pathwise_eval"):
        ops.pathwise_eval(X, q["Z"], q["raw_ls"], q["raw_os"], q["omega"], coef[:-1])
    with pytest.raises(ValueError, match="pathwise_eval"):
        ops.pathwise_eval(X[:, :2], q["Z"], q["raw_ls"], q["raw_os"], q["omega"], coef)


def _svgp(M=5, D=3, N=12, mean="zero", kernel="scale_rbf", whiten=True):
    from tgp.pytorch_amd.kernels import instance_kernel
    from tgp.pytorch_amd.likelihoods import GaussianLinearMean
    from tgp.pytorch_amd.models import sparse_MF_GP
    X = torch.randn(N, D, dtype=F64, generator=torch.Generator().manual_seed(1))
    K = instance_kernel(kernel, ard_num_dim=D, num_multioutput=1, kernel_is_shared=False)
    return X, sparse_MF_GP([mean, K], X, X[:M].clone(), float(N), GaussianLinearMean(1, 0.05, False), 1, whiten, False, False, False,
                           False, 0.0)


def test_model_posterior_paths_draws_in_order_and_keeps_clones(stub):
    lib = stub()
    X, model = _svgp(kernel="scale_matern32")
    paths = model.posterior_paths(2, num_frequencies=4, generator=torch.Generator().manual_seed(9))
    g = torch.Generator().manual_seed(9)
    omega = pw.spectral_frequencies("scale_matern32", 4, 3, g)
    W = torch.randn(2, 8, dtype=F64, generator=g)
    eps = torch.randn(2, 5, dtype=F64, generator=g)
    c = lib.of("coeff")[-1]
    assert c["omega"] == omega.reshape(-1).tolist() and c["W"] == W.reshape(-1).tolist() and c["eps"] == eps.reshape(-1).tolist()
    assert (c["kernel"], c["R2"], c["S"], c["jitter"]) == (L.KERNEL_SCALE_MATERN32, 4, 2, 0.0)
    assert c["Z"] == model.Z[0].reshape(-1).tolist() and c["m"] == model.q_U.variational_mean[0].tolist()
    assert isinstance(paths, pw.PosteriorPaths) and paths.S == 2 and paths.num_frequencies == 4 and paths.kernel == "scale_matern32"
    # detached clones: the model moves, the drawn functions do not
    kept = [t.clone() for t in (paths.Z, paths.raw_ls, paths.raw_os, paths.omega, paths.coef)]
    assert not any(t.requires_grad for t in kept) and paths.Z.data_ptr() != model.Z.data_ptr()
    with torch.no_grad():
        for prm in model.parameters():
            prm.add_(0.5)
    for t, k in zip((paths.Z, paths.raw_ls, paths.raw_os, paths.omega, paths.coef), kept):
        assert torch.equal(t, k)
    F = paths.f0(X)
    e = lib.of("eval")[-1]
    assert F.shape == (2, 12) and e["Z"] == kept[0].reshape(-1).tolist() and e["coef"] == kept[4].reshape(-1).tolist()
    assert torch.equal(paths(X), F)                                         # SVGP: identity flow
    lib.calls.clear()
    assert torch.equal(paths(X, batch_rows=5), F) and [c["N"] for c in lib.of("eval")] == [5, 5, 2]
    assert torch.equal(paths.f0(X.unsqueeze(0), batch_rows=7), F)
    with pytest.raises(ValueError, match="PosteriorPaths"):
        paths.f0(X[:, :2])


def test_model_refusals_reach_no_library_call(stub):
    from tgp.pytorch_amd.kernels import instance_kernel
    from tgp.pytorch_amd.likelihoods import MulticlassCategorical
    from tgp.pytorch_amd.models import sparse_MF_GP
    lib = stub()
    X = torch.randn(20, 3, generator=torch.Generator().manual_seed(0), dtype=F64)
    K = instance_kernel("scale_rbf", ard_num_dim=3, num_multioutput=3, kernel_is_shared=False)
    model = sparse_MF_GP(["zero", K], X, X[:4].clone(), 20.0, MulticlassCategorical(3), 3, True, False, False, False, False, 0.0)
    with pytest.raises(NotImplementedError, match="multi-class"):
        model.posterior_paths(2)
    _, model = _svgp()
    model.be_fully_bayesian(True)
    with pytest.raises(NotImplementedError, match="be_fully_bayesian"):
        model.posterior_paths(2)
    assert lib.calls == []
