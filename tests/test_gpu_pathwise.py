"""GPU (-m gpu): pathwise posterior function draws in HIP (tgp_pathwise_coeff_f64, tgp_pathwise_eval_f64), through the C ABI and
through ops, against the float64 CPU restatement of tests/pathwise_model.py; then PosteriorPaths and model.posterior_paths.

Largest errors seen on an MI355X against the restatement: see DESIGN.md §8."""
import functools

import pytest
import torch

import pathwise_model as pm

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F64 = torch.float64
TOL = 1e-9            # the project's tolerance for a float64 kernel against its restatement
ids = lambda c: "%d-%d-%d-%d-%d-%s" % c          # noqa: E731
SENTINEL = -7.0
BIG_MAX_M = 4096      # TGP_BIG_MAX_M


@pytest.fixture(scope="module", autouse=True)
def f64():
    from tgp.pytorch_amd import config as cg
    old = torch.get_default_dtype()
    cg.set_maximum_precission()
    cg.device = DEV
    yield
    torch.set_default_dtype(old)


def _dev(p, *names):
    return [p[n].to(DEV).contiguous() for n in names]


def _model(p, Z, rl, ro, m, Lam, **over):
    from tgp.pytorch_amd import lib as L
    md = L.TgpModel()
    md.N, md.D, md.M, md.S = p["M"], p["D"], p["M"], 1
    md.kernel = L.KERNELS[p["kernel"]]
    md.scale, md.kl_scale, md.jitter = 1.0, 1.0, float(p["jitter"])
    md.Z, md.raw_ls, md.raw_os, md.m, md.Lam = L.ptr(Z), L.ptr(rl), L.ptr(ro), L.ptr(m), L.ptr(Lam)
    for k, v in over.items():
        setattr(md, k, v)
    return md


def abi_coeff(p, expect=0, ws_bytes=None, R2=None, S=None, null=(), W=None, eps=None, **over):
    """One call of tgp_pathwise_coeff_f64 on a case: (coef on the host, status on the host); coef and the status start as
    sentinels so that an entry never written shows.  `R2`, `S`, `over` (model fields) and `null` (argument names passed as NULL)
    make the refused calls."""
    from tgp.pytorch_amd import lib as L
    lib = L.load()
    Z, rl, ro, m, Lam, om = _dev(p, "Z", "raw_ls", "raw_os", "m", "Lam", "omega")
    W = (p["W"] if W is None else W).to(DEV).contiguous()
    eps = (p["eps"] if eps is None else eps).to(DEV).contiguous()
    r2 = p["R2"] if R2 is None else R2
    s = p["S"] if S is None else S
    md = _model(p, Z, rl, ro, m, Lam, **over)
    need = lib.tgp_pathwise_workspace_bytes(1, p["D"], p["M"], p["R2"], p["S"])
    assert need > 0
    ws = torch.empty(need // 8 + 1, dtype=F64, device=DEV)
    coef = torch.full((2 * p["R2"] + p["M"], p["S"]), SENTINEL, dtype=F64, device=DEV)
    status = torch.full((8,), -7, dtype=torch.int32, device=DEV) if expect else torch.zeros(8, dtype=torch.int32, device=DEV)
    arg = dict(omega=L.ptr(om), W=L.ptr(W), eps=L.ptr(eps), coef=L.ptr(coef), status=L.ptr(status), workspace=L.ptr(ws))
    for n in null:
        arg[n] = None
    rc = lib.tgp_pathwise_coeff_f64(md, arg["omega"], r2, arg["W"], arg["eps"], s, arg["coef"], arg["status"], arg["workspace"],
                                    need if ws_bytes is None else ws_bytes, L.stream_ptr())
    assert rc == expect, (rc, lib.tgp_last_error())
    torch.cuda.synchronize()
    return coef.cpu(), status.cpu()


def abi_eval(p, coef, X=None, expect=0, null=(), **over):
    """One call of tgp_pathwise_eval_f64: F0 (S, N) on the host, sentinels where nothing was written."""
    from tgp.pytorch_amd import lib as L
    lib = L.load()
    X = (p["X"] if X is None else X).to(DEV).contiguous()
    Z, rl, ro, om = _dev(p, "Z", "raw_ls", "raw_os", "omega")
    coef = coef.to(DEV).contiguous()
    a = dict(kernel=L.KERNELS[p["kernel"]], N=X.shape[0], D=p["D"], M=p["M"], R2=p["R2"], S=p["S"])
    a.update(over)
    F0 = torch.full((p["S"], X.shape[0]), SENTINEL, dtype=F64, device=DEV)
    arg = dict(X=L.ptr(X), Z=L.ptr(Z), raw_ls=L.ptr(rl), raw_os=L.ptr(ro), omega=L.ptr(om), coef=L.ptr(coef), F0=L.ptr(F0))
    for n in null:
        arg[n] = None
    rc = lib.tgp_pathwise_eval_f64(a["kernel"], arg["X"], a["N"], a["D"], arg["Z"], a["M"], arg["raw_ls"], arg["raw_os"],
                                   arg["omega"], a["R2"], arg["coef"], a["S"], arg["F0"], L.stream_ptr())
    assert rc == expect, (rc, lib.tgp_last_error())
    torch.cuda.synchronize()
    return F0.cpu()


@functools.lru_cache(maxsize=None)
def _case(case):
    """(inputs, the device's coef and F0, the restatement's coef and F0): once per case."""
    p = pm.make_case(*case)
    coef, status = abi_coeff(p)
    assert int(status[0]) == 0 and int(status[1]) == 0, status
    F0 = abi_eval(p, coef)
    cref = pm.coeff(p)
    return p, coef, F0, cref, pm.evaluate(p, cref)


# ---- 1. parity with the restatement ------------------------------------------------------------------------------
@pytest.mark.parametrize("case", pm.CASES, ids=ids)
def test_parity_with_the_restatement(case):
    """coef and F0 within 1e-9 of the case's largest |coef| and |F0|; cond(K_ZZ) is the table's and <= 1e5."""
    p, coef, F0, cref, Fref = _case(case)
    cond = pm.cond_K(p)
    assert cond <= pm.COND_MAX and abs(cond / pm.PATHWISE_CPU[case]["cond"] - 1.0) < 0.1
    assert bool(torch.isfinite(coef).all()) and bool(torch.isfinite(F0).all())
    ec = float((coef - cref).abs().max() / cref.abs().max())
    ef = float((F0 - Fref).abs().max() / Fref.abs().max())
    print(case, "cond %.1e  coef %.3g  F0 %.3g" % (cond, ec, ef))
    assert ec <= TOL and ef <= TOL, (ec, ef)


@pytest.mark.parametrize("case", [pm.CASES[3], pm.CASES[11]], ids=ids)
def test_ops_give_the_abis_bits(case):
    from tgp.pytorch_amd import ops
    p, coef, F0, _, _ = _case(case)
    Z, rl, ro, m, Lam, om, W, eps, X = _dev(p, "Z", "raw_ls", "raw_os", "m", "Lam", "omega", "W", "eps", "X")
    info = {}
    c2 = ops.pathwise_coeff(Z, rl, ro, m, Lam, om, W, eps, kernel=p["kernel"], info=info)
    assert info["jitter"] == 0.0 and torch.equal(c2.cpu(), coef)
    assert torch.equal(ops.pathwise_eval(X, Z, rl, ro, om, c2, kernel=p["kernel"]).cpu(), F0)


# ---- 2. interpolation ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", pm.CASES, ids=ids)
def test_a_draw_interpolates_its_inducing_values(case):
    """Jitter 0: F0 at X = Z is u_s = L (m + Lam eps_s) of the CPU, within 1e-9 max |u|."""
    p, coef, _, _, _ = _case(case)
    u = pm.inducing_values(p)                     # (M, S)
    FZ = abi_eval(p, coef, X=p["Z"])
    err = float((FZ.T - u).abs().max() / u.abs().max())
    print(case, "interpolation %.3g" % err)
    assert err <= TOL


# ---- 3. mean ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", pm.CASES, ids=ids)
def test_zero_noise_draws_are_the_posterior_mean(case):
    """W = 0 and eps = 0: every draw is mu of ops.qf_moments on the same rows, within 1e-9 max |mu|."""
    from tgp.pytorch_amd import ops
    p = _case(case)[0]
    coef, _ = abi_coeff(p, W=torch.zeros_like(p["W"]), eps=torch.zeros_like(p["eps"]))
    F0 = abi_eval(p, coef)
    X, Z, rl, ro, m, Lam = _dev(p, "X", "Z", "raw_ls", "raw_os", "m", "Lam")
    mu, _ = ops.qf_moments(X, Z, rl, ro, m, Lam, kernel=p["kernel"])
    mu = mu.cpu()
    err = float((F0 - mu.reshape(1, -1)).abs().max() / mu.abs().max())
    print(case, "mean %.3g" % err)
    assert err <= TOL


# ---- 4. a draw is a function --------------------------------------------------------------------------------------
def test_pieces_and_batches_give_the_same_bits():
    from tgp.pytorch_amd import ops
    case = pm.CASES[13]                            # N = 1000
    p, coef, F0, _, _ = _case(case)
    assert p["N"] == 1000
    X, Z, rl, ro, om = _dev(p, "X", "Z", "raw_ls", "raw_os", "omega")
    cd = coef.to(DEV)
    for step in (1, 63, 257):
        parts = [ops.pathwise_eval(X[a:a + step], Z, rl, ro, om, cd, kernel=p["kernel"]) for a in range(0, 1000, step)]
        assert torch.equal(torch.cat(parts, 1).cpu(), F0), step
        assert torch.equal(ops.pathwise_eval(X, Z, rl, ro, om, cd, kernel=p["kernel"], batch_rows=step).cpu(), F0), step
    # rows in another order, and a row beside other neighbours: the same values
    perm = torch.randperm(1000, generator=torch.Generator().manual_seed(3))
    assert torch.equal(ops.pathwise_eval(X[perm.to(DEV)].contiguous(), Z, rl, ro, om, cd, kernel=p["kernel"]).cpu(), F0[:, perm])


@pytest.mark.parametrize("case", pm.CASES[15:], ids=ids)
def test_both_row_tilings_give_the_same_bits(case):
    """N = 16 450 runs the 64-row workgroups, its pieces of 5000 rows and of 16 384 + 66 rows the 16-row ones (the switch is at
    16 384 rows): every sample tiling of the row kernel, the same bits."""
    from tgp.pytorch_amd import ops
    p, coef, F0, _, _ = _case(case)
    assert p["N"] == 16450
    X, Z, rl, ro, om = _dev(p, "X", "Z", "raw_ls", "raw_os", "omega")
    cd = coef.to(DEV)
    assert torch.equal(ops.pathwise_eval(X, Z, rl, ro, om, cd, kernel=p["kernel"], batch_rows=5000).cpu(), F0)
    assert torch.equal(ops.pathwise_eval(X, Z, rl, ro, om, cd, kernel=p["kernel"], batch_rows=16384).cpu(), F0)
    assert torch.equal(ops.pathwise_eval(X[:16385], Z, rl, ro, om, cd, kernel=p["kernel"]).cpu(), F0[:, :16385])


@pytest.mark.parametrize("case", [pm.CASES[5], pm.CASES[11]], ids=ids)
def test_two_coeff_calls_are_bit_identical(case):
    p, coef, F0, _, _ = _case(case)
    c2, _ = abi_coeff(p)
    assert torch.equal(c2, coef)
    assert torch.equal(abi_eval(p, c2), F0)


# ---- 5. model level -----------------------------------------------------------------------------------------------
MODEL_N, MODEL_D, MODEL_M, MODEL_R2, MODEL_S = 300, 4, 40, 64, 5
MODELS = ("svgp", "tgp_sal2", "idtgp", "linear_mean", "unwhitened")


def _build(kind, p):
    from tgp.pytorch_amd.flow import compile_flow, instance_flow
    from tgp.pytorch_amd.flows import SAL
    from tgp.pytorch_amd.kernels import instance_kernel
    from tgp.pytorch_amd.likelihoods import GaussianLinearMean, GaussianNonLinearMean
    from tgp.pytorch_amd.models import sparse_MF_GP, sparse_MF_SP
    torch.manual_seed(0)
    N, D, M = MODEL_N, MODEL_D, MODEL_M
    K = instance_kernel(p["kernel"], ard_num_dim=D, num_multioutput=1, kernel_is_shared=False)
    ip = {"variational_distribution": {"variance_scale": 1e-5, "mean_scale": 0.0}}
    mean = "linear" if kind == "linear_mean" else "zero"
    whiten = kind != "unwhitened"
    if kind in ("svgp", "linear_mean", "unwhitened"):
        model = sparse_MF_GP([mean, K], p["X"], p["Z"].clone(), N, GaussianLinearMean(1, 0.05, False), 1, whiten, False, False, False,
                             False, 0.0, init_params=ip)
    else:
        if kind == "idtgp":
            flow = instance_flow(SAL(1, input_dependent=True, input_dim=D, num_hidden_layers=2, batch_norm=0, dropout=0.25,
                                     hidden_dim=50, hidden_activation="relu", inference="MC_dropout"))
            flow.turn_off_initializer_parameters()
        else:
            flow = SAL(2)
        model = sparse_MF_SP(["zero", K], p["X"], p["Z"].clone(), N, GaussianNonLinearMean(1, 0.05, False, quadrature_points=8), 1,
                             True, False, False, False, False, [flow], "single", 0.0, init_params=ip)
    g = torch.Generator().manual_seed(17)
    with torch.no_grad():
        model.Z.data = p["Z"].reshape(1, M, D).clone()
        model.q_U.variational_mean.data = p["m"].reshape(1, M).clone()
        model.q_U.chol_variational_covar.data = p["Lam"].reshape(1, M, M).clone()
        model.covariance_function.raw_outputscale.data = p["raw_os"].reshape(1).clone()
        model.covariance_function.base_kernel.raw_lengthscale.data = p["raw_ls"].reshape(1, 1, D).clone()
        if kind in ("tgp_sal2", "idtgp"):
            for prm in compile_flow(model.G_matrix[0])[1]:
                prm.data = prm.data + 0.3 * torch.randn((), dtype=F64, generator=g)
        if kind == "linear_mean":
            model.mean_function.a.data = 0.2 * torch.randn(1, D, 1, dtype=F64, generator=g)
            model.mean_function.b.data = torch.full((1, 1, 1), 0.4, dtype=F64)
    return model.to(DEV)


@pytest.mark.parametrize("kind", MODELS)
def test_model_posterior_paths(kind):
    from tgp.pytorch_amd import ops
    from tgp.pytorch_amd.flow import compile_flow, nets_rowp
    from tgp.pytorch_amd.pathwise import PosteriorPaths, spectral_frequencies
    kern = "scale_matern32" if kind == "tgp_sal2" else "scale_rbf"
    p = pm.make_case(MODEL_N, MODEL_D, MODEL_M, MODEL_R2, MODEL_S, kern)
    model = _build(kind, p)
    X = p["X"].to(DEV)
    paths = model.posterior_paths(MODEL_S, num_frequencies=MODEL_R2, generator=torch.Generator().manual_seed(23))
    assert isinstance(paths, PosteriorPaths) and paths.S == MODEL_S and paths.coef.shape == (2 * MODEL_R2 + MODEL_M, MODEL_S)
    f0, f = paths.f0(X), paths(X)
    assert f0.shape == f.shape == (MODEL_S, MODEL_N) and not f.requires_grad
    # the restatement on the numbers the generator gives, in the order draw_paths takes them
    g = torch.Generator().manual_seed(23)
    q = dict(p)
    q["omega"] = spectral_frequencies(kern, MODEL_R2, MODEL_D, g)
    q["W"] = torch.randn(MODEL_S, 2 * MODEL_R2, dtype=F64, generator=g)
    q["eps"] = torch.randn(MODEL_S, MODEL_M, dtype=F64, generator=g)
    assert torch.equal(paths.omega.cpu(), q["omega"])
    mean = torch.zeros(MODEL_N, dtype=F64)
    if kind == "linear_mean":
        a, b = model.mean_function.a.detach().cpu().reshape(-1), float(model.mean_function.b.detach())
        mean = p["X"] @ a + b
    if kind == "unwhitened":              # (m, L_q) describe q(u): the whitened pair is L^-1 m, L^-1 tril(L_q)
        L = torch.linalg.cholesky(pm.k_zz(p))
        q["m"] = torch.linalg.solve_triangular(L, p["m"].reshape(-1, 1), upper=False).reshape(-1)
        q["Lam"] = torch.linalg.solve_triangular(L, torch.tril(p["Lam"]), upper=False)
    ref = pm.evaluate(q, pm.coeff(q)) + mean.reshape(1, -1)
    err = float((f0.cpu() - ref).abs().max() / ref.abs().max())
    print(kind, "f0 against the restatement %.3g" % err)
    assert err <= TOL
    # paths(X) is G(f0) of the existing flow route, with the per-row parameters of an input-dependent flow
    spec, theta_list, nets = compile_flow(model.G_matrix[0])
    if spec.nblk == 0:
        assert torch.equal(f, f0)
    else:
        model.G_matrix[0].eval()
        theta = torch.stack([t.detach().reshape(()) for t in theta_list]) if theta_list else None
        rowp = nets_rowp(nets, X) if nets else None
        want = ops.flow_eval(f0, spec, theta, rowp, want=("G",))["G"]
        model.G_matrix[0].train()
        assert torch.equal(f, want) and not torch.equal(f, f0)
        with torch.no_grad():             # and what sample_from_variational_marginal does with G_matrix on repeated rows
            model.G_matrix[0].eval()
            assert torch.equal(f.reshape(-1), model.G_matrix[0](f0.reshape(-1), X.repeat(MODEL_S, 1)))
            model.G_matrix[0].train()
    # pieces, and the same function after the model has moved
    assert torch.equal(paths(X, batch_rows=77), f) and torch.equal(paths.f0(X, batch_rows=1000), f0)
    with torch.no_grad():
        for prm in model.parameters():
            prm.add_(0.37)
    assert torch.equal(paths(X), f) and torch.equal(paths.f0(X), f0)


def test_model_refusals():
    from tgp.pytorch_amd.kernels import instance_kernel
    from tgp.pytorch_amd.likelihoods import MulticlassCategorical
    from tgp.pytorch_amd.models import sparse_MF_GP
    X = torch.randn(20, 3, generator=torch.Generator().manual_seed(0), dtype=F64)
    K = instance_kernel("scale_rbf", ard_num_dim=3, num_multioutput=3, kernel_is_shared=False)
    model = sparse_MF_GP(["zero", K], X, X[:4].clone(), 20.0, MulticlassCategorical(3), 3, True, False, False, False, False, 0.0).to(DEV)
    with pytest.raises(NotImplementedError, match="multi-class"):
        model.posterior_paths(2)
    p = pm.make_case(MODEL_N, MODEL_D, MODEL_M, MODEL_R2, MODEL_S, "scale_rbf")
    model = _build("idtgp", p)
    model.be_fully_bayesian(True)
    with pytest.raises(NotImplementedError, match="be_fully_bayesian"):
        model.posterior_paths(2)


# ---- 6. refusals at the ABI ---------------------------------------------------------------------------------------
def test_abi_refusals_leave_the_outputs_untouched():
    from tgp.pytorch_amd import lib as L
    lib = L.load()
    case = pm.CASES[3]
    p, coef, _, _, _ = _case(case)
    U, WS = L.E_UNSUPPORTED, L.E_WORKSPACE

    def untouched_coeff(expect, **kw):
        c, st = abi_coeff(p, expect=expect, **kw)
        assert bool((c == SENTINEL).all()) and bool((st == -7).all()), kw
        if expect in (U, WS):
            assert b"tgp_pathwise_coeff_f64" in lib.tgp_last_error(), kw

    def untouched_eval(expect, **kw):
        F = abi_eval(p, coef, expect=expect, **kw)
        assert bool((F == SENTINEL).all()), kw
        if expect == U:
            assert b"tgp_pathwise_eval_f64" in lib.tgp_last_error(), kw

    for kw in (dict(D=0), dict(D=17), dict(M=0), dict(M=BIG_MAX_M + 1), dict(kernel=2), dict(kernel=-1)):
        untouched_coeff(U, **kw)
        untouched_eval(U, **kw)
    for kw in (dict(R2=0), dict(R2=L.PATHWISE_MAX_R2 + 1), dict(S=0), dict(S=L.PATHWISE_MAX_S + 1)):
        untouched_coeff(U, **kw)
        untouched_eval(U, **kw)
    untouched_eval(U, N=0)
    untouched_eval(U, N=-5)
    need = lib.tgp_pathwise_workspace_bytes(1, p["D"], p["M"], p["R2"], p["S"])
    untouched_coeff(WS, ws_bytes=need - 64)
    untouched_coeff(WS, ws_bytes=0)
    for name, code in (("omega", -2), ("W", -4), ("eps", -5), ("coef", -7), ("status", -8), ("workspace", -9)):
        if name in ("coef", "status"):
            abi_coeff(p, expect=code, null=(name,))
        else:
            untouched_coeff(code, null=(name,))
    for name, code in (("X", -2), ("Z", -5), ("raw_ls", -7), ("raw_os", -8), ("omega", -9), ("coef", -11)):
        untouched_eval(code, null=(name,))
    abi_eval(p, coef, expect=-13, null=("F0",))
    assert lib.tgp_pathwise_coeff_f64(None, None, 1, None, None, 1, None, None, None, 0, None) == -1
    # the sizer knows the same limits
    f = lib.tgp_pathwise_workspace_bytes
    assert f(1, 4, 40, 64, 5) > 0 and f(1, 4, 40, 64, 5) == f(250000, 4, 40, 64, 5) and (f(1, 4, 40, 64, 5) - 16) % 512 == 0
    for bad in ((0, 4, 40, 64, 5), (1, 0, 40, 64, 5), (1, 17, 40, 64, 5), (1, 4, 0, 64, 5), (1, 4, 4097, 64, 5), (1, 4, 40, 0, 5),
                (1, 4, 40, 8193, 5), (1, 4, 40, 64, 0), (1, 4, 40, 64, 257)):
        assert f(*bad) == 0, bad


def test_ops_refusals():
    from tgp.pytorch_amd import lib as L
    from tgp.pytorch_amd import ops
    p = _case(pm.CASES[3])[0]
    Z, rl, ro, m, Lam, om, W, eps, X = _dev(p, "Z", "raw_ls", "raw_os", "m", "Lam", "omega", "W", "eps", "X")
    with pytest.raises(L.TgpError, match=r"-101 .*tgp_pathwise_coeff_f64"):
        ops.pathwise_coeff(Z, rl, ro, m, Lam, om, W, eps, kernel=p["kernel"], workspace_bytes=1024)
    with pytest.raises(ValueError):
        ops.pathwise_coeff(Z, rl, ro, m, Lam, om, W[:, :-1], eps, kernel=p["kernel"])
    with pytest.raises(ValueError):
        ops.pathwise_eval(X, Z, rl, ro, om, torch.zeros(3, 2, dtype=F64, device=DEV), kernel=p["kernel"])
    torch.cuda.synchronize()
