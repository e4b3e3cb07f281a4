"""Linear and identity mean functions on the GPU: tgp_mean_forward_f64 / tgp_mean_backward_f64 against torch, the per-row AFFINE
block of the existing step kernels against the CPU oracle, and the model classes, the trainer and the captured engine against
the reference's fixtures (tools/gen_golden_mean.py)."""
import functools

import pytest
import torch

from conftest import load_golden, rel_err

from oracle import tgp_oracle as orc
import mean_model as mm
from test_mean_host import (CASES, REGRESSION, TOL_ADAM_HISTORY, TOL_ADAM_PARAMS, TOL_GRAD, TOL_VAL, build_model, tolerances)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F64 = torch.float64
SHAPES = ((1, 1), (63, 4), (64, 16), (65, 13), (257, 3), (4133, 4))
CANARY = -7.25


@pytest.fixture(scope="module", autouse=True)
def f64():
    from tgp.pytorch_amd import config as cg
    old = torch.get_default_dtype()
    cg.set_maximum_precission()
    cg.device = DEV
    yield
    torch.set_default_dtype(old)


def _inputs(N, D, seed=0):
    gen = torch.Generator().manual_seed(1000 * D + N + seed)
    return {"X": torch.randn(N, D, generator=gen, dtype=F64), "a": torch.randn(D, generator=gen, dtype=F64),
            "b": torch.randn(1, generator=gen, dtype=F64), "in": torch.randn(N, generator=gen, dtype=F64),
            "g": torch.randn(N, generator=gen, dtype=F64)}


# ---- the two kernels against torch ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,D", SHAPES)
@pytest.mark.parametrize("variant", ("plain", "rowp", "residual", "wide"))
def test_forward(N, D, variant):
    """|out - ref| <= 1e-14 (sum_d |x_d a_d| + |b| + |in|) per row; nothing outside the addressed columns is written."""
    from tgp.pytorch_amd import ops
    t = _inputs(N, D)
    X, a, b, inp = (t[k].to(DEV) for k in ("X", "a", "b", "in"))
    ld, col, one_col, alpha, use_in, use_b = {"plain": (1, 0, -1, 1.0, False, True), "rowp": (2, 1, 0, 1.0, False, True),
                                              "residual": (1, 0, -1, -1.0, True, True),
                                              "wide": (3, 2, -1, 0.5, True, False)}[variant]
    pad = 8
    buf = torch.full((N * ld + 2 * pad,), CANARY, dtype=F64, device=DEV)
    out = buf[pad:pad + N * ld].view((N, ld) if ld > 1 else (N,))
    res = ops.mean_forward(X, a, b if use_b else None, alpha=alpha, inp=inp if use_in else None, out=out, col=col, one_col=one_col)
    assert res.data_ptr() == out.data_ptr()
    got = buf.cpu()
    body = got[pad:pad + N * ld].view(N, ld)
    ref = alpha * ((t["X"] * t["a"]).sum(1) + (t["b"] if use_b else 0.0)) + (t["in"] if use_in else 0.0)
    bound = 1e-14 * ((t["X"] * t["a"]).abs().sum(1) + (t["b"].abs() if use_b else 0.0) + (t["in"].abs() if use_in else 0.0))
    err = (body[:, col] - ref).abs()
    print("forward %s N=%d D=%d: max err / bound %.3f" % (variant, N, D, float((err / bound).max())))
    assert bool((err <= bound).all())
    assert bool((got[:pad] == CANARY).all()) and bool((got[pad + N * ld:] == CANARY).all())
    for c in range(ld):
        if c == one_col:
            assert bool((body[:, c] == 1.0).all())
        elif c != col:
            assert bool((body[:, c] == CANARY).all())


@pytest.mark.parametrize("N,D", SHAPES)
def test_backward(N, D):
    """g_a = X^T g, g_b = sum g, g_X = g a^T with g read from column 1 of an (N, 2) buffer whose column 0 holds NaN:
    |err| <= 1e-13 sum_n |g_n x_nd|; two calls give the same bits; the doubles behind g_a keep their canary."""
    from tgp.pytorch_amd import lib as L
    t = _inputs(N, D)
    X, a = t["X"].to(DEV), t["a"].to(DEV)
    g2 = torch.stack((torch.full((N,), float("nan"), dtype=F64), t["g"]), 1).contiguous().to(DEV)
    lib = L.load()
    nbytes = lib.tgp_mean_backward_workspace_bytes(N, D)
    assert nbytes == ((N + 1023) // 1024) * 17 * 8

    def run():
        ga = torch.full((D + 8,), CANARY, dtype=F64, device=DEV)
        gb = torch.full((4,), CANARY, dtype=F64, device=DEV)
        gX = torch.full((N * D + 8,), CANARY, dtype=F64, device=DEV)
        ws = torch.full((nbytes // 8 + 8,), CANARY, dtype=F64, device=DEV)
        L.check(lib.tgp_mean_backward_f64(L.ptr(X), N, D, L.ptr(a), L.ptr(g2), 2, 1, L.ptr(ga), L.ptr(gb), L.ptr(gX), L.ptr(ws),
                                          nbytes, L.stream_ptr()), "tgp_mean_backward_f64")
        return ga.cpu(), gb.cpu(), gX.cpu(), ws.cpu()
    ga, gb, gX, ws = run()
    ref_a = t["X"].t() @ t["g"]
    bound_a = 1e-13 * (t["X"].abs() * t["g"].abs().reshape(-1, 1)).sum(0)
    assert bool(((ga[:D] - ref_a).abs() <= bound_a).all())
    assert float((gb[0] - t["g"].sum()).abs()) <= 1e-13 * float(t["g"].abs().sum())
    ref_X = t["g"].reshape(-1, 1) * t["a"].reshape(1, -1)
    assert bool(((gX[:N * D].view(N, D) - ref_X).abs() <= 1e-15 * ref_X.abs()).all())
    assert bool((ga[D:] == CANARY).all()) and bool((gb[1:] == CANARY).all()) and bool((gX[N * D:] == CANARY).all())
    assert bool((ws[nbytes // 8:] == CANARY).all())
    again = run()
    assert all(torch.equal(x, y) for x, y in zip((ga, gb, gX), again[:3]))
    # g_b and g_X skipped (identity mean): g_a unchanged bit for bit, a may be NULL
    ga3 = torch.full((D + 8,), CANARY, dtype=F64, device=DEV)
    w3 = torch.empty(nbytes // 8, dtype=F64, device=DEV)
    L.check(lib.tgp_mean_backward_f64(L.ptr(X), N, D, None, L.ptr(g2), 2, 1, L.ptr(ga3), None, None, L.ptr(w3), nbytes,
                                      L.stream_ptr()), "tgp_mean_backward_f64")
    assert torch.equal(ga3.cpu(), ga)


@pytest.mark.parametrize("N,D", ((65, 13), (1030, 4)))
def test_mean_function_autograd(N, D):
    """ops.MeanFunction against torch autograd: the (N, 2) row parameters, and the vector form alpha m(X) + in with X's gradient."""
    from tgp.pytorch_amd import ops
    t = _inputs(N, D, seed=3)
    w2 = torch.randn(N, 2, generator=torch.Generator().manual_seed(5), dtype=F64)
    leaves = [t[k].clone().requires_grad_(True) for k in ("X", "a", "b")]
    dl = [t[k].to(DEV).requires_grad_(True) for k in ("X", "a", "b")]
    (mm.mean_rowp(*leaves) * w2).sum().backward()
    rp = ops.MeanFunction.apply(dl[0], dl[1], dl[2], True, 1.0, None)
    assert tuple(rp.shape) == (N, 2) and bool((rp[:, 0] == 1.0).all())
    (rp * w2.to(DEV)).sum().backward()
    for k, x, y in zip("Xab", dl, leaves):
        assert rel_err(x.grad.cpu(), y.grad) < 1e-13, k
    for x in dl + leaves:
        x.grad = None
    (-(mm.mean(*leaves)) + t["in"]).mul(w2[:, 1]).sum().backward()
    vec = ops.MeanFunction.apply(dl[0], dl[1], dl[2], False, -1.0, t["in"].to(DEV))
    assert rel_err(vec.detach().cpu(), t["in"] - mm.mean(t["X"], t["a"], t["b"])) < 1e-13
    (vec * w2[:, 1].to(DEV)).sum().backward()
    for k, x, y in zip("Xab", dl, leaves):
        assert rel_err(x.grad.cpu(), y.grad) < 1e-13, k
    # identity mean: no offset, a without gradient
    W = t["a"].to(DEV)
    out = ops.MeanFunction.apply(dl[0], W, None, False, 1.0, None)
    assert rel_err(out.detach().cpu(), t["X"] @ t["a"]) < 1e-13


# ---- the per-row AFFINE block of the existing step kernels against the CPU oracle -------------------------------------------
@functools.lru_cache(maxsize=None)
def oracle_step(name):
    """The CPU oracle's ELBO and gradients of fixture `name` with the per-row block (1, m(x_n)) at the head of the program and
    rowp as a leaf.  Computed once, shared, never written to."""
    g = load_golden(name)
    a, b = mm.mean_params(g)
    rowp = mm.mean_rowp(g["X"], a, b)
    prog = mm.mean_program(g["program"])
    if int(g["bernoulli"]):
        leaves = {k: v.clone().requires_grad_(True) for k, v in g["params"].items()}
        rp = rowp.clone().requires_grad_(True)
        mu, v = orc.qf_moments(g["X"], leaves["Z"], leaves["raw_lengthscale"], leaves["raw_outputscale"], leaves["m"], leaves["Lam"])
        ell = float(g["N_total"]) / g["X"].shape[0] * mm.ell_bernoulli(g["Y"].reshape(-1), mu, v, prog, leaves["theta"], g["xs"],
                                                                          g["ws"], rp)
        kl = orc.kld_whitened(leaves["m"], leaves["Lam"])
        (ell - kl).backward()
        grads = {k: v.grad for k, v in leaves.items()}
        grads["rowp"] = rp.grad
        out = ((ell - kl).detach(), ell.detach(), kl.detach())
    else:
        out, grads = orc.elbo_and_grads(g["X"], g["Y"], g["params"], float(g["N_total"]), prog, g["xs"], g["ws"], rowp,
                                        kernel=g["kernel"])
    return g, rowp, prog, out, grads


def gpu_step(name, plan=0):
    from tgp.pytorch_amd import lib as L
    from tgp.pytorch_amd import ops
    g, rowp, prog, _, _ = oracle_step(name)
    p = {k: v.to(DEV) for k, v in g["params"].items()}
    bern = bool(int(g["bernoulli"]))
    lvn = torch.zeros(1, dtype=F64, device=DEV) if bern else p["log_var_noise"]
    flow = ops.FlowSpec(prog, p["theta"].numel() if "theta" in p else 0, 2, DEV)
    out, gr, status, _ = ops.elbo_step(g["X"].to(DEV), g["Y"].to(DEV), p["Z"], p["raw_lengthscale"], p["raw_outputscale"], p["m"],
                                       p["Lam"], lvn, float(g["N_total"]), flow=flow, theta=p.get("theta"), rowp=rowp.to(DEV),
                                       S=g["xs"].numel(), kernel=g["kernel"], plan=plan, lik=L.LIK_BERNOULLI if bern else None)
    torch.cuda.synchronize()
    assert int(status[0]) == 0 and int(status[1]) == 0
    return out, gr


STEP_KEYS = (("Z", "Z"), ("raw_ls", "raw_lengthscale"), ("raw_os", "raw_outputscale"), ("m", "m"), ("Lam", "Lam"),
             ("lvn", "log_var_noise"), ("theta", "theta"))
#             fixture              plan              what it reaches
AFFINE_CASES = (("mean_tiny_svgp_lin", "PLAN_ROWS_AUTO"),     # the block alone under TGP_LIK_FLOW: the engine's Gaussian route
                ("mean_tiny_sal1_lin", "PLAN_ROWS_AUTO"),     # k_rows, 16 rows per wave
                ("mean_tiny_sal1_lin", "PLAN_ROWS_K16"),
                ("mean_tiny_sal1_lin", "PLAN_ROWS4_NW4"),     # k_rows4 forced by the plan
                ("mean_med_sal2_lin", "PLAN_ROWS_AUTO"),      # MT = 7, three row blocks with a tail
                ("mean_edge128_tanh_id", "PLAN_ROWS_AUTO"),   # M = 128, D = 13
                ("mean_bigm_matern_lin", "PLAN_ROWS_AUTO"),   # general-M path, k_ell_quad
                ("mean_bern_tiny_lin", "PLAN_ROWS_AUTO"))     # k_ell_quad<EllBern>


@pytest.mark.parametrize("name,plan", AFFINE_CASES)
def test_per_row_affine_block(name, plan):
    """The step with (a_n, b_n) = (1, b_n) per row: every output and g_rowp[:, 1] = dELBO/db_n against the CPU oracle."""
    from tgp.pytorch_amd import lib as L
    g, rowp, prog, ref, og = oracle_step(name)
    out, gr = gpu_step(name, getattr(L, plan))
    e = [rel_err(out[i].cpu(), ref[i]) for i in range(3)]
    print("%s %s: ELBO %.2e  ELL %.2e  KL %.2e" % ((name, plan) + tuple(e)))
    assert max(e) < TOL_VAL
    for k_hip, k_or in STEP_KEYS:
        if k_or in og and k_hip in gr:
            e = rel_err(gr[k_hip].cpu(), og[k_or])
            print("%s %s: d/d%s %.2e" % (name, plan, k_or, e))
            assert e < TOL_GRAD, k_or
    e = rel_err(gr["rowp"][:, 1].cpu(), og["rowp"][:, 1])
    print("%s %s: g_rowp[:, 1] %.2e" % (name, plan, e))
    assert e < TOL_GRAD
    assert bool(torch.isfinite(gr["rowp"][:, 0]).all())


def test_plans_agree_on_the_mean_gradient():
    """mean_tiny_sal1_lin under the three row-kernel plans: a_bar, b_bar from g_rowp[:, 1] through tgp_mean_backward_f64 agree
    with the reference's and with each other."""
    from tgp.pytorch_amd import lib as L
    from tgp.pytorch_amd import ops
    g = load_golden("mean_tiny_sal1_lin")
    X = g["X"].to(DEV)
    res = []
    for plan in (L.PLAN_ROWS_AUTO, L.PLAN_ROWS4_NW4, L.PLAN_ROWS_K16):
        out, gr = gpu_step("mean_tiny_sal1_lin", plan)
        g_a, g_b, _ = ops.mean_backward(X, gr["rowp"], col=1)
        res.append((out[0].cpu(), g_a.cpu(), g_b.cpu()))
        assert rel_err(res[-1][0], g["ELBO"]) < TOL_VAL
        assert rel_err(res[-1][1], g["g_mean_a"]) < TOL_GRAD and rel_err(res[-1][2], g["g_mean_b"]) < TOL_GRAD
    for r in res[1:]:
        assert rel_err(r[0], res[0][0]) < TOL_VAL and rel_err(r[1], res[0][1]) < TOL_GRAD and rel_err(r[2], res[0][2]) < TOL_GRAD


# ---- the model classes against the reference ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_model_matches_reference(name):
    from tgp.pytorch_amd.flow import compile_flow
    g = load_golden(name)
    tol_v, tol_g = tolerances(name)
    model = build_model(g, name, DEV)
    model.set_is_training(True)
    X, Y = g["X"].to(DEV), g["Y"].to(DEV)
    with torch.no_grad():
        mu, v = model.marginal_variational_qf_parameters(X, diagonal=True, is_duvenaud=False)
        kld0 = model.KLD()
    e = (rel_err(mu.cpu(), g["mu"]), rel_err(v.cpu(), g["v"]), rel_err(kld0.cpu(), g["KLD"]))
    print("%s: mu %.2e  v %.2e  KLD %.2e (tol %.1e)" % ((name,) + e + (tol_v,)))
    assert max(e) < tol_v
    elbo, ell, kld = model.ELBO(X, Y)
    (-elbo).backward()
    e = (rel_err(elbo.detach().cpu(), g["ELBO"]), rel_err(ell.detach().cpu(), g["ELL"]), rel_err(kld.detach().cpu(), g["KLD"]))
    print("%s: ELBO %.2e  ELL %.2e  KLD %.2e (tol %.1e)" % ((name,) + e + (tol_v,)))
    assert max(e) < tol_v
    k = model.covariance_function
    got = {"g_Z": model.Z.grad[0], "g_m": model.q_U.variational_mean.grad[0], "g_Lam": model.q_U.chol_variational_covar.grad[0],
           "g_raw_outputscale": k.raw_outputscale.grad, "g_raw_lengthscale": k.base_kernel.raw_lengthscale.grad.reshape(-1)}
    if "g_log_var_noise" in g:
        got["g_log_var_noise"] = model.likelihood.log_var_noise.grad.reshape(-1)
    if "g_theta" in g:
        got["g_theta"] = torch.stack([q.grad.reshape(()) for q in compile_flow(model.G_matrix[0])[1]])
    if "g_mean_a" in g:
        got["g_mean_a"] = model.mean_function.a.grad.reshape(-1)
        got["g_mean_b"] = model.mean_function.b.grad.reshape(-1)
    else:
        assert not list(model.mean_function.parameters())
    for gk in sorted(got):
        e = rel_err(-got[gk].cpu(), g[gk])
        print("%s: %s %.2e (tol %.1e)" % (name, gk, e, tol_g))
        assert e < tol_g, gk
    assert all(q.grad is not None for q in model.parameters())


@pytest.mark.parametrize("name", REGRESSION)
def test_prediction_matches_reference(name):
    """mu, v, m1, m2 and the test log-likelihood on the 16 held-out rows; every method downstream of (mu, v) sees the mean once."""
    g = load_golden(name)
    tol_v, _ = tolerances(name)
    model = build_model(g, name, DEV)
    model.set_is_training(False)
    X, Y = g["X_te"].to(DEV), g["Y_te"].to(DEV)
    logp, (m1, m2) = model.test_log_likelihood(X, Y, return_moments=True, Y_std=g["Y_std"].to(DEV), S_MC_NNet=None)
    p1, p2, mu, v = model.predictive_distribution(X)
    e = (rel_err(mu.cpu(), g["mu_te"]), rel_err(v.cpu(), g["v_te"]), rel_err(m1.cpu(), g["pred_m1"]), rel_err(m2.cpu(), g["pred_m2"]),
         rel_err(logp.cpu(), g["test_logp_sum"]))
    print("%s: mu %.2e  v %.2e  m1 %.2e  m2 %.2e  logp %.2e (tol %.1e)" % ((name,) + e + (tol_v,)))
    assert max(e) < tol_v
    assert torch.equal(p1, m1) and torch.equal(p2, m2)
    mu = mu.reshape(-1)
    # the full covariance's mean, the sampling path's moments and the quantile inputs: the same mu, the mean in it once
    with torch.no_grad():
        mu_f, Sig = model.marginal_variational_qf_parameters(X, diagonal=False, is_duvenaud=False)
    # (another kernel, tgp_qf_cov_f64: held to the reference like the first, not to the first's bits)
    assert rel_err(mu_f.reshape(-1).cpu(), g["mu_te"]) < tol_v and rel_err(Sig[0].diagonal().cpu(), g["v_te"]) < tol_v
    _, mean_s, _ = model.sample_from_variational_marginal_base(X, diagonal=True, is_duvenaud=False)
    assert torch.equal(mean_s.reshape(-1), mu)
    qi = model._quantile_inputs(X, "test")
    assert torch.equal(qi[0], mu)
    samples, _, _ = model.sample_from_predictive_distribution(X, S=3)
    assert tuple(samples.shape) == (1, 3, X.shape[0], 1) and bool(torch.isfinite(samples).all())
    cdf = model.predictive_cdf(X, Y)
    assert tuple(cdf.shape) == (1, X.shape[0]) and bool(((cdf >= 0) & (cdf <= 1)).all())
    if g["program"] is None:
        # Gaussian likelihood: the median of the predictive and of the posterior is mu, with m(X) included
        q = model.predictive_quantiles(X, [0.5])
        assert float((q.reshape(-1) - mu).abs().max()) <= 1e-12 * max(1.0, float(mu.abs().max()))
        q = model.posterior_quantiles(X, [0.5])
        assert float((q.reshape(-1) - mu).abs().max()) <= 1e-12 * max(1.0, float(mu.abs().max()))
        assert float((model.predictive_cdf(X, mu.reshape(-1, 1)) - 0.5).abs().max()) < 1e-12


def test_bernoulli_prediction_sees_the_mean():
    from test_bernoulli_host import pred_torch
    g = load_golden("mean_bern_tiny_lin")
    model = build_model(g, "mean_bern_tiny_lin", DEV)
    model.set_is_training(False)
    P, _, mu, v = model.predictive_distribution(g["X"].to(DEV))
    assert rel_err(mu.cpu(), g["mu"]) < TOL_VAL
    ref = pred_torch(g["mu"], g["v"], g["program"], g["params"]["theta"], g["xs"], g["ws"])
    assert rel_err(P.reshape(-1).cpu(), ref) < TOL_VAL


# ---- training ---------------------------------------------------------------------------------------------------------
def _final(model):
    from tgp.pytorch_amd.flow import compile_flow
    k = model.covariance_function
    return {"final_Z": model.Z.detach()[0], "final_m": model.q_U.variational_mean.detach()[0],
            "final_Lam": torch.tril(model.q_U.chol_variational_covar.detach()[0]),
            "final_theta": torch.stack([q.detach().reshape(()) for q in compile_flow(model.G_matrix[0])[1]]),
            "final_mean_a": model.mean_function.a.detach().reshape(-1), "final_mean_b": model.mean_function.b.detach().reshape(-1),
            "final_raw_lengthscale": k.base_kernel.raw_lengthscale.detach().reshape(-1),
            "final_raw_outputscale": k.raw_outputscale.detach().reshape(-1),
            "final_log_var_noise": model.likelihood.log_var_noise.detach().reshape(-1)}


@pytest.mark.parametrize("path", ("eager", "engine"))
def test_trainer_first_steps_match_reference(path):
    """mean_adam5_sal2_lin: five Adam steps of the eager loop and of the captured ElboEngine against the reference's history and
    final parameters (tests/mean_model.py under torch.optim.Adam is 5e-14 / 5e-12 from them: the project's 1e-9 / 1e-8 hold)."""
    from tgp.pytorch_amd import config as cg
    from tgp.pytorch_amd.data import DeviceLoader
    from tgp.pytorch_amd.trainers import Trainer_SP_regression
    g = load_golden("mean_adam5_sal2_lin")
    model = build_model(g, "mean_adam5_sal2_lin", DEV)
    loader = DeviceLoader(g["X"], g["Y"], 10000, shuffle=False, device=DEV)
    tr = Trainer_SP_regression(model, [loader, None, None], 1e20, False, False, torch.ones(1, device=DEV), -1, 100, False)
    old = getattr(cg, "use_step_engine", True)
    cg.use_step_engine = path == "engine"
    try:
        tr.train(epochs=g["history"].shape[0], lr_ALL=0.01, opt="adam", keep_parameter_groups=True)
    finally:
        cg.use_step_engine = old
    assert (tr._engine is not None) == (path == "engine")
    if path == "engine":
        assert tr._engine.mean == "linear" and not tr._engine.fused_adam and tr._engine.graph == "full"
    hist = torch.tensor([[-l, e, k] for l, e, k in zip(tr.loss_arr, tr.ELL_arr, tr.KLD_arr)], dtype=F64)
    e_h = rel_err(hist, g["history"])
    fin = _final(model)
    errs = {k: rel_err(fin[k].cpu(), torch.tril(g[k]) if k == "final_Lam" else g[k]) for k in fin}
    print("mean_adam5_sal2_lin %s: history %.2e  %s" % (path, e_h, "  ".join("%s %.2e" % (k[6:], e) for k, e in errs.items())))
    assert e_h < TOL_ADAM_HISTORY
    assert max(errs.values()) < TOL_ADAM_PARAMS


@pytest.mark.parametrize("name", ("mean_tiny_svgp_lin", "mean_edge128_tanh_id"))
def test_engine_step_matches_model(name):
    """One captured-engine step at lr = 0 against the fixture: the Gaussian likelihood through the affine block under
    quadrature (the eager model's closed form, to rounding), and the identity mean whose row parameters are written once."""
    from tgp.pytorch_amd.engine import ElboEngine
    g = load_golden(name)
    a, b = mm.mean_params(g)
    eng = ElboEngine(g["X"], g["Y"], g["params"], float(g["N_total"]), flow_blocks=g["program"], S=g["xs"].numel(), lr=0.0,
                     device=DEV, kernel=g["kernel"], mean=("identity", a, None) if b is None else ("linear", a, b))
    eng.capture()
    eng.replay()
    torch.cuda.synchronize()
    eng.check_status()
    out = eng.fp.out.cpu()
    e = (rel_err(out[0], g["ELBO"]), rel_err(out[1], g["ELL"]), rel_err(out[2], g["KLD"]))
    print("%s engine: ELBO %.2e  ELL %.2e  KLD %.2e" % ((name,) + e))
    assert max(e) < TOL_VAL
    for k, gk in (("Z", "g_Z"), ("m", "g_m"), ("raw_ls", "g_raw_lengthscale"), ("raw_os", "g_raw_outputscale"), ("lvn", "g_log_var_noise"),
                  ("mean_a", "g_mean_a"), ("mean_b", "g_mean_b")):
        if gk in g:
            assert rel_err(eng.fp.gview(k).cpu(), g[gk]) < TOL_GRAD, k
    assert ("mean_a" in eng.fp.offsets) == (b is not None)
