"""GPU (-m gpu): the posterior derivative in HIP -- the slope variance under q(f) (tgp_qf_input_grad_var_f64, csrc/tgp_xgrad.hip) and
the input gradients of pathwise draws (tgp_pathwise_grad_f64, k_pw_grad of csrc/tgp_pathwise.hip) -- through the C ABI, ops, the
models, PosteriorPaths and the CLI.

The yardstick is the float64 restatement of tests/derivative_model.py (held to torch autograd on the CPU,
tests/test_derivative_host.py), an existing kernel (the zero-noise draws against tgp_qf_input_grad_f64) or a central difference
of the draws themselves.  Tolerances: the project's TOL_GRAD = 1e-7 for derivative quantities and TOL_VAL = 1e-9 for values,
through conftest.rel_err, as in tests/test_gpu_input_grad.py."""
import functools
import math
import re
import subprocess
import sys

import pytest
import torch

from conftest import REPO, rel_err
from oracle import tgp_oracle as orc

import derivative_model as DM
import pathwise_model as pm

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F64 = torch.float64
TOL_VAL = 1e-9
TOL_GRAD = 1e-7
TOL_FD = 1e-6        # a central difference with h = 1e-5 in float64: h^2 |f'''| / 6 + eps |f| / h, about 2e-11 + 1e-10 at |f'''| ~ 1
KEYS = ("Z", "raw_lengthscale", "raw_outputscale", "m", "Lam")
RQ_ALPHA = 2.0
SENTINEL = -7.0


@pytest.fixture(scope="module", autouse=True)
def f64():
    from tgp.pytorch_amd import config as cg
    old = torch.get_default_dtype()
    cg.set_maximum_precission()
    cg.device = DEV
    yield
    torch.set_default_dtype(old)


def _dev(p, kernel="scale_rbf"):
    from tgp.pytorch_amd import ops
    t = [p[k].to(DEV) for k in KEYS]
    if kernel == "scale_rq":
        t[2] = ops.rq_scale(t[2], RQ_ALPHA)
    return tuple(t)


# ---- dvar: tile edges against the restatement ---------------------------------------------------------------------
EDGE_N = (1, 63, 65, 130)
EDGE_MD = ((5, 1), (100, 4), (150, 13), (130, 16))     # M < 16, D = 1; M < 128; M > 128, odd D; M = 128 + 2, D = 16
SAME_ROW = (40, 3)                                      # row 40 of X is row 3 of Z bit for bit


@functools.lru_cache(maxsize=None)
def _edge(M, D, kernel):
    """One problem of 130 rows per (M, D, kernel), restated once on the CPU: a row's slope variance depends on that row only, so
    the first N rows of the reference serve every N."""
    prob = orc.synthetic_problem(300, D, M, seed=7, flow=None, S=8)
    p, X = prob["params"], prob["X"][:130].clone()
    if D == 1:      # five points on a line: length-scale 0.7 keeps cond(K_ZZ) where the reference itself is good
        p["raw_lengthscale"] = orc.inv_softplus(torch.full((1,), 0.7, dtype=F64))
    X[SAME_ROW[0]] = p["Z"][SAME_ROW[1]]
    alpha = RQ_ALPHA if kernel == "scale_rq" else None
    return X, p, DM.slope_var(X, *(p[k] for k in KEYS), kernel=kernel, alpha=alpha)


def _check_edge(N, M, D, kernel):
    from tgp.pytorch_amd import ops
    X, p, ref = _edge(M, D, kernel)
    Xd = X[:N].contiguous().to(DEV)
    dvar = ops.qf_input_grad_var(Xd, *_dev(p, kernel), kernel=kernel)
    assert dvar.shape == (N, D) and dvar.is_contiguous() and bool(torch.isfinite(dvar).all())
    e = rel_err(dvar.cpu(), ref[:N])
    print("dvar N=%d M=%d D=%d %s: %.3e (tol %.1e)" % (N, M, D, kernel, e, TOL_GRAD))
    assert e <= TOL_GRAD
    if N > SAME_ROW[0]:        # the row that coincides with an inducing point, on its own scale
        assert rel_err(dvar[SAME_ROW[0]].cpu(), ref[SAME_ROW[0]]) <= TOL_GRAD
    assert torch.equal(dvar, ops.qf_input_grad_var(Xd, *_dev(p, kernel), kernel=kernel))


@pytest.mark.parametrize("kernel", ("scale_rbf", "scale_matern32"))
@pytest.mark.parametrize("M,D", EDGE_MD)
@pytest.mark.parametrize("N", EDGE_N)
def test_dvar_tile_edges(N, M, D, kernel):
    _check_edge(N, M, D, kernel)


@pytest.mark.parametrize("kernel", ("scale_matern52", "scale_rq"))
@pytest.mark.parametrize("N", EDGE_N)
def test_dvar_other_kernels(N, kernel):
    _check_edge(N, 100, 4, kernel)


def test_dvar_pass_boundary():
    """N = TGP_XGRAD_PASS_ROWS + 1: two passes, the second of one row, whose result is the bits of a call on that row alone."""
    from tgp.pytorch_amd import lib as L
    from tgp.pytorch_amd import ops
    R = L.XGRAD_PASS_ROWS
    prob = orc.synthetic_problem(R + 1, 1, 5, seed=11, flow=None, S=8)
    p, X = prob["params"], prob["X"]
    p["raw_lengthscale"] = orc.inv_softplus(torch.full((1,), 0.7, dtype=F64))
    ref = DM.slope_var(X, *(p[k] for k in KEYS))
    Xd = X.to(DEV)
    dvar = ops.qf_input_grad_var(Xd, *_dev(p))
    assert bool(torch.isfinite(dvar).all())
    e = rel_err(dvar.cpu(), ref)
    print("dvar pass boundary: %.3e" % e)
    assert e <= TOL_GRAD
    for r in (R - 1, R):
        assert rel_err(dvar[r].cpu(), ref[r]) <= TOL_GRAD, r
    assert torch.equal(ops.qf_input_grad_var(Xd[R:].contiguous(), *_dev(p))[0], dvar[R])
    assert torch.equal(ops.qf_input_grad_var(Xd, *_dev(p)), dvar)


def test_dvar_of_the_prior_is_the_priors():
    """tril(Lam) = I: W = 0 exactly, the slope variance is k_g(0) / l_d^2 in every row."""
    from tgp.pytorch_amd import ops
    X, p, _ = _edge(100, 4, "scale_matern32")
    q = dict(p, Lam=torch.eye(100, dtype=F64))
    dvar = ops.qf_input_grad_var(X.to(DEV), *_dev(q, "scale_matern32"), kernel="scale_matern32").cpu()
    prior = DM.prior_slope_var(p["raw_lengthscale"], p["raw_outputscale"], "scale_matern32")
    assert rel_err(dvar, prior.reshape(1, -1).expand(130, 4)) <= TOL_VAL and bool((dvar == dvar[0:1]).all())


# ---- posterior_derivative on models ---------------------------------------------------------------------------------
@pytest.mark.parametrize("mean", ("zero", "linear"))
@pytest.mark.parametrize("whiten", (True, False), ids=("whitened", "unwhitened"))
@pytest.mark.parametrize("flow", (None, "sal2"), ids=("svgp", "tgp-sal2"))
def test_posterior_derivative(flow, whiten, mean):
    from test_gpu_input_grad import _build, _problem
    prob, white = _problem(flow, whiten, mean)
    model = _build(prob, flow, whiten, mean)
    model.set_is_training(False)
    Xd = prob["X"].to(DEV)
    mean_d, var_d = model.posterior_derivative(Xd)
    N, D = prob["X"].shape
    assert mean_d.shape == (1, N, D) and var_d.shape == (1, N, D) and model.training and not var_d.requires_grad
    assert torch.equal(mean_d, model.posterior_input_gradients(Xd)[0])
    ref = DM.slope_var(prob["X"], *white)
    e = rel_err(var_d[0].cpu(), ref)
    print("posterior_derivative %s whiten=%s mean=%s: var %.2e" % (flow, whiten, mean, e))
    assert e <= TOL_GRAD
    from tgp.pytorch_amd.utils import slope_significance
    sig = slope_significance(model, Xd, batch_rows=16).cpu()                     # in pieces: 16 x 4 + 1 rows
    want = (mean_d[0].abs() > 1.96 * torch.sqrt(var_d[0].clamp_min(0.0))).to(F64).mean(0).cpu()
    assert sig.shape == (D,) and torch.equal(sig, want) and bool(((sig >= 0) & (sig <= 1)).all())


def test_posterior_derivative_of_a_heteroscedastic_model():
    from test_gpu_hetero import _build_model, _set_gp_params
    N, D, M = 65, 4, 20
    pa = orc.synthetic_problem(N, D, M, 5, None, 20)
    pb = orc.synthetic_problem(N, D, M, 6, None, 20)
    pf = {k: pa["params"][k].clone() for k in KEYS}
    ph = {k: pb["params"][k].clone() for k in KEYS}
    model = _build_model(pa["X"], M, "sal2", S=20)
    _set_gp_params(model, pf, ph)
    model.set_is_training(False)
    Xd = pa["X"].to(DEV)
    mean_d, var_d = model.posterior_derivative(Xd)
    assert mean_d.shape == (2, N, D) and var_d.shape == (2, N, D)
    assert torch.equal(mean_d, model.posterior_input_gradients(Xd)[0])
    for c, p in enumerate((pf, ph)):
        e = rel_err(var_d[c].cpu(), DM.slope_var(pa["X"], *(p[k] for k in KEYS)))
        print("hetero GP %d: var %.2e" % (c, e))
        assert e <= TOL_GRAD


# ---- tgp_pathwise_grad_f64 against the restatement ------------------------------------------------------------------
GRAD_CASES = [
    (1, 1, 1, 1, 1, "scale_rbf"),
    (63, 4, 65, 130, 64, "scale_rbf"),
    (65, 13, 129, 15, 65, "scale_rbf"),
    (65, 16, 200, 64, 100, "scale_matern32"),
    (257, 8, 129, 15, 100, "scale_matern32"),
    (1000, 1, 1, 15, 100, "scale_rbf"),
    (16450, 4, 16, 15, 3, "scale_rbf"),
    (16450, 16, 16, 15, 17, "scale_matern32"),
]
ids = lambda c: "%d-%d-%d-%d-%d-%s" % c          # noqa: E731


def _pdev(p, *names):
    return [p[n].to(DEV).contiguous() for n in names]


def abi_grad(p, coef, X=None, expect=0, null=(), **over):
    """One call of tgp_pathwise_grad_f64: dF0 (D, S, N) on the host, sentinels where nothing was written."""
    from tgp.pytorch_amd import lib as L
    lib = L.load()
    X = (p["X"] if X is None else X).to(DEV).contiguous()
    Z, rl, ro, om = _pdev(p, "Z", "raw_ls", "raw_os", "omega")
    coef = coef.to(DEV).contiguous()
    a = dict(kernel=L.KERNELS[p["kernel"]], N=X.shape[0], D=p["D"], M=p["M"], R2=p["R2"], S=p["S"])
    a.update(over)
    G = torch.full((p["D"], p["S"], X.shape[0]), SENTINEL, dtype=F64, device=DEV)
    arg = dict(X=L.ptr(X), Z=L.ptr(Z), raw_ls=L.ptr(rl), raw_os=L.ptr(ro), omega=L.ptr(om), coef=L.ptr(coef), dF0=L.ptr(G))
    for n in null:
        arg[n] = None
    rc = lib.tgp_pathwise_grad_f64(a["kernel"], arg["X"], a["N"], a["D"], arg["Z"], a["M"], arg["raw_ls"], arg["raw_os"],
                                   arg["omega"], a["R2"], arg["coef"], a["S"], arg["dF0"], L.stream_ptr())
    assert rc == expect, (rc, lib.tgp_last_error())
    torch.cuda.synchronize()
    return G.cpu()


@functools.lru_cache(maxsize=None)
def _case(case):
    """(inputs, the restatement's coef, the device's dF0 (D, S, N) from it): once per case."""
    p = pm.make_case(*case)
    coef = pm.coeff(p)
    return p, coef, abi_grad(p, coef)


@pytest.mark.parametrize("case", GRAD_CASES, ids=ids)
def test_draw_gradient_against_the_restatement(case):
    p, coef, G = _case(case)
    ref = DM.draw_grad(p, coef)                                       # (S, N, D)
    assert G.shape == (p["D"], p["S"], p["N"]) and bool(torch.isfinite(G).all())
    e = rel_err(G.permute(1, 2, 0), ref)
    worst_d = max(rel_err(G[d], ref[:, :, d]) for d in range(p["D"]))  # each input on its own scale
    print(case, "dF0 %.3e, worst single input %.3e (tol %.1e)" % (e, worst_d, TOL_GRAD))
    assert e <= TOL_GRAD and worst_d <= TOL_GRAD
    assert torch.equal(abi_grad(p, coef), G)


# ---- bit identities ---------------------------------------------------------------------------------------------------
def test_pieces_give_the_same_bits_and_ops_the_abis():
    from tgp.pytorch_amd import ops
    p, coef, G = _case(GRAD_CASES[4])                                 # N = 257
    X, Z, rl, ro, om = _pdev(p, "X", "Z", "raw_ls", "raw_os", "omega")
    cd = coef.to(DEV)
    whole = ops.pathwise_grad(X, Z, rl, ro, om, cd, kernel=p["kernel"])
    assert whole.shape == (p["S"], 257, p["D"]) and torch.equal(whole.cpu(), G.permute(1, 2, 0))
    pieces = ops.pathwise_grad(X, Z, rl, ro, om, cd, kernel=p["kernel"], batch_rows=100)
    assert pieces.shape == whole.shape and torch.equal(pieces, whole)
    one = ops.pathwise_grad(X[200:201].contiguous(), Z, rl, ro, om, cd, kernel=p["kernel"])
    assert torch.equal(one[:, 0], whole[:, 200])


@pytest.mark.parametrize("case", GRAD_CASES[6:], ids=ids)
def test_both_row_tilings_give_the_same_bits(case):
    """N = 16 450 runs the 64-row workgroups, a call on its first 64 rows the 16-row ones."""
    p, coef, G = _case(case)
    assert p["N"] == 16450
    assert torch.equal(abi_grad(p, coef, X=p["X"][:64]), G[:, :, :64])


# ---- against an existing kernel -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [GRAD_CASES[1], GRAD_CASES[3]], ids=ids)
def test_zero_noise_draws_have_the_posterior_means_gradient(case):
    """W = 0 and eps = 0: the draw is the posterior mean, its gradient tgp_qf_input_grad_f64's dmu on the same rows."""
    from tgp.pytorch_amd import ops
    p = _case(case)[0]
    X, Z, rl, ro, m, Lam, om = _pdev(p, "X", "Z", "raw_ls", "raw_os", "m", "Lam", "omega")
    coef = ops.pathwise_coeff(Z, rl, ro, m, Lam, om, torch.zeros_like(p["W"]).to(DEV), torch.zeros_like(p["eps"]).to(DEV),
                              kernel=p["kernel"])
    g = ops.pathwise_grad(X, Z, rl, ro, om, coef, kernel=p["kernel"])
    dmu, _ = ops.qf_input_grad(X, Z, rl, ro, m, Lam, kernel=p["kernel"])
    e = max(rel_err(g[s].cpu(), dmu.cpu()) for s in range(p["S"]))
    print(case, "zero-noise gradient against dmu %.3e" % e)
    assert e <= TOL_GRAD


# ---- PosteriorPaths --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flow,mean", (("sal2", "zero"), ("tanh3x2", "zero"), ("sal2", "linear")))
def test_paths_grad_is_the_slope_of_the_paths(flow, mean):
    from test_gpu_input_grad import _build, _problem
    prob, _ = _problem(flow, True, mean)
    model = _build(prob, flow, True, mean)
    paths = model.posterior_paths(3, num_frequencies=32, generator=torch.Generator().manual_seed(29))
    X = prob["X"].to(DEV)
    N, D = X.shape
    g = paths.grad(X)
    g0 = paths.grad_f0(X)
    assert g.shape == (3, N, D) and g0.shape == (3, N, D) and not torch.equal(g, g0)
    assert torch.equal(paths.grad(X, batch_rows=16), g) and torch.equal(paths.grad_f0(X, batch_rows=16), g0)
    h = 1e-5
    worst = 0.0
    for fn, got, name in ((paths, g, "grad"), (paths.f0, g0, "grad_f0")):
        fd = torch.empty_like(got)
        for d in range(D):
            Xp, Xm = X.clone(), X.clone()
            Xp[:, d] += h
            Xm[:, d] -= h
            fd[:, :, d] = (fn(Xp) - fn(Xm)) / (Xp[:, d] - Xm[:, d]).reshape(1, -1)
        e = rel_err(got.cpu(), fd.cpu())
        print("paths.%s %s mean=%s against the central difference: %.3e (bound %.0e)" % (name, flow, mean, e, TOL_FD))
        worst = max(worst, e)
    assert worst <= TOL_FD


# ---- refusals at the ABI -------------------------------------------------------------------------------------------------
def test_abi_refusals_leave_the_outputs_untouched():
    from tgp.pytorch_amd import lib as L
    from tgp.pytorch_amd import ops
    lib = L.load()
    p, coef, _ = _case(GRAD_CASES[1])
    U = L.E_UNSUPPORTED

    def untouched(expect, **kw):
        G = abi_grad(p, coef, expect=expect, **kw)
        assert bool((G == SENTINEL).all()), kw
        if expect == U:
            assert lib.tgp_last_error().startswith(b"tgp_pathwise_grad_f64"), kw
    for kw in (dict(D=0), dict(D=17), dict(M=0), dict(M=L.BIG_MAX_M + 1), dict(kernel=2), dict(kernel=-1), dict(R2=0),
               dict(R2=L.PATHWISE_MAX_R2 + 1), dict(S=0), dict(S=L.PATHWISE_MAX_S + 1), dict(N=0), dict(N=-5)):
        untouched(U, **kw)
    for name, code in (("X", -2), ("Z", -5), ("raw_ls", -7), ("raw_os", -8), ("omega", -9), ("coef", -11)):
        untouched(code, null=(name,))
    abi_grad(p, coef, expect=-13, null=("dF0",))
    # the slope variance: a short workspace leaves dvar and the status as they were
    prob = orc.synthetic_problem(10, 4, 5, seed=1, flow=None, S=8)
    X = prob["X"].to(DEV)
    need = lib.tgp_qf_input_grad_var_workspace_bytes(10, 4, 5)
    with pytest.raises(L.TgpError, match=r"-101 .*tgp_qf_input_grad_var_f64"):
        ops.qf_input_grad_var(X, *_dev(prob["params"]), workspace_bytes=need - 8)
    Z, rl, ro, m, Lam = _dev(prob["params"])
    md = L.TgpModel()
    md.N, md.D, md.M, md.S, md.kernel = 10, 4, 5, 1, L.KERNEL_SCALE_RBF
    md.scale, md.kl_scale, md.jitter = 1.0, 1.0, 0.0
    keep = [t.reshape(-1).contiguous() if t.dim() < 2 else t.contiguous() for t in (Z, rl, ro, m, Lam)]
    md.Z, md.raw_ls, md.raw_os, md.m, md.Lam = (L.ptr(t) for t in keep)
    dvar = torch.full((10, 4), SENTINEL, dtype=F64, device=DEV)
    status = torch.full((8,), -7, dtype=torch.int32, device=DEV)
    ws = torch.empty(need // 8 + 1, dtype=F64, device=DEV)
    for kw, code in ((dict(nbytes=need - 1), L.E_WORKSPACE), (dict(D=17), U), (dict(N=0), U), (dict(kernel=4), U)):
        md.N, md.D, md.kernel = kw.get("N", 10), kw.get("D", 4), kw.get("kernel", L.KERNEL_SCALE_RBF)
        rc = lib.tgp_qf_input_grad_var_f64(md, L.ptr(X), L.ptr(dvar), L.ptr(status), L.ptr(ws), kw.get("nbytes", need), L.stream_ptr())
        torch.cuda.synchronize()
        assert rc == code and lib.tgp_last_error().startswith(b"tgp_qf_input_grad_var_f64"), kw
        assert bool((dvar == SENTINEL).all()) and bool((status == -7).all()), kw


# ---- end to end ---------------------------------------------------------------------------------------------------------------
def test_cli_slope_significance_end_to_end():
    r = subprocess.run([sys.executable, "-m", "tgp.pytorch_amd.main", "--model", "SVGP", "--dataset", "synthetic_relevance",
                        "--train_test_seed_split", "1", "--num_inducing", "20", "--epochs", "5", "--relevance",
                        "--slope_significance"], cwd=REPO, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.strip().splitlines()
    rows = [re.search(r"input (\d) slope significant \(95%\) on ([0-9.]+) of the test rows$", ln) for ln in lines[-6:]]
    assert all(rows), r.stdout[-2000:]
    assert [int(t.group(1)) for t in rows] == list(range(6))
    sig = [float(t.group(2)) for t in rows]
    print("slope significance after 5 epochs: %s" % " ".join("%.4f" % x for x in sig))
    assert all(math.isfinite(x) and 0.0 <= x <= 1.0 for x in sig)
    assert len(re.findall(r"input \d relevance ", r.stdout)) == 6          # --relevance's lines are still there, before the new ones
