"""GPU (-m gpu): the heteroscedastic Gaussian likelihood (TGP_LIK_HETERO: y ~ N(G(f), exp(c + h)), a second latent GP h for the
log noise variance) through every layer -- the ELL kernel and its gradients against torch autograd (tests/hetero_model.py
restates the formulae), its reduction to the homoscedastic kernel, the extremes, the prediction kernel, the refusals of the
real library, the composed training step against the CPU restatement, the model classes and the CLI."""
import math
import re
import subprocess
import sys
import warnings

import numpy as np
import pytest
import torch

from conftest import REPO, load_golden, rel_err

import hetero_model as HM
from oracle import tgp_oracle as O
from poisson_model import flow_any

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL_VAL, TOL_GRAD = 1e-9, 1e-7
F64 = torch.float64
SAL, PER_ROW = 1, 4
C0 = math.log(0.07)


@pytest.fixture(autouse=True)
def _f64():
    from tgp.pytorch_amd import config as cg
    old = torch.get_default_dtype()
    cg.set_maximum_precission()
    cg.device = DEV
    yield
    torch.set_default_dtype(old)


def _spec(program, P, RP=0):
    from tgp.pytorch_amd import ops
    return ops.FlowSpec([tuple(int(v) for v in b) for b in (program or [])], P, RP, DEV)


def _hermite(S):
    return tuple(torch.tensor(a) for a in np.polynomial.hermite.hermgauss(S))


def _dev(t):
    return None if t is None else t.to(DEV).contiguous()


_CASE_CACHE = {}


def _case(case, N, g):
    """(program, theta, rowp) of a named flow case; the per-row parameters of `idsal` come from the generator `g`."""
    if case == "idsal":
        rowp = torch.stack([0.1 * torch.randn(N, generator=g, dtype=F64), 0.8 + 0.05 * torch.randn(N, generator=g, dtype=F64)], 1)
        return [(SAL, 0, 0, PER_ROW)], None, rowp
    if case not in _CASE_CACHE:
        if case == "empty":
            _CASE_CACHE[case] = ([], None)
        elif case in ("sal2", "tanh3x2"):
            prob = O.synthetic_problem(64, 4, 8, seed=5 if case == "sal2" else 0, flow=case)
            _CASE_CACHE[case] = ([tuple(int(v) for v in b) for b in prob["program"]], prob["params"]["theta"].clone())
        else:
            z = load_golden(case)
            _CASE_CACHE[case] = (z["program"], z["p_theta"].clone())
    program, theta = _CASE_CACHE[case]
    return program, theta, None


_INPUT_CACHE = {}


def _inputs(case, N):
    """The inputs of the likelihood comparisons, seeded by N and made once per (case, N): mu1 = 0.5 randn, v1 = 0.3 rand,
    mu2 = 0.7 randn, v2 = 1.5 rand, the first seven v1 and the next seven v2 at -1e-12, Y = G(mu1) + 0.3 randn."""
    if (case, N) not in _INPUT_CACHE:
        g = torch.Generator().manual_seed(N)
        mu = torch.stack([0.5 * torch.randn(N, generator=g, dtype=F64), 0.7 * torch.randn(N, generator=g, dtype=F64)])
        v = torch.stack([0.3 * torch.rand(N, generator=g, dtype=F64), 1.5 * torch.rand(N, generator=g, dtype=F64)])
        v[0, :7] = -1e-12
        v[1, 7:14] = -1e-12
        program, theta, rowp = _case(case, N, g)
        Y = flow_any(mu[0].reshape(1, -1), program, theta, rowp).reshape(-1) + 0.3 * torch.randn(N, generator=g, dtype=F64)
        _INPUT_CACHE[(case, N)] = (mu, v, Y, program, theta, rowp)
    return _INPUT_CACHE[(case, N)]


def _autograd(Y, mu, v, c, program, theta, xs, ws, rowp, scale):
    """(ell, dict of gradients) of the restatement; the adjoint of a variance <= 0 is 0 (autograd leaves NaN / 0 there)."""
    wrt = [mu.clone().requires_grad_(True), v.clone().requires_grad_(True), c.clone().requires_grad_(True)]
    th = theta.clone().requires_grad_(True) if theta is not None else None
    rp = rowp.clone().requires_grad_(True) if rowp is not None else None
    ell = HM.ell_torch(Y, wrt[0], wrt[1], wrt[2], program, th, xs, ws, rp, scale)
    extra = [t for t in (th, rp) if t is not None]
    grads = torch.autograd.grad(ell, wrt + extra)
    gv = grads[1].clone()
    gv[v <= 0] = 0.0
    out = {"g_mu": grads[0], "g_v": gv, "g_c": grads[2]}
    if th is not None:
        out["g_theta"] = grads[3]
    if rp is not None:
        out["g_rowp"] = grads[-1]
    return ell.detach(), out


# ---- 1. the ELL kernel against autograd ---------------------------------------------------------------------------------
CASES = ["empty", "sal2", "tanh3x2", "flows_med_arcsl2", "idsal"]


# a single row; 32, 16 and 4 lanes per row (none a multiple of the 8, 16 or 64 rows of a workgroup); several nodes in flight
@pytest.mark.parametrize("N,S", [(1, 32), (300, 32), (4000, 32), (13000, 32), (300, 80), (4000, 40)],
                         ids=["1", "300", "4000", "13000", "300-S80", "4000-S40"])
@pytest.mark.parametrize("case", CASES)
def test_ell_kernel_matches_autograd(case, N, S):
    from tgp.pytorch_amd import ops
    mu, v, Y, program, theta, rowp = _inputs(case, N)
    xs, ws = _hermite(S)
    P, RP = (0 if theta is None else theta.numel()), (0 if rowp is None else rowp.shape[1])
    scale = 3.5
    c = torch.tensor([C0], dtype=F64)

    def run():
        return ops.ell_hetero(Y.to(DEV), mu.to(DEV), v.to(DEV), c.to(DEV), _spec(program, P, RP), _dev(theta), S, _dev(rowp),
                              scale=scale)

    res = run()
    ell, ref = _autograd(Y, mu, v, c, program, theta, xs, ws, rowp, scale)
    errs = {"ell": rel_err(res["ell"].cpu(), ell),
            "mu_bar[0]": rel_err(res["g_mu"].cpu(), ref["g_mu"][0]), "mu_bar[1]": rel_err(res["g_mu_h"].cpu(), ref["g_mu"][1]),
            "v_bar[0]": rel_err(res["g_v"].cpu(), ref["g_v"][0]), "v_bar[1]": rel_err(res["g_v_h"].cpu(), ref["g_v"][1]),
            "out[1]": rel_err(res["g_lvn"].cpu().reshape(1), ref["g_c"])}
    if theta is not None:
        errs["g_theta"] = rel_err(res["g_theta"].cpu(), ref["g_theta"])
    if rowp is not None:
        errs["g_rowp"] = rel_err(res["g_rowp"].cpu(), ref["g_rowp"])
    print(errs)
    assert errs.pop("ell") < TOL_VAL
    assert torch.all(res["g_v"].cpu()[v[0] <= 0] == 0) and torch.all(res["g_v_h"].cpu()[v[1] <= 0] == 0)
    for k, e in errs.items():
        assert e < TOL_GRAD, (k, e)
    # same input, same bits
    res2 = run()
    for k in res:
        assert (res[k] is None and res2[k] is None) or torch.equal(res[k], res2[k]), k


# ---- 2. reduction to the homoscedastic kernel -----------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["empty", "sal2", "idsal"])
def test_reduces_to_the_flow_likelihood(case):
    """mu2 = v2 = 0: p_n = exp(-c) for every row, the likelihood is TGP_LIK_FLOW's at log_var_noise = c."""
    from tgp.pytorch_amd import ops
    N, S = 1000, 32
    mu, v, Y, program, theta, rowp = _inputs(case, N)
    mu, v = mu.clone(), v.clone().clamp(min=0.0)          # (the flow kernel does not clamp v: keep the comparison on v >= 0)
    mu[1], v[1] = 0.0, 0.0
    P, RP = (0 if theta is None else theta.numel()), (0 if rowp is None else rowp.shape[1])
    c = torch.tensor([C0], dtype=F64, device=DEV)
    spec = _spec(program, P, RP)
    res = ops.ell_hetero(Y.to(DEV), mu.to(DEV), v.to(DEV), c, spec, _dev(theta), S, _dev(rowp), scale=3.5)
    ref = ops.ell_flow(Y.to(DEV), _dev(mu[0]), _dev(v[0]), c, spec, _dev(theta), S, _dev(rowp), scale=3.5)
    errs = {"ell": rel_err(res["ell"].cpu(), ref["ell"].cpu()), "g_mu": rel_err(res["g_mu"].cpu(), ref["g_mu"].cpu()),
            "g_v": rel_err(res["g_v"].cpu()[v[0] > 0], ref["g_v"].cpu()[v[0] > 0]),
            "out[1]": rel_err(res["g_lvn"].cpu().reshape(1), ref["g_lvn"].cpu().reshape(1))}
    if theta is not None:
        errs["g_theta"] = rel_err(res["g_theta"].cpu(), ref["g_theta"].cpu())
    print(errs)
    assert errs.pop("ell") < TOL_VAL
    for k, e in errs.items():
        assert e < TOL_GRAD, (k, e)
    assert torch.all(res["g_v_h"] == 0)                    # v2 = 0: clamped, adjoint 0


# ---- 3. extremes ------------------------------------------------------------------------------------------------------------
def test_extremes():
    """Residuals of +-1e8 sigma, v1 = 0, v2 = 0 and mu2 = +-20: every output finite and equal to the restatement row by row;
    the predictive density finite and within TOL_VAL."""
    from tgp.pytorch_amd import ops
    S = 16
    sig = math.sqrt(0.04)
    c = torch.tensor([math.log(0.04)], dtype=F64)
    mu = torch.tensor([[0.0, 0.0, 0.3, -0.2, 1.0, 0.5, -0.5], [0.0, 0.0, 0.0, 0.4, 20.0, -20.0, 0.1]], dtype=F64)
    v = torch.tensor([[0.0, 1e-3, 0.5, 0.0, 0.2, 0.3, 0.1], [0.0, 0.3, 0.0, 0.0, 0.5, 0.5, 1.5]], dtype=F64)
    Y = torch.tensor([1e8 * sig, -1e8 * sig, 1e8 * sig, -0.25, 1.1, 0.45, 0.0], dtype=F64)
    xs, ws = _hermite(S)
    res = ops.ell_hetero(Y.to(DEV), mu.to(DEV), v.to(DEV), c.to(DEV), _spec([], 0), None, S)
    ell, ref = _autograd(Y, mu, v, c, [], None, xs, ws, None, 1.0)
    for k in ("ell", "g_mu", "g_v", "g_mu_h", "g_v_h", "g_lvn"):
        assert torch.isfinite(res[k]).all(), k
    assert rel_err(res["ell"].cpu(), ell) < TOL_VAL
    assert rel_err(res["g_lvn"].cpu().reshape(1), ref["g_c"]) < TOL_GRAD

    def rowwise(a, b):
        d = (a.cpu() - b).abs()
        return float((d / b.abs().clamp(min=1e-300))[b != 0].max()) if bool((b != 0).any()) else 0.0

    pairs = {"mu_bar[0]": (res["g_mu"], ref["g_mu"][0]), "mu_bar[1]": (res["g_mu_h"], ref["g_mu"][1]),
             "v_bar[0]": (res["g_v"], ref["g_v"][0]), "v_bar[1]": (res["g_v_h"], ref["g_v"][1])}
    for k, (a, b) in pairs.items():
        e = rowwise(a, b)
        print(k, e)
        assert e < TOL_GRAD, (k, e)
        assert torch.all(a.cpu()[b == 0] == 0), k
    _, _, lp = ops.predict_hetero(mu.to(DEV), v.to(DEV), c.to(DEV), _spec([], 0), None, S, Y=Y.to(DEV), Y_std=3.0)
    _, _, lp_ref = HM.pred_torch(mu, v, c, [], None, xs, ws, Y=Y, Y_std=3.0)
    print("logp", lp.cpu().tolist(), "restatement", lp_ref.tolist())
    assert torch.isfinite(lp).all() and float(((lp.cpu() - lp_ref).abs() / lp_ref.abs()).max()) < TOL_VAL


# ---- 4. the prediction kernel -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [20, 50])
@pytest.mark.parametrize("case", ["empty", "sal2", "flows_med_arcsl2", "idsal"])
def test_predict_matches_restatement(case, S):
    from tgp.pytorch_amd import ops
    N = 1000
    mu, v, Y, program, theta, rowp = _inputs(case, N)
    xs, ws = _hermite(S)
    P, RP = (0 if theta is None else theta.numel()), (0 if rowp is None else rowp.shape[1])
    c = torch.tensor([C0], dtype=F64)
    args = (mu.to(DEV), v.to(DEV), c.to(DEV), _spec(program, P, RP), _dev(theta), S, _dev(rowp))
    m1, m2, lp = ops.predict_hetero(*args, Y=Y.to(DEV), Y_std=7.0)
    r1, r2, rlp = HM.pred_torch(mu, v, c, program, theta, xs, ws, rowp, Y=Y, Y_std=7.0)
    # m1 is a mean of either sign, so its error is rel_err's (against the largest entry); m2 and logp row by row
    errs = [rel_err(m1.cpu(), r1), float(((m2.cpu() - r2).abs() / r2).max()), float(((lp.cpu() - rlp).abs() / rlp.abs()).max())]
    print("errors m1, m2 (per row), logp (per row):", errs)
    assert max(errs) < TOL_VAL
    if case == "empty":
        noise = torch.exp(C0 + mu[1] + 0.5 * v[1].clamp(min=0.0))
        assert torch.equal(m1.cpu(), mu[0])
        assert float(((m2.cpu() - (v[0].clamp(min=0.0) + noise)).abs() / m2.cpu()).max()) < TOL_VAL
    # without targets: the same moments, no logp; same input, same bits
    m1b, m2b, none = ops.predict_hetero(*args)
    assert none is None and torch.equal(m1b, m1) and torch.equal(m2b, m2)
    _, _, lp2 = ops.predict_hetero(*args, Y=Y.to(DEV), Y_std=7.0, want_moments=False)
    assert torch.equal(lp2, lp)


# ---- 5. refusals through the real library ---------------------------------------------------------------------------------
def test_library_refusals():
    from tgp.pytorch_amd import lib as L
    from tgp.pytorch_amd import ops
    h = L.load()
    N, S = 40, 8
    buf = torch.zeros(2, N, dtype=F64, device=DEV)
    one = torch.zeros(N, dtype=F64, device=DEV)
    lvn = torch.zeros(1, dtype=F64, device=DEV)
    st = torch.zeros(2, dtype=torch.int32, device=DEV)
    spec = _spec([], 0)
    md, keep = ops._flow_model(N, S, spec, None, lvn, DEV, lik=L.LIK_HETERO)
    p, po, ps = L.ptr(buf), L.ptr(one), L.ptr(st)
    gr, adam = L.TgpGrads(), L.TgpAdamArgs()
    ws = torch.empty(h.tgp_ell_workspace_bytes(N, 0, 0) // 8, dtype=F64, device=DEV)
    calls = {
        "tgp_elbo_step_f64": lambda: h.tgp_elbo_step_f64(md, p, po, None, po, gr, None, None, ps, L.ptr(ws), ws.numel() * 8, None),
        "tgp_elbo_step_adam_f64": lambda: h.tgp_elbo_step_adam_f64(md, p, po, None, po, gr, None, None, ps, L.ptr(ws),
                                                                   ws.numel() * 8, adam, None),
        "tgp_optimal_qu_f64": lambda: h.tgp_optimal_qu_f64(md, p, po, po, po, ps, L.ptr(ws), ws.numel() * 8, None),
        "tgp_ell_flow_f64": lambda: h.tgp_ell_flow_f64(md, po, po, po, None, po, None, None, None, None, L.ptr(ws), ws.numel() * 8,
                                                       L.stream_ptr()),
        "tgp_predict_f64": lambda: h.tgp_predict_f64(md, po, po, None, None, 1.0, po, po, None, L.stream_ptr()),
        "tgp_predict_quantile_f64": lambda: h.tgp_predict_quantile_f64(md, po, po, None, po, po, 1, po, ps, L.stream_ptr()),
        "tgp_predict_cdf_f64": lambda: h.tgp_predict_cdf_f64(md, po, po, None, po, po, None, L.stream_ptr()),
    }
    for name, call in calls.items():
        assert call() == L.E_UNSUPPORTED, name
        assert b"tgp_ell_hetero_f64" in h.tgp_last_error(), name
    for bad_S in (0, 257):
        md.S = bad_S
        rc = h.tgp_predict_hetero_f64(md, p, p, None, None, 1.0, po, po, None, L.stream_ptr())
        assert rc == L.E_UNSUPPORTED, (bad_S, rc)
    md.S = S
    assert h.tgp_predict_hetero_f64(md, p, p, None, None, 1.0, po, po, None, L.stream_ptr()) == 0
    # the workspace: exactly the sizer's bytes pass, one double less is refused
    need = h.tgp_ell_workspace_bytes(N, 0, 0)
    out = torch.zeros(2, dtype=F64, device=DEV)
    ell = lambda nbytes: h.tgp_ell_hetero_f64(md, po, p, p, None, L.ptr(out), None, None, None, None, L.ptr(ws), nbytes,
                                              L.stream_ptr())
    assert ell(need - 8) == L.E_WORKSPACE and b"tgp_ell_workspace_bytes" in h.tgp_last_error()
    assert ell(need) == 0
    torch.cuda.synchronize()
    # every output pointer is optional: no `out` either
    assert h.tgp_ell_hetero_f64(md, po, p, p, None, None, None, None, None, None, L.ptr(ws), need, L.stream_ptr()) == 0
    torch.cuda.synchronize()


# ---- 6. the composed step against the CPU restatement ---------------------------------------------------------------------
def _flow_specs(flow):
    from tgp.pytorch_amd import flows as G
    np.random.seed(3)                                    # (StepTanhL draws its initial steps from numpy's global generator)
    return {"sal2": lambda: G.SAL(2), "sal1": lambda: G.SAL(1), "tanh3x2": lambda: G.StepTanhL(3, 2, add_f0=True)}[flow]()


def _build_model(X, M, flow="none", kernel="scale_rbf", whiten=True, S=20, N_total=None):
    from tgp.pytorch_amd.kernels import instance_kernel
    from tgp.pytorch_amd.likelihoods import HeteroscedasticGaussian
    from tgp.pytorch_amd.models import sparse_MF_GP, sparse_MF_SP
    D = X.shape[1]
    K = instance_kernel(kernel, ard_num_dim=D, num_multioutput=2, kernel_is_shared=False,
                        init_params={"length_scale": 2.0, "kernel_scale": 2.0, "noisy_variance": 1e-6})
    ip = {"variational_distribution": {"variance_scale": 1e-5, "mean_scale": 0.0}}
    lik = HeteroscedasticGaussian(0.07, S)
    Ntot = X.shape[0] if N_total is None else N_total
    if flow == "none":
        model = sparse_MF_GP(["zero", K], X, X[:M].clone(), Ntot, lik, 2, whiten, False, False, False, False, 0.0, init_params=ip)
    else:
        model = sparse_MF_SP(["zero", K], X, X[:M].clone(), Ntot, lik, 2, whiten, False, False, False, False,
                             [_flow_specs(flow), [("identity", [])]], "single", 0.0, init_params=ip)
    return model.to(DEV)


def _set_gp_params(model, pf, ph):
    """The two latent GPs' parameters from two dicts (Z, raw_lengthscale, raw_outputscale, m, Lam)."""
    k = model.covariance_function
    with torch.no_grad():
        model.Z.data = torch.stack([pf["Z"], ph["Z"]]).to(DEV)
        k.base_kernel.raw_lengthscale.data = torch.stack([pf["raw_lengthscale"].reshape(1, -1), ph["raw_lengthscale"].reshape(1, -1)]).to(DEV)
        k.raw_outputscale.data = torch.stack([pf["raw_outputscale"].reshape(()), ph["raw_outputscale"].reshape(())]).to(DEV)
        model.q_U.variational_mean.data = torch.stack([pf["m"], ph["m"]]).to(DEV)
        model.q_U.chol_variational_covar.data = torch.stack([pf["Lam"], ph["Lam"]]).to(DEV)


def _model_flow(model, perturb_seed=None):
    """(program, theta on the CPU or None) of the model's flow on f; `perturb_seed`: move the flow's parameters off their
    initial values first."""
    from tgp.pytorch_amd.flow import compile_flow
    spec, theta_list, _ = compile_flow(model.G_matrix[0])
    if perturb_seed is not None and theta_list:
        g = torch.Generator().manual_seed(perturb_seed)
        with torch.no_grad():
            for q in theta_list:
                q.add_((0.1 * torch.randn(q.shape, generator=g, dtype=F64)).to(q.device))
    theta = torch.stack([q.detach().reshape(()) for q in theta_list]).cpu() if theta_list else None
    return list(spec.blocks), theta, theta_list


STEPS = [(300, 4, 20, "sal2", 20, "scale_rbf", True), (257, 13, 128, "none", 16, "scale_rbf", True),
         (400, 5, 150, "tanh3x2", 32, "scale_rbf", True), (300, 3, 33, "sal1", 20, "scale_matern32", True),
         (300, 4, 20, "sal2", 20, "scale_rbf", False)]


@pytest.mark.parametrize("N,D,M,flow,S,kernel,whiten", STEPS,
                         ids=["sal2-M20", "svgp-M128", "tanh3x2-M150", "sal1-M33-matern32", "sal2-M20-unwhitened"])
def test_composed_step_matches_cpu(N, D, M, flow, S, kernel, whiten):
    """model.ELBO (two q(f) launches with their adjoints, two KL terms, one tgp_ell_hetero_f64) against step_torch: ELBO, ELL,
    KLD and the gradient of every parameter of both GPs, c and theta."""
    from tgp.pytorch_amd import ops
    pa = O.synthetic_problem(N, D, M, 5, "none", S)
    pb = O.synthetic_problem(N, D, M, 6, "none", S)
    X, Y = pa["X"], pa["Y"]
    keys = ("Z", "raw_lengthscale", "raw_outputscale", "m", "Lam")
    pf = {k: pa["params"][k].clone() for k in keys}
    ph = {k: pb["params"][k].clone() for k in keys}
    ph["m"] = 0.3 * ph["m"]                              # (a moderate log-noise function)
    if not whiten:                                       # (m, Lam) describe q(u) itself: keep L_q's diagonal away from 0
        for p in (pf, ph):
            p["Lam"] = torch.tril(p["Lam"]) + 0.5 * torch.eye(M, dtype=F64)
    model = _build_model(X, M, flow, kernel, whiten, S, N_total=float(2 * N))
    _set_gp_params(model, pf, ph)
    program, theta, theta_list = _model_flow(model, perturb_seed=9)
    if theta is not None:
        pf["theta"] = theta
    c = model.likelihood.log_var_noise.detach().reshape(-1).cpu()
    xs, ws = _hermite(S)
    (elbo, ell, kld), gf, gh, gc = HM.step_torch(X, Y, pf, ph, c, float(2 * N), program, xs, ws, kernel, jitter=1e-6, whiten=whiten)
    model.set_is_training(True)
    # every factorisation of the composed step reads its status words and climbs the jitter ladder with a NumericalWarning
    # when they are not 0: none may be raised, and the transform of an unwhitened model must end at jitter 0 too
    with warnings.catch_warnings():
        warnings.simplefilter("error", ops.NumericalWarning)
        e, l, k = model.ELBO(X.to(DEV), Y.to(DEV))
        e.backward()
        torch.cuda.synchronize()
        for gp in (0, 1):
            info = {}
            with torch.no_grad():
                model._gp_params(gp, info=info)
            assert info["jitter"] == 0.0
    errs = {"elbo": rel_err(e.detach().cpu(), elbo), "ell": rel_err(l.detach().cpu(), ell), "kld": rel_err(k.detach().cpu(), kld)}
    kf = model.covariance_function
    for gp, ref in ((0, gf), (1, gh)):
        got = {"Z": model.Z.grad[gp], "raw_lengthscale": kf.base_kernel.raw_lengthscale.grad[gp].reshape(-1),
               "raw_outputscale": kf.raw_outputscale.grad[gp].reshape(-1), "m": model.q_U.variational_mean.grad[gp],
               "Lam": model.q_U.chol_variational_covar.grad[gp]}
        for name in keys:
            want = torch.tril(ref[name]) if name == "Lam" else ref[name].reshape(got[name].shape)
            errs["g%d_%s" % (gp, name)] = rel_err(got[name].cpu(), want)
    errs["g_c"] = rel_err(model.likelihood.log_var_noise.grad.reshape(-1).cpu(), gc.reshape(-1))
    if theta is not None:
        errs["g_theta"] = rel_err(torch.stack([q.grad.reshape(()) for q in theta_list]).cpu(), gf["theta"])
    print(errs)
    for name in ("elbo", "ell", "kld"):
        assert errs.pop(name) < TOL_VAL, name
    for name, err in errs.items():
        assert err < TOL_GRAD, (name, err)


# ---- 7. the model classes -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hetero():
    """300 rows of synthetic_hetero, standardised."""
    from tgp.pytorch_amd import synthetic
    X, Y, sigma = synthetic.hetero_dataset(1)
    X, Y = X[:300], Y[:300]
    Y = (Y - Y.mean()) / Y.std()
    return torch.tensor(X, dtype=F64), torch.tensor(Y, dtype=F64)


def _move_qu(model, M=20):
    gen = torch.Generator().manual_seed(11)
    with torch.no_grad():
        model.q_U.variational_mean.data = (0.3 * torch.randn(2, M, generator=gen, dtype=F64)).to(DEV)
        model.q_U.chol_variational_covar.data = (0.1 * torch.eye(M, dtype=F64).repeat(2, 1, 1) +
                                                 0.02 * torch.randn(2, M, M, generator=gen, dtype=F64).tril()).to(DEV)


@pytest.mark.parametrize("flow", ["none", "sal1"], ids=["svgp", "tgp"])
def test_model(hetero, flow):
    X, Y = hetero
    model = _build_model(X, 20, flow)
    _move_qu(model)
    program, theta, _ = _model_flow(model, perturb_seed=4)
    Xd, Yd = X.to(DEV), Y.to(DEV)
    S = model.quad_points
    xs, ws = _hermite(S)
    c = model.likelihood.log_var_noise.detach().reshape(-1).cpu()
    model.set_is_training(False)
    n, ystd = 20, 2.5
    with torch.no_grad():
        mu, v = model.marginal_variational_qf_parameters(Xd[:n], diagonal=True, is_duvenaud=False)
    assert mu.shape == (2, n, 1) and v.shape == (2, n, 1)
    mu, v = mu.squeeze(2).cpu(), v.squeeze(2).cpu()
    r1, r2, rlp = HM.pred_torch(mu, v, c, program, theta, xs, ws, Y=Y[:n].reshape(-1), Y_std=ystd)
    lp_sum, (m1, m2) = model.test_log_likelihood(Xd[:n], Yd[:n], return_moments=True, Y_std=torch.full((1,), ystd, device=DEV))
    assert m1.shape == (1, n) and m2.shape == (1, n)
    assert rel_err(lp_sum.cpu(), rlp.sum().reshape(1)) < TOL_VAL
    assert rel_err(m1.reshape(-1).cpu(), r1) < TOL_VAL and float(((m2.reshape(-1).cpu() - r2).abs() / r2).max()) < TOL_VAL
    pm1, pm2, mq, vq = model.predictive_distribution(Xd[:n])
    assert torch.equal(pm1, m1) and torch.equal(pm2, m2) and mq.shape == (2, n, 1)
    lp_only, none = model.test_log_likelihood(Xd[:n], Yd[:n], return_moments=False, Y_std=torch.full((1,), ystd, device=DEV))
    assert none is None and torch.equal(lp_only, lp_sum)
    # the noise level: closed-form quantiles of exp((c + h) / 2)
    q = model.predictive_noise_std(Xd[:n], [0.025, 0.5, 0.975])
    z = 1.959963984540054
    want = torch.exp(0.5 * (c + mu[1].reshape(1, -1) + torch.tensor([-z, 0.0, z], dtype=F64).reshape(-1, 1) * torch.sqrt(v[1].clamp(min=0.0)).reshape(1, -1)))
    assert q.shape == (3, n) and float(((q.cpu() - want).abs() / want).max()) < 1e-8
    # draws of y: G(f) + exp((c + h) / 2) eps; their variance is m2's
    torch.manual_seed(0)
    s, f_k, f_0 = model.sample_from_predictive_distribution(Xd[:n], S=4000)
    assert s.shape == (1, 4000, n, 1) and torch.isfinite(s).all() and f_k.shape == (2, 4000 * n)
    ratio = s[0, :, :, 0].var(dim=0).cpu() / r2
    print("sample variance / m2 per row:", ratio.min().item(), ratio.max().item())
    assert float((ratio - 1.0).abs().max()) < 0.10
    assert bool(((s[0, :, :, 0].mean(dim=0).cpu() - r1).abs() < 5.0 * torch.sqrt(r2 / 4000.0)).all())   # five standard errors
    pq = model.posterior_quantiles(Xd[:n], [0.1, 0.9])         # G(f)'s quantiles: output 0
    assert pq.shape == (1, 2, n) and bool((pq[0, 0] < pq[0, 1]).all())
    want_q = flow_any((mu[0] + 1.2815515655446004 * torch.sqrt(v[0].clamp(min=0.0))).reshape(1, -1), program, theta).reshape(-1)
    assert rel_err(pq[0, 1].cpu(), want_q) < 1e-8


def test_trainer_raises_the_elbo(hetero):
    from tgp.pytorch_amd.data import DeviceLoader
    from tgp.pytorch_amd.trainers import Trainer_SP_regression
    X, Y = hetero
    model = _build_model(X, 20, "sal1")
    loader = DeviceLoader(X, Y, 10000, shuffle=False, device=DEV)
    # (Y_std: one entry per latent GP, the trainer's rule; the first is the targets')
    tr = Trainer_SP_regression(model, [loader, None, None], 1e20, False, False, torch.ones(2, device=DEV), -1, 100, True)
    tr.train(epochs=20, lr_ALL=0.01, opt="adam", keep_parameter_groups=True)
    assert tr._engine is None                            # the eager loop: the step engines refuse the likelihood
    elbo = [-l for l in tr.loss_arr]
    print("ELBO first %.6f last %.6f" % (elbo[0], elbo[-1]))
    assert len(elbo) == 20 and all(math.isfinite(e) for e in elbo) and elbo[-1] > elbo[0]


# ---- 8. the CLI -------------------------------------------------------------------------------------------------------------
def _cli(model, likelihood):
    cmd = [sys.executable, "-m", "tgp.pytorch_amd.main", "--model", model, "--likelihood", likelihood, "--dataset", "synthetic_hetero",
           "--train_test_seed_split", "1", "--num_inducing", "20", "--epochs", "300"]
    r = subprocess.run(["timeout", "-k", "10", "300"] + cmd, cwd=REPO, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    m = re.search(r"Test Negative LOGL (-?[0-9.]+(?:e[-+]?\d+)?|nan|inf), Test RMSE (-?[0-9.]+(?:e[-+]?\d+)?|nan|inf)", r.stdout)
    assert m is not None, r.stdout[-2000:]
    return float(m.group(1)), float(m.group(2)), r.stdout


@pytest.mark.parametrize("model", ["SVGP", "TGP"])
def test_cli_beats_the_constant_noise_model(model):
    """`--likelihood hetero` on synthetic_hetero: finite numbers, a test NLL strictly below the same command with `--likelihood
    gaussian`, and a positive correlation of the learned with the true log noise level."""
    nll_h, rmse_h, out = _cli(model, "hetero")
    nll_g, rmse_g, _ = _cli(model, "gaussian")
    m = re.search(r"log noise std correlation (-?[0-9.]+)", out)
    assert m is not None, out[-2000:]
    corr = float(m.group(1))
    print("%s: hetero NLL %.3f RMSE %.3f | gaussian NLL %.3f RMSE %.3f | correlation %.3f" % (model, nll_h, rmse_h, nll_g, rmse_g, corr))
    assert all(math.isfinite(x) for x in (nll_h, rmse_h, nll_g, rmse_g, corr))
    assert nll_h < nll_g
    assert corr > 0.0
