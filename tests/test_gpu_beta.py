"""GPU (-m gpu): the Beta likelihood (TGP_LIK_BETA: proportions in (0, 1), the flow as the log-odds of the mean, a trained
precision in the noise slot) through every layer -- the stand-alone ELL kernel and its gradients, dELL/dlog phi among them,
against torch autograd (tests/beta_model.py restates the formula), the extremes, the prediction kernel, the training step
(general-M path at every M) against the CPU composition, the exact CDF and quantiles of the mixture of Betas against the
reference CDF, order and bit-identical repeats, the model classes and the CLI.

Bars: TOL_VAL = 1e-9 on values, TOL_GRAD = 1e-7 on gradients, those of tests/test_gpu_gamma.py for the same comparisons.  The CDF
and quantile bars are those of tests/test_beta_host.py: every tail of the CDF entry within 10x RESIDUAL_CF_CPU of the case's phi
of the reference (beta_model.tails_ref: mpmath, with scipy.special.betainc where the host test holds it to mpmath; mpmath alone where the case is small), every root within
the same allowance through `beta_model.residual_within_ulp` (F of the reference at the doubles next to the returned t brackets
p): see the host test's docstring for why a root handed back as a double is held to its neighbours."""
import math
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import REPO, rel_err

import beta_model as BM
from oracle import tgp_oracle as O
from test_beta_host import (HARD_CASES, HARD_PROBS, QUANT_CASES, RESIDUAL_CF_CPU, hard_problem, node_values, quant_problem,
                            worst_root_residual)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL_VAL, TOL_GRAD = 1e-9, 1e-7
F64 = torch.float64
PHIS = [0.5, 1.0, 10.0, 1000.0]
KINDS = ["empty", "sal2", "tanh3x2", "bcl_al"]       # empty, SAL x 2, tanh 3 x 2, an extended kind (Box-Cox + affine)
DATA_PHI = 5.0             # the targets of the likelihood comparisons are Beta(5 mu, 5 (1 - mu)) whatever the model's precision
CLIP = 1e-6


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


def _dev(t):
    return None if t is None or t.numel() == 0 else t.to(DEV).contiguous()


def _lam(phi):
    return torch.tensor([math.log(phi)], dtype=F64)


def _beta_draw(mean, phi, g):
    a = torch._standard_gamma(mean * phi, generator=g)
    b = torch._standard_gamma((1.0 - mean) * phi, generator=g)
    return (a / (a + b)).clamp(CLIP, 1.0 - CLIP)


def _inputs(kind, N, S, phi, v0=True):
    """mu, v (the first rows at -1e-12 and 0 when there are more than two), proportions around sigmoid(G(mu)), the flow and the
    rule: a problem dict of test_beta_host.quant_problem with Y."""
    pr = quant_problem(kind, N, S, phi, seed=N + S)
    g = torch.Generator().manual_seed(7000 + N + S)
    pr["mu"] = 0.5 * torch.randn(N, generator=g, dtype=F64)
    pr["v"] = 0.3 * torch.rand(N, generator=g, dtype=F64)
    if v0 and N > 2:
        pr["v"][0], pr["v"][1] = -1e-12, 0.0
    mean = torch.sigmoid(BM.G(pr["mu"].reshape(1, -1), pr["program"], pr["theta"]).reshape(-1)).clamp(1e-3, 1.0 - 1e-3)
    pr["Y"] = _beta_draw(mean, DATA_PHI, g)
    return pr


def _theta(pr):
    return pr["theta"] if pr["theta"].numel() else None


# ---- 1. the stand-alone ELL kernel against autograd --------------------------------------------------------------------
@pytest.mark.parametrize("phi", PHIS)
@pytest.mark.parametrize("kind", KINDS)
def test_ell_kernel_matches_autograd(kind, phi):
    from tgp.pytorch_amd import ops
    worst = {}
    for N in (1, 5, 67, 300):
        for S in (1, 5, 16, 17, 32):
            pr = _inputs(kind, N, S, phi)
            lam, theta, scale = _lam(phi), _theta(pr), 3.5
            P = 0 if theta is None else theta.numel()
            res = ops.ell_beta(pr["Y"].to(DEV), pr["mu"].to(DEV), pr["v"].to(DEV), lam.to(DEV), _spec(pr["program"], P), _dev(theta),
                               S, scale=scale)
            wrt = [pr["mu"].clone().requires_grad_(True), pr["v"].clone().requires_grad_(True), lam.clone().requires_grad_(True)]
            th = theta.clone().requires_grad_(True) if theta is not None else None
            ell = BM.ell_torch(pr["Y"], wrt[0], wrt[1], wrt[2], pr["program"], th, pr["xs"], pr["wn"], None, scale)
            grads = torch.autograd.grad(ell, wrt + ([th] if th is not None else []))
            gv = grads[1].clone()
            nz = pr["v"] <= 0.0
            gv[nz] = 0.0                                        # v <= 0: the adjoint of v is 0
            if S == 1:
                gv[:] = 0.0                                     # one node at x = 0: no dependence on v
            assert torch.all(res["g_v"].cpu()[nz] == 0)
            errs = {"ell": rel_err(res["ell"].cpu(), ell.detach()), "g_mu": rel_err(res["g_mu"].cpu(), grads[0]),
                    "g_lvn": rel_err(res["g_lvn"].cpu(), grads[2])}
            errs["g_v"] = rel_err(res["g_v"].cpu(), gv) if S > 1 else float(res["g_v"].abs().max())
            if th is not None:
                errs["g_theta"] = rel_err(res["g_theta"].cpu(), grads[3])
            for k, e in errs.items():
                worst[k] = max(worst.get(k, 0.0), e)
                assert e < (TOL_VAL if k == "ell" else TOL_GRAD), (kind, phi, N, S, k, e)
    print("%s phi = %g: worst over N, S" % (kind, phi), worst)


@pytest.mark.parametrize("phi", [0.5, 1000.0])
def test_ell_kernel_per_row_program(phi):
    """A per-row SAL program (TGP_FLAG_PER_ROW): g_rowp beside the other gradients, N = 67 and 300, S = 17."""
    from tgp.pytorch_amd import ops
    from test_quantiles_host import seeded_problem
    for N in (67, 300):
        S = 17
        pr = seeded_problem("idsal1", N, S, seed=N)
        g = torch.Generator().manual_seed(N)
        mu, v = 0.5 * torch.randn(N, generator=g, dtype=F64), 0.3 * torch.rand(N, generator=g, dtype=F64)
        v[0], v[1] = -1e-12, 0.0
        mean = torch.sigmoid(BM.G(mu.reshape(1, -1), pr["program"], pr["theta"], pr["rowp"]).reshape(-1)).clamp(1e-3, 1.0 - 1e-3)
        Y = _beta_draw(mean, DATA_PHI, g)
        lam, theta, rowp = _lam(phi), pr["theta"], pr["rowp"]
        spec = _spec(pr["program"], theta.numel(), rowp.shape[1])
        res = ops.ell_beta(Y.to(DEV), mu.to(DEV), v.to(DEV), lam.to(DEV), spec, _dev(theta), S, rowp=_dev(rowp), scale=2.0)
        wrt = [t.clone().requires_grad_(True) for t in (mu, v, lam, theta, rowp)]
        ell = BM.ell_torch(Y, wrt[0], wrt[1], wrt[2], pr["program"], wrt[3], pr["xs"], pr["wn"], wrt[4], 2.0)
        grads = torch.autograd.grad(ell, wrt)
        gv = grads[1].clone()
        gv[v <= 0.0] = 0.0
        assert rel_err(res["ell"].cpu(), ell.detach()) < TOL_VAL
        for k, ref in (("g_mu", grads[0]), ("g_v", gv), ("g_lvn", grads[2]), ("g_theta", grads[3]), ("g_rowp", grads[4])):
            assert rel_err(res[k].cpu(), ref) < TOL_GRAD, (phi, N, k, rel_err(res[k].cpu(), ref))


# ---- 2. extremes ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("phi", [0.5, 10.0, 1000.0])
def test_extremes(phi):
    """Targets at 1e-6 and 1 - 1e-6, |G| up to 30, rows without variance, a node of weight 0: every row on its own (one launch
    each), value and gradients finite where the float64 formula is finite and equal to the restatement's; the same infinity where
    it is not."""
    from tgp.pytorch_amd import lib as L
    from tgp.pytorch_amd import ops
    rows = [(CLIP, -30.0, 0.0), (CLIP, 30.0, 0.0), (1.0 - CLIP, 30.0, 0.0), (1.0 - CLIP, -30.0, 0.0), (CLIP, 25.0, 0.5),
            (1.0 - CLIP, -25.0, 0.5), (0.5, 0.0, 0.0), (0.3, 12.0, 1e-3)]
    S = 16
    xs, ws = O.hermgauss(S)
    wn = ws / math.sqrt(math.pi)
    wz = wn.clone()
    wz[3] = 0.0                                                 # a node of weight 0 does not enter
    lam = _lam(phi)
    for y, m, vv in rows:
        Y, mu, v = (torch.tensor([t], dtype=F64) for t in (y, m, vv))
        res = ops.ell_beta(Y.to(DEV), mu.to(DEV), v.to(DEV), lam.to(DEV), _spec([], 0), None, S)
        mg, lg = mu.clone().requires_grad_(True), lam.clone().requires_grad_(True)
        ell = BM.ell_torch(Y, mg, v, lg, [], None, xs, wn)
        gm, gl = torch.autograd.grad(ell, [mg, lg])
        print("phi = %g, y = %g, mu = %g, v = %g: ell %.17g restatement %.17g" % (phi, y, m, vv, float(res["ell"]), float(ell.detach())))
        if bool(torch.isfinite(ell)):
            assert bool(torch.isfinite(res["ell"])) and rel_err(res["ell"].cpu(), ell.detach()) < TOL_VAL
            assert bool(torch.isfinite(res["g_mu"]).all()) and rel_err(res["g_mu"].cpu(), gm) < TOL_GRAD
            assert bool(torch.isfinite(res["g_lvn"]).all()) and rel_err(res["g_lvn"].cpu(), gl) < TOL_GRAD
        else:
            assert float(res["ell"]) == float(ell)
        if vv == 0.0:
            assert float(res["g_v"]) == 0.0
        _, _, lp = ops.predict(mu.to(DEV), v.to(DEV), lam.to(DEV), _spec([], 0), None, S, Y=Y.to(DEV), lik=L.LIK_BETA)
        lp_ref = BM.pred_torch(mu, v, lam, [], None, xs, wn, Y=Y)[2]
        if bool(torch.isfinite(lp_ref)):
            assert float((lp.cpu() - lp_ref).abs()) <= TOL_VAL * float(lp_ref.abs()) + 1e-15
        else:
            assert float(lp) == float(lp_ref)
    # the zero-weight node, through the library's own entry (ops builds the rule itself): the model's wn pointer
    lam_d, wz_d, spec0 = lam.to(DEV), wz.to(DEV), _spec([], 0)
    md, keep = ops._flow_model(1, S, spec0, None, lam_d, torch.device(DEV), 1.0, lik=L.LIK_BETA)
    md.wn = L.ptr(wz_d)
    Y, mu, v = (torch.tensor([t], dtype=F64, device=DEV) for t in (0.3, 0.4, 0.5))
    h = L.load()
    ws_ = torch.empty(h.tgp_ell_workspace_bytes(1, 0, 0) // 8 + 16, dtype=F64, device=DEV)
    out, gmu, gv, gth = (torch.empty(n, dtype=F64, device=DEV) for n in (2, 1, 1, 1))
    L.check(h.tgp_ell_flow_f64(md, L.ptr(Y), L.ptr(mu), L.ptr(v), None, L.ptr(out), L.ptr(gmu), L.ptr(gv), L.ptr(gth), None,
                               L.ptr(ws_), ws_.numel() * 8, L.stream_ptr()), "tgp_ell_flow_f64")
    mg = mu.cpu().clone().requires_grad_(True)
    ell = BM.ell_torch(Y.cpu(), mg, v.cpu(), lam, [], None, xs, wz)
    gm, = torch.autograd.grad(ell, [mg])
    assert rel_err(out[0].cpu(), ell.detach()) < TOL_VAL and rel_err(gmu.cpu(), gm) < TOL_GRAD
    m1, m2, lp = (torch.empty(1, dtype=F64, device=DEV) for _ in range(3))
    L.check(h.tgp_predict_f64(md, L.ptr(mu), L.ptr(v), None, L.ptr(Y), 1.0, L.ptr(m1), L.ptr(m2), L.ptr(lp), L.stream_ptr()),
            "tgp_predict_f64")
    keep_nodes = wz > 0.0
    g = BM.nodes(mu.cpu(), v.cpu(), xs, [], None)[keep_nodes]
    w = wz[keep_nodes].reshape(-1, 1)
    r1 = (w * torch.sigmoid(g)).sum(0)
    rlp = torch.logsumexp(torch.log(w) + BM.log_p(Y.cpu().reshape(1, -1), g, lam.reshape(())), 0)
    assert rel_err(m1.cpu(), r1) < TOL_VAL and rel_err(lp.cpu(), rlp) < TOL_VAL


# ---- 3. the prediction kernel ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_predict_matches_restatement(kind):
    from tgp.pytorch_amd import lib as L
    from tgp.pytorch_amd import ops
    for phi in PHIS:
        for S in (1, 5, 32):
            N = 257                                     # a ragged last workgroup
            pr = _inputs(kind, N, S, phi)
            lam, theta = _lam(phi), _theta(pr)
            spec = _spec(pr["program"], 0 if theta is None else theta.numel())
            m1, m2, lp = ops.predict(pr["mu"].to(DEV), pr["v"].to(DEV), lam.to(DEV), spec, _dev(theta), S, Y=pr["Y"].to(DEV),
                                     lik=L.LIK_BETA)
            r1, r2, rlp = BM.pred_torch(pr["mu"], pr["v"], lam, pr["program"], theta, pr["xs"], pr["wn"], Y=pr["Y"])
            assert float(((m1.cpu() - r1).abs() / r1).max()) < TOL_VAL
            assert float(((m2.cpu() - r2).abs() / r2).max()) < TOL_VAL
            assert float(((lp.cpu() - rlp).abs() / rlp.abs().clamp_min(1.0)).max()) < TOL_VAL
            assert bool(((m1 > 0) & (m1 < 1) & (m2 > 0) & (m2 < 0.25)).all())
            # Y_std is ignored: proportions have no units
            m1s, m2s, lps = ops.predict(pr["mu"].to(DEV), pr["v"].to(DEV), lam.to(DEV), spec, _dev(theta), S, Y=pr["Y"].to(DEV),
                                        Y_std=2.5, lik=L.LIK_BETA)
            assert torch.equal(m1s, m1) and torch.equal(m2s, m2) and torch.equal(lps, lp)
            m1b, m2b, none = ops.predict(pr["mu"].to(DEV), pr["v"].to(DEV), lam.to(DEV), spec, _dev(theta), S, lik=L.LIK_BETA)
            assert none is None and torch.equal(m1b, m1) and torch.equal(m2b, m2)


# ---- 4. the training step against the CPU composition ---------------------------------------------------------------------
def step_torch(X, Y, params, N_total, program, xs, ws, kernel="scale_rbf", jitter=None):
    """((ELBO, ELL, KLD), grads) of one Beta training step under autograd: O.qf_moments, BM.ell_torch scaled by N_total / N,
    minus O.kld_whitened.  `params`: Z, raw_lengthscale, raw_outputscale, m, Lam, log_var_noise (= log phi)[, theta]."""
    lv = {k: t.detach().clone().requires_grad_(True) for k, t in params.items()}
    mu, v = O.qf_moments(X, lv["Z"], lv["raw_lengthscale"], lv["raw_outputscale"], lv["m"], lv["Lam"], jitter, kernel)
    prog = [tuple(int(q) for q in b) for b in (program or [])]
    ell = BM.ell_torch(Y.reshape(-1), mu, v, lv["log_var_noise"], prog, lv.get("theta"), xs, ws / math.sqrt(math.pi), None,
                       float(N_total) / X.shape[0])
    kld = O.kld_whitened(lv["m"], lv["Lam"])
    elbo = ell - kld
    elbo.backward()
    return (elbo.detach(), ell.detach(), kld.detach()), {k: t.grad for k, t in lv.items()}


STEPS = [(67, 4, 3, 5, "sal2", 16, "scale_rbf", 10.0), (300, 4, 20, 1, "sal2", 20, "scale_rbf", 1.0),
         (300, 5, 130, 0, "tanh3x2", 32, "scale_rbf", 0.5), (300, 3, 33, 2, "sal1", 20, "scale_matern32", 1000.0)]


@pytest.mark.parametrize("N,D,M,seed,flow,S,kernel,phi", STEPS, ids=["sal2-M3", "sal2-M20", "tanh3x2-M130", "sal1-M33-matern32"])
def test_step_matches_cpu(N, D, M, seed, flow, S, kernel, phi):
    """ops.elbo_step(lik=LIK_BETA) against step_torch, log_var_noise (= log phi) among the gradients.  The general-M path is used
    at every M (the workspace is the one a Gamma step of the shape takes); M = 130 crosses the 128 boundary."""
    from tgp.pytorch_amd import lib as L
    from tgp.pytorch_amd import ops
    prob = O.synthetic_problem(N, D, M, seed, flow, S)
    p = {k: t.clone() for k, t in prob["params"].items()}
    p["raw_outputscale"] = O.inv_softplus(0.3).reshape(1)
    p["m"] = 0.3 * p["m"]
    p["log_var_noise"] = _lam(phi)
    g = torch.Generator().manual_seed(100 + seed)
    w = torch.randn(D, generator=g, dtype=F64)
    mean = torch.sigmoid(0.3 + 0.8 * torch.sin(prob["X"] @ w))
    Y = _beta_draw(mean, DATA_PHI, g).reshape(N, 1)
    program = prob["program"]
    (elbo, ell, kld), rg = step_torch(prob["X"], Y, p, float(N), program, prob["xs"], prob["ws"], kernel, jitter=1e-6)
    theta = p.get("theta") if program is not None else None
    spec = _spec(program, 0 if theta is None else theta.numel())
    h = L.load()
    shape = (N, D, M, S, spec.nblk, spec.P, 0, L.KERNELS[kernel], 0)
    assert h.tgp_workspace_bytes_lik(*shape, L.LIK_BETA) == h.tgp_workspace_bytes_lik(*shape, L.LIK_GAMMA)

    def run():
        out, grads, status, _ = ops.elbo_step(prob["X"].to(DEV), Y.to(DEV), _dev(p["Z"]), _dev(p["raw_lengthscale"]),
                                              _dev(p["raw_outputscale"]), _dev(p["m"]), _dev(p["Lam"]), _dev(p["log_var_noise"]),
                                              float(N), flow=spec, theta=_dev(theta), S=S, kernel=kernel, lik=L.LIK_BETA)
        torch.cuda.synchronize()
        assert int(status[0]) == 0 and int(status[1]) == 0
        return out.cpu(), {k: t.cpu() for k, t in grads.items()}

    out, grads = run()
    errs = {"elbo": rel_err(out[0], elbo), "ell": rel_err(out[1], ell), "kld": rel_err(out[2], kld)}
    pairs = [("Z", "Z"), ("raw_ls", "raw_lengthscale"), ("raw_os", "raw_outputscale"), ("m", "m"), ("Lam", "Lam"),
             ("lvn", "log_var_noise")]
    if theta is not None:
        pairs.append(("theta", "theta"))
    for k_hip, k_ref in pairs:
        errs["g_" + k_hip] = rel_err(grads[k_hip], rg[k_ref])
    print(errs)
    for k in ("elbo", "ell", "kld"):
        assert errs.pop(k) < TOL_VAL, k
    for k, e in errs.items():
        assert e < TOL_GRAD, (k, e)
    assert grads["lvn"].numel() == 1 and float(grads["lvn"].abs()) > 0.0
    out2, grads2 = run()
    assert torch.equal(out, out2) and all(torch.equal(grads[k], grads2[k]) for k in grads)


# ---- 5. the CDF -----------------------------------------------------------------------------------------------------------
def gpu_cdf(pr, Y):
    from tgp.pytorch_amd import lib as L
    from tgp.pytorch_amd import ops
    theta = _theta(pr)
    spec = _spec(pr["program"], 0 if theta is None else theta.numel())
    cdf, sf = ops.predict_cdf(_dev(pr["mu"]), _dev(pr["v"]), _dev(pr["lvn"]), Y.to(DEV), spec, _dev(theta), pr["S"], lik=L.LIK_BETA)
    return cdf.cpu(), sf.cpu()


def gpu_quantiles(pr, probs):
    from tgp.pytorch_amd import lib as L
    from tgp.pytorch_amd import ops
    theta = _theta(pr)
    spec = _spec(pr["program"], 0 if theta is None else theta.numel())
    t, status = ops.predict_quantiles(_dev(pr["mu"]), _dev(pr["v"]), _dev(pr["lvn"]), probs, spec, _dev(theta), pr["S"], check=False,
                                      lik=L.LIK_BETA)
    return t.cpu(), int(status[0])


@pytest.mark.parametrize("phi", PHIS)
@pytest.mark.parametrize("kind", KINDS)
def test_cdf_matches_reference(kind, phi):
    """cdf and sf at N in {1, 3, 5, 9} (four rows per workgroup) and S in {1, 15, 16, 17, 33} (16 lanes per row), targets from
    far in the lower tail to far in the upper one (logit y within 6 sqrt(4 / phi + v) of the flow's value: six widths of the
    row's predictive in the logit), each tail relative to itself, within 10x the CPU figure of phi; the two tails add up to sum wn; at S = 17 the same against mpmath itself; targets outside (0, 1)."""
    allow = 10.0 * RESIDUAL_CF_CPU[phi]
    worst = 0.0
    for N in (1, 3, 5, 9):
        for S in (1, 15, 16, 17, 33):
            pr = quant_problem(kind, N, S, phi, seed=N + S)
            g = torch.Generator().manual_seed(N * 100 + S)
            gm = BM.G(pr["mu"].reshape(1, -1), pr["program"], pr["theta"]).reshape(-1)
            Y = torch.sigmoid(gm + 6.0 * torch.sqrt(4.0 / phi + pr["v"]) * (2.0 * torch.rand(N, generator=g, dtype=F64) - 1.0))
            cdf, sf = gpu_cdf(pr, Y)
            gn = node_values(pr)
            for tails in (BM.tails_ref,) + ((BM.tails_mp,) if S == 17 and N <= 5 else ()):
                lo, up, _ = tails(gn, pr["wn"], phi, t=Y, want="lu")
                keep = torch.minimum(lo, up) > 1e-290
                err = torch.maximum((cdf - lo).abs() / lo, (sf - up).abs() / up)
                worst = max(worst, float(err[keep].max()) if bool(keep.any()) else 0.0)
                assert bool((err[keep] <= allow).all()), (kind, phi, N, S, tails.__name__, float(err[keep].max()))
            assert float((cdf + sf - float(pr["wn"].sum())).abs().max()) <= 1e-12
            assert bool(((cdf >= 0) & (sf >= 0)).all())
    print("%s phi = %g: worst relative error of a tail %.3e (allowance %.3e)" % (kind, phi, worst, allow))
    # targets on and outside the ends: nothing below 0, nothing above 1; a NaN stays one
    pr = quant_problem(kind, 7, 16, phi, seed=3)
    cdf, sf = gpu_cdf(pr, torch.tensor([0.0, -1.0, 1.0, 2.0, float("nan"), 1e-300, 0.5], dtype=F64))
    tot = float(pr["wn"].sum())
    assert cdf[:2].tolist() == [0.0, 0.0] and float((sf[:2] - tot).abs().max()) <= 1e-15
    assert sf[2:4].tolist() == [0.0, 0.0] and float((cdf[2:4] - tot).abs().max()) <= 1e-15
    assert math.isnan(float(cdf[4])) and math.isnan(float(sf[4]))
    assert 0.0 <= float(cdf[5]) < float(cdf[6]) < 1.0


# ---- 6. quantiles ---------------------------------------------------------------------------------------------------------
def _check_roots(pr, probs, label):
    phi = round(BM.precision_of(pr["lvn"]), 9)
    allow = 10.0 * RESIDUAL_CF_CPU[phi]
    t, failed = gpu_quantiles(pr, probs)
    assert failed == 0 and t.shape == (len(probs), pr["mu"].numel()) and bool(torch.isfinite(t).all())
    assert bool(((t > 0) & (t < 1)).all())
    r = worst_root_residual(pr, probs, t)
    print("residual %-30s %.3e   (allowance at phi = %g: %.3e)" % (label, r, phi, allow))
    assert r <= allow
    if len(probs) <= 3:                                                # mpmath itself where it is quick
        assert worst_root_residual(pr, probs, t, BM.tails_mp) <= allow
    # strictly increasing in p, row by row
    order = sorted(range(len(probs)), key=lambda i: probs[i])
    assert bool((t[order][1:] > t[order][:-1]).all())
    # against the restated rule's own roots, in x = logit t where both resolve it
    tc, failed_c, xc = BM.quantiles(pr["mu"], pr["v"], pr["lvn"], probs, pr["xs"], pr["wn"], pr["program"], pr["theta"], pr["rowp"])
    assert failed_c == 0
    inner = (tc > 1e-3) & (tc < 1.0 - 1e-3)
    assert float(((t - tc).abs() / tc)[inner].max() if bool(inner.any()) else 0.0) <= TOL_VAL
    return t


@pytest.mark.parametrize("kind,N,S,phi,probs", QUANT_CASES,
                         ids=["%s-N%d-S%d-phi%g-Q%d" % (k, n, s, a, len(q)) for k, n, s, a, q in QUANT_CASES])
def test_quantiles(kind, N, S, phi, probs):
    _check_roots(quant_problem(kind, N, S, phi, seed=N + S), probs, "%s-N%d-S%d-phi%g-Q%d" % (kind, N, S, phi, len(probs)))


@pytest.mark.parametrize("kind,phi", HARD_CASES, ids=["%s-phi%g" % c for c in HARD_CASES])
def test_hard_quantiles(kind, phi):
    """p = 1e-6 and 1 - 1e-6 at both ends of the precision range (the rows: test_beta_host.hard_problem)."""
    _check_roots(hard_problem(kind, phi), HARD_PROBS, "hard-%s-phi%g" % (kind, phi))


def test_repeats_are_bit_identical():
    from tgp.pytorch_amd import lib as L
    from tgp.pytorch_amd import ops
    pr = quant_problem("tanh3x2", 67, 33, 1000.0, seed=9)
    a, fa = gpu_quantiles(pr, [0.975, 0.025, 0.5])
    b, fb = gpu_quantiles(pr, [0.975, 0.025, 0.5])
    assert fa == 0 and fb == 0 and torch.equal(a, b)
    ca, sa = gpu_cdf(pr, a[0])
    cb, sb = gpu_cdf(pr, a[0])
    assert torch.equal(ca, cb) and torch.equal(sa, sb)
    pe = _inputs("sal2", 300, 32, 10.0)
    spec, lam = _spec(pe["program"], pe["theta"].numel()), _lam(10.0).to(DEV)
    ea = ops.ell_beta(pe["Y"].to(DEV), pe["mu"].to(DEV), pe["v"].to(DEV), lam, spec, _dev(pe["theta"]), 32, scale=2.0)
    eb = ops.ell_beta(pe["Y"].to(DEV), pe["mu"].to(DEV), pe["v"].to(DEV), lam, spec, _dev(pe["theta"]), 32, scale=2.0)
    for k in ("ell", "g_lvn", "g_mu", "g_v", "g_theta"):
        assert torch.equal(ea[k], eb[k]), k
    pa = ops.predict(pe["mu"].to(DEV), pe["v"].to(DEV), lam, spec, _dev(pe["theta"]), 32, Y=pe["Y"].to(DEV), lik=L.LIK_BETA)
    pb = ops.predict(pe["mu"].to(DEV), pe["v"].to(DEV), lam, spec, _dev(pe["theta"]), 32, Y=pe["Y"].to(DEV), lik=L.LIK_BETA)
    assert all(torch.equal(x, y) for x, y in zip(pa, pb))


def test_refusals_on_the_device():
    from tgp.pytorch_amd import lib as L
    from tgp.pytorch_amd import ops
    pr = quant_problem("sal2", 5, 16, 10.0, seed=1)
    Y = torch.full((5,), 0.5, dtype=F64, device=DEV)
    spec = _spec(pr["program"], pr["theta"].numel())
    with pytest.raises(L.TgpError, match="tgp_predict_crps_f64.*lik = 12"):
        md, keep = ops._flow_model(5, 16, spec, _dev(pr["theta"]), _dev(pr["lvn"]), torch.device(DEV), lik=L.LIK_BETA)
        out = torch.empty(5, dtype=F64, device=DEV)
        L.check(L.load().tgp_predict_crps_f64(md, L.ptr(_dev(pr["mu"])), L.ptr(_dev(pr["v"])), None, L.ptr(Y), L.ptr(out), None,
                                              L.stream_ptr()), "tgp_predict_crps_f64")
    with pytest.raises(L.TgpError, match="S = 257"):
        ops.predict_cdf(_dev(pr["mu"]), _dev(pr["v"]), _dev(pr["lvn"]), Y, spec, _dev(pr["theta"]), 257, lik=L.LIK_BETA)


# ---- 7. the model classes -------------------------------------------------------------------------------------------------
N_MODEL, M_MODEL, PHI_MODEL = 200, 10, 10.0


def _build_model(X, tgp=False, mean="zero", whiten=True, var_scale=None):
    from tgp.pytorch_amd import flows as G
    from tgp.pytorch_amd.kernels import instance_kernel
    from tgp.pytorch_amd.likelihoods import Beta
    from tgp.pytorch_amd.models import sparse_MF_GP, sparse_MF_SP
    D, M = X.shape[1], M_MODEL
    K = instance_kernel("scale_rbf", ard_num_dim=D, num_multioutput=1, kernel_is_shared=False,
                        init_params={"length_scale": 2.0, "kernel_scale": 0.3, "noisy_variance": 1e-6})
    ip = {"variational_distribution": {"variance_scale": 1e-5 if var_scale is None else var_scale, "mean_scale": 0.0}}
    lik = Beta(precision_init=PHI_MODEL)
    if tgp:
        model = sparse_MF_SP([mean, K], X, X[:M].clone(), X.shape[0], lik, 1, whiten, False, False, False, False,
                             [G.SAL(1)], "single", 0.0, init_params=ip)
    else:
        model = sparse_MF_GP([mean, K], X, X[:M].clone(), X.shape[0], lik, 1, whiten, False, False, False, False, 0.0,
                             init_params=ip)
    model = model.to(DEV)
    if var_scale is not None:
        return model
    gen = torch.Generator().manual_seed(11)
    mw = torch.randn(M, generator=gen, dtype=F64).to(DEV)
    Lw = (0.1 * torch.eye(M, dtype=F64) + 0.02 * torch.randn(M, M, generator=gen, dtype=F64).tril()).to(DEV)
    if not whiten:             # the same q(f): u = L_Z v, with L_Z the factor of K_ZZ (+ the kernel's 1e-6 on the diagonal)
        from tgp.pytorch_amd import ops
        cf = model.covariance_function
        Kzz = ops.kmm(model.Z.detach()[0], cf.base_kernel.raw_lengthscale.detach().reshape(-1), cf.raw_outputscale.detach().reshape(-1))
        Lz = torch.linalg.cholesky(Kzz + 1e-6 * torch.eye(M, dtype=F64, device=DEV))
        mw, Lw = Lz @ mw, Lz @ Lw
    with torch.no_grad():      # a q(u) away from its initial value
        model.q_U.variational_mean.data = mw.reshape(1, M)
        model.q_U.chol_variational_covar.data = Lw.reshape(1, M, M)
    return model


@pytest.fixture(scope="module")
def proportions():
    from tgp.pytorch_amd import synthetic
    X, Y = synthetic.synthetic_proportions()
    return torch.tensor(X[:N_MODEL], dtype=F64), torch.tensor(Y[:N_MODEL], dtype=F64)


def _flow_of(model):
    from tgp.pytorch_amd.flow import compile_flow
    spec, theta_list, _ = compile_flow(model.G_matrix[0])
    theta = torch.stack([q.detach().reshape(()) for q in theta_list]) if theta_list else None
    return spec, theta


def _rule(S):
    xs, ws = O.hermgauss(S)
    return xs, ws / math.sqrt(math.pi)


@pytest.mark.parametrize("tgp", [False, True], ids=["svgp", "tgp"])
def test_model_elbo_logp_and_quantiles(proportions, tgp):
    from tgp.pytorch_amd import ops
    X, Y = proportions
    model = _build_model(X, tgp=tgp)
    Xd, Yd = X.to(DEV), Y.to(DEV)
    model.set_is_training(True)
    elbo, ell, kld = model.ELBO(Xd, Yd)
    Z, rl, ro, m, Lam, lvn = (None if t is None else t.detach() for t in model._raw_params())
    assert lvn.data_ptr() == model.likelihood.log_precision.data_ptr()
    spec, theta = _flow_of(model)
    assert (spec.nblk > 0) == tgp
    S = model.quad_points
    mu, v = ops.qf_moments(Xd, Z, rl, ro, m, Lam, kernel="scale_rbf")
    lam = model.likelihood.log_precision.detach()
    kl = ops.kl_whitened(m, Lam)[0]
    xs, wn = _rule(S)
    prog = [tuple(int(q) for q in b) for b in spec.blocks]
    th = None if theta is None else theta.cpu()
    lam_c = lam.cpu().clone().requires_grad_(True)
    ref = BM.ell_torch(Y.reshape(-1), mu.cpu(), v.cpu(), lam_c, prog, th, xs, wn)
    gref, = torch.autograd.grad(ref, [lam_c])
    assert rel_err(ell.detach().cpu(), ref.detach()) < TOL_VAL and rel_err(kld.detach().cpu(), kl.cpu()) < TOL_VAL
    assert rel_err(elbo.detach().cpu(), ref.detach() - kl.cpu()) < TOL_VAL
    (-elbo).backward()
    assert all(q.grad is not None and torch.isfinite(q.grad).all() for q in model.parameters())
    gl = model.likelihood.log_precision.grad
    assert gl.shape == (1,) and rel_err(-gl.cpu(), gref) < TOL_GRAD and float(gl.abs()) > 0
    for bad in (0.0, 1.0, float("nan")):
        Yb = Yd.clone()
        Yb[7] = bad
        with pytest.raises(ValueError, match="proportions"):
            model.ELBO(Xd, Yb)

    model.set_is_training(False)
    n = 50
    lp_sum, (m1, m2) = model.test_log_likelihood(Xd[:n], Yd[:n], return_moments=True, Y_std=2.5 * torch.ones(1, device=DEV))
    r1, r2, rlp = BM.pred_torch(mu[:n].cpu(), v[:n].cpu(), lam.cpu(), prog, th, xs, wn, Y=Y[:n].reshape(-1))
    assert m1.shape == (1, n) and m2.shape == (1, n)
    assert rel_err(lp_sum.cpu(), rlp.sum()) < TOL_VAL                              # Y_std is ignored
    assert rel_err(m1.reshape(-1).cpu(), r1) < TOL_VAL and rel_err(m2.reshape(-1).cpu(), r2) < TOL_VAL
    # exact quantiles, the CDF back, the interval score
    probs = [0.975, 0.025, 0.5]
    q = model.predictive_quantiles(Xd[:n], probs)
    assert q.shape == (1, 3, n) and q.is_cuda and bool((q[0, 1] < q[0, 2]).all()) and bool((q[0, 2] < q[0, 0]).all())
    assert bool(((q > 0) & (q < 1)).all())
    pr = {"mu": mu[:n].cpu(), "v": v[:n].cpu(), "lvn": lam.cpu(), "program": prog, "theta": th if th is not None else torch.zeros(0, dtype=F64),
          "rowp": None, "xs": xs, "wn": wn, "S": S}
    assert worst_root_residual(pr, probs, q[0].cpu()) <= 10.0 * RESIDUAL_CF_CPU[10.0]
    gn = node_values(pr)
    for qi, p in enumerate(probs):
        pit = model.predictive_cdf(Xd[:n], q[0, qi].reshape(-1, 1))
        assert pit.shape == (1, n) and float((pit.cpu() - p).abs().max()) <= 1e-9
    lo, up, _ = BM.tails_ref(gn, wn, PHI_MODEL, t=Y[:n].reshape(-1))
    pit = model.predictive_cdf(Xd[:n], Yd[:n])
    assert float(((pit[0].cpu() - lo).abs() / lo).max()) <= 10.0 * RESIDUAL_CF_CPU[10.0]
    isc = model.predictive_interval_score(Xd[:n], Yd[:n], alpha=0.05)
    want = ops.interval_score(q[0, 1], q[0, 0], Yd[:n].reshape(-1), 0.05)
    assert isc.shape == (1, n) and torch.equal(isc[0], want)
    # the CRPS: no closed pair term, the sampled estimator works; no pmf
    with pytest.raises(NotImplementedError, match="no closed pair term"):
        model.predictive_crps(Xd[:n], Yd[:n])
    torch.manual_seed(0)
    crps = model.predictive_crps(Xd[:n], Yd[:n], samples=200)
    assert crps.shape == (1, n) and bool(torch.isfinite(crps).all()) and bool((crps > 0).all())
    with pytest.raises(NotImplementedError, match="predictive_pmf"):
        model.predictive_pmf(Xd[:n], 5)
    s, _, _ = model.sample_from_predictive_distribution(Xd[:n], S=4)
    assert s.shape == (1, 4, n, 1) and bool(((s >= 0) & (s <= 1)).all())
    # a precision that has left the range
    with torch.no_grad():
        model.likelihood.log_precision.fill_(math.log(0.1))
    for call in (lambda: model.predictive_quantiles(Xd[:n], [0.5]), lambda: model.predictive_cdf(Xd[:n], Yd[:n]),
                 lambda: model.predictive_interval_score(Xd[:n], Yd[:n])):
        with pytest.raises(ValueError, match=r"\[0\.5, 1000\]"):
            call()


@pytest.mark.parametrize("variant", ["linear-mean", "unwhitened"])
def test_model_variants_match_the_restatement(proportions, variant):
    X, Y = proportions
    Xd, Yd = X.to(DEV), Y.to(DEV)
    model = _build_model(X, mean="linear" if variant == "linear-mean" else "zero", whiten=variant != "unwhitened")
    if variant == "linear-mean":
        with torch.no_grad():
            model.mean_function.a.data.copy_(torch.tensor([0.2, -0.1], dtype=F64).reshape(model.mean_function.a.shape))
            model.mean_function.b.data.fill_(0.3)
    model.set_is_training(True)
    elbo, ell, kld = model.ELBO(Xd, Yd)
    (-elbo).backward()
    gl = model.likelihood.log_precision.grad
    assert gl is not None and torch.isfinite(gl).all() and float(gl.abs()) > 0
    if variant == "linear-mean":
        ga = model.mean_function.a.grad
        assert ga is not None and torch.isfinite(ga).all() and float(ga.abs().max()) > 0
    with torch.no_grad():
        mu, v = model.marginal_variational_qf_parameters(Xd, diagonal=True, is_duvenaud=False)
        kl = model.KLD().sum()
    xs, wn = _rule(model.quad_points)
    lam = model.likelihood.log_precision.detach().cpu().clone().requires_grad_(True)
    ref = BM.ell_torch(Y.reshape(-1), mu.reshape(-1).cpu(), v.reshape(-1).cpu(), lam, [], None, xs, wn)
    gref, = torch.autograd.grad(ref, [lam])
    assert rel_err(ell.detach().cpu(), ref.detach()) < TOL_VAL
    assert rel_err(kld.detach().cpu(), kl.cpu()) < TOL_VAL and rel_err(elbo.detach().cpu(), ref.detach() - kl.cpu()) < TOL_VAL
    assert rel_err(-gl.cpu(), gref) < TOL_GRAD


@pytest.mark.parametrize("tgp", [False, True], ids=["svgp", "tgp"])
def test_one_natgrad_step_is_finite(proportions, tgp):
    """natgrad_step_qu(lr = 0.5) with its default floor from q(u) = N(0, I): finite `info` and a finite ELBO afterwards.  The Beta
    likelihood is not log-concave in g (d2/dg2 changes sign with y* - psi(a) + psi(b)), so no increase is asserted."""
    X, Y = proportions
    Xd, Yd = X.to(DEV), Y.to(DEV)
    model = _build_model(X, tgp=tgp, var_scale=1.0)
    before = float(model.ELBO(Xd, Yd)[0].detach())
    info = model.natgrad_step_qu(Xd, Yd, lr=0.5)
    after = float(model.ELBO(Xd, Yd)[0].detach())
    print("ELBO", before, "->", after, info)
    assert math.isfinite(before) and math.isfinite(after)
    assert all(math.isfinite(float(x)) for x in info.values() if isinstance(x, (int, float)) or torch.is_tensor(x) and x.numel() == 1)


def test_exact_intervals_bracket_the_sampled_ones(proportions):
    """compute_95_and_median_confidence_intervals(exact=True) against exact=False at S = 2000 samples on synthetic_proportions:
    six standard errors of a sample quantile, 6 sqrt(p (1 - p) / S) / F'(t_exact), on rows near the inducing inputs -- the rule
    of tests/test_gpu_quantiles.py, F' (in t) from the package's own CDF entry."""
    from tgp.pytorch_amd import utils
    X, _ = proportions
    model = _build_model(X, tgp=True)
    model.set_is_training(False)
    g = torch.Generator().manual_seed(3)
    Z = model.Z.detach()[0].cpu()
    Xn = (Z[torch.arange(24) % Z.shape[0]] + 0.05 * torch.randn(24, Z.shape[1], generator=g, dtype=F64)).to(DEV)
    S = 2000
    torch.manual_seed(11)
    exact = utils.compute_95_and_median_confidence_intervals(model, Xn, S, "predictive", False, exact=True)
    sampled = utils.compute_95_and_median_confidence_intervals(model, Xn, S, "predictive", False)
    t = torch.tensor(np.stack([a[:, 0] for a in exact[0]]))
    for qi, p in enumerate((0.025, 0.5, 0.975)):
        Yq = t[qi].to(DEV)
        h = 1e-6 * torch.minimum(Yq, 1.0 - Yq)
        d = (model.predictive_cdf(Xn, (Yq + h).reshape(-1, 1)) - model.predictive_cdf(Xn, (Yq - h).reshape(-1, 1)))[0].cpu() / (2 * h.cpu())
        bound = 6.0 * math.sqrt(p * (1.0 - p) / S) / d
        diff = (t[qi] - torch.tensor(sampled[0][qi][:, 0])).abs()
        print("exact vs sampled p=%.3f: worst |diff| / bound %.3f" % (p, float((diff / bound).max())))
        assert bool((diff <= bound).all()), p


# ---- 8. the CLI -----------------------------------------------------------------------------------------------------------
CLI = ["--model", "TGP", "--likelihood", "beta", "--dataset", "synthetic_proportions", "--train_test_seed_split", "1",
       "--num_inducing", "10", "--epochs", "5", "--coverage", "exact"]
NUM = r"(-?(?:\d+\.\d+|nan|inf))"


def test_cli():
    """The command line in a child process, 5 epochs with --coverage exact: exit 0, finite NLL, RMSE, coverage and precision, the
    baseline's line, and no fall-back to the sampled coverage."""
    r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, "-m", "tgp.pytorch_amd.main"] + CLI, cwd=REPO,
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "sampled coverage instead" not in r.stdout
    line = re.search(r"model TGP, Test Negative LOGL %s, Test RMSE %s" % (NUM, NUM), r.stdout)
    cov = re.search(r"Test coverage \(95%%, exact\) %s" % NUM, r.stdout)
    prc = re.search(r"learned precision %s \(true precision 10\.000\)" % NUM, r.stdout)
    base = re.search(r"constant Beta \(mean %s, precision %s\), Test Negative LOGL %s, Test RMSE %s" % (NUM, NUM, NUM, NUM), r.stdout)
    assert line and cov and prc and base, r.stdout[-2000:]
    vals = [float(line.group(1)), float(line.group(2)), float(cov.group(1)), float(prc.group(1))] + [float(x) for x in base.groups()]
    assert all(math.isfinite(x) for x in vals) and 0.0 <= vals[2] <= 1.0 and vals[3] > 0
