"""CPU: the posterior derivative above the kernels -- the torch restatement (tests/derivative_model.py) of the slope variance and
of the draws' input gradients against torch autograd, the deterministic link between the two, the ABI's three symbols and their
refusals (before any device is touched), the hosts' refusals, utils.slope_significance and the CLI flag."""
import ctypes
import os
import re
import subprocess
import sys

import pytest
import torch

from conftest import REPO

import derivative_model as DM
import input_grad_model as IG
import pathwise_model as PM
from oracle import tgp_oracle as orc
from tgp.pytorch_amd import lib as L

F64 = torch.float64
TOL = 1e-12          # the issue's bound on a restatement against autograd (measured: dvar 2e-15 .. 2e-14 in the posterior part, 0 .. 1e-16 in the prior part; draw gradient 3e-16 .. 9e-16)
RQ_ALPHA = 2.0
SAME_ROW = (7, 11)   # row 7 of X is row 11 of Z bit for bit


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


def _problem(N=65, D=4, M=20):
    prob = orc.synthetic_problem(N, D, M, seed=3, flow=None, S=8)
    X = prob["X"].clone()
    X[SAME_ROW[0]] = prob["params"]["Z"][SAME_ROW[1]]
    p = prob["params"]
    return X, (p["Z"], p["raw_lengthscale"], p["raw_outputscale"], p["m"], p["Lam"])


def _mixed(fn, X):
    """(N, D): d^2 fn(x1, x2)_n / dx1_nd dx2_nd at x1 = x2 = X, fn row-wise."""
    x1, x2 = X.clone().requires_grad_(True), X.clone().requires_grad_(True)
    g1, = torch.autograd.grad(fn(x1, x2).sum(), x1, create_graph=True)
    out = torch.empty_like(X)
    for d in range(X.shape[1]):
        out[:, d] = torch.autograd.grad(g1[:, d].sum(), x2, retain_graph=True)[0][:, d]
    return out


@pytest.mark.parametrize("kernel", IG.KERNELS)
def test_slope_variance_is_the_mixed_second_derivative(kernel):
    X, (Z, rl, ro, m, Lam) = _problem()
    alpha = RQ_ALPHA if kernel == "scale_rq" else None
    jit = 1e-6
    post = DM.posterior_slope_var(X, Z, rl, ro, Lam, jit, kernel, alpha)
    post_ref = _mixed(lambda a, b: DM.rowwise_cov_posterior(a, b, Z, rl, ro, Lam, jit, kernel, alpha), X)
    e_post = _rel(post, post_ref)
    prior = DM.prior_slope_var(rl, ro, kernel)
    e_prior = []
    if kernel in ("scale_rbf", "scale_rq"):          # smooth in d2 at 0: autograd takes both derivatives of k itself
        e_prior.append(_rel(prior.expand_as(X), _mixed(lambda a, b: DM.rowwise_cov_prior(a, b, rl, ro, kernel, alpha), X)))
    if kernel != "scale_matern32":                   # the restated first derivative, differentiated in x' by autograd
        x2 = X.clone().requires_grad_(True)
        ref = torch.stack([torch.autograd.grad(DM.rowwise_slope_prior(X, x2, rl, ro, kernel, alpha)[:, d].sum(), x2)[0][:, d]
                           for d in range(X.shape[1])], 1)
        e_prior.append(_rel(prior.expand_as(X), ref))
    else:                                            # its second derivative at coincident points is not autograd's to take
        s2, l = torch.nn.functional.softplus(ro.reshape(-1)[0]), torch.nn.functional.softplus(rl.reshape(-1))
        e_prior.append(_rel(prior, 3.0 * s2 / (l * l)))
    print("dvar %s: posterior part %.2e, prior part %s (bound %.0e)" % (kernel, e_post, " ".join("%.2e" % e for e in e_prior), TOL))
    assert e_post <= TOL and max(e_prior) <= TOL
    dvar = DM.slope_var(X, Z, rl, ro, m, Lam, jit, kernel, alpha)
    assert dvar.shape == X.shape and torch.equal(dvar, prior.reshape(1, -1) + post) and bool(torch.isfinite(dvar).all())
    # the coincident pair contributes an exact zero column of J
    assert float(IG.kernel_jacobian(X, Z, rl, ro, kernel, alpha)[SAME_ROW[0], SAME_ROW[1]].abs().max()) == 0.0
    # q(u) = the prior (Lam = I): W = 0, the slope variance is the prior's
    eye = torch.eye(Z.shape[0], dtype=F64)
    assert torch.equal(DM.slope_var(X, Z, rl, ro, m, eye, jit, kernel, alpha), prior.reshape(1, -1).expand_as(X).clone())


@pytest.mark.parametrize("D", (1, 4))
@pytest.mark.parametrize("kind", PM.KINDS)
def test_draw_gradient_is_autograd_of_the_draw(kind, D):
    p = PM.make_case(17, D, 16, 15, 3, kind)
    coef = PM.coeff(p)
    Xg = p["X"].clone().requires_grad_(True)
    F0 = PM.evaluate(p, coef, Xg)                               # (S, N): each value depends on its row only
    ref = torch.stack([torch.autograd.grad(F0[s].sum(), Xg, retain_graph=True)[0] for s in range(F0.shape[0])])
    g = DM.draw_grad(p, coef)
    e = _rel(g, ref)
    print("draw gradient %s D=%d: %.2e (bound %.0e)" % (kind, D, e, TOL))
    assert g.shape == (3, 17, D) and e <= TOL


@pytest.mark.parametrize("kind", PM.KINDS)
def test_link_between_the_draws_and_the_slope_variance(kind):
    """Deterministic: the slope variance of the draws is that of q(f) up to the Fourier approximation of the prior."""
    gaps = {R2: DM.link_gap(DM.link_case(kind, R2)) for R2 in (256, 2048)}
    print("link %s: gap %.3e at R2 = 256, %.3e at R2 = 2048 (recorded %.3e, %.3e)"
          % (kind, gaps[256], gaps[2048], DM.LINK_GAP_CPU[(kind, 256)], DM.LINK_GAP_CPU[(kind, 2048)]))
    assert gaps[2048] < gaps[256]
    for R2, gap in gaps.items():
        rec = DM.LINK_GAP_CPU[(kind, R2)]
        assert rec / 2.0 <= gap <= 2.0 * rec, (R2, gap, rec)


def test_abi_declares_the_entries():
    hdr = open(os.path.join(REPO, "include", "tgp_hip.h")).read()
    for name in ("tgp_qf_input_grad_var_workspace_bytes", "tgp_qf_input_grad_var_f64", "tgp_pathwise_grad_f64"):
        assert re.search(r"\b%s\(" % name, hdr), name
        assert name in L.EXPORTS
        assert getattr(L.load(), name).argtypes is not None
    f = L.load().tgp_qf_input_grad_var_workspace_bytes
    rows = L.XGRAD_PASS_ROWS
    # sized for min(N, TGP_XGRAD_PASS_ROWS) rows, and not for D: one dimension's operands at a time
    assert f(rows, 4, 100) == f(rows + 1, 4, 100) == f(100 * rows, 16, 100) > f(rows - 128, 4, 100) > 0


def test_library_refusals_before_any_device():
    """Each refusal comes before a pointer is read: the arrays are host memory."""
    h = L.load()
    buf = torch.zeros(16, dtype=F64)
    st = torch.zeros(8, dtype=torch.int32)
    p, ps = ctypes.c_void_p(buf.data_ptr()), ctypes.c_void_p(st.data_ptr())

    def model(N=10, D=4, M=5, kernel=L.KERNEL_SCALE_RBF):
        md = L.TgpModel()
        md.N, md.D, md.M, md.S, md.kernel = N, D, M, 1, kernel
        md.Z = md.raw_ls = md.raw_os = md.m = md.Lam = md.log_var_noise = p
        return md

    entry = b"tgp_qf_input_grad_var_f64"
    unknown = 2                                                      # (2 and 4 are not assigned)
    rc = h.tgp_qf_input_grad_var_f64(model(kernel=unknown), p, p, ps, p, 1 << 40, None)
    assert rc == L.E_UNSUPPORTED and h.tgp_last_error().startswith(entry) and b"kernel = %d" % unknown in h.tgp_last_error()
    for kw in ({"D": 17}, {"M": L.BIG_MAX_M + 1}, {"D": 0}, {"M": 0}, {"N": 0}):
        rc = h.tgp_qf_input_grad_var_f64(model(**kw), p, p, ps, p, 1 << 40, None)
        assert rc == L.E_UNSUPPORTED and h.tgp_last_error().startswith(entry), kw
        assert h.tgp_qf_input_grad_var_workspace_bytes(kw.get("N", 10), kw.get("D", 4), kw.get("M", 5)) == 0
    need = h.tgp_qf_input_grad_var_workspace_bytes(10, 4, 5)
    rc = h.tgp_qf_input_grad_var_f64(model(), p, p, ps, p, need - 1, None)
    assert rc == L.E_WORKSPACE and h.tgp_last_error().startswith(entry) and str(need).encode() in h.tgp_last_error()
    args = [model(), p, p, ps, p, need, None]
    for pos, code in ((1, -2), (2, -3), (3, -4), (4, -5)):         # null pointers in the house order
        a = list(args)
        a[pos] = None
        assert h.tgp_qf_input_grad_var_f64(*a) == code, pos
    assert h.tgp_qf_input_grad_var_f64(None, *args[1:]) == -1
    md = model()
    md.Lam = None
    assert h.tgp_qf_input_grad_var_f64(md, *args[1:]) == -1

    entry = b"tgp_pathwise_grad_f64"
    good = dict(kernel=L.KERNEL_SCALE_RBF, N=10, D=4, M=5, R2=8, S=3)

    def call(**kw):
        a = dict(good, **kw)
        return h.tgp_pathwise_grad_f64(a["kernel"], p, a["N"], a["D"], p, a["M"], p, p, p, a["R2"], p, a["S"], p, None)
    for kw in ({"kernel": unknown}, {"N": 0}, {"D": 0}, {"D": 17}, {"M": 0}, {"M": L.BIG_MAX_M + 1}, {"R2": 0},
               {"R2": L.PATHWISE_MAX_R2 + 1}, {"S": 0}, {"S": L.PATHWISE_MAX_S + 1}):
        assert call(**kw) == L.E_UNSUPPORTED and h.tgp_last_error().startswith(entry), kw
    args = [good["kernel"], p, good["N"], good["D"], p, good["M"], p, p, p, good["R2"], p, good["S"], p, None]
    for pos in (1, 4, 6, 7, 8, 10, 12):                             # a null pointer: the negative index of its argument
        a = list(args)
        a[pos] = None
        assert h.tgp_pathwise_grad_f64(*a) == -(pos + 1), pos


def _model(kind, D=3, M=5):
    from tgp.pytorch_amd import config as cg
    from tgp.pytorch_amd.flows import SAL
    from tgp.pytorch_amd.kernels import instance_kernel
    from tgp.pytorch_amd.likelihoods import GaussianNonLinearMean
    from tgp.pytorch_amd.models import sparse_MF_SP
    cg.set_maximum_precission()
    X = torch.randn(30, D, dtype=F64)
    K = instance_kernel("scale_rbf", ard_num_dim=D, num_multioutput=1, kernel_is_shared=False,
                        init_params={"length_scale": 2.0, "kernel_scale": 2.0, "noisy_variance": 1e-6})
    lik = GaussianNonLinearMean(1, 0.05, False, 20)
    if kind == "idtgp":
        from tgp.pytorch_amd.flow import instance_flow
        flow = instance_flow(SAL(1, input_dependent=True, input_dim=D, num_hidden_layers=1, batch_norm=0, dropout=0.5, hidden_dim=8,
                                 hidden_activation="tanh", inference="MC_dropout"))
        flow.turn_off_initializer_parameters()
    else:
        flow = SAL(1)
    return sparse_MF_SP(["zero", K], X, X[:M].clone(), 30, lik, 1, True, False, False, False, False, [flow], "single", 0.0), X


def test_host_refusals_name_the_reason():
    from tgp.pytorch_amd import ops
    from tgp.pytorch_amd.pathwise import PosteriorPaths
    from tgp.pytorch_amd.utils import slope_significance
    old = torch.get_default_dtype()
    try:
        model, X = _model("tgp")
        with pytest.raises(L.TgpError, match="GPU only"):           # (no CPU fall-back behind the new method)
            model.posterior_derivative(X)
        with pytest.raises(L.TgpError, match="GPU only"):
            slope_significance(model, X)
        with pytest.raises(ValueError, match="batch_rows"):
            slope_significance(model, X, batch_rows=0)
        with pytest.raises(ValueError, match="z >= 0"):
            slope_significance(model, X, z=-1.0)
        # a flow with per-row networks: refused before anything is launched (host tensors throughout)
        idm, _ = _model("idtgp")
        D, M, R2, S = 3, 5, 4, 2
        paths = PosteriorPaths(torch.zeros(M, D, dtype=F64), torch.zeros(D, dtype=F64), torch.zeros(1, dtype=F64),
                               torch.zeros(R2, D, dtype=F64), torch.zeros(2 * R2 + M, S, dtype=F64), "scale_rbf", None,
                               idm.G_matrix[0])
        with pytest.raises(NotImplementedError, match="depend on x through the networks"):
            paths.grad(X)
        with pytest.raises(ValueError, match=r"X \(N, 3\)"):
            paths.grad_f0(torch.zeros(4, 2, dtype=F64))
        with pytest.raises(ValueError, match="pathwise_grad"):
            ops.pathwise_grad(torch.zeros(4, 3, dtype=F64), torch.zeros(M, 2, dtype=F64), torch.zeros(3, dtype=F64),
                              torch.zeros(1, dtype=F64), torch.zeros(R2, 3, dtype=F64), torch.zeros(2 * R2 + M, S, dtype=F64))
    finally:
        torch.set_default_dtype(old)


class _HandMade:
    """posterior_derivative from a table: rows of (mean, var) by position."""

    def __init__(self, mean, var, X):
        self.mean, self.var, self.X, self.calls = mean, var, X, []

    def posterior_derivative(self, Xp):
        r0 = int((self.X[:, 0] == Xp[0, 0]).nonzero()[0])
        self.calls.append(Xp.shape[0])
        return self.mean[:, r0:r0 + Xp.shape[0]], self.var[:, r0:r0 + Xp.shape[0]]


def test_slope_significance_on_a_hand_made_posterior():
    from tgp.pytorch_amd.utils import slope_significance
    X = torch.arange(5, dtype=F64).reshape(5, 1).repeat(1, 3)
    #            input 0: always significant;  input 1: never;  input 2: rows 0, 3 only (row 4: a negative variance counts as 0)
    mean = torch.tensor([[[2.0, 0.1, 2.0], [-2.0, 0.1, 1.9], [3.0, -0.1, -1.0], [2.5, 0.0, -2.0], [2.0, 1.0, 0.0]]], dtype=F64)
    var = torch.tensor([[[1.0, 1.0, 1.0], [1.0, 1.0, 1.0], [1.0, 1.0, 1.0], [1.0, 1.0, 1.0], [1.0, 1.0, -1e-18]]], dtype=F64)
    model = _HandMade(mean, var, X)
    out = slope_significance(model, X)
    assert out.shape == (3,) and out.tolist() == [1.0, 0.0, 0.4] and model.calls == [5]
    model.calls = []
    assert torch.equal(slope_significance(model, X, batch_rows=2), out) and model.calls == [2, 2, 1]
    assert slope_significance(model, X, z=0.0).tolist() == [1.0, 0.8, 0.8]        # |mean| > 0: the two exact zeros are not
    assert slope_significance(model, X, z=0.95).tolist() == [1.0, 0.2, 0.8]
    two = _HandMade(mean.repeat(2, 1, 1), var.repeat(2, 1, 1), X)
    with pytest.raises(NotImplementedError, match="one latent GP"):
        slope_significance(two, X)


def test_cli_slope_significance():
    run = lambda *a: subprocess.run([sys.executable, "-m", "tgp.pytorch_amd.main"] + list(a), cwd=REPO, capture_output=True,
                                    text=True, timeout=120)
    out = run("--help")
    assert out.returncode == 0 and "--slope_significance" in out.stdout and "--relevance" in out.stdout
    bad = run("--model", "SVGP", "--likelihood", "poisson", "--slope_significance", "--dataset", "synthetic_counts",
              "--train_test_seed_split", "1", "--num_inducing", "5")
    assert bad.returncode == 2 and "--slope_significance: SVGP or TGP with --likelihood gaussian only" in bad.stderr
    bad = run("--model", "ID_TGP", "--slope_significance", "--dataset", "synthetic_power", "--train_test_seed_split", "1",
              "--num_inducing", "5")
    assert bad.returncode == 2 and "--slope_significance" in bad.stderr
