"""CPU: the acquisition functions above the kernel -- the branches of log h against mpmath, the torch restatement
(tests/acquisition_model.py) against an independent integral of the Gaussian mixture and against its own central differences,
utils.suggest_candidates' best-seen rule on a stand-in model, the ABI's symbol and the library's refusals (before any device is
touched)."""
import ctypes
import math
import os
import re

import pytest
import torch

from conftest import REPO

import acquisition_model as AM
from oracle import tgp_oracle as orc
from tgp.pytorch_amd import lib as L

F64 = torch.float64
Z_GRID = (10.0, 5.0, 1.0, 0.0, -0.5, -1.0, -2.0, -5.0, -10.0, -20.0, -29.9, -30.0, -30.1, -50.0, -100.0, -300.0, -1e3, -1e4, -1e5)
# DESIGN.md section 8, "Acquisition functions": the largest relative errors found on Z_GRID against mpmath at 60 digits with
# the branch points of acquisition_model (Z_DIRECT = -1, Z_SERIES = -30); the test allows 10 x what is recorded there.
LOGH_RECORDED = 1.3e-15
RATIO_RECORDED = 2.6e-13


def _design_record(name):
    text = open(os.path.join(REPO, "DESIGN.md")).read()
    m = re.search(r"%s\s*=\s*([0-9.]+e-[0-9]+)" % re.escape(name), text)
    assert m, "DESIGN.md does not record %s" % name
    return float(m.group(1))


def test_log_h_against_mpmath():
    """log h and Phi / h on the issue's grid: relative error against 60-digit arithmetic, each <= 10 x the figure DESIGN.md records."""
    import mpmath                                                # (no skip: the bound must not vanish where the package is absent)
    assert _design_record("max_rel_err_log_h") == LOGH_RECORDED and _design_record("max_rel_err_Phi_over_h") == RATIO_RECORDED
    assert (AM.Z_DIRECT, AM.Z_SERIES) == (-1.0, -30.0)          # the branch points the recorded figures belong to
    mpmath.mp.dps = 60
    z = torch.tensor(Z_GRID, dtype=F64)
    logh, ratio, _, _ = AM.log_h(z)
    worst_l = worst_r = 0.0
    for i, zi in enumerate(Z_GRID):
        zz = mpmath.mpf(zi)
        Phi = mpmath.ncdf(zz)
        h = zz * Phi + mpmath.npdf(zz)
        el = abs((mpmath.mpf(float(logh[i])) - mpmath.log(h)) / mpmath.log(h))
        er = abs((mpmath.mpf(float(ratio[i])) - Phi / h) / (Phi / h))
        print("z = %10g: log h %.17g rel %.2e   Phi/h %.17g rel %.2e" % (zi, float(logh[i]), float(el), float(ratio[i]), float(er)))
        worst_l, worst_r = max(worst_l, float(el)), max(worst_r, float(er))
    print("largest: log h %.3e, Phi/h %.3e" % (worst_l, worst_r))
    assert worst_l <= 10.0 * LOGH_RECORDED
    assert worst_r <= 10.0 * RATIO_RECORDED


def _case(flow, S, N=3):
    prob = orc.synthetic_problem(8, 2, 4, seed=5, flow=flow, S=S)
    g = torch.Generator().manual_seed(17)
    mu = torch.randn(N, generator=g, dtype=F64)
    v = 0.05 + torch.rand(N, generator=g, dtype=F64)
    xs, ws = orc.hermgauss(S)
    return mu, v, prob["program"], prob["params"]["theta"], xs, ws / math.sqrt(math.pi)


@pytest.mark.parametrize("c", (1.0, -1.0))
@pytest.mark.parametrize("S", (8, 32))
@pytest.mark.parametrize("flow", ("sal2", "tanh3x2"))
def test_ei_and_pi_against_an_independent_integral(flow, S, c):
    """EI = int (c (y - b))_+ p(y) dy and PI = the mass beyond b under p(y) = sum_s wn_s N(y | g_s, sigma^2), by adaptive
    quadrature of the explicit mixture density.  Bound: quad's own error estimate plus 1e-12."""
    from scipy.integrate import quad
    mu, v, program, theta, xs, wn = _case(flow, S)
    lvn = torch.log(torch.tensor([0.05], dtype=F64))
    sigma = math.sqrt(0.05)
    g = AM.nodes(mu, v, xs, program, theta)
    for n in range(mu.numel()):
        gn = [float(t) for t in g[:, n]]
        best = float((wn * g[:, n]).sum()) + 0.3 * c                      # an incumbent a little better than the mean
        ei = float(AM.acquisition(mu, v, lvn, "ei", best, c, xs, wn, program, theta)[n])
        pi = float(AM.acquisition(mu, v, lvn, "pi", best, c, xs, wn, program, theta)[n])

        def dens(y):
            return sum(float(w) * math.exp(-0.5 * ((y - gs) / sigma) ** 2) for w, gs in zip(wn, gn)) / (sigma * math.sqrt(2.0 * math.pi))
        lo, hi = (best, max(gn) + 12.0 * sigma) if c > 0 else (min(gn) - 12.0 * sigma, best)     # (beyond 12 sigma: < 1e-32)
        if hi <= lo:
            hi = lo
        pts = sorted(t for t in gn if lo < t < hi)
        kw = dict(points=pts or None, limit=400, epsabs=1e-15, epsrel=1e-14)
        ei_q, ei_e = quad(lambda y: c * (y - best) * dens(y), lo, hi, **kw)
        pi_q, pi_e = quad(dens, lo, hi, **kw)
        print("%s S=%d c=%+d row %d: EI %.15g quad %.15g (est %.1e)  PI %.15g quad %.15g (est %.1e)"
              % (flow, S, c, n, ei, ei_q, ei_e, pi, pi_q, pi_e))
        assert abs(ei - ei_q) <= ei_e + 1e-12
        assert abs(pi - pi_q) <= pi_e + 1e-12


@pytest.mark.parametrize("c", (1.0, -1.0))
@pytest.mark.parametrize("kind", AM.KINDS)
@pytest.mark.parametrize("flow", ("sal2", "tanh3x2", None))
def test_partials_against_central_differences(flow, kind, c):
    """The partials in mu and v against central differences of the restatement's own value, step h = 1e-6, at a noise of
    sigma = 2 and an incumbent 0.3 sigma beyond each row's predictive mean (so that every partial is of the order of its value).
    The error of such a difference is h^2 |f'''| / 6 + eps |f| / h.  Each derivative in mu brings a factor of at most
    max G' / sigma (75 / 2 for the steepest program here, tanh 3 x 2), so |f'''| <= 5.3e4 |f| and the first term is below
    1e-8 |f|; the second is 2.2e-10 |f|; |f| <= 10 max |partial| over these cases.  The bound is 1e-7 of the largest partial."""
    TOL_FD = 1e-7
    S = 32
    mu, v, program, theta, xs, wn = _case(flow or "sal2", S, N=7)
    if flow is None:
        program = []
    v[3] = 0.0
    lvn = torch.log(torch.tensor([4.0], dtype=F64))
    m1 = mu if flow is None else (wn.reshape(-1, 1) * AM.nodes(mu, v, xs, program, theta)).sum(0)
    best = m1 + 0.6 * c
    args = (xs, wn, program, theta)
    val, part = AM.acquisition(mu, v, lvn, kind, best, c, *args, want_partials=True)
    plain = AM.acquisition(mu, v, lvn, kind, best, c, *args)
    assert float((val - plain).abs().max()) <= 1e-13 * float(plain.abs().max())      # (two statements of the flow)
    assert bool((val.abs().max() <= 10.0 * part.abs().max()))
    h = 1e-6
    fd_mu = (AM.acquisition(mu + h, v, lvn, kind, best, c, *args) - AM.acquisition(mu - h, v, lvn, kind, best, c, *args)) / (2.0 * h)
    fd_v = (AM.acquisition(mu, v + h, lvn, kind, best, c, *args) - AM.acquisition(mu, v - h, lvn, kind, best, c, *args)) / (2.0 * h)
    keep = v > 0.0
    e_mu = float((part[0] - fd_mu).abs().max() / part.abs().max())
    e_v = float((part[1] - fd_v)[keep].abs().max() / part.abs().max())
    print("%s %s c=%+d: mu %.2e v %.2e" % (flow, kind, c, e_mu, e_v))
    assert e_mu <= TOL_FD and e_v <= TOL_FD
    assert float(part[1, 3]) == 0.0                              # v = 0: an exact zero in the v row


class _Toy:
    """A stand-in model: a concave acquisition surface -(x - x0)^2 summed over the inputs, any kind."""

    def __init__(self, x0):
        self.x0 = torch.as_tensor(x0, dtype=F64)
        self.calls = 0

    def acquisition(self, X, kind="log_ei", best=None, maximize=True, beta=2.0, return_grad=False):
        self.calls += 1
        d = X - self.x0
        val = -(d * d).sum(1)
        return (val, -2.0 * d) if return_grad else val


def test_suggest_candidates_best_seen_rule():
    from tgp.pytorch_amd import utils
    bounds = torch.tensor([[-1.0, 0.0, 2.0], [1.0, 3.0, 5.0]], dtype=F64)
    toy = _Toy([0.3, 1.7, 6.0])                                  # the third coordinate's optimum lies outside the box
    starts = bounds[0] + torch.rand(9, 3, generator=torch.Generator().manual_seed(2), dtype=F64) * (bounds[1] - bounds[0])
    best_start = float(toy.acquisition(starts).max())
    x, val, finals = utils.suggest_candidates(toy, bounds, kind="log_ei", best=0.0, starts=starts, steps=30)
    assert toy.calls == 1 + 31                                   # one batch per step, every start in it
    assert x.shape == (3,) and finals["X"].shape == (9, 3) and finals["value"].shape == (9,)
    assert float(val) >= best_start                              # never below the best start ...
    assert float(val) > best_start                               # ... and strictly above it on a concave surface
    assert float(val) == float(toy.acquisition(x.unsqueeze(0))[0]) == float(finals["value"].max())
    assert bool((finals["value"] >= toy.acquisition(starts)).all())
    assert bool(((finals["X"] >= bounds[0]) & (finals["X"] <= bounds[1])).all()) and bool(((x >= bounds[0]) & (x <= bounds[1])).all())
    # steps = 0: the best start itself
    x0, v0, _ = utils.suggest_candidates(toy, bounds, best=0.0, starts=starts, steps=0)
    assert float(v0) == best_start and bool((x0 == starts[int(toy.acquisition(starts).argmax())]).all())
    # starts outside the box are projected onto it
    _, _, f2 = utils.suggest_candidates(toy, bounds, best=0.0, starts=starts + 10.0, steps=3)
    assert bool(((f2["X"] >= bounds[0]) & (f2["X"] <= bounds[1])).all())
    # uniform draws: the same seed, the same result; another seed, another
    a = utils.suggest_candidates(toy, bounds, best=0.0, num_starts=8, steps=10, generator=torch.Generator().manual_seed(5))
    b = utils.suggest_candidates(toy, bounds, best=0.0, num_starts=8, steps=10, generator=torch.Generator().manual_seed(5))
    d = utils.suggest_candidates(toy, bounds, best=0.0, num_starts=8, steps=10, generator=torch.Generator().manual_seed(6))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2]["X"], b[2]["X"])
    assert not torch.equal(a[2]["X"], d[2]["X"])
    assert a[2]["X"].shape == (8, 3) and bool(((a[2]["X"] >= bounds[0]) & (a[2]["X"] <= bounds[1])).all())
    with pytest.raises(ValueError, match="bounds"):
        utils.suggest_candidates(toy, torch.zeros(3, 2), best=0.0)


def test_abi_declares_the_entry():
    hdr = open(os.path.join(REPO, "include", "tgp_hip.h")).read()
    assert re.search(r"\bint tgp_predict_acquisition_f64\(const tgp_model\* model,", hdr)
    for name, val in (("TGP_ACQ_EI", 0), ("TGP_ACQ_LOG_EI", 1), ("TGP_ACQ_PI", 2)):
        assert re.search(r"#define %s %d\b" % (name, val), hdr), name
    assert (L.ACQ_EI, L.ACQ_LOG_EI, L.ACQ_PI) == (0, 1, 2)
    assert "tgp_predict_acquisition_f64" in L.EXPORTS
    assert re.search(r"#define TGP_VERSION 104\b", hdr) and L.load().tgp_version() == 104


def test_library_refusals_before_any_device():
    """Each refusal comes before a pointer is read: the arrays are host memory."""
    h = L.load()
    buf = torch.zeros(16, dtype=F64)
    p = ctypes.c_void_p(buf.data_ptr())
    entry = b"tgp_predict_acquisition_f64"

    def model(lik=L.LIK_GAUSS, S=8):
        md = L.TgpModel()
        md.N, md.D, md.M, md.S, md.lik = 4, 1, 1, S, lik
        md.log_var_noise = p
        return md

    def call(md, mu=p, v=p, rowp=None, kind=L.ACQ_EI, best=0.5, minimize=0, value=p, partials=p, dmu=None, dv=None, D=0, grad=None):
        return h.tgp_predict_acquisition_f64(md, mu, v, rowp, kind, best, minimize, value, partials, dmu, dv, D, grad, None)

    rc = call(model(L.LIK_POISSON))
    assert rc == L.E_UNSUPPORTED and h.tgp_last_error().startswith(entry) and b"lik = %d" % L.LIK_POISSON in h.tgp_last_error()
    for lik in (L.LIK_BERNOULLI, L.LIK_WARPED, L.LIK_STUDENT, L.LIK_HETERO, L.LIK_NEGBIN, L.LIK_ORDINAL, L.LIK_GAMMA, L.LIK_BETA):
        assert call(model(lik)) == L.E_UNSUPPORTED and h.tgp_last_error().startswith(entry), lik
    rc = call(model(L.LIK_FLOW, L.QUANTILE_MAX_S + 1))
    assert rc == L.E_UNSUPPORTED and h.tgp_last_error().startswith(entry) and b"S = " in h.tgp_last_error()
    assert call(model(L.LIK_FLOW, 0)) == L.E_UNSUPPORTED and h.tgp_last_error().startswith(entry)
    for kind in (3, -1):
        rc = call(model(), kind=kind)
        assert rc == L.E_UNSUPPORTED and h.tgp_last_error().startswith(entry) and b"kind = %d" % kind in h.tgp_last_error()
    for bad in (float("nan"), float("inf"), -float("inf")):
        rc = call(model(), best=bad)
        assert rc == L.E_UNSUPPORTED and h.tgp_last_error().startswith(entry) and b"best" in h.tgp_last_error()
    # null pointers in the house order: the negative position of the argument
    assert h.tgp_predict_acquisition_f64(None, p, p, None, 0, 0.5, 0, p, p, None, None, 0, None, None) == -1
    md = model()
    md.log_var_noise = None
    assert call(md) == -1
    assert call(model(), mu=None) == -2
    assert call(model(), v=None) == -3
    assert call(model(), mu=None, v=None, value=None) == -2
    assert call(model(), value=None) == -8
    # grad_x without its Jacobians, or without D
    assert call(model(), grad=p) == -10
    assert call(model(), grad=p, dmu=p) == -11
    assert call(model(), grad=p, dmu=p, dv=p, D=0) == -12
    assert call(model(), grad=p, value=None) == -8
    # an unknown kind and a bad incumbent come before the output pointers
    assert call(model(), kind=3, value=None) == L.E_UNSUPPORTED
    assert call(model(), best=float("nan"), value=None) == L.E_UNSUPPORTED
    assert bool((buf == 0.0).all())                             # nothing was written
