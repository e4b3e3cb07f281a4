"""CPU restatement of the Gamma likelihood (TGP_LIK_GAMMA, include/tgp_hip.h) in float64 torch, the autograd oracle of
tests/test_gamma_host.py and tests/test_gpu_gamma.py.  With g = G(f0) the log-mean, lam = log a the log shape, l = log y and
z = l - g:

    log p(y | g) = [a log a - lgamma(a) - l] + a (z - e^z)
    d/dg         = a (e^z - 1)
    d/dlam       = a (log a + 1 - psi(a)) + a (z - e^z)

`ell_torch` is the Gauss-Hermite expected log-likelihood (its gradients are autograd's), `pred_torch` the predictive mean,
variance and log density (by torch.logsumexp).  The predictive is a mixture of Gammas, a location family in tau = log t:

    F_n(tau) = sum_s wn_s P(a, a e^(tau - g_ns)),   F_n'(tau) = sum_s wn_s h(tau - g_ns),   h(z) = (a e^z)^a e^(-a e^z) / Gamma(a)

`tails` evaluates F, 1 - F and F' through torch.special.gammainc / gammaincc -- independent of the kernel's series.  `pq` is the
kernel's own algorithm (csrc/tgp_quantile.hip gamma_pq: power series for x < a + 1, modified-Lentz continued fraction otherwise,
the leading factor as exp(a (z - expm1(z)) + [a log a - a - lgamma(a)])) with its iteration count, `tails_pq` the kernel's F on
it, `quantiles` the kernel's root rule on tau (start G(mu + zq sqrt v) + s(a, p), s the larger of the Wilson-Hilferty and the
small-argument value; first step max(1 / sqrt a, 1 / a, |tau0| 2^-20); doubling bracket, Newton with bisection, stop at an exact
hit or a step <= 2^-50 max(1, |tau|), at most 128 evaluations per phase; no closed form for a row without variance) and
`bisect_quantiles` plain bisection on tau over `tails`, which shares nothing with the rule.  The flow is warp_model.flow_forward
(through quantile_model.G, the same block table)."""
import math

import torch

from quantile_model import G, nodes      # noqa: F401  (warp_model.flow_forward; re-exported for the tests)

F64 = torch.float64
MAXIT = 128                          # Q_MAXIT: evaluations of F per phase
STEP_TOL = 8.8817841970012523e-16    # 2^-50
START_REL = 9.5367431640625e-07      # 2^-20
PQ_EPS = 1.1102230246251565e-16      # 2^-53: the series and the continued fraction stop at a term below this share
PQ_FPMIN = 1e-300
AMIN, AMAX = 0.1, 1e3                # TGP_GAMMA_MIN_SHAPE, TGP_GAMMA_MAX_SHAPE


def shape_of(lam):
    return float(torch.exp(torch.as_tensor(lam, dtype=F64).detach().reshape(-1)[0]))


def row_term(y, lam):
    """a log a - lgamma(a) - log y: the part of log p that depends on y and a only."""
    a = torch.exp(lam)
    return a * lam - torch.lgamma(a) - torch.log(y)


def log_p(y, g, lam):
    """log Gamma(y | shape a = exp(lam), rate a exp(-g)); broadcasts."""
    z = torch.log(y) - g
    return row_term(y, lam) + torch.exp(lam) * (z - torch.exp(z))


def _ell_nodes(mu, v, program, theta, xs, rowp):
    """(S,N) node values with the graph to mu, v, theta and rowp; v <= 0 counts as 0."""
    f0 = mu.reshape(1, -1) + torch.sqrt(2.0 * v.clamp(min=0.0)).reshape(1, -1) * xs.reshape(-1, 1)
    return G(f0, program, theta, rowp)


def ell_rows(Y, mu, v, lam, program, theta, xs, wn, rowp=None):
    """(N,): sum_s wn_s log p(y_n | g_ns)."""
    g = _ell_nodes(mu, v, program, theta, xs, rowp)
    lam = lam.reshape(())
    z = torch.log(Y.reshape(1, -1)) - g
    return (wn.reshape(-1, 1) * (torch.exp(lam) * (z - torch.exp(z)))).sum(0) + row_term(Y.reshape(-1), lam)


def ell_torch(Y, mu, v, lam, program, theta, xs, wn, rowp=None, scale=1.0):
    """scale * sum_n ell_rows."""
    return scale * ell_rows(Y, mu, v, lam, program, theta, xs, wn, rowp).sum()


def ell_closed_rows(Y, mu, v, lam):
    """(N,): the identity flow in closed form, E log p = a log a - lgamma(a) - l + a (l - mu) - a exp(l - mu + v / 2)."""
    a, l = torch.exp(lam.reshape(())), torch.log(Y.reshape(-1))
    return a * lam.reshape(()) - torch.lgamma(a) - l + a * (l - mu) - a * torch.exp(l - mu + 0.5 * v.clamp(min=0.0))


def pred_terms(Y, mu, v, lam, program, theta, xs, wn, rowp=None):
    """(S, N): log wn_s + log p(y_n | g_ns), the terms of the log predictive density (model units)."""
    g = nodes(mu, v, xs, program, theta, rowp)
    return torch.log(wn).reshape(-1, 1) + log_p(Y.reshape(1, -1), g, lam.reshape(()))


def pred_torch(mu, v, lam, program, theta, xs, wn, rowp=None, Y=None, Y_std=1.0):
    """(m1, m2, logp): E[y] = sum wn exp(g), Var[y] = (1 + 1/a) sum wn exp(2 g) - m1^2 (the empty program: the log-normal closed
    forms E[mean] = exp(mu + v / 2), E[mean^2] = exp(2 mu + 2 v)), logp = logsumexp_s of pred_terms - log Y_std (None without Y)."""
    g = nodes(mu, v, xs, program, theta, rowp)
    w = wn.reshape(-1, 1)
    c = 1.0 + torch.exp(-lam.reshape(()))
    if len(program) == 0:
        vc = v.clamp(min=0.0)
        m1 = torch.exp(mu + 0.5 * vc)
        e2 = torch.exp(2.0 * mu + 2.0 * vc)
    else:
        m1 = (w * torch.exp(g)).sum(0)
        e2 = (w * torch.exp(2.0 * g)).sum(0)
    m2 = c * e2 - m1 * m1
    logp = None if Y is None else torch.logsumexp(pred_terms(Y, mu, v, lam, program, theta, xs, wn, rowp), 0) - math.log(Y_std)
    return m1, m2, logp


# ---------------------------------------------------------------------------------------------------
# F, its tails and its density
# ---------------------------------------------------------------------------------------------------
def density(a, z):
    """h(z) = x^a e^-x / Gamma(a) at x = a e^z, formed the plain way."""
    return torch.exp(a * z - a * torch.exp(z) + a * math.log(a) - math.lgamma(a))


def tails(g, wn, a, tau):
    """(lower, upper, density) at tau of shape (N,) from the node values g (S,N), through torch.special."""
    z = tau.unsqueeze(0) - g
    x = a * torch.exp(z)
    at = torch.full_like(x, a)
    w = wn.unsqueeze(1)
    return (w * torch.special.gammainc(at, x)).sum(0), (w * torch.special.gammaincc(at, x)).sum(0), (w * density(a, z)).sum(0)


def pq(a, z):
    """(P, Q, h, iterations): the kernel's gamma_pq at x = a e^z, elementwise over the tensor z for the float a; `iterations` is
    the largest trip count any element took."""
    a = float(a)
    z = torch.as_tensor(z, dtype=F64)
    c = a * math.log(a) - a - math.lgamma(a)
    x = a * torch.exp(z)
    h = torch.exp(a * (z - torch.expm1(z)) + c)
    zero, inf = x == 0.0, torch.isinf(x)
    ser = (x < a + 1.0) & ~zero
    cf = ~(x < a + 1.0) & ~inf & ~torch.isnan(x)
    iters = 0
    # ---- the power series
    ap, s, d = a, torch.full_like(x, 1.0 / a), torch.full_like(x, 1.0 / a)
    act = ser.clone()
    xs_ = torch.where(ser, x, torch.zeros_like(x))
    for n in range(10 ** 6):
        if not bool(act.any()):
            break
        ap += 1.0
        d = torch.where(act, d * xs_ / ap, d)
        s = torch.where(act, s + d, s)
        act = act & ~(d.abs() < s.abs() * PQ_EPS)
        iters = max(iters, n + 1)
    P_ser = s * h
    # ---- the continued fraction, modified Lentz
    xc = torch.where(cf, x, torch.full_like(x, a + 1.0))
    b = xc + 1.0 - a
    cc = torch.full_like(x, 1.0 / PQ_FPMIN)
    dd = 1.0 / b
    f = dd.clone()
    act = cf.clone()
    for i in range(1, 10 ** 6):
        if not bool(act.any()):
            break
        an = -float(i) * (float(i) - a)
        b = b + 2.0
        dn = an * dd + b
        dn = torch.where(dn.abs() < PQ_FPMIN, torch.full_like(dn, PQ_FPMIN), dn)
        cn = b + an / cc
        cn = torch.where(cn.abs() < PQ_FPMIN, torch.full_like(cn, PQ_FPMIN), cn)
        dn = 1.0 / dn
        de = dn * cn
        dd, cc = torch.where(act, dn, dd), torch.where(act, cn, cc)
        f = torch.where(act, f * de, f)
        act = act & ~((de - 1.0).abs() < PQ_EPS)
        iters = max(iters, i)
    Q_cf = f * h
    P = torch.where(ser, P_ser, 1.0 - Q_cf)
    Q = torch.where(ser, 1.0 - P_ser, Q_cf)
    one, nul = torch.ones_like(x), torch.zeros_like(x)
    P = torch.where(zero, nul, torch.where(inf, one, P))
    Q = torch.where(zero, one, torch.where(inf, nul, Q))
    h = torch.where(zero | inf, nul, h)
    return P, Q, h, iters


def tails_pq(g, wn, a, tau):
    """(lower, upper, density) as the kernel forms them: through pq, each tail from its own sum."""
    P, Q, h, _ = pq(a, tau.unsqueeze(0) - g)
    w = wn.unsqueeze(1)
    return (w * P).sum(0), (w * Q).sum(0), (w * h).sum(0)


def residual(g, wn, a, tau, p):
    """|F(tau) - p| / min(p, 1 - p) per row on `tails`, F from the tail that is small at p."""
    lower, upper, _ = tails(g, wn, a, tau)
    if p > 0.5:
        return (upper - (1.0 - p)).abs() / (1.0 - p)
    return (lower - p).abs() / p


def _signed(g, wn, a, tau, p, fn):
    lower, upper, dens = fn(g, wn, a, tau)
    return ((1.0 - p) - upper if p > 0.5 else lower - p), dens


def shift(a, p, zq):
    """s(a, p): the log-quantile of one Gamma(a, rate a), roughly -- the larger of the Wilson-Hilferty value (where its argument
    is positive) and the small-argument value."""
    wh = 1.0 - 1.0 / (9.0 * a) + zq / (3.0 * math.sqrt(a))
    sm = (math.log(p) + math.lgamma(a + 1.0)) / a - math.log(a)
    return max(3.0 * math.log(wh), sm) if wh > 0.0 else sm


def quantiles(mu, v, lam, probs, xs, wn, program, theta, rowp=None, count=None):
    """(t = exp(tau) of shape (Q,N), number of roots that ran out of evaluations, tau): the kernel's rule, all rows at once.
    `count` (a list) receives the largest number of evaluations of F a root took."""
    a = shape_of(lam)
    probs = [float(p) for p in probs]
    zqs = torch.special.ndtri(torch.tensor(probs, dtype=F64))
    g = nodes(mu, v, xs, program, theta, rowp)
    out, failed = [], 0
    for p, zq in zip(probs, zqs):
        x = G(mu + zq * torch.sqrt(v.clamp_min(0.0)), program, theta, rowp) + shift(a, p, float(zq))
        fx, dn = _signed(g, wn, a, x, p, tails_pq)
        evals = torch.ones_like(x)
        done = fx == 0.0
        step = torch.maximum(torch.full_like(x, max(1.0 / math.sqrt(a), 1.0 / a)), x.abs() * START_REL)
        up = fx < 0.0
        lo, hi = torch.where(up, x, x - step), torch.where(up, x + step, x)
        ok = done.clone()
        for _ in range(MAXIT):
            if bool(ok.all()):
                break
            probe = torch.where(ok, x, torch.where(up, hi, lo))
            fb, _d = _signed(g, wn, a, probe, p, tails_pq)
            evals = evals + (~ok).to(F64)
            hit = torch.where(up, fb >= 0.0, fb <= 0.0)
            grow = ~ok & ~hit
            ok = ok | hit
            step = torch.where(grow, step * 2.0, step)
            lo_n = torch.where(up, hi, lo - step)
            hi_n = torch.where(up, hi + step, lo)
            lo, hi = torch.where(grow, lo_n, lo), torch.where(grow, hi_n, hi)
        fail = ~ok
        done = done | fail
        for _ in range(MAXIT):
            act = ~done
            zero = act & (fx == 0.0)
            mv = act & ~zero
            lo = torch.where(mv & (fx < 0.0), x, lo)
            hi = torch.where(mv & ~(fx < 0.0), x, hi)
            xn = x - fx / dn
            xn = torch.where((xn > lo) & (xn < hi), xn, 0.5 * (lo + hi))
            dx = (xn - x).abs()
            x = torch.where(mv, xn, x)
            done = done | zero | (mv & (dx <= STEP_TOL * x.abs().clamp_min(1.0)))
            if bool(done.all()):
                break
            f2, d2 = _signed(g, wn, a, x, p, tails_pq)
            evals = evals + (~done).to(F64)
            fx, dn = torch.where(done, fx, f2), torch.where(done, dn, d2)
        fail = fail | ~done
        failed += int(fail.sum())
        if count is not None:
            count.append(int(evals.max()))
        out.append(torch.where(fail, torch.full_like(x, float("nan")), x))
    tau = torch.stack(out)
    return torch.exp(tau), failed, tau


def bisect_quantiles(mu, v, lam, probs, xs, wn, program, theta, rowp=None):
    """tau (Q,N): the same roots by plain bisection on `tails`, from a bracket grown by doubling around the node values until F
    straddles p, until the midpoint is one of the two ends."""
    a = shape_of(lam)
    g = nodes(mu, v, xs, program, theta, rowp)
    out = []
    for p in probs:
        p = float(p)
        f = lambda t: _signed(g, wn, a, t, p, tails)[0]
        lo, hi = g.min(0).values - 1.0, g.max(0).values + 1.0
        w = torch.ones_like(lo)
        for _ in range(12):
            lo = torch.where(f(lo) < 0.0, lo, lo - w)
            hi = torch.where(f(hi) > 0.0, hi, hi + w)
            w = 2.0 * w
        assert bool((f(lo) < 0.0).all()) and bool((f(hi) > 0.0).all())
        for _ in range(4000):
            mid = 0.5 * (lo + hi)
            stuck = (mid <= lo) | (mid >= hi)
            if bool(stuck.all()):
                break
            below = f(mid) < 0.0
            lo = torch.where(~stuck & below, mid, lo)
            hi = torch.where(~stuck & ~below, mid, hi)
        out.append(0.5 * (lo + hi))
    return torch.stack(out)


def cdf(mu, v, lam, Y, xs, wn, program, theta, rowp=None):
    """(cdf, sf) at Y per row; Y <= 0: (0, sum wn)."""
    a = shape_of(lam)
    g = nodes(mu, v, xs, program, theta, rowp)
    pos = Y > 0.0
    lower, upper, _ = tails(g, wn, a, torch.log(torch.where(pos, Y, torch.ones_like(Y))))
    return torch.where(pos, lower, torch.zeros_like(lower)), torch.where(pos, upper, torch.full_like(upper, float(wn.sum())))
