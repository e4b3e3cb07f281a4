"""CPU restatement of the Beta likelihood (TGP_LIK_BETA, include/tgp_hip.h) in float64 torch, the autograd oracle of
tests/test_beta_host.py and tests/test_gpu_beta.py.  With g = G(f0) the log-odds of the mean, lam = log phi the log precision,
mu = sigmoid(g), nu = sigmoid(-g), a = mu phi, b = nu phi, ly = log y, l1 = log1p(-y) and y* = ly - l1:

    log p(y | g) = lgamma(phi) - lgamma(a) - lgamma(b) + a y* + phi l1 - ly - l1
    d/dg         = mu nu phi [y* - psi(a) + psi(b)]
    d/dlam       = phi [psi(phi) - mu psi(a) - nu psi(b) + mu y* + l1]

`ell_torch` is the Gauss-Hermite expected log-likelihood (its gradients are autograd's), `pred_torch` the predictive mean,
variance and log density (by torch.logsumexp).  The predictive is a mixture of Betas; on x = logit t

    F_n(x) = sum_s wn_s I_t(a_s, b_s),   1 - F_n = sum_s wn_s I_{1-t}(b_s, a_s),   F_n'(x) = sum_s wn_s t^a_s (1 - t)^b_s / B(a_s, b_s).

`tails_mp` evaluates the three through mpmath (mpmath.betainc at MP_DPS digits, from g, phi and x themselves: it shares nothing
with the kernel, not even the rounded a_s and b_s), at x or at a quantile t given as a double (1 - t is then exact); `tails_ref` is
the same made quick: scipy.special.betainc for the components whose shape parameters are both at least 1 -- where
tests/test_beta_host.py holds it to mpmath -- and mpmath for the others.  `beta_cf` is a line-for-line numpy port of the device's continued fraction (csrc/tgp_quantile.hip beta_cf, modified
Lentz, two coefficients per step) with its step count, `node_table` QBeta::prep, `tails_port` QBeta::eval on them -- the kernel's
F -- and `quantiles` the kernel's root rule on x (start G(mu + zq sqrt v) + zq sqrt(1 / a + 1 / b) at the flow's value, first step
max(2 / sqrt phi, |x0| 2^-20); doubling bracket, Newton with bisection, stop at an exact hit or a step <= 2^-50 max(1, |x|), at
most 128 evaluations per phase; no closed form for a row without variance).  The flow is warp_model.flow_forward (through
quantile_model.G, the same block table)."""
import math

import numpy as np
import torch

from quantile_model import G, nodes      # noqa: F401  (warp_model.flow_forward; re-exported for the tests)

F64 = torch.float64
MAXIT = 128                          # Q_MAXIT: evaluations of F per phase
STEP_TOL = 8.8817841970012523e-16    # 2^-50
START_REL = 9.5367431640625e-07      # 2^-20
CF_EPS = 2.2204460492503131e-16      # 2^-52: the continued fraction stops at a factor this close to 1
CF_FPMIN = 1e-300
CF_MAXIT = 174                       # TGP_BETA_CF_MAXIT
PMIN, PMAX = 0.5, 1e3                # TGP_BETA_MIN_PRECISION, TGP_BETA_MAX_PRECISION
SCIPY_MIN_SHAPE = 1.0                # tails_ref: scipy.special.betainc serves the components with min(a, b) at least this
MP_DPS = 50                          # digits of the mpmath reference (tests/test_beta_host.py holds the port to 120)


def precision_of(lam):
    return float(torch.exp(torch.as_tensor(lam, dtype=F64).detach().reshape(-1)[0]))


def row_term(y, lam):
    """lgamma(phi) + phi l1 - ly - l1: the part of log p that depends on y and phi only."""
    phi, l1 = torch.exp(lam), torch.log1p(-y)
    return torch.lgamma(phi) + phi * l1 - torch.log(y) - l1


def node_term(y, g, lam):
    """a y* - lgamma(a) - lgamma(b): the part of log p that changes with the node."""
    phi = torch.exp(lam)
    a, b = torch.sigmoid(g) * phi, torch.sigmoid(-g) * phi
    return a * (torch.log(y) - torch.log1p(-y)) - torch.lgamma(a) - torch.lgamma(b)


def log_p(y, g, lam):
    """log Beta(y | sigmoid(g) phi, sigmoid(-g) phi), phi = exp(lam); broadcasts."""
    return row_term(y, lam) + node_term(y, g, lam)


def _ell_nodes(mu, v, program, theta, xs, rowp):
    """(S,N) node values with the graph to mu, v, theta and rowp; v <= 0 counts as 0."""
    f0 = mu.reshape(1, -1) + torch.sqrt(2.0 * v.clamp(min=0.0)).reshape(1, -1) * xs.reshape(-1, 1)
    return G(f0, program, theta, rowp)


def ell_rows(Y, mu, v, lam, program, theta, xs, wn, rowp=None):
    """(N,): sum_s wn_s log p(y_n | g_ns); a node of weight 0 adds nothing."""
    g = _ell_nodes(mu, v, program, theta, xs, rowp)
    lam = lam.reshape(())
    w = wn.reshape(-1, 1)
    t = node_term(Y.reshape(1, -1), g, lam)
    return torch.where(w > 0.0, w * t, torch.zeros_like(t)).sum(0) + row_term(Y.reshape(-1), lam)


def ell_torch(Y, mu, v, lam, program, theta, xs, wn, rowp=None, scale=1.0):
    """scale * sum_n ell_rows."""
    return scale * ell_rows(Y, mu, v, lam, program, theta, xs, wn, rowp).sum()


def pred_terms(Y, mu, v, lam, program, theta, xs, wn, rowp=None):
    """(S, N): log wn_s + log p(y_n | g_ns), the terms of the log predictive density."""
    g = nodes(mu, v, xs, program, theta, rowp)
    return torch.log(wn).reshape(-1, 1) + log_p(Y.reshape(1, -1), g, lam.reshape(()))


def pred_torch(mu, v, lam, program, theta, xs, wn, rowp=None, Y=None):
    """(m1, m2, logp): E[y] = sum wn mu_s, Var[y] = sum wn mu_s nu_s / (1 + phi) + sum wn mu_s^2 - m1^2 (the last two as the
    centred sum sum wn (mu_s - m1)^2), logp = logsumexp_s of pred_terms (None without Y); the empty program goes through the same
    sums."""
    g = nodes(mu, v, xs, program, theta, rowp)
    w = wn.reshape(-1, 1)
    m, n = torch.sigmoid(g), torch.sigmoid(-g)
    m1, n1 = (w * m).sum(0), (w * n).sum(0)
    d = torch.where(m1 <= n1, m - m1, n - n1)      # mu_s - m1 from the side on which it is a difference of small numbers
    m2 = (w * m * n).sum(0) / (1.0 + torch.exp(lam.reshape(()))) + (w * d * d).sum(0)
    logp = None if Y is None else torch.logsumexp(pred_terms(Y, mu, v, lam, program, theta, xs, wn, rowp), 0)
    return m1, m2, logp


# ---------------------------------------------------------------------------------------------------
# F, its tails and its density: the reference (mpmath)
# ---------------------------------------------------------------------------------------------------
def _mp(dps=None):
    import mpmath
    mpmath.mp.dps = MP_DPS if dps is None else dps
    return mpmath


def mp_component(phi, g, x=None, t=None, dps=None, want="lud"):
    """(lower, upper, density in x) of one Beta(phi sigmoid(g), phi sigmoid(-g)) as mpmath numbers, at x = logit t, or at the
    double t (1 - t exact); `want` names the ones to compute (l, u, d), the others come back as 0."""
    mp = _mp(dps)
    phi, g = mp.mpf(float(phi)), mp.mpf(float(g))
    a, b = phi / (1 + mp.exp(-g)), phi / (1 + mp.exp(g))
    if t is None:
        x = mp.mpf(float(x))
        t, u = 1 / (1 + mp.exp(-x)), 1 / (1 + mp.exp(x))
    else:
        t = mp.mpf(float(t))
        u = 1 - t
    lower = mp.betainc(a, b, 0, t, regularized=True) if "l" in want else mp.mpf(0)
    upper = mp.betainc(b, a, 0, u, regularized=True) if "u" in want else mp.mpf(0)
    dens = (mp.exp(a * mp.log(t) + b * mp.log(u) - (mp.loggamma(a) + mp.loggamma(b) - mp.loggamma(phi))) if "d" in want
            else mp.mpf(0))
    return lower, upper, dens


def tails_mp(g, wn, phi, x=None, t=None, want="lud"):
    """(lower, upper, density) per row as float64 tensors, summed in mpmath: g (S,N), x or t (N,); `want` as in mp_component."""
    mp = _mp()
    S, N = g.shape
    lo, up, dn = [], [], []
    for n in range(N):
        acc = [mp.mpf(0), mp.mpf(0), mp.mpf(0)]
        for s in range(S):
            w = mp.mpf(float(wn[s]))
            r = mp_component(phi, float(g[s, n]), None if x is None else float(x[n]), None if t is None else float(t[n]),
                             want=want)
            for i in range(3):
                acc[i] += w * r[i]
        lo.append(float(acc[0]))
        up.append(float(acc[1]))
        dn.append(float(acc[2]))
    return torch.tensor(lo, dtype=F64), torch.tensor(up, dtype=F64), torch.tensor(dn, dtype=F64)


def tails_ref(g, wn, phi, x=None, t=None, want="lu"):
    """(lower, upper, 0) per row at the double t (1 - t exact): the reference of the CDF and quantile tests.  A component whose
    two shape parameters are both at least SCIPY_MIN_SHAPE goes through scipy.special.betainc, which tests/test_beta_host.py holds
    to mpmath there (2e-13; below that shape it is off by up to 2e-8, and is not used); every other component goes through
    mpmath (tails_mp's mp_component).  mpmath alone costs 5 ms a component at phi = 1000, 15 s for 3 rows x 32 nodes x 32
    probabilities; it is quick where the shapes are small.  Shares nothing with the kernel but the two products."""
    from scipy.special import betainc
    assert x is None
    gn, tn = g.detach().numpy(), np.broadcast_to(t.detach().numpy()[None, :], g.shape)
    a, b = phi / (1.0 + np.exp(-gn)), phi / (1.0 + np.exp(gn))
    big = np.minimum(a, b) >= SCIPY_MIN_SHAPE
    w = wn.detach().numpy()[:, None]
    out = []
    for key, (p_, q_, arg) in (("l", (a, b, tn)), ("u", (b, a, 1.0 - tn))):
        if key not in want:
            out.append(torch.zeros(g.shape[1], dtype=F64))
            continue
        with np.errstate(all="ignore"):
            val = np.where(big, betainc(p_, q_, arg), 0.0)
        for s, n in zip(*np.nonzero(~big)):
            val[s, n] = float(mp_component(phi, float(gn[s, n]), t=float(tn[s, n]), want=key)[0 if key == "l" else 1])
        out.append(torch.from_numpy((w * val).sum(0)))
    return out[0], out[1], torch.zeros(g.shape[1], dtype=F64)


def residual_within_ulp(g, wn, phi, t, p, tails=tails_ref):
    """How far, relative to min(p, 1 - p), the root of F = p lies outside [t-, t+], the doubles next to the double t: 0 where
    F(t-) <= p <= F(t+), else the smaller of the two misses (F from the tail that is small at p, through mpmath).  Where the
    spacing of the doubles around t does not matter this is at most residual_mp -- F is increasing -- and it is what a quantile
    handed back as a double can be held to where it does: next to 1 a step of 2^-53 in t moves an upper tail of the size
    (1 - t)^b by the share b 2^-53 / (1 - t).  `tails`: tails_ref or tails_mp."""
    tm = torch.nextafter(t, torch.zeros_like(t))
    tp = torch.nextafter(t, torch.ones_like(t))
    lm, um, _ = tails(g, wn, phi, t=tm, want="u" if p > 0.5 else "l")
    lp, up, _ = tails(g, wn, phi, t=tp, want="u" if p > 0.5 else "l")
    if p > 0.5:
        q = 1.0 - p        # the upper tail falls with t
        return torch.maximum((up - q).clamp_min(0.0), (q - um).clamp_min(0.0)) / q
    return torch.maximum((lm - p).clamp_min(0.0), (p - lp).clamp_min(0.0)) / p


# ---------------------------------------------------------------------------------------------------
# the kernel's own algorithm, in numpy
# ---------------------------------------------------------------------------------------------------
def beta_cf(a, b, t, maxit=CF_MAXIT):
    """(h, steps): csrc/tgp_quantile.hip beta_cf elementwise over numpy arrays; `steps` the trip count of each element."""
    a, b, t = np.broadcast_arrays(np.asarray(a, np.float64), np.asarray(b, np.float64), np.asarray(t, np.float64))
    with np.errstate(all="ignore"):
        qab, qap, qam = a + b, a + 1.0, a - 1.0
        c = np.ones_like(a)
        d = 1.0 - qab * t / qap
        d = np.where(np.abs(d) < CF_FPMIN, CF_FPMIN, d)
        d = 1.0 / d
        h = d.copy()
        act = np.ones(a.shape, bool)
        steps = np.zeros(a.shape, np.int64)
        for m in range(1, maxit + 1):
            if not act.any():
                break
            dm, m2 = float(m), 2.0 * float(m)
            aa = dm * (b - dm) * t / ((qam + m2) * (a + m2))
            dn = 1.0 + aa * d
            dn = np.where(np.abs(dn) < CF_FPMIN, CF_FPMIN, dn)
            cn = 1.0 + aa / c
            cn = np.where(np.abs(cn) < CF_FPMIN, CF_FPMIN, cn)
            dn = 1.0 / dn
            hn = h * (dn * cn)
            aa = -(a + dm) * (qab + dm) * t / ((a + m2) * (qap + m2))
            dn = 1.0 + aa * dn
            dn = np.where(np.abs(dn) < CF_FPMIN, CF_FPMIN, dn)
            cn = 1.0 + aa / cn
            cn = np.where(np.abs(cn) < CF_FPMIN, CF_FPMIN, cn)
            dn = 1.0 / dn
            de = dn * cn
            hn = hn * de
            h, c, d = np.where(act, hn, h), np.where(act, cn, c), np.where(act, dn, d)
            steps = np.where(act, m, steps)
            act = act & ~(np.abs(de - 1.0) < CF_EPS)
    return h, steps


def node_table(g, phi):
    """(a, b, nlb) of QBeta::prep from the node values g (numpy): a = phi sigmoid(g), b = phi sigmoid(-g), each from the same
    exp(-|g|) and division, nlb = lgamma(phi) - lgamma(a) - lgamma(b)."""
    g = np.asarray(g, np.float64)
    e = np.exp(-np.abs(g))
    d = 1.0 / (1.0 + e)
    ed = e * d
    a, b = np.where(g > 0.0, d, ed) * phi, np.where(g > 0.0, ed, d) * phi
    lg = lambda z: torch.lgamma(torch.as_tensor(z, dtype=F64)).numpy()
    return a, b, math.lgamma(phi) - lg(a) - lg(b)


def component_port(a, b, nlb, x):
    """(lower, upper, density, steps) of QBeta::eval's node term at x = logit t, elementwise (numpy)."""
    x = np.asarray(x, np.float64)
    with np.errstate(all="ignore"):
        e = np.exp(-np.abs(x))
        d = 1.0 / (1.0 + e)
        ed, l1e = e * d, np.log1p(e)
        t, u = np.where(x > 0.0, d, ed), np.where(x > 0.0, ed, d)
        lt, lu = np.where(x > 0.0, -l1e, x - l1e), np.where(x > 0.0, -x - l1e, -l1e)
        h = np.exp(a * lt + b * lu + nlb)
        low = t < (a + 1.0) / (a + b + 2.0)
        cf, steps = beta_cf(np.where(low, a, b), np.where(low, b, a), np.where(low, t, u))
        small = h * cf / np.where(low, a, b)
        big = 1.0 - small
    return np.where(low, small, big), np.where(low, big, small), h, steps


def tails_port(g, wn, phi, x):
    """(lower, upper, density) as the kernel forms them, float64 tensors: g (S,N) node values, x (N,)."""
    a, b, nlb = node_table(g.detach().numpy(), phi)
    lo, up, h, _ = component_port(a, b, nlb, x.detach().numpy()[None, :])
    w = wn.detach().numpy()[:, None]
    return (torch.from_numpy((w * lo).sum(0)), torch.from_numpy((w * up).sum(0)), torch.from_numpy((w * h).sum(0)))


def _signed(g, wn, phi, x, p):
    lower, upper, dens = tails_port(g, wn, phi, x)
    return ((1.0 - p) - upper if p > 0.5 else lower - p), dens


def quantiles(mu, v, lam, probs, xs, wn, program, theta, rowp=None, count=None):
    """(t = sigmoid(x) of shape (Q,N), number of roots that ran out of evaluations, x): the kernel's rule, all rows at once.
    `count` (a list) receives the largest number of evaluations of F a root took."""
    phi = precision_of(lam)
    probs = [float(p) for p in probs]
    zqs = torch.special.ndtri(torch.tensor(probs, dtype=F64))
    g = nodes(mu, v, xs, program, theta, rowp)
    out, failed = [], 0
    for p, zq in zip(probs, zqs):
        gq = G(mu + zq * torch.sqrt(v.clamp_min(0.0)), program, theta, rowp)
        e = torch.exp(-gq.abs())
        x = gq + zq * torch.sqrt((1.0 + e) * (1.0 + e) / (e * phi))
        fx, dn = _signed(g, wn, phi, x, p)
        evals = torch.ones_like(x)
        done = fx == 0.0
        step = torch.maximum(torch.full_like(x, 2.0 / math.sqrt(phi)), x.abs() * START_REL)
        up = fx < 0.0
        lo, hi = torch.where(up, x, x - step), torch.where(up, x + step, x)
        ok = done.clone()
        for _ in range(MAXIT):
            if bool(ok.all()):
                break
            probe = torch.where(ok, x, torch.where(up, hi, lo))
            fb, _d = _signed(g, wn, phi, probe, p)
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
            f2, d2 = _signed(g, wn, phi, x, p)
            evals = evals + (~done).to(F64)
            fx, dn = torch.where(done, fx, f2), torch.where(done, dn, d2)
        fail = fail | ~done
        failed += int(fail.sum())
        if count is not None:
            count.append(int(evals.max()))
        out.append(torch.where(fail, torch.full_like(x, float("nan")), x))
    x = torch.stack(out)
    return torch.sigmoid(x), failed, x


def cdf_ref(mu, v, lam, Y, xs, wn, program, theta, rowp=None, tails=tails_ref):
    """(cdf, sf) at Y per row through `tails` (tails_ref or tails_mp); Y <= 0: (0, sum wn); Y >= 1: (sum wn, 0)."""
    phi = precision_of(lam)
    g = nodes(mu, v, xs, program, theta, rowp)
    inside = (Y > 0.0) & (Y < 1.0)
    lower, upper, _ = tails(g, wn, phi, t=torch.where(inside, Y, torch.full_like(Y, 0.5)), want="lu")
    tot = float(wn.sum())
    lower = torch.where(inside, lower, torch.where(Y <= 0.0, torch.zeros_like(lower), torch.full_like(lower, tot)))
    upper = torch.where(inside, upper, torch.where(Y <= 0.0, torch.full_like(upper, tot), torch.zeros_like(upper)))
    return lower, upper
