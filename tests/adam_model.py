"""One torch.optim.Adam step in extended precision: the reference every copy of the Adam arithmetic is held to
(k_adam, k_adam_dev, adam_elem, k_mlp_reduce, k_big_glam), plus the plain float64 restatement whose distance from it
sets the GPU tolerance (tests/test_adam_host.py measures it, tests/test_gpu_adam.py uses it).

torch.optim.Adam (dsp/trainers/optimizers.py:12), single tensor, no amsgrad:
    g <- -g if maximize;  g <- g + wd p;  m <- b1 m + (1 - b1) g;  v <- b2 v + (1 - b2) g^2
    p <- p - (lr / (1 - b1^t)) m / (sqrt(v) / sqrt(1 - b2^t) + eps)

Arithmetic: numpy.longdouble (64-bit mantissa on x86: eps 1.1e-19), beta^t by repeated multiplication (t <= 1e5 products:
relative error <= 1e5 x 5.4e-20 of beta^t, i.e. <= 5.4e-15 x beta^t absolute in 1 - beta^t -- nothing next to 2^-53).  Where the
platform's longdouble is no wider than that bar (finfo.eps >= 1e-18) the same formulas run in mpmath (40 digits) on the
indices check_indices() picks: at most 2 000, the caller's boundary indices among them.
(1 - beta) is exact in float64 for 0.5 <= beta <= 1 (Sterbenz), so the kernels' fl(1 - beta) is the reference's.
"""
import functools

import numpy as np

WIDE = bool(np.finfo(np.longdouble).eps < 1e-18)
MAX_MP = 2000

# Measured by tests/test_adam_host.py::test_float64_restatement_against_the_reference (x86-64, numpy 2.2; the GPU tests' own inputs:
# make_inputs(n, seed_of(n)) at every size, steps 1-5, 999-1003, 99 996-100 000 from zero state, and 999-1001 from the synthetic
# non-zero state; beta^t both as b**t and as exp(t ln b)): the largest per-step error of a plain float64 restatement, per
# hyper-parameter set, in the metrics of errors() below -- (p, exp_avg, exp_avg_sq), written with 10 % of headroom:
#   torch_defaults  4.99e-13  1.71e-16  2.07e-16
#   engine          4.68e-14  2.20e-16  3.24e-16
#   short_memory    4.37e-13  1.52e-16  3.57e-16
# The p figure is the parameter's own last-bit rounding (|p| in [4, 8): half an ulp is 4.4e-16) over max|dp| ~ 0.9 lr, hence ten
# times smaller at lr = 0.01; the moments' are their own last-bit rounding.  The host test asserts the measurement stays at or
# below these and above half of them (they are not slack); the GPU tolerance is 4 x them (FMA contraction and the compiler's
# ordering, nothing else).  The copies inside the training step run the engine's set (without its weight decay, which the
# figures do not depend on) and are held to its row.
F64 = {"torch_defaults": (5.5e-13, 1.9e-16, 2.3e-16), "engine": (5.2e-14, 2.5e-16, 3.6e-16), "short_memory": (4.9e-13, 1.7e-16, 4.0e-16)}
GPU_MARGIN = 4.0

HYPER = {   # lr, beta1, beta2, eps, weight_decay, maximize
    "torch_defaults": (1e-3, 0.9, 0.999, 1e-8, 0.0, 0),
    "engine": (0.01, 0.9, 0.999, 1e-8, 1e-5, 1),
    "short_memory": (1e-3, 0.5, 0.9, 1e-3, 0.1, 0),
}
STEP_STARTS = (0, 998, 99995)        # five consecutive steps from each: 1-5, 999-1003, 99 996-100 000
WARM_SIZES, WARM_START, WARM_STEPS = (257, 131073), 998, 3      # the walk from make_inputs' non-zero state: steps 999-1001


def seed_of(n):
    """The seed of the inputs of size n.  n = 1 takes 5: its five gradients span 1e-12 ... 1e-2 without making the single update so
    small (eps-dominated from the first step) that the parameter's own rounding, measured against it, outgrows the larger sizes'."""
    return n if n > 1 else 5


def make_inputs(n, seed, steps=5):
    """p standard normal; `steps` gradients normal x 10^U(-12, 3) (eps-dominated to sqrt(v)-dominated), a handful exactly 0;
    a non-zero (exp_avg, exp_avg_sq) to start from where a test wants one."""
    rng = np.random.default_rng(seed)
    p = rng.standard_normal(n)
    gs = []
    for _ in range(steps):
        g = rng.standard_normal(n) * 10.0 ** rng.uniform(-12.0, 3.0, n)
        zeros = rng.integers(0, n, size=min(n, 5))
        if n > 5:                       # (a buffer of one element keeps its only gradient: a zero there would test nothing)
            g[zeros] = 0.0
        gs.append(g)
    # (moments of one past: |exp_avg| <= sqrt(exp_avg_sq), as every state Adam itself produces has it up to the bias factors --
    # unrelated draws give updates of 1e9 and then measure the rounding of a parameter of that size, not the step)
    h = rng.standard_normal(n) * 10.0 ** rng.uniform(-12.0, 3.0, n)
    return p, gs, 0.3 * h, h * h


def check_indices(n, boundaries=(), seed=0):
    """The indices the reference is evaluated at: all of them with a wide longdouble, else <= 2 000 with the boundaries."""
    if WIDE or n <= MAX_MP:
        return np.arange(n)
    b = np.unique(np.clip(np.asarray(list(boundaries) + [0, n - 1], dtype=np.int64), 0, n - 1))
    rest = np.random.default_rng(seed).choice(n, MAX_MP - len(b), replace=False)
    return np.unique(np.concatenate([b, rest]))


if WIDE:
    def _lift(x):
        return np.asarray(x, dtype=np.longdouble)

    _sqrt = np.sqrt

    def _one():
        return np.longdouble(1)
else:                                   # pragma: no cover - x86 has the 80-bit type
    import mpmath
    mpmath.mp.dps = 40

    def _lift(x):
        return np.vectorize(lambda t: mpmath.mpf(float(t)), otypes=[object])(np.asarray(x, dtype=np.float64))

    _sqrt = np.vectorize(mpmath.sqrt, otypes=[object])

    def _one():
        return mpmath.mpf(1)


@functools.lru_cache(maxsize=None)
def beta_pow(beta, t):
    """beta^t by t exact-type multiplications."""
    b, r = _lift(beta)[()], _one()
    for _ in range(int(t)):
        r = r * b
    return r


def adam_ref(p, g, m, v, step, lr, b1, b2, eps, wd=0.0, maximize=False):
    """(p', m', v', dp) of one step from float64 state; `wd` a scalar or a per-element array (parameter groups).  Extended
    precision throughout; the caller rounds or compares as it likes."""
    p, g, m, v, wd = _lift(p), _lift(g), _lift(m), _lift(v), _lift(wd)
    lr, B1, B2, eps, one = _lift(lr)[()], _lift(b1)[()], _lift(b2)[()], _lift(eps)[()], _one()
    if maximize:
        g = -g
    g = g + wd * p
    m1 = B1 * m + (one - B1) * g
    v1 = B2 * v + (one - B2) * g * g
    bc1, bc2 = one - beta_pow(float(b1), int(step)), one - beta_pow(float(b2), int(step))
    dp = -(lr / bc1) * m1 / (_sqrt(v1) / _sqrt(_lift(bc2))[()] + eps)
    return p + dp, m1, v1, dp


def adam_f64(p, g, m, v, step, lr, b1, b2, eps, wd=0.0, maximize=False, power="pow"):
    """The same step in plain float64 numpy, written as the kernels write it; `power`: beta^t as b**t or exp(t ln b)."""
    p, g, m, v = (np.asarray(a, dtype=np.float64) for a in (p, g, m, v))
    g = -g if maximize else g
    g = g + np.asarray(wd, dtype=np.float64) * p
    m1 = b1 * m + (1.0 - b1) * g
    v1 = b2 * v + (1.0 - b2) * g * g
    if power == "pow":
        pw1, pw2 = b1 ** float(step), b2 ** float(step)
    else:
        pw1, pw2 = np.exp(float(step) * np.log(b1)), np.exp(float(step) * np.log(b2))
    bc1, bc2s = 1.0 - pw1, np.sqrt(1.0 - pw2)
    return p - (lr / bc1) * m1 / (np.sqrt(v1) / bc2s + eps), m1, v1


def _amax(x):
    x = np.abs(x)
    return x.max() if x.size else x.dtype.type(0)


def errors(p1, m1, v1, ref):
    """(max|p - p_ref| / max|dp_ref|, max|m - m_ref| / max|m_ref|, the same for exp_avg_sq) of float64 results against
    adam_ref's tuple (at the same indices).  The update, not the parameter, is the denominator: comparing parameters with
    parameters hides an update error behind the factor lr."""
    pr, mr, vr, dp = ref
    tiny = 1e-300
    return (float(_amax(_lift(p1) - pr) / (_amax(dp) + tiny)), float(_amax(_lift(m1) - mr) / (_amax(mr) + tiny)),
            float(_amax(_lift(v1) - vr) / (_amax(vr) + tiny)))


def tolerances(name):
    return tuple(GPU_MARGIN * c for c in F64[name])
