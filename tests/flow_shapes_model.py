"""Float64 torch restatement of the sinh, normal-CDF, Tukey g-and-h, exp and softplus flow kinds: test infrastructure only.

Written from the formulas of include/tgp_hip.h (x = (f - c)/d; sp = softplus):
    7  SINH      g = a + b sinh(x) [+ f]                      RESTRICT: b = sp(b), d = sp(d)
    8  NORMCDF   g = a + b Phi(x) [+ f]                       same rule
    9  TUKEY     g = expm1(gam f)/gam * exp(h f^2/2)          h = sp(h_raw) always; gam = raw (flags 0), sp(raw) (RESTRICT),
                                                              -sp(raw) (RESTRICT | NEGATE); gam == 0 is taken as 1e-11
    10 EXP       g = exp(f)
    11 SOFTPLUS  g = log(1 + exp(f)), g = f for f > 20 (torch.nn.functional.softplus)
Derivatives come from torch autograd, never from a second set of hand-written formulas.  `flow` also knows AFFINE (0), SAL (1)
and ARCSINH (3) so that mixed chains can be stated; every other kind goes to the oracle's own flow_forward.

`patched()` makes oracle.tgp_oracle.flow_forward know these kinds for the length of a `with` block (kernel_family_model.patched's
pattern: the attribute is swapped at run time, no file of the oracle changes): inside it orc.elbo_and_grads is the whole step's
CPU truth for a program that holds them."""
import contextlib
import math

import torch
from torch.nn.functional import softplus

from oracle import tgp_oracle as orc

F64 = torch.float64
AFFINE, SAL, STEPTANH, ARCSINH, BOXCOX, INV_BOXCOX = 0, 1, 2, 3, 4, 5
SINH, NORMCDF, TUKEY, EXP, SOFTPLUS = 7, 8, 9, 10, 11
RESTRICT, ADD_F0, PER_ROW, NEGATE = 1, 2, 4, 8
MINE = (SINH, NORMCDF, TUKEY, EXP, SOFTPLUS)
NPARAMS = {AFFINE: 2, SAL: 2, ARCSINH: 4, BOXCOX: 1, INV_BOXCOX: 1, SINH: 4, NORMCDF: 4, TUKEY: 2, EXP: 0, SOFTPLUS: 0}


def Phi(x):
    return 0.5 * torch.erfc(-x / math.sqrt(2.0))


def _asinh_ref(x):
    return torch.log(x + (x ** 2 + 1) ** 0.5)


def block(f, kind, flags, t):
    """One block of the kinds this file states; t = the block's raw parameters."""
    R, A = flags & RESTRICT, flags & ADD_F0
    if kind == AFFINE:
        return (softplus(t[0]) if R else t[0]) * f + t[1]
    if kind == SAL:
        g = torch.sinh((softplus(t[1]) if R else t[1]) * _asinh_ref(f) - t[0])
    elif kind in (ARCSINH, SINH, NORMCDF):
        b, d = (softplus(t[1]), softplus(t[3])) if R else (t[1], t[3])
        x = (f - t[2]) / d
        g = t[0] + b * {ARCSINH: _asinh_ref, SINH: torch.sinh, NORMCDF: Phi}[kind](x)
    elif kind == TUKEY:
        gam = t[0]
        if R:
            gam = -softplus(gam) if flags & NEGATE else softplus(gam)
        elif float(gam.detach()) == 0.0:
            gam = gam + 1e-11
        return torch.expm1(gam * f) / gam * torch.exp(softplus(t[1]) * f ** 2 / 2)
    elif kind == EXP:
        return torch.exp(f)
    elif kind == SOFTPLUS:
        return softplus(f)
    else:
        raise ValueError("flow_shapes_model states no kind %r" % (kind,))
    return g + f if A else g


def flow(f, program, theta):
    """The whole program (shared parameters) on f; kinds this file does not state go to the oracle's flow_forward."""
    for kind, K, poff, flags in program:
        if kind in NPARAMS and not (flags & PER_ROW):
            f = block(f, kind, flags, [theta[poff + j] for j in range(NPARAMS[kind])])
        else:
            f = _ORIG(f, [(kind, K, poff, flags)], theta)
    return f


_ORIG = orc.flow_forward


@contextlib.contextmanager
def patched():
    """Inside the block oracle.tgp_oracle.flow_forward knows kinds 7 .. 11 (and ARCSINH): programs that hold one go to `flow`,
    every other program to the oracle's own code."""
    def f(x, program, theta, rowp=None):
        if any(b[0] in MINE for b in program):
            assert rowp is None or not any(b[3] & PER_ROW for b in program)
            return flow(x, program, theta)
        return _ORIG(x, program, theta, rowp)
    orc.flow_forward = f
    try:
        yield orc
    finally:
        orc.flow_forward = _ORIG


# ---- programs and raw parameters the GPU and host tests share -------------------------------------------------------------
R_, A_, N_ = RESTRICT, ADD_F0, NEGATE
PROGRAMS = {
    "sinh": [(SINH, 0, 0, 0)], "sinh_r": [(SINH, 0, 0, R_)], "sinh_rf0": [(SINH, 0, 0, R_ | A_)],
    "ncdf": [(NORMCDF, 0, 0, 0)], "ncdf_r": [(NORMCDF, 0, 0, R_)], "ncdf_rf0": [(NORMCDF, 0, 0, R_ | A_)],
    "tukey": [(TUKEY, 0, 0, 0)], "tukey_right": [(TUKEY, 0, 0, R_)], "tukey_left": [(TUKEY, 0, 0, R_ | N_)],
    "exp": [(EXP, 0, 0, 0)], "softplus": [(SOFTPLUS, 0, 0, 0)],
    # SAL, affine, arcsinh and all five: theta offsets 0 2 4 8 12 14 18 20 (exp and softplus take none)
    "chain": [(SAL, 0, 0, R_), (AFFINE, 0, 2, 0), (SINH, 0, 4, R_), (ARCSINH, 0, 8, R_ | A_), (TUKEY, 0, 12, R_ | N_),
              (NORMCDF, 0, 14, R_ | A_), (AFFINE, 0, 18, 0), (SOFTPLUS, 0, 20, 0), (AFFINE, 0, 20, R_), (EXP, 0, 22, 0)],
}
THETA = {
    "sinh": [0.3, 1.2, -0.4, 1.8], "sinh_r": [0.3, 0.2, -0.4, 1.5], "sinh_rf0": [-0.2, 0.4, 0.3, 1.1],
    "ncdf": [-0.5, 2.2, 0.2, 1.3], "ncdf_r": [0.1, 1.5, -0.3, 0.4], "ncdf_rf0": [-0.2, 0.4, 0.3, -0.1],
    # |gam| >= 0.1: raw -2.2 -> softplus = 0.105
    "tukey": [0.35, -2.5], "tukey_right": [-1.2, -3.0], "tukey_left": [-2.2, -2.0],
    "exp": [], "softplus": [],
    "chain": [0.1, 0.4, 0.9, 0.2, 0.2, 0.1, -0.3, 1.4, -0.2, 0.4, 0.3, 0.6, -2.0, -3.5, -0.3, 0.8, 0.1, 0.5, 0.4, -0.2,
              -1.5, 0.1],
}
P_OF = {k: len(v) for k, v in THETA.items()}


def f_values(name, n=700, seed=7):
    """3 x n points f = 2 randn; |f| <= 4 for the kinds that grow exponentially (SINH, TUKEY) and the chain."""
    g = torch.Generator().manual_seed(seed)
    f = 2.0 * torch.randn(3, n, generator=g, dtype=F64)
    if name.startswith(("sinh", "tukey")):
        f = f.clamp(-4.0, 4.0)
    if name == "chain":
        f = f.clamp(-2.5, 2.5)
    return f
