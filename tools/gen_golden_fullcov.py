"""Generate the fixtures of the full-covariance q(f) (tests/golden/fullcov_*.npz) by executing the reference's own
files (build container only; never runs on the GPU box).

Run:  python tools/gen_golden_fullcov.py

The reference on sys.path with the oracle/shims stand-ins, build_reference_model and the parameter recipe come from
oracle/gen_golden.py, imported read-only.  Each case calls the reference's

    marginal_variational_qf_parameters(X, diagonal=False, is_duvenaud=False, init_Z=None)      (sparse_MF_SP.py:384)

on a build_reference_model model.  That branch subtracts a tensor from what the kernel returns for K_xx; a real gpytorch
lazy tensor supports the subtraction, the stand-in's `_Dense` does not.  This file gives `_Dense` a `__sub__` AT RUN TIME,
here and nowhere else (oracle/ stays as it is): `_Dense - tensor` is the dense difference.

Each fixture stores X, the parameters (p_*, the flow's program), the reference's mu (N) and Sigma (N, N), eps (4, N) from a seeded generator
and the kernel name.  The generator's own checks per case: the diagonal of Sigma against the reference's diagonal=True
variance, the closed form K + A^T W A of tests/fullcov_model.py against Sigma, and the smallest eigenvalue of Sigma (printed).
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

from oracle import gen_golden as gg        # noqa: E402  (sets up the reference, the shims and float64)

import numpy as np                          # noqa: E402
import torch                                # noqa: E402
from gpytorch import kernels as shim_kernels   # noqa: E402  (the stand-in of oracle/shims)

from oracle import tgp_oracle as orc        # noqa: E402
import fullcov_model as fm                  # noqa: E402

# the subtraction a real gpytorch lazy tensor has (see the docstring)
shim_kernels._Dense.__sub__ = lambda self, other: self._t - other

#        fixture                 N    D   M    flow       kernel
CASES = (("fullcov_tiny_svgp", 37, 4, 5, None, "scale_rbf"),
         ("fullcov_med_sal2", 130, 4, 100, "sal2", "scale_rbf"),
         ("fullcov_bigm_matern", 150, 13, 150, "tanh3x2", "scale_matern32"))


def one(name, N, D, M, flow, kernel):
    prob = orc.synthetic_problem(N, D, M, seed=3, flow=flow, S=8)
    model = gg.build_reference_model(prob, flow, kernel)
    X, p = prob["X"], prob["params"]
    with torch.no_grad():
        mu, Sigma = model.marginal_variational_qf_parameters(X, diagonal=False, is_duvenaud=False, init_Z=None)
        mu_d, v_d = model.marginal_variational_qf_parameters(X, diagonal=True, is_duvenaud=False, init_Z=None)
    mu, Sigma = mu.reshape(N), Sigma.reshape(N, N)
    assert float((mu - mu_d.reshape(N)).abs().max()) == 0.0
    d_diag = float((Sigma.diagonal() - v_d.reshape(N)).abs().max())
    mu_c, Sig_c = fm.qf_cov(X, p["Z"], p["raw_lengthscale"], p["raw_outputscale"], p["m"], p["Lam"], kernel=kernel)
    d_closed = float((Sig_c - Sigma).abs().max())
    lam_min = float(torch.linalg.eigvalsh(0.5 * (Sigma + Sigma.t())).min())
    print("%s: max|Sigma| %.3g  |diag - v| %.2g  |closed form - Sigma| %.2g  |mu_c - mu| %.2g  min eig %.3g"
          % (name, float(Sigma.abs().max()), d_diag, d_closed, float((mu_c - mu).abs().max()), lam_min))
    assert d_diag < 1e-12 and d_closed < 1e-12, name
    g = torch.Generator().manual_seed(4000 + N)
    out = {"X": X, "mu": mu, "Sigma": Sigma, "eps": torch.randn(4, N, generator=g, dtype=torch.float64),
           "kernel": np.array(kernel)}
    for k, v in p.items():
        out["p_" + k] = v
    if prob["program"] is not None:
        out["program"] = np.array(prob["program"], dtype=np.int32)
    gg.save(name, out)


def main():
    for case in CASES:
        one(*case)


if __name__ == "__main__":
    main()
