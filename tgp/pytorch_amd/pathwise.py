"""Pathwise posterior function draws (Wilson et al. 2020, "Efficiently sampling functions from Gaussian process posteriors").

A draw of the sparse GP posterior is a fixed weight vector over 2 R2 random Fourier features of the prior and the M kernel
columns at the inducing points (ops.pathwise_coeff); it is then a function that ops.pathwise_eval evaluates on any rows, in any
batches, consistently, in O(N (R2 + M) S).  The inducing-point update is exact; the Fourier part approximates the prior only."""
import copy

import torch

from . import ops
from .flow import compile_flow, nets_rowp


# the kernels whose spectral density this module samples: a set of its own, not lib.KERNELS ('scale_matern52' evaluates on the
# device like the others but its sampler, Student-t frequencies with 5 degrees of freedom, is not here yet)
SPECTRAL_KERNELS = ("scale_rbf", "scale_matern32", "scale_rq")


def spectral_frequencies(kernel_name, R2, D, generator=None, device=None, alpha=None):
    """omega (R2, D) float64: frequencies of the unit-length-scale kernel, drawn on the host from `generator` (a seeded CPU
    torch.Generator; None: torch's global one).  'scale_rbf': N(0, I_D).  'scale_matern32': g sqrt(3 / c) row-wise with
    g ~ N(0, I_D) and c ~ chi^2(3) -- the multivariate Student-t with 2 nu = 3 degrees of freedom.  'scale_rq': g sqrt(tau)
    row-wise with tau ~ Gamma(shape alpha, rate alpha) -- the kernel is the RBF of precision tau averaged over that law; `alpha`
    is required for it (lib.RQ_MIN_ALPHA .. lib.RQ_MAX_ALPHA) and read by no other kernel."""
    if kernel_name not in SPECTRAL_KERNELS:
        raise ops.L.TgpError("kernel '%s' has no spectral sampler (have: %s)" % (kernel_name, ", ".join(SPECTRAL_KERNELS)))
    R2, D = int(R2), int(D)
    if R2 < 1 or D < 1:
        raise ValueError("spectral_frequencies: R2 >= 1, D >= 1")
    g = torch.randn(R2, D, dtype=torch.float64, generator=generator)
    if kernel_name == "scale_matern32":
        c = torch.randn(R2, 3, dtype=torch.float64, generator=generator).pow(2).sum(1, keepdim=True)
        g = g * torch.sqrt(3.0 / c)
    elif kernel_name == "scale_rq":
        if alpha is None:
            raise ops.L.TgpError("spectral_frequencies: 'scale_rq' needs its alpha")
        a = ops.check_rq_alpha(alpha)
        tau = torch._standard_gamma(torch.full((R2, 1), a, dtype=torch.float64), generator=generator) / a
        g = g * torch.sqrt(tau)
    return g if device is None else g.to(device)


class PosteriorPaths:
    """S drawn posterior functions.  Holds detached clones of Z, raw_ls, raw_os, omega and coef, the kernel's name and frozen
    copies of the model's mean function and flow: a later optimiser step does not change a drawn function.

    paths.f0(X)  (S, N): the latent draws, plus the mean function where the model has one
    paths(X)     (S, N): the same values through the flow, with the per-row parameters of an input-dependent flow
    paths.grad_f0(X), paths.grad(X)  (S, N, D): their gradients in the rows of X (a flow with per-row networks: refused)
    `batch_rows` evaluates a large X in pieces of that many rows; the values are the same bits."""

    def __init__(self, Z, raw_ls, raw_os, omega, coef, kernel, mean_function=None, flow=None):
        self.Z, self.raw_ls, self.raw_os, self.omega, self.coef = (t.detach().clone().contiguous()
                                                                   for t in (Z, raw_ls, raw_os, omega, coef))
        self.kernel = str(kernel)
        self.mean_function = copy.deepcopy(mean_function)
        self.flow = copy.deepcopy(flow)
        if self.flow is not None:
            self.flow.eval()      # a point estimate: the parameter networks' dropout stays off
        self.S = int(self.coef.shape[1])
        self.num_frequencies = int(self.omega.shape[0])

    def _rows(self, X):
        X2 = X[0] if X.dim() == 3 else X
        if X2.dim() != 2 or X2.shape[1] != self.Z.shape[1]:
            raise ValueError("PosteriorPaths: X (N, %d)" % self.Z.shape[1])
        return X2.detach().contiguous()

    def _f0(self, X2):
        f0 = ops.pathwise_eval(X2, self.Z, self.raw_ls, self.raw_os, self.omega, self.coef, kernel=self.kernel)
        if self.mean_function is not None:
            f0 += self.mean_function.vector(X2).detach().reshape(1, -1)
        return f0

    def _flowed(self, X2):
        f0 = self._f0(X2)
        if self.flow is None:
            return f0
        spec, theta_list, nets = compile_flow(self.flow)
        if spec.nblk == 0:
            return f0
        theta = torch.stack([p.detach().reshape(()) for p in theta_list]).to(f0.device) if theta_list else None
        rowp = nets_rowp(nets, X2) if nets else None
        return ops.flow_eval(f0, spec, theta, rowp, want=("G",))["G"]

    def _grad_f0(self, X2):
        g = ops.pathwise_grad(X2, self.Z, self.raw_ls, self.raw_os, self.omega, self.coef, kernel=self.kernel)
        if self.mean_function is not None:      # the slope of m(x) = x a + b (identity: a = W)
            g = g + self.mean_function._ab()[0].detach().reshape(1, 1, -1).to(g.device)
        return g

    def _grad_flowed(self, X2):
        g = self._grad_f0(X2)
        if self.flow is None:
            return g
        spec, theta_list, nets = compile_flow(self.flow)
        if spec.nblk == 0:
            return g
        f0 = self._f0(X2)
        theta = torch.stack([p.detach().reshape(()) for p in theta_list]).to(f0.device) if theta_list else None
        dG = ops.flow_eval(f0, spec, theta, None, want=("dG",))["dG"]
        return dG.unsqueeze(2) * g

    def _grad_pieces(self, fn, X, batch_rows):
        X2 = self._rows(X)
        N = X2.shape[0]
        with torch.no_grad():
            if batch_rows is None or int(batch_rows) >= N:
                return fn(X2)
            step = int(batch_rows)
            if step < 1:
                raise ValueError("PosteriorPaths: batch_rows >= 1")
            out = torch.empty(self.S, N, X2.shape[1], dtype=torch.float64, device=X2.device)
            for a in range(0, N, step):
                b = min(N, a + step)
                out[:, a:b] = fn(X2[a:b])
            return out

    def grad_f0(self, X, batch_rows=None):
        """(S, N, D): d f0_s(x_n) / d x_nd of the latent draws (ops.pathwise_grad), plus the mean function's slope."""
        return self._grad_pieces(self._grad_f0, X, batch_rows)

    def grad(self, X, batch_rows=None):
        """(S, N, D): the gradient of paths(X) in the rows, G'(f0_s(x_n)) grad_f0.  NotImplementedError for a flow with
        input-dependent parameters."""
        if self.flow is not None and compile_flow(self.flow)[2]:
            raise NotImplementedError("PosteriorPaths.grad: the flow has input-dependent parameters -- its per-row parameters "
                                      "depend on x through the networks, and that path has no input gradient")
        return self._grad_pieces(self._grad_flowed, X, batch_rows)

    def _pieces(self, fn, X, batch_rows):
        X2 = self._rows(X)
        N = X2.shape[0]
        with torch.no_grad():
            if batch_rows is None or int(batch_rows) >= N:
                return fn(X2)
            step = int(batch_rows)
            if step < 1:
                raise ValueError("PosteriorPaths: batch_rows >= 1")
            out = torch.empty(self.S, N, dtype=torch.float64, device=X2.device)
            for a in range(0, N, step):
                b = min(N, a + step)
                out[:, a:b] = fn(X2[a:b])
            return out

    def f0(self, X, batch_rows=None):
        return self._pieces(self._f0, X, batch_rows)

    def __call__(self, X, batch_rows=None):
        return self._pieces(self._flowed, X, batch_rows)


def draw_paths(Z, raw_ls, raw_os, m, Lam, kernel, S, num_frequencies=1024, generator=None, jitter=0.0, info=None,
               mean_function=None, flow=None):
    """PosteriorPaths of S draws of the whitened q(u) = N(m, Lam Lam^T) at these hyper-parameters: omega, W (S, 2 R2) and
    eps (S, M) come from `generator` on the host, in that order; the coefficients from ops.pathwise_coeff."""
    S, R2 = int(S), int(num_frequencies)
    M, D = Z.shape
    # (the RQ kernel's alpha sits behind the raw output scale: ops.rq_scale)
    omega = spectral_frequencies(kernel, R2, D, generator, alpha=float(raw_os.reshape(-1)[1]) if kernel == "scale_rq" else None)
    W = torch.randn(S, 2 * R2, dtype=torch.float64, generator=generator)
    eps = torch.randn(S, M, dtype=torch.float64, generator=generator)
    dev = Z.device
    omega, W, eps = omega.to(dev), W.to(dev), eps.to(dev)
    coef = ops.pathwise_coeff(Z, raw_ls, raw_os, m, Lam, omega, W, eps, jitter=jitter, kernel=kernel, info=info)
    return PosteriorPaths(Z, raw_ls, raw_os, omega, coef, kernel, mean_function, flow)


__all__ = ["spectral_frequencies", "PosteriorPaths", "draw_paths"]
