"""Mean functions of the sparse GP models (reference: models/means.py, chosen by model_specs[0] through return_mean,
models/utils_models.py:285-294): 'zero', 'linear' m(x) = x a + b and 'identity' m(x) = x W.

The classes hold the parameters under the reference's names and shapes -- a (Dy, Dx, 1), b (Dy, 1, 1), W (Dy, Dx, 1) -- and
evaluate through the HIP kernels of csrc/tgp_mean.hip (ops.MeanFunction): there is no torch fallback, a CPU tensor raises.
One output GP (Dy = 1) in this build.
"""
import numpy
import torch
import torch.nn as nn

from . import config as cg
from . import ops

MEAN_NAMES = ("zero", "linear", "identity")


class ZeroMean(nn.Module):
    name = "zero"

    def forward(self, x):
        return torch.zeros(x.shape[:-1], dtype=x.dtype, device=x.device)


class _HipMean(nn.Module):
    """m(X) of one output through tgp_mean_forward_f64 / tgp_mean_backward_f64."""

    def _ab(self):
        raise NotImplementedError

    def _check(self, X):
        if self._ab()[0].shape[0] != 1:
            raise NotImplementedError("the '%s' mean function is built for one output GP (Dy = 1)" % self.name)
        X2 = X[0] if X.dim() == 3 else X
        if not X2.is_cuda:
            raise ops.L.TgpError("the '%s' mean function runs on the GPU only (got a %s tensor)" % (self.name, X2.device))
        return X2

    def _eval(self, X2, rowp, alpha, inp):
        a, b = self._ab()
        if torch.is_grad_enabled() and (a.requires_grad or (b is not None and b.requires_grad) or X2.requires_grad):
            return ops.MeanFunction.apply(X2, a, b, rowp, alpha, inp)
        return ops.mean_forward(X2.detach(), a.detach(), None if b is None else b.detach(), alpha=1.0 if rowp else alpha,
                                inp=None if rowp else inp, col=1 if rowp else 0, one_col=0 if rowp else -1)

    def forward(self, X):
        """m(X) of shape (Dy, MB, 1) for X (Dy, MB, Dx) or (MB, Dx), as the reference's __call__."""
        return self._eval(self._check(X), False, 1.0, None).reshape(1, -1, 1)

    def vector(self, X, alpha=1.0, inp=None):
        """alpha m(X) + inp as an (MB,) vector in one launch (inp (MB,) without gradient, or None)."""
        return self._eval(self._check(X), False, alpha, inp)

    def rowp(self, X):
        """The (MB, 2) row parameters (1, m(x_n)) of the per-row affine block at the head of a flow program."""
        return self._eval(self._check(X), True, 1.0, None)


class Linear(_HipMean):
    """m(x) = x a + b, a (Dy, Dx, 1) and b (Dy, 1, 1) trainable (models/means.py Linear).  a is drawn by numpy's randn after
    numpy.random.seed(config.config_seed), b starts at 0.  (The reference seeds with `cg.seed`, an attribute its config.py does not
    define -- its Linear cannot be built as it stands; the seed of the run, config_seed, is what it means.)"""
    name = "linear"

    def __init__(self, input_dim, output_dim):
        super().__init__()
        numpy.random.seed(cg.config_seed)
        self.a = nn.Parameter(torch.tensor(numpy.random.randn(output_dim, input_dim, 1), dtype=cg.dtype))
        self.b = nn.Parameter(torch.zeros(output_dim, 1, 1, dtype=cg.dtype))

    def _ab(self):
        return self.a, self.b


class Identity(_HipMean):
    """m(x) = x W with W (Dy, Dx, 1) a fixed buffer (models/means.py Identity; Salimbeni & Deisenroth's skip mean): the
    projection of return_projection_matrix, handed over as (Dx, Dy)."""
    name = "identity"

    def __init__(self, W, num_inputs, num_outputs):
        super().__init__()
        self.register_buffer("W", W.t().reshape(num_outputs, num_inputs, 1).to(cg.dtype).contiguous(), False)

    def _ab(self):
        return self.W, None


def return_projection_matrix(input_dim, output_dim, X):
    """(Dx, Dy) projection of the identity mean (models/utils_models.py:299-315): the identity for Dy = Dx, the identity padded
    with zero columns for Dy > Dx, the first Dy right singular vectors of X (PCA directions, numpy.linalg.svd on the host) for
    Dy < Dx.  A singular vector's sign is LAPACK's choice."""
    X = X.detach().to("cpu").numpy()
    if output_dim == input_dim:
        W = numpy.eye(input_dim)
    elif output_dim > input_dim:
        W = numpy.concatenate([numpy.eye(input_dim), numpy.zeros((input_dim, output_dim - input_dim))], 1)
    else:
        _, _, V = numpy.linalg.svd(X, full_matrices=False)
        W = V[:output_dim, :].T
    return torch.tensor(W, dtype=cg.dtype)


def return_mean(name, input_dim, output_dim, W=None):
    """models/utils_models.py:285-294."""
    if name == "zero":
        return ZeroMean()
    if name == "identity":
        return Identity(W, input_dim, output_dim)
    if name == "linear":
        return Linear(input_dim, output_dim)
    raise NotImplementedError("mean function '%s' is not implemented (have: %s)" % (name, ", ".join(MEAN_NAMES)))
