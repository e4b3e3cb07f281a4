"""Seeded synthetic workloads of the dataset shapes main.py trains on: what bench.py feeds the
engine and what a user without the UCI files can train on.  Product code, self-contained: the parity tests'
own generator is held to the same draws by tests/test_host_logic.py."""
import math

import numpy as np
import torch

from . import lib as L


def _isp(x):
    """Inverse softplus in float64 whatever the default dtype is (gpytorch.utils.transforms.inv_softplus)."""
    x = torch.as_tensor(x, dtype=torch.float64)
    return x + torch.log(-torch.expm1(-x))


class FlowProgram:
    """Accumulates (kind, K, offset, flags) blocks and the shared parameter vector they index."""

    def __init__(self):
        self.blocks, self.theta, self.row_cols = [], [], 0

    def affine(self):                       # dsp/flows.py: every block ends in an identity-initialised affine
        self.blocks.append((L.FLOW_AFFINE, 0, len(self.theta), 0))
        self.theta += [1.0, 0.0]

    def sal(self, per_row):                 # dsp/flows.py:115-136 (a=0, b=1 is the identity)
        if per_row:
            self.blocks.append((L.FLOW_SAL, 0, self.row_cols, L.FLAG_PER_ROW))
            self.row_cols += 2
        else:
            self.blocks.append((L.FLOW_SAL, 0, len(self.theta), 0))
            self.theta += [0.0, 1.0]

    def steptanh(self, K, rng):             # dsp/flows.py:239-277 StepTanhL initialisation, add_f0=True
        self.blocks.append((L.FLOW_STEPTANH, K, len(self.theta), L.FLAG_ADD_F0))
        for _ in range(K):
            e = rng.standard_normal(4)
            self.theta += [e[0], float(_isp(abs((e[1] + 1.0) / K))), e[2], float(_isp(abs((e[3] + 1.0) / K)))]

    def vector(self):
        return torch.tensor(self.theta, dtype=torch.float64)


def flow_program(flow, seed=0):
    """'sal<B>' | 'idsal<B>' | 'tanh<B>x<K>' | None -> (blocks, theta, per-row columns)."""
    if flow is None:
        return None, None, 0
    fp = FlowProgram()
    if flow.startswith("tanh"):
        nb, K = (int(t) for t in flow[4:].split("x"))
        rng = np.random.default_rng(seed)
        for _ in range(nb):
            fp.steptanh(K, rng)
            fp.affine()
    else:
        per_row = flow.startswith("idsal")
        for _ in range(int(flow[5 if per_row else 3:])):
            fp.sal(per_row)
            fp.affine()
    return fp.blocks, fp.vector(), fp.row_cols


# binary classification stand-ins of the paper's UCI classification sets: (rows, inputs)
BINARY_SHAPES = {"heart": (299, 12), "banknote": (1372, 4)}


def binary_dataset(name, seed=0):
    """Seeded binary data set of `name`'s shape: X ~ N(0, 1), latent f = 8 (sin(X w) + 0.5 x0), y ~ Bernoulli(Phi(f)).
    Returns numpy float64 X (n, d) and Y (n, 1) with labels in {0, 1}."""
    n, d = BINARY_SHAPES[name]
    rng = np.random.default_rng(7919 + 31 * seed + n)
    X = rng.standard_normal((n, d))
    w = rng.standard_normal(d) / math.sqrt(d)
    f = 8.0 * (np.sin(X @ w) + 0.5 * X[:, 0])
    p = 0.5 * np.array([math.erfc(-v / math.sqrt(2.0)) for v in f])
    Y = (rng.uniform(size=n) < p).astype(np.float64)
    return X, Y.reshape(-1, 1)


# count-regression stand-in: (rows, inputs)
COUNTS_SHAPE = (800, 2)


def counts_dataset(seed=0):
    """Seeded `synthetic_counts`: X ~ N(0, 1), y ~ Poisson(exp(1 + sin(2 x0) + 0.5 x1)).  Returns numpy float64 X (n, d) and
    Y (n, 1) with integer counts >= 0."""
    n, d = COUNTS_SHAPE
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, d))
    Y = rng.poisson(np.exp(1.0 + np.sin(2.0 * X[:, 0]) + 0.5 * X[:, 1]))
    return X, Y.astype(np.float64).reshape(-1, 1)


OVERDISPERSED_R = 2.0      # the dispersion of synthetic_overdispersed


def overdispersed_dataset(seed=0):
    """Seeded `synthetic_overdispersed`: the inputs and the latent log-mean of synthetic_counts, y ~ NB(mean = exp(1 + sin(2 x0)
    + 0.5 x1), r = OVERDISPERSED_R) drawn as a Gamma-Poisson mixture, y ~ Poisson(mean Gamma(r, 1) / r): Var = mean + mean^2 / r.
    Returns numpy float64 X (n, d) and Y (n, 1) with integer counts >= 0."""
    n, d = COUNTS_SHAPE
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, d))
    mean = np.exp(1.0 + np.sin(2.0 * X[:, 0]) + 0.5 * X[:, 1])
    Y = rng.poisson(mean * rng.gamma(OVERDISPERSED_R, 1.0 / OVERDISPERSED_R, size=n))
    return X, Y.astype(np.float64).reshape(-1, 1)


# ordinal-regression stand-in: (rows, inputs), the number of classes and the cuts of the latent that separate them
RATINGS_SHAPE = (800, 2)
RATINGS_CLASSES = 5
RATINGS_CUTS = (-1.0, -0.6, 0.3, 1.2)


def synthetic_ratings(seed=0):
    """Seeded `synthetic_ratings`: X ~ N(0, 1), latent h = sin(2 x0) + 0.5 x1, y = #{j : h + 0.3 eps > c_j} in {0, .., 4} with the
    UNEVENLY spaced cuts c = RATINGS_CUTS -- the spacing of the levels is what a flow under evenly spaced bin edges has to learn.
    Returns numpy float64 X (n, d) and Y (n, 1) with integer classes."""
    n, d = RATINGS_SHAPE
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, d))
    z = np.sin(2.0 * X[:, 0]) + 0.5 * X[:, 1] + 0.3 * rng.standard_normal(n)
    Y = (z.reshape(-1, 1) > np.asarray(RATINGS_CUTS).reshape(1, -1)).sum(1)
    return X, Y.astype(np.float64).reshape(-1, 1)


# positive-target stand-in: (rows, inputs) and the shape of the Gamma noise
CLAIMS_SHAPE = (500, 2)
CLAIMS_SHAPE_A = 3.0


def synthetic_claims(seed=0):
    """Seeded `synthetic_claims`: X ~ N(0, 1), y ~ Gamma(shape CLAIMS_SHAPE_A, mean exp(sin(2 x0) + 0.5 x1)) -- positive, skewed
    targets whose variance is proportional to their squared mean.  Returns numpy float64 X (n, d) and Y (n, 1), every y > 0."""
    n, d = CLAIMS_SHAPE
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, d))
    mean = np.exp(np.sin(2.0 * X[:, 0]) + 0.5 * X[:, 1])
    Y = np.maximum(mean * rng.gamma(CLAIMS_SHAPE_A, 1.0 / CLAIMS_SHAPE_A, size=n), np.finfo(np.float64).tiny)
    return X, Y.astype(np.float64).reshape(-1, 1)


# proportion stand-in: (rows, inputs), the precision of the Beta noise and how far the targets are kept from 0 and 1
PROPORTIONS_SHAPE = (500, 2)
PROPORTIONS_PRECISION = 10.0
PROPORTIONS_CLIP = 1e-6


def synthetic_proportions(seed=0):
    """Seeded `synthetic_proportions`: X ~ N(0, 1), y ~ Beta(mu phi, (1 - mu) phi) with phi = PROPORTIONS_PRECISION and
    mu = Phi(1.5 sin(2 x0) + 0.5 x1) -- the probit, on purpose not the logistic link of the likelihood, so that the flow has a
    link function to learn.  y is clipped to [PROPORTIONS_CLIP, 1 - PROPORTIONS_CLIP].  Returns numpy float64 X (n, d) and
    Y (n, 1), every y strictly inside (0, 1)."""
    from math import erf, sqrt
    n, d = PROPORTIONS_SHAPE
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, d))
    eta = 1.5 * np.sin(2.0 * X[:, 0]) + 0.5 * X[:, 1]
    mu = 0.5 * (1.0 + np.vectorize(erf)(eta / sqrt(2.0)))
    Y = np.clip(rng.beta(mu * PROPORTIONS_PRECISION, (1.0 - mu) * PROPORTIONS_PRECISION), PROPORTIONS_CLIP, 1.0 - PROPORTIONS_CLIP)
    return X, Y.astype(np.float64).reshape(-1, 1)


# robust-regression stand-in: (rows, inputs, training rows)
OUTLIERS_SHAPE = (1000, 2, 900)
OUTLIERS_SHARE = 0.1


def outliers_dataset(seed=0):
    """Seeded `synthetic_outliers`: X ~ N(0, 1), y = sin(2 x0) + 0.5 x1 + 0.1 eps, a smooth regression problem with Gaussian
    noise.  Returns numpy float64 X (n, d) and the CLEAN targets Y (n, 1); `gross_errors` corrupts a training split."""
    n, d, _ = OUTLIERS_SHAPE
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, d))
    Y = np.sin(2.0 * X[:, 0]) + 0.5 * X[:, 1] + 0.1 * rng.standard_normal(n)
    return X, Y.reshape(-1, 1)


def gross_errors(Y, seed=0, share=OUTLIERS_SHARE):
    """A copy of the targets Y (n, 1) with round(share n) seeded rows replaced by gross errors: +-(5 to 15), either sign, against
    clean targets of standard deviation ~0.9.  Returns (Y_dirty, the replaced rows' indices, sorted)."""
    rng = np.random.default_rng(seed + 7919)
    n = Y.shape[0]
    idx = np.sort(rng.choice(n, size=int(round(share * n)), replace=False))
    out = Y.copy()
    out[idx, 0] = rng.choice([-1.0, 1.0], size=idx.size) * rng.uniform(5.0, 15.0, size=idx.size)
    return out, idx


# input-relevance stand-in: (rows, inputs, training rows); inputs 2 .. 5 carry nothing
RELEVANCE_SHAPE = (1000, 6, 900)


def relevance_dataset(seed=0):
    """Seeded `synthetic_relevance`: X ~ N(0, 1)^6, y = sin(2 x0) + 0.5 x1 + 0.1 eps -- the targets depend on the first two inputs
    only, the other four carry nothing (what utils.input_relevance should report).  Returns numpy float64 X (n, d), Y (n, 1)."""
    n, d, _ = RELEVANCE_SHAPE
    rng = np.random.default_rng(32452843 + 31 * seed)
    X = rng.standard_normal((n, d))
    Y = np.sin(2.0 * X[:, 0]) + 0.5 * X[:, 1] + 0.1 * rng.standard_normal(n)
    return X, Y.reshape(-1, 1)


# input-dependent-noise stand-in: (rows, inputs, training rows) and the range of the noise standard deviation
HETERO_SHAPE = (1000, 2, 900)
HETERO_NOISE = (0.05, 1.0)


def hetero_noise_std(X):
    """The true noise standard deviation of `synthetic_hetero` at the rows of X (n, d): log-linear in x0 over [-2, 2], from
    HETERO_NOISE[0] at x0 = -2 to HETERO_NOISE[1] at x0 = 2."""
    lo, hi = HETERO_NOISE
    return lo * (hi / lo) ** ((np.asarray(X)[:, 0] + 2.0) / 4.0)


def hetero_dataset(seed=0):
    """Seeded `synthetic_hetero`: X ~ U(-2, 2)^2, y = sin(2 x0) + 0.5 x1 + sigma(x0) eps, a smooth mean under Gaussian noise whose
    standard deviation runs log-uniformly from 0.05 to 1.0 across x0 (hetero_noise_std).  mean log sigma = -1.50 against
    log sqrt(mean sigma^2) = -0.90: a perfect noise model gains about 0.6 nats per point over the best constant one.  Returns
    numpy float64 X (n, d), Y (n, 1) and sigma (n,), the rows' true noise standard deviation."""
    n, d, _ = HETERO_SHAPE
    rng = np.random.default_rng(15485863 + 31 * seed)
    X = rng.uniform(-2.0, 2.0, size=(n, d))
    sigma = hetero_noise_std(X)
    Y = np.sin(2.0 * X[:, 0]) + 0.5 * X[:, 1] + sigma * rng.standard_normal(n)
    return X, Y.reshape(-1, 1), sigma


# multi-class stand-in: (rows, inputs, classes)
BLOBS_SHAPE = (1200, 4, 4)


def blobs_dataset(seed=0):
    """Seeded `synthetic_blobs`: 4 Gaussian blobs in 4 dimensions, centres ~ 2 N(0, 1), unit noise, balanced labels in a
    seeded order.  Returns numpy float64 X (n, d) and Y (n, 1) with labels in {0, .., 3}."""
    n, d, k = BLOBS_SHAPE
    rng = np.random.default_rng(104729 + 31 * seed)
    centres = 2.0 * rng.standard_normal((k, d))
    y = rng.permutation(np.arange(n) % k)
    X = centres[y] + rng.standard_normal((n, d))
    return X, y.astype(np.float64).reshape(-1, 1)


def synthetic_problem(N, D, M, seed=0, flow="sal2", S=32, perturb=True):
    """X ~ N(0,1); Y = zscore(sin(Xw) + 0.1 x0^2 + 0.05 eps); Z = M rows of a seeded permutation; lengthscale 2,
    outputscale 2, noise 0.05; q(u): m ~ 0.5 N(0,1), Lq = sqrt(1e-5) I + 0.05 N(0,1) (dense -- the strict upper
    part must be ignored by the consumer); SAL parameters = identity + 0.3 N(0,1), StepTanhL at its own init."""
    f64 = torch.float64
    gd = torch.Generator().manual_seed(seed)            # data stream
    X = torch.randn(N, D, generator=gd, dtype=f64)
    w = torch.randn(D, generator=gd, dtype=f64)
    Y = torch.sin(X @ w) + 0.1 * X[:, 0] ** 2 + 0.05 * torch.randn(N, generator=gd, dtype=f64)
    Y = ((Y - Y.mean()) / Y.std()).reshape(N, 1)
    Z = X[torch.randperm(N, generator=gd)[:M]].clone()

    gp = torch.Generator().manual_seed(seed + 1)        # parameter stream (draw order matters)
    m = torch.zeros(M, dtype=f64)
    Lam = math.sqrt(1e-5) * torch.eye(M, dtype=f64)
    rls = _isp(torch.full((D,), 2.0))
    if perturb:
        m = 0.5 * torch.randn(M, generator=gp, dtype=f64)
        Lam = Lam + 0.05 * torch.randn(M, M, generator=gp, dtype=f64)
        rls = rls + 0.1 * torch.randn(D, generator=gp, dtype=f64)
    params = {"Z": Z, "raw_lengthscale": rls, "raw_outputscale": _isp(2.0).reshape(1), "m": m, "Lam": Lam,
              "log_var_noise": torch.log(torch.tensor([0.05], dtype=f64))}

    program, theta, row_cols = flow_program(flow, seed)
    rowp = None
    if program is not None:
        if perturb and not flow.startswith("tanh"):
            theta = theta + 0.3 * torch.randn(theta.shape, generator=gp, dtype=f64)
        params["theta"] = theta
        if row_cols:
            ident = torch.tensor([0.0, 1.0] * (row_cols // 2), dtype=f64)
            rowp = ident.reshape(1, -1) + 0.2 * torch.randn(N, row_cols, generator=gp, dtype=f64)
    x, wq = np.polynomial.hermite.hermgauss(int(S))
    return {"X": X, "Y": Y, "params": params, "program": program, "xs": torch.tensor(x, dtype=f64),
            "ws": torch.tensor(wq, dtype=f64), "rowp": rowp, "N_total": float(N)}
