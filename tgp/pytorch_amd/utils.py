"""Small helpers with the reference's names (code/dsp/utils.py)."""
import torch

from . import config as cg


def inv_softplus(x):
    """gpytorch.utils.transforms.inv_softplus."""
    x = torch.as_tensor(x, dtype=torch.get_default_dtype())
    return x + torch.log(-torch.expm1(-x))


def positive_transform(x):
    """dsp/utils.py:39-46 ('exp' is the only transform main.py configures)."""
    if cg.positive_transform == "exp":
        return torch.exp(x)
    if cg.positive_transform == "softplus":
        return torch.log(torch.exp(x) + 1)
    raise NotImplementedError("positive_transform function %s is not implemented." % cg.positive_transform)


def inverse_positive_transform(x):
    if cg.positive_transform == "exp":
        return torch.log(x)
    if cg.positive_transform == "softplus":
        return torch.log(torch.exp(x) - 1.0)
    raise NotImplementedError("inverse_positive_transform for %s is not implemented." % cg.positive_transform)


def KMEANS(X, num_Z, n_init=1, seed=None, backend="hip", max_iter=300, tol=1e-4, return_info=False):
    """Inducing-point initialisation (dsp/utils.py:143-159).  The reference calls
    sklearn.cluster.KMeans(n_clusters, init='k-means++', n_init, random_state=seed).fit(X) on the host; `backend='hip'`
    runs the same algorithm on the GPU -- sklearn 1.x's sequence restated: centre X, k-means++ seeding with
    2 + log(k) local trials, Lloyd iterations until the labels repeat or the squared centre shift drops under
    tol * mean(var(X)), best of n_init by inertia -- with the random draws taken from the same
    numpy RandomState(seed) in the same order, so that the result agrees with sklearn's up to floating-point
    rounding of the distances (tests/test_gpu_models.py).  `backend='sklearn'` is the reference's own call."""
    if seed is None:
        seed = cg.config_seed
    if backend == "sklearn":
        from sklearn.cluster import KMeans
        km = KMeans(n_clusters=num_Z, init="k-means++", n_init=n_init, random_state=seed).fit(X.to("cpu").numpy())
        return torch.tensor(km.cluster_centers_, dtype=cg.dtype).to(cg.device)
    if backend != "hip":
        raise ValueError("KMEANS backend must be 'hip' or 'sklearn'")
    import numpy as np
    from . import lib as L
    from . import ops
    lib = L.load()
    if not torch.cuda.is_available():
        raise L.TgpError("KMEANS(backend='hip') needs a HIP device; backend='sklearn' is the reference's host path")
    dev = X.device if X.is_cuda else torch.device("cuda", torch.cuda.current_device())
    Xd = X.detach().to(dev, torch.float64).contiguous()
    N, D = Xd.shape
    K = int(num_Z)
    if D > 16:
        raise L.TgpError("KMEANS(backend='hip'): D <= 16")
    st = L.stream_ptr
    tolv = float(Xd.var(dim=0, unbiased=False).mean()) * tol          # sklearn _tolerance (before centring)
    Xmean = Xd.mean(dim=0)
    Xc = (Xd - Xmean).contiguous()                                       # KMeans.fit: X -= X.mean(axis=0)
    rs = np.random.RandomState(seed)                                     # check_random_state(int)
    T = 2 + int(np.log(K))                                               # n_local_trials
    labels = torch.empty(N, dtype=torch.int32, device=dev)
    mind2 = torch.empty(N, dtype=torch.float64, device=dev)
    trial = torch.empty(max(T, 1), N, dtype=torch.float64, device=dev)

    def assign(C):
        L.check(lib.tgp_kmeans_assign_f64(L.ptr(Xc), N, D, L.ptr(C), K, L.ptr(labels), L.ptr(mind2), st()), "tgp_kmeans_assign_f64")

    def seeding():
        """sklearn.cluster._kmeans._kmeans_plusplus with unit sample weights."""
        centers = torch.empty(K, D, dtype=torch.float64, device=dev)
        cid = int(rs.choice(N, p=np.full(N, 1.0 / N)))
        centers[0] = Xc[cid]
        cand = torch.tensor([cid], dtype=torch.int64, device=dev)
        L.check(lib.tgp_kmeans_pp_f64(L.ptr(Xc), N, D, L.ptr(cand), 1, None, L.ptr(trial), st()), "tgp_kmeans_pp_f64")
        closest = trial[0].clone()
        pot = closest.sum()
        for c in range(1, K):
            rv = torch.from_numpy(rs.uniform(size=T)).to(dev) * pot
            cand = torch.searchsorted(torch.cumsum(closest, 0), rv).clamp_(max=N - 1)
            L.check(lib.tgp_kmeans_pp_f64(L.ptr(Xc), N, D, L.ptr(cand), T, L.ptr(closest), L.ptr(trial), st()),
                    "tgp_kmeans_pp_f64")
            pots = trial[:T].sum(dim=1)
            best = torch.argmin(pots)
            pot = pots[best]
            closest = trial[best].clone()
            centers[c] = Xc[cand[best]]
        return centers

    def lloyd(C):
        """sklearn _kmeans_single_lloyd: returns (labels, inertia, centers, n_iter)."""
        C = C.clone()
        labels_old = torch.full((N,), -1, dtype=torch.int32, device=dev)
        strict = False
        it = 0
        for it in range(max_iter):
            assign(C)
            order = torch.argsort(labels, stable=True)
            counts = torch.bincount(labels, minlength=K)
            offs = torch.zeros(K + 1, dtype=torch.int64, device=dev)
            offs[1:] = torch.cumsum(counts, 0)
            sums = torch.empty(K, D, dtype=torch.float64, device=dev)
            L.check(lib.tgp_kmeans_segsum_f64(L.ptr(Xc), D, L.ptr(order), L.ptr(offs), K, L.ptr(sums), st()),
                    "tgp_kmeans_segsum_f64")
            w = counts.to(torch.float64)
            if int((counts == 0).sum()) > 0:
                # sklearn _relocate_empty_clusters_dense: the farthest points become the empty clusters' centres
                empty = torch.nonzero(counts == 0).reshape(-1)
                far = torch.argsort(mind2, descending=True)[: empty.numel()]
                for e, f in zip(empty.tolist(), far.tolist()):
                    old = int(labels[f])
                    sums[old] -= Xc[f]
                    sums[e] = Xc[f]
                    w[e] = 1.0
                    w[old] -= 1.0
            Cn = sums / w.reshape(-1, 1)
            shift2 = float(((Cn - C) ** 2).sum())
            C = Cn
            if torch.equal(labels, labels_old):
                strict = True
                break
            if shift2 <= tolv:
                break
            labels_old.copy_(labels)
        if not strict:
            assign(C)                      # E-step again so that the labels match the returned centres
        inertia = float(((Xc - C[labels.to(torch.int64)]) ** 2).sum())
        return labels.clone(), inertia, C, it + 1

    best = None
    for _ in range(int(n_init)):
        lab, inertia, C, nit = lloyd(seeding())
        if best is None or (inertia < best[1] and not _same_clustering(lab, best[0], K)):
            best = (lab, inertia, C, nit)
    centers = best[2] + Xmean
    Z = centers.to(cg.dtype).to(cg.device)
    if return_info:
        return Z, {"inertia": best[1], "n_iter": best[3], "labels": best[0]}
    return Z


def _hip_device(X, who):
    """The device a selection on X runs on: X's own when it lives on one, else the current HIP device."""
    from . import lib as L
    if X.is_cuda:
        return X.device
    if not torch.cuda.is_available():
        raise L.TgpError("%s needs a HIP device" % who)
    return torch.device("cuda", torch.cuda.current_device())


def GREEDY_VARIANCE(X, num_Z, kernel, min_var=1e-8, return_info=False):
    """Inducing-point initialisation by greedy conditional-variance selection, the pivoted Cholesky factorisation of K_XX (Burt,
    Rasmussen, van der Wilk 2020): the num_Z rows of X that greedily most reduce tr(K_XX - Q_XX) under `kernel`, a
    kernels.ScaleKernel whose name and raw parameters (output 0) are read as they stand (ops.greedy_inducing on the GPU).
    Returns Z (num_Z, D), rows of X bit for bit; with return_info=True also {"idx": (num_Z,) int64, "trace": (num_Z + 1,)},
    trace[j] = tr(K_XX - Q_XX) with the first j rows picked -- the term of the collapsed bound that Z controls.  A model needs
    exactly num_Z rows: ValueError when fewer clear min_var (the jitter K_ZZ gets anyway: such a row conditions K_ZZ + jitter I
    no better than a duplicate would)."""
    from . import kernels
    from . import lib as L
    from . import ops
    if not isinstance(kernel, kernels.ScaleKernel):
        raise TypeError("GREEDY_VARIANCE: kernel must be a kernels.ScaleKernel (instance_kernel builds one), got %s"
                        % type(kernel).__name__)
    if X.dim() != 2:
        raise ValueError("GREEDY_VARIANCE: X (N, D), got shape %s" % (tuple(X.shape),))
    N, D = X.shape
    num_Z = int(num_Z)
    if not 1 <= num_Z <= N:
        raise ValueError("GREEDY_VARIANCE: 1 <= num_Z <= N = %d, got %d" % (N, num_Z))
    raw_ls, raw_os = kernel._params()
    if raw_ls.numel() not in (1, D):
        raise ValueError("GREEDY_VARIANCE: the kernel has %d length-scales, X has %d columns" % (raw_ls.numel(), D))
    if not min_var >= 0.0:
        raise ValueError("GREEDY_VARIANCE: min_var >= 0, got %r" % (min_var,))
    dev = _hip_device(X, "GREEDY_VARIANCE")
    Xd = X.detach().to(dev, torch.float64).contiguous()
    raw_ls = raw_ls.to(dev, torch.float64).expand(D).contiguous()
    idx, Z, trace, m_eff = ops.greedy_inducing(Xd, num_Z, raw_ls, raw_os.to(dev, torch.float64), kernel=kernel.hip_kernel,
                                               min_var=min_var)
    if m_eff < num_Z:
        raise ValueError("GREEDY_VARIANCE: M_eff = %d of the %d rows asked for have a conditional variance above min_var = %g; "
                         "ask for at most M_eff inducing points or lower min_var" % (m_eff, num_Z, min_var))
    Z = Z.to(cg.dtype).to(cg.device)
    if return_info:
        return Z, {"idx": idx, "trace": trace}
    return Z


def _same_clustering(a, b, K):
    """sklearn _is_same_clustering: equal up to a permutation of the labels."""
    m = torch.full((K,), -1, dtype=torch.int64, device=a.device)
    a64, b64 = a.to(torch.int64), b.to(torch.int64)
    m[a64] = b64                      # last write wins; consistent mapping <=> m[a] == b everywhere
    return bool(torch.equal(m[a64], b64))


def psd_safe_cholesky(A, upper=False, out=None, jitter=None):
    """dsp/utils.py:222-270 on the GPU (HIP blocked Cholesky + the reference's jitter ladder): (L, A_used)."""
    from . import ops
    if cg.constant_jitter is not None:
        A.diagonal(dim1=-2, dim2=-1).add_(cg.constant_jitter)
    squeeze = A.dim() == 3
    A2 = A[0] if squeeze else A
    L, Ap = ops.psd_safe_cholesky(A2, jitter)
    if upper:
        L = L.transpose(-1, -2)
    return (L.unsqueeze(0), Ap.unsqueeze(0)) if squeeze else (L, Ap)


# ---------------------------------------------------------------------------------------------------
# confidence intervals (dsp/models/utils_models.py:33-140)
# ---------------------------------------------------------------------------------------------------
def confidence_intervals(model, X, intervals, S, distribution, is_deep, exact=False):
    """Point-wise intervals at the rows of X: a list over the outputs of a list over `intervals` of (N,1) numpy arrays, in the
    model's standardised units.  exact=False is the reference's recipe: S samples of the predictive distribution
    ('predictive') or of the flowed posterior marginal ('posterior') per row, numpy.quantile over them.  exact=True takes the
    quantiles themselves (model.predictive_quantiles / model.posterior_quantiles) and ignores S; a warped model's predictive
    intervals are then the reference's 'special case' T^-1(mu + z sqrt(v + noise)), for any `intervals`."""
    import numpy
    if is_deep:
        raise NotImplementedError("is_deep=True: this package has no deep (DGP) models")
    if distribution not in ("predictive", "posterior"):
        raise ValueError("Invalid arguments")
    N = X.shape[0]
    with torch.no_grad():
        if exact:
            fn = model.predictive_quantiles if distribution == "predictive" else model.posterior_quantiles
            q = fn(X, list(intervals)).detach().to("cpu").numpy()                     # (Dy, Q, N)
            return [[q[l, i].reshape(N, 1) for i in range(len(intervals))] for l in range(model.out_dim)]
        if distribution == "predictive":
            samples = model.sample_from_predictive_distribution(X, S)[0]              # (Dy, S, N, 1)
        else:
            samples, _, _, _ = model.sample_from_variational_marginal(X, S, diagonal=True, is_duvenaud=False, init_Z=None)
            samples = samples.view(model.out_dim, S, N, 1)
        found = []
        for l in range(model.out_dim):
            s_l = samples[l].detach().to("cpu").numpy()
            found.append([numpy.quantile(s_l, interval, axis=0) for interval in intervals])
    return found


def compute_95_and_median_confidence_intervals(model, X, S, distribution, is_deep, exact=False):
    """The [0.025, 0.5, 0.975] intervals at X: median and the 95 % band (dsp/models/utils_models.py:123-140)."""
    assert distribution in ["posterior", "predictive"], \
        "Invalid arguments for distribution. Got {}, expected one of [posterior, predictive]".format(distribution)
    return confidence_intervals(model, X, [0.025, 0.5, 0.975], S, distribution, is_deep, exact=exact)


def input_relevance(model, X, batch_rows=65536):
    """(D,) relevance of each input: the root-mean-square over the rows of X of d m1 / d x_d, the slope of the predictive mean
    (model.predictive_input_gradients, standardised units), evaluated in pieces of `batch_rows` rows.  Where ARD length-scales
    are a proxy -- an input can have a short length-scale and no effect -- this is the sensitivity itself.  Raises what
    predictive_input_gradients raises for the models it does not serve."""
    X2 = X[0] if X.dim() == 3 else X
    if X2.shape[0] < 1 or int(batch_rows) < 1:
        raise ValueError("input_relevance: at least one row of X and batch_rows >= 1")
    sq = torch.zeros(X2.shape[1], dtype=X2.dtype, device=X2.device)
    for r0 in range(0, X2.shape[0], int(batch_rows)):
        g = model.predictive_input_gradients(X2[r0:r0 + int(batch_rows)])["m1"]
        sq += (g * g).sum(0)
    return torch.sqrt(sq / X2.shape[0])


def slope_significance(model, X, z=1.96, batch_rows=65536):
    """(D,) share of the rows of X at which the slope of the latent function in input d is significant: |mean_d| > z
    sqrt(max(var_d, 0)) with (mean, var) = model.posterior_derivative, evaluated in pieces of `batch_rows` rows.  G is
    increasing, so the sign of the latent slope is the sign of the slope of G(f): a share near 1 says the input moves the
    prediction almost everywhere, a share near 1 - the coverage of z says the slope input_relevance reports is posterior noise.
    A model of several latent GPs is refused (a share per GP: call posterior_derivative)."""
    X2 = X[0] if X.dim() == 3 else X
    if X2.shape[0] < 1 or int(batch_rows) < 1:
        raise ValueError("slope_significance: at least one row of X and batch_rows >= 1")
    if not float(z) >= 0.0:
        raise ValueError("slope_significance: z >= 0")
    hits = torch.zeros(X2.shape[1], dtype=X2.dtype, device=X2.device)
    for r0 in range(0, X2.shape[0], int(batch_rows)):
        mean, var = model.posterior_derivative(X2[r0:r0 + int(batch_rows)])
        if mean.shape[0] != 1:
            raise NotImplementedError("slope_significance: one latent GP only (this model has %d: take the share per GP from "
                                      "posterior_derivative)" % mean.shape[0])
        hits += (mean[0].abs() > float(z) * torch.sqrt(var[0].clamp_min(0.0))).to(hits.dtype).sum(0)
    return hits / X2.shape[0]


def suggest_candidates(model, bounds, kind="log_ei", best=None, maximize=True, num_starts=64, steps=50, lr=0.05, starts=None,
                       generator=None, beta=2.0):
    """Where to evaluate next: projected Adam ascent of model.acquisition(X, kind, best, maximize, beta, return_grad=True) inside
    the box `bounds` (2, D) = (lower, upper), from `num_starts` uniform draws (`generator`: a CPU torch.Generator; the same seed
    gives the same result) or from the rows of `starts` (S, D).  All starts move together, one (num_starts, D) batch and one
    acquisition call per step -- on the GPU one tgp_qf_input_grad_f64 and one tgp_predict_acquisition_f64 launch -- and every
    iterate is clamped to the box.  The step is lr (1 - t / steps) times the box width per coordinate (Adam's unit step, decaying
    linearly to 0 so that the last iterates settle).
    Returns (x, value, finals): the BEST ITERATE SEEN over all steps and all starts, the starting points included -- so the
    result is never below the best start -- its acquisition value, and finals = {"X": (num_starts, D), "value": (num_starts,)},
    the best iterate of each start and its value of the ascent variable.
    kind="ei" ascends "log_ei" -- EI's own gradient vanishes (underflows with EI) far from the incumbent, exactly where a
    start needs a direction, and the logarithm has the same maximisers -- and `value` is the EI at the winner.  kind="ucb" with
    maximize=False descends m1 - beta sqrt(m2) (its negative is the ascent variable; `value` is the bound itself)."""
    bounds = torch.as_tensor(bounds)
    if bounds.dim() != 2 or bounds.shape[0] != 2 or not bool((bounds[1] >= bounds[0]).all()):
        raise ValueError("suggest_candidates: bounds must be (2, D) with lower <= upper")
    if int(steps) < 0 or int(num_starts) < 1:
        raise ValueError("suggest_candidates: steps >= 0 and num_starts >= 1")
    lo, hi = bounds[0], bounds[1]
    width = hi - lo
    if starts is None:
        u = torch.rand(int(num_starts), bounds.shape[1], generator=generator, dtype=bounds.dtype)
        x = lo + u.to(bounds.device) * width
    else:
        x = torch.as_tensor(starts, dtype=bounds.dtype, device=bounds.device).reshape(-1, bounds.shape[1])
    x = torch.maximum(torch.minimum(x, hi), lo).contiguous()
    ascent = "log_ei" if kind == "ei" else kind
    sign = -1.0 if (kind == "ucb" and not maximize) else 1.0
    b1, b2, eps = 0.9, 0.999, 1e-8
    m, s = torch.zeros_like(x), torch.zeros_like(x)
    top_x = x.clone()
    top = torch.full((x.shape[0],), float("-inf"), dtype=x.dtype, device=x.device)
    steps = int(steps)
    for t in range(steps + 1):
        val, g = model.acquisition(x, kind=ascent, best=best, maximize=maximize, beta=beta, return_grad=True)
        val, g = sign * val.reshape(-1), sign * g
        better = val > top                                   # (a NaN is never better)
        top = torch.where(better, val, top)
        top_x = torch.where(better.unsqueeze(1), x, top_x)
        if t == steps:
            break
        g = torch.nan_to_num(g, nan=0.0, posinf=0.0, neginf=0.0)
        m = b1 * m + (1.0 - b1) * g
        s = b2 * s + (1.0 - b2) * g * g
        step = (m / (1.0 - b1 ** (t + 1))) / (torch.sqrt(s / (1.0 - b2 ** (t + 1))) + eps)
        x = torch.maximum(torch.minimum(x + (lr * (1.0 - t / steps)) * width * step, hi), lo).contiguous()
    i = int(torch.argmax(top))
    x_best = top_x[i].clone()
    if kind == "ei":
        value = model.acquisition(x_best.unsqueeze(0), kind="ei", best=best, maximize=maximize, beta=beta).reshape(-1)[0]
    else:
        value = sign * top[i]
    return x_best, value, {"X": top_x, "value": top}
