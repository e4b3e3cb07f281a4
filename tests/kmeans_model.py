"""The k-means kernels (tgp_kmeans_assign_f64, tgp_kmeans_segsum_f64, tgp_kmeans_pp_f64) in numpy.longdouble, the inputs of
tests/test_gpu_kmeans.py, and the error bounds -- DERIVED from the kernels' operation order with u = 2^-53, not measured.

assign / pp: d2 = fma(t_D, t_D, ... fma(t_1, t_1, 0)), t_d = fl(x_d - c_d).  Every t_d carries one rounding, (1 + d)^2 on its
    square; the fma chain adds one rounding per term, so term d carries at most D - d + 1 more.  All terms are >= 0, so
    |d2 - exact| <= ((D + 2) u + O(u^2)) exact; (D + 3) u covers the second order and the reference's own rounding to float64.
    x = c bit for bit gives t = 0 and d2 = 0 exactly.
labels: the kernel keeps the FIRST k whose computed d2 is strictly smallest.  Two centres whose exact distances differ by more
    than 2 (D + 3) u of the smaller cannot swap order; the test excludes rows closer than 8 (D + 3) u (four times that) -- and
    the chosen inputs have no such row (tests/test_kmeans_host.py).  Bit-identical centres give bit-identical d2: first index wins.
segsum: lane j adds its ceil(len / 64) rows in order from 0 (the first add is exact: <= ceil(len / 64) - 1 roundings), then
    six butterfly levels add six roundings: |s - exact| <= (ceil(len / 64) + 6) u sum|x| per entry.  An empty segment adds
    nothing to 0.0 and sums zeros: exactly 0.
"""
import numpy as np

LD = np.longdouble
U = 2.0 ** -53
ASSIGN_NS, ASSIGN_DS, ASSIGN_KS = (1, 255, 256, 257, 1000), (1, 3, 16), (1, 2, 255, 256, 257, 513)
# one sweep per axis around (257, 3, 257), plus the corner
ASSIGN_CASES = sorted({(N, 3, 257) for N in ASSIGN_NS} | {(257, D, 257) for D in ASSIGN_DS} | {(257, 3, K) for K in ASSIGN_KS}
                      | {(257, 16, 513)})
SEGSUM_CASES = [(1, (1000,)), (1, (0,)), (3, (0, 0, 63)), (3, (64, 1, 0)), (4, (65, 64, 0, 1000)), (5, (1000, 0, 64, 1, 63)),
                (9, (0, 1, 63, 64, 65, 1000, 0, 65, 1))]


def d2_bound(D):
    return (D + 3) * U


def assign_inputs(N, D, K, seed=0):
    """Rows and centres ~ N(0, 1).  Exact ties: centre K - 1 duplicates centre 0 (K >= 3), centre 300 duplicates centre 3 (across
    the 256-centre chunk boundary, K > 300); row 0 IS centre 0 and row 1 IS centre 3, so the duplicates are those rows' minima."""
    rng = np.random.default_rng([seed, N, D, K])
    X, C = rng.standard_normal((N, D)), rng.standard_normal((K, D))
    if K >= 3:
        C[K - 1] = C[0]
    if K > 300:
        C[300] = C[3]
    X[0] = C[0]
    if N > 1 and K > 300:
        X[1] = C[3]
    return X, C


def pairwise_d2(X, C):
    X, C = np.asarray(X, LD), np.asarray(C, LD)
    out = np.zeros((X.shape[0], C.shape[0]), LD)
    for d in range(X.shape[1]):
        t = X[:, d:d + 1] - C[None, :, d]
        out += t * t
    return out


def assign_ref(X, C):
    """(labels = first minimum, mind2 (longdouble), near = rows whose two smallest distances to DISTINCT centres differ by less
    than 8 (D + 3) u of the smaller: their label is not checked)."""
    d2 = pairwise_d2(X, C)
    labels = d2.argmin(1)                               # numpy: first minimum
    mind2 = d2[np.arange(len(labels)), labels]
    _, first = np.unique(C, axis=0, return_index=True)  # bit-identical centres: keep the first occurrence
    keep = np.zeros(C.shape[0], bool)
    keep[first] = True
    dd = np.sort(np.where(keep[None, :], d2, np.inf), axis=1)
    near = np.zeros(len(labels), bool)
    if dd.shape[1] > 1:
        near = (dd[:, 1] - dd[:, 0]) < 8 * d2_bound(X.shape[1]) * dd[:, 0]
        near &= np.isfinite(dd[:, 1])
    return labels, mind2, near


def segsum_inputs(K, lens, D, seed=0):
    """X (N, D) with N = sum(lens) (at least one row), `order` a permutation of the rows, offs (K + 1)."""
    rng = np.random.default_rng([seed, K, D, sum(lens)])
    N = max(1, int(sum(lens)))
    X = rng.standard_normal((N, D)) * 10.0 ** rng.uniform(-3, 3, (N, 1))
    return X, rng.permutation(N).astype(np.int64), np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)


def segsum_ref(X, order, offs):
    """(sums, bound) per (k, d): the exact sums and (ceil(len / 64) + 6) u sum|x|."""
    X = np.asarray(X, LD)
    K = len(offs) - 1
    sums, bound = np.zeros((K, X.shape[1]), LD), np.zeros((K, X.shape[1]), LD)
    for k in range(K):
        rows = X[order[offs[k]:offs[k + 1]]]
        n = rows.shape[0]
        sums[k] = rows.sum(0)
        bound[k] = (-(-n // 64) + 6) * U * np.abs(rows).sum(0)
    return sums, bound
