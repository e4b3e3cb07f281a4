"""GPU (-m gpu): the k-means kernels on their own against longdouble references with DERIVED bounds (tests/kmeans_model.py states
each derivation; tests/test_kmeans_host.py shows the inputs have no near-tie row).

Who owns what:
  the second (and third) 256-centre LDS chunk of k_kmeans_assign, the first-minimum rule across it   test_assign[*-257|513]
  mind2 == NULL                                                                                      test_assign_without_distances
  empty segments, four clusters per workgroup, segments of 0 / 1 / 63 / 64 / 65 / 1000 rows           test_segsum
  closest == NULL, T = 1 and 16, a repeated candidate, closest kept bit for bit                       test_pp
"""
import numpy as np
import pytest
import torch

import kmeans_model as km

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _assign(X, C, want_d2=True):
    from tgp.pytorch_amd import lib as L
    N, D = X.shape
    labels = torch.full((N,), -1, dtype=torch.int32, device=DEV)
    mind2 = torch.full((N,), -1.0, dtype=torch.float64, device=DEV) if want_d2 else None
    Xd, Cd = _dev(X), _dev(C)
    L.check(L.load().tgp_kmeans_assign_f64(L.ptr(Xd), N, D, L.ptr(Cd), C.shape[0], L.ptr(labels), L.ptr(mind2), L.stream_ptr()),
            "tgp_kmeans_assign_f64")
    torch.cuda.synchronize()
    return labels.cpu().numpy(), None if mind2 is None else mind2.cpu().numpy()


@pytest.mark.parametrize("N,D,K", km.ASSIGN_CASES)
def test_assign(N, D, K):
    X, C = km.assign_inputs(N, D, K)
    ref_l, ref_d, near = km.assign_ref(X, C)
    assert near.mean() <= 0.01                                   # (none, in fact: the host test)
    labels, mind2 = _assign(X, C)
    assert np.array_equal(labels[~near], ref_l[~near]), np.nonzero(labels != ref_l)[0][:10]
    err = np.abs(mind2.astype(km.LD) - ref_d)
    assert (err <= km.d2_bound(D) * ref_d).all(), float((err / (ref_d + km.LD(1e-300))).max())
    assert mind2[0] == 0.0 and labels[0] == 0                    # a row equal to a centre: exactly 0, the first of the twins
    if K >= 3:
        assert not (labels == K - 1).any()                       # the bit-identical twin at the higher index is never returned
    if K > 300:
        assert not (labels == 300).any() and (N == 1 or (labels[1] == 3 and mind2[1] == 0.0))


def test_assign_without_distances():
    X, C = km.assign_inputs(257, 3, 513)
    labels, none = _assign(X, C, want_d2=False)
    assert none is None and np.array_equal(labels, km.assign_ref(X, C)[0])


@pytest.mark.parametrize("K,lens", km.SEGSUM_CASES)
@pytest.mark.parametrize("D", [1, 16])
def test_segsum(K, lens, D):
    from tgp.pytorch_amd import lib as L
    X, order, offs = km.segsum_inputs(K, lens, D)
    ref, bound = km.segsum_ref(X, order, offs)
    Xd, od, fd = _dev(X), _dev(order), _dev(offs)
    sums = torch.full((K, D), float("nan"), dtype=torch.float64, device=DEV)
    L.check(L.load().tgp_kmeans_segsum_f64(L.ptr(Xd), D, L.ptr(od), L.ptr(fd), K, L.ptr(sums), L.stream_ptr()),
            "tgp_kmeans_segsum_f64")
    torch.cuda.synchronize()
    got = sums.cpu().numpy()
    for k in range(K):
        if lens[k] == 0:
            assert (got[k] == 0.0).all() and not np.signbit(got[k]).any()
    assert (np.abs(got.astype(km.LD) - ref) <= bound).all(), float((np.abs(got.astype(km.LD) - ref) - bound).max())


@pytest.mark.parametrize("N", km.ASSIGN_NS)
@pytest.mark.parametrize("T", [1, 16])
@pytest.mark.parametrize("D,given", [(3, False), (3, True), (16, True)])
def test_pp(N, T, D, given):
    from tgp.pytorch_amd import lib as L
    rng = np.random.default_rng([7, N, T, D])
    X = rng.standard_normal((N, D))
    cand = rng.integers(0, N, T).astype(np.int64)
    cand[-1] = cand[0]                                           # a repeated candidate (T = 1: itself)
    ref = km.pairwise_d2(X, X[cand]).T                           # (T, N)
    closest = None
    if given:        # around the candidates' own distances: some rows keep closest, some take a candidate's distance
        closest = (np.asarray(ref.min(0), np.float64) + 0.05) * rng.uniform(0.2, 3.0, N)
    Xd, cd = _dev(X), _dev(cand)
    cl = None if closest is None else _dev(closest)
    out = torch.full((T, N), float("nan"), dtype=torch.float64, device=DEV)
    L.check(L.load().tgp_kmeans_pp_f64(L.ptr(Xd), N, D, L.ptr(cd), T, L.ptr(cl), L.ptr(out), L.stream_ptr()), "tgp_kmeans_pp_f64")
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    b = km.d2_bound(D)
    want = ref if closest is None else np.minimum(ref, np.asarray(closest, km.LD)[None, :])
    assert (np.abs(got.astype(km.LD) - want) <= b * want).all()
    assert (got[np.arange(T), cand] == 0.0).all()                        # a candidate's distance to itself
    if closest is not None:
        below = np.asarray(closest, km.LD)[None, :] < ref * (1 - b)     # closest under every rounding of the candidate's distance
        assert N < 255 or (below.any() and (~below).any())
        assert np.array_equal(got[below], np.broadcast_to(closest[None, :], got.shape)[below])
        keeps_all = below.all(0)                                         # closest[n] below EVERY candidate: the column is closest[n]
        assert (got[:, keeps_all] == closest[None, keeps_all]).all()
