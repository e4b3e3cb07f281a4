"""Host pins of tests/kmeans_model.py (no GPU): the chosen assign inputs have no near-tie row (so the GPU test checks EVERY
label), their planted exact ties are where the model says, and the references agree with plain float64 numpy within the
derived bounds (which a float64 restatement of the same operation order must meet as well)."""
import numpy as np
import pytest

import kmeans_model as km


@pytest.mark.parametrize("N,D,K", km.ASSIGN_CASES)
def test_assign_inputs_have_no_near_ties_and_the_planted_exact_ones(N, D, K):
    X, C = km.assign_inputs(N, D, K)
    labels, mind2, near = km.assign_ref(X, C)
    assert not near.any(), int(near.sum())
    assert labels[0] == 0 and mind2[0] == 0                          # row 0 is centre 0; its duplicate K - 1 never wins
    if K >= 3:
        assert np.array_equal(C[K - 1], C[0]) and not (labels == K - 1).any()
    if K > 300:
        assert np.array_equal(C[300], C[3]) and not (labels == 300).any()
        if N > 1:
            assert labels[1] == 3 and mind2[1] == 0
    # the same operation order in float64 (the subtraction, then one product-and-add per dimension) meets the derived bound
    d2 = np.zeros((N, K))
    for d in range(D):
        t = X[:, d:d + 1] - C[None, :, d]
        d2 = t * t + d2
    assert np.array_equal(d2.argmin(1), labels)
    got = d2[np.arange(N), labels]
    assert (np.abs(got.astype(km.LD) - mind2) <= km.d2_bound(D) * mind2).all()


@pytest.mark.parametrize("K,lens", km.SEGSUM_CASES)
@pytest.mark.parametrize("D", [1, 16])
def test_segsum_reference(K, lens, D):
    X, order, offs = km.segsum_inputs(K, lens, D)
    assert sorted(order.tolist()) == list(range(X.shape[0])) and offs[-1] == sum(lens) and len(offs) == K + 1
    sums, bound = km.segsum_ref(X, order, offs)
    for k in range(K):
        seg = X[order[offs[k]:offs[k + 1]]]
        if lens[k] == 0:
            assert (sums[k] == 0).all() and (bound[k] == 0).all()
            continue
        # a left-to-right float64 sum has len - 1 roundings: inside len x u x sum|x|
        plain = np.zeros(D)
        for r in seg:
            plain = plain + r
        assert (np.abs(plain.astype(km.LD) - sums[k]) <= lens[k] * km.U * np.abs(seg).sum(0)).all()
