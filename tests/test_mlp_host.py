"""Host pins of tests/mlp_model.py (no GPU): the longdouble forward / hand-written backward of the packed networks against torch
autograd (the suite's own _torch_mlps), on every case tests/test_gpu_mlp_variants.py runs, eval mode and training mode with the
masks of ops.mlp_keep_mask -- and the measurement that float64 torch stays within a tenth of the GPU tolerances there."""
import numpy as np
import pytest
import torch

import mlp_model as mm
from test_gpu_models import _torch_mlps

SEED, STEP = 1234, 7


def masks_of(case, step=STEP, seed=SEED):
    from tgp.pytorch_amd import ops
    N, D, H, L, nnets, act, p = case
    return [[ops.mlp_keep_mask(seed, step, k, l, N, H, p) for l in range(L)] for k in range(nnets)]


def _torch_side(case, X, W, G, masks):
    from tgp.pytorch_amd import ops
    N, D, H, L, nnets, act, p = case
    spec = ops.MlpSpec(D, H, L, nnets, act=act, drop_p=p, seed=SEED)
    Wt = torch.from_numpy(W).requires_grad_(True)
    tm = None if masks is None else [[torch.from_numpy(m.astype(np.float64)) for m in row] for row in masks]
    out = _torch_mlps(torch.from_numpy(X), Wt, spec, tm)
    gW, = torch.autograd.grad((out * torch.from_numpy(G)).sum(), Wt)
    return out.detach().numpy(), gW.numpy()


def test_the_case_list_covers_every_instantiation():
    """18 (L, H class, activation) triples, and every H class at its upper edge and at its first size."""
    cls = lambda H: 0 if H <= 32 else 1 if H <= 52 else 2
    seen = {(L, cls(H), act) for (_, _, H, L, _, act, _) in mm.CASES["variants"]}
    assert len(seen) == 18 and len(mm.CASES["variants"]) == 18
    hs = {H for (_, _, H, _, _, _, _) in mm.CASES["variants"]}
    assert hs == {1, 32, 33, 52, 53, 64}


@pytest.mark.parametrize("case", mm.ALL_CASES, ids=lambda c: "N%d-D%d-H%d-L%d-n%d-%s" % c[:6])
def test_float64_torch_is_well_inside_the_gpu_tolerances(case):
    """The model against torch autograd, which pins the model (a wrong backward is wrong by far more than 1e-13) and measures
    float64: within a tenth of the GPU tolerances on every case, and within the constants recorded in mlp_model.py."""
    N, D, H, L, nnets, act, p = case
    X, W, G = mm.make_case(case)
    for masks in (None, masks_of(case)):
        ref_out, ref_gW = mm.forward_backward(X, W, G, D, H, L, nnets, act, p, masks)
        out, gW = _torch_side(case, X, W, G, masks)
        eo, eg = mm.rel(out, ref_out), mm.rel(gW, ref_gW)
        assert eo <= 0.1 * mm.TOL_OUT and eg <= 0.1 * mm.TOL_GW, (eo, eg)
        assert eo <= mm.F64_OUT and eg <= mm.F64_GW, (eo, eg)


def test_host_lds_sizing_is_the_kernels():
    """ops.MlpSpec.lds_bytes() against mlp_lds(D, H, L, bwd) of tgp_mlp.hip worked out by hand.  It used to pad to H instead of the
    kernel variant's 4 NKS units and answered 147 600 bytes for 5 -> 54 x 3 (163 216 in the kernel): flow compilation accepted
    networks whose backward launch then failed with TGP_E_LDS."""
    from tgp.pytorch_amd import ops
    for (N, D, H, L, nnets, act, p), nbytes in mm.LDS_LIMIT_CASES:
        assert ops.MlpSpec(D, H, L, nnets, act=act, drop_p=p).lds_bytes() == nbytes, (D, H, L)
    assert ops.MLP_LDS_MAX == 162816
    fits = [nbytes <= ops.MLP_LDS_MAX for _, nbytes in mm.LDS_LIMIT_CASES]
    assert fits == [True, False, False, True]


def test_rows_beyond_N_do_not_reach_the_gradient():
    """The property the short-N GPU cases check, stated on the model: g_W of N rows is the sum over exactly those rows (a kernel
    that lets the repeated last row of a padded chunk contribute would differ by that row's term)."""
    case = (17, 4, 50, 2, 2, "tanh", 0.25)
    X, W, G = mm.make_case(case)
    _, g17 = mm.forward_backward(X, W, G, 4, 50, 2, 2, "tanh")
    _, g16 = mm.forward_backward(X[:16], W, G[:16], 4, 50, 2, 2, "tanh")
    _, g1 = mm.forward_backward(X[16:], W, G[16:], 4, 50, 2, 2, "tanh")
    assert mm.rel(g16 + g1, g17) < 1e-17
    assert mm.rel(g16 + 2 * g1, g17) > 1e-3
