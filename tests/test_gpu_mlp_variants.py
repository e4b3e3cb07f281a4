"""GPU (-m gpu): every instantiation of k_mlp_fwd / k_mlp_bwd (L in {1,2,3} x NKS in {8,13,16} x {relu,tanh}) and their edges against
the longdouble model (tests/mlp_model.py, pinned to torch autograd by tests/test_mlp_host.py), eval mode and training mode with
the dropout masks restated by ops.mlp_keep_mask (which also checks the unit -> hash-group map at each padded width).
Tolerances: the project's, 1e-12 (outputs) and 1e-11 (g_W) relative to the largest entry; float64 torch is within a tenth of them
on every case here (host test).

Who owns what:
  the 18 + 18 instantiations           test_every_instantiation (cases: mlp_model.CASES["variants"]; H class edges 32|33, 52|53)
  H < 4, H = 17                        test_small_widths
  D = 1 ... 64                         test_input_widths
  N below / at / over a 16-row wave and a 64-row chunk; padded rows contribute nothing to g_W      test_short_row_counts
  several chunks per workgroup (fwd 2, bwd 3, short last workgroup, 7 reduce slots)                test_several_chunks_per_workgroup
"""
import numpy as np
import pytest
import torch

import mlp_model as mm

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED, STEP = 1234, 7


def _id(c):
    return "N%d-D%d-H%d-L%d-n%d-%s" % c[:6]


def _run(case):
    from tgp.pytorch_amd import ops
    N, D, H, L, nnets, act, p = case
    X, W, G = mm.make_case(case)
    spec = ops.MlpSpec(D, H, L, nnets, act=act, drop_p=p, seed=SEED)
    Xd, Wd, Gd = (torch.from_numpy(a).to(DEV) for a in (X, W, G))
    step = torch.tensor([STEP, 0], dtype=torch.int32, device=DEV)
    for training in (False, True):
        masks = None
        if training:
            masks = [[ops.mlp_keep_mask(SEED, STEP, k, l, N, H, p) for l in range(L)] for k in range(nnets)]
        ref_out, ref_gW = mm.forward_backward(X, W, G, D, H, L, nnets, act, p, masks)
        out = ops.mlp_forward(spec, Xd, Wd, training, step)
        gW = ops.mlp_backward(spec, Xd, Wd, Gd, training, step)
        torch.cuda.synchronize()
        eo, eg = mm.rel(out.cpu().numpy(), ref_out), mm.rel(gW.cpu().numpy(), ref_gW)
        print("%s training=%d: out %.3g  g_W %.3g" % (_id(case), training, eo, eg))
        assert out.shape == (N, nnets) and bool(torch.isfinite(out).all()) and bool(torch.isfinite(gW).all())
        assert eo < mm.TOL_OUT and eg < mm.TOL_GW, (training, eo, eg)
    assert step.tolist() == [STEP, 0]                     # the step word is read only


@pytest.mark.parametrize("case", mm.CASES["variants"], ids=_id)
def test_every_instantiation(case):
    _run(case)


@pytest.mark.parametrize("case", mm.CASES["small_H"], ids=_id)
def test_small_widths(case):
    _run(case)


@pytest.mark.parametrize("case", mm.CASES["wide_D"], ids=_id)
def test_input_widths(case):
    _run(case)


@pytest.mark.parametrize("case", mm.CASES["short_N"], ids=_id)
def test_short_row_counts(case):
    """In the last chunk the rows beyond N repeat the last row: at 1e-11 of the largest gradient entry any contribution of theirs
    to g_W (a whole row's term, 1 / N of the sum) fails the comparison."""
    _run(case)


@pytest.mark.parametrize("case,nbytes", mm.LDS_LIMIT_CASES, ids=lambda c: _id(c) if isinstance(c, tuple) else str(c))
def test_backward_runs_exactly_what_its_lds_sizing_admits(case, nbytes):
    """Around the LDS ceiling of k_mlp_bwd (three layers, H = 53 | 54): a shape whose ops.MlpSpec.lds_bytes() fits runs and matches
    the model; one that does not is refused by tgp_mlp_backward_f64 with TGP_E_LDS before any launch (its forward, which has no
    strips, still runs).  flow compilation goes by the same number, so it never hands the kernels a net they refuse."""
    from tgp.pytorch_amd import lib as L
    from tgp.pytorch_amd import ops
    N, D, H, Lh, nnets, act, p = case
    spec = ops.MlpSpec(D, H, Lh, nnets, act=act, drop_p=p, seed=SEED)
    assert spec.lds_bytes() == nbytes
    if nbytes <= ops.MLP_LDS_MAX:
        _run(case)
        return
    X, W, G = mm.make_case(case)
    Xd, Wd, Gd = (torch.from_numpy(a).to(DEV) for a in (X, W, G))
    out = ops.mlp_forward(spec, Xd, Wd, False, None)
    ref_out, _ = mm.forward_backward(X, W, G, D, H, Lh, nnets, act)
    assert mm.rel(out.cpu().numpy(), ref_out) < mm.TOL_OUT
    with pytest.raises(L.TgpError, match="code -102"):
        ops.mlp_backward(spec, Xd, Wd, Gd, False, None)


@pytest.mark.parametrize("case", mm.CASES["chunks"], ids=_id)
def test_several_chunks_per_workgroup(case):
    _run(case)
