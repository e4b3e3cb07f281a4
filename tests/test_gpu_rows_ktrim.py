"""GPU (-m gpu): the fused row kernel no longer multiplies the padding of M up to the next multiple of 16.  The training kernels
k_rows<MT, DP, 1 | TGP_ROWS_KT(KT), RW> exist for KT = Plan::KL = 1 .. 3 k-steps of the last 16-row tile (KL = ceil(MR / 4), MR = M - 16 (MT - 1)
real rows there): registers KT .. 3 of that tile of K, A, C, Abar and Kbar are the literal 0.0, and the forward substitution, the
product C = (S - I) A and the back substitution leave out the k-steps that would multiply them.  lib.PLAN_FULL_PAD sets KL = 4 and
runs the untrimmed kernel.

A product skipped is a product with an exact zero, so the trimmed step must agree with the PLAN_FULL_PAD step BIT FOR BIT
(torch.equal: +0 and -0 compare equal, the only difference a skipped zero product can make), and two trimmed steps with each other.
tests/test_gpu_pad_trim.py holds this at 16 rows per wave for M in {5, 17, 20, 60, 100, 112, 128} and at 10 rows per wave for
M in {60, 100}; this file adds what it leaves open:

  10 rows per wave (PLAN_ROWS_K, N = 4 003: rows_rw picks 10 only above 4 000 rows; 100 full workgroups and one of 3 rows) at
      (M, MT, KT) = (5, 1, 2), (17, 2, 1), (40, 3, 2), (112, 7, 4)
  16 rows per wave (PLAN_ROWS_K16, N = 77) at M = 40 (MT = 3, MR = 8, KT = 2), and at D = 8, M = 100 (the DP = 8 kernels)

Every step runs on a workspace filled with garbage first (another value per run), so a read of a tile that no launch wrote cannot
pass by luck.  Every (MT, DP, KT) of the training mode is built trimmed; what stays on the untrimmed kernel -- the moments-only
launch, the one-node-in-flight mode, the extended flow kinds and k_rows4 -- is reached by tests/test_gpu_pad_trim.py.
"""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _problem(N, D, M, flow, S):
    from oracle import tgp_oracle as orc       # generator only
    prob = orc.synthetic_problem(max(N, 160), D, M, seed=37, flow=flow, S=S)
    prob["X"], prob["Y"] = prob["X"][:N].contiguous(), prob["Y"][:N].contiguous()
    return prob


def _step(key, plan, garbage, monkeypatch):
    from tgp.pytorch_amd import ops
    dev = torch.device("cuda:0")
    N, D, M, flow, S = key
    prob = _problem(*key)
    p = {k: v.to(dev) for k, v in prob["params"].items()}
    fs = ops.FlowSpec(prob["program"], p["theta"].numel(), 0, dev)
    cached = ops.workspace
    monkeypatch.setattr(ops, "workspace", lambda *a, **kw: cached(*a, **kw).fill_(garbage))   # as a recycled allocation would be
    try:
        out, g, status, (mu, v) = ops.elbo_step(prob["X"].to(dev), prob["Y"].to(dev), p["Z"], p["raw_lengthscale"],
                                                p["raw_outputscale"], p["m"], p["Lam"], p["log_var_noise"], float(N), flow=fs,
                                                theta=p["theta"], S=S, plan=plan, want_moments=True)
        torch.cuda.synchronize()
    finally:
        monkeypatch.setattr(ops, "workspace", cached)
    assert int(status[0]) == 0 and int(status[1]) == 0, (key, plan, status.tolist())
    res = {"out": out.cpu(), "mu": mu.cpu(), "v": v.cpu()}
    res.update({"g_" + k: t.cpu() for k, t in g.items()})
    return res


def _assert_same(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        assert torch.isfinite(a[k]).all(), (what, k, "not finite")
        diff = float((a[k] - b[k]).abs().max()) if a[k].numel() else 0.0
        print("rows k-trim", what, k, "max |difference| = %.3e" % diff, flush=True)
        assert torch.equal(a[k], b[k]), (what, k, diff)


def _check(key, plan, monkeypatch):
    from tgp.pytorch_amd import lib
    trimmed = _step(key, plan, 12345.678, monkeypatch)
    again = _step(key, plan, -8765.4321, monkeypatch)
    full = _step(key, plan | lib.PLAN_FULL_PAD, 3.25e7, monkeypatch)
    _assert_same(trimmed, again, (key, "trimmed twice"))
    _assert_same(trimmed, full, (key, "trimmed against PLAN_FULL_PAD"))


@pytest.mark.parametrize("M", [5, 17, 40, 112])
def test_step_rw10_bit_equal(M, monkeypatch):
    """The 10-rows-per-wave kernel at KT = 2, 1, 2, 4 (MT = 1, 2, 3, 7)."""
    from tgp.pytorch_amd import lib
    _check((4003, 4, M, "tanh3x2", 32), lib.PLAN_ROWS_K, monkeypatch)


def test_step_rw16_bit_equal_m40(monkeypatch):
    """16 rows per wave, MT = 3 with MR = 8 real rows in the last tile: KT = 2."""
    from tgp.pytorch_amd import lib
    _check((77, 4, 40, "tanh3x2", 32), lib.PLAN_ROWS_K16, monkeypatch)


def test_step_rw16_bit_equal_d8(monkeypatch):
    """D = 8: the DP = 8 instantiation, M = 100 (MT = 7, KT = 1)."""
    from tgp.pytorch_amd import lib
    _check((77, 8, 100, "tanh3x2", 32), lib.PLAN_ROWS_K16, monkeypatch)
