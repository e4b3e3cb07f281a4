"""GPU (-m gpu): the M x M backward launch of the fused path (M <= 128, k_bwd) no longer contracts over the padding of M up to the
next multiple of 16: its products stop after the 4 (MT - 1) + KL k-steps that carry data (MR = M - 16 (MT - 1) real rows in the
last 16-row tile, KL = ceil(MR / 4)) and do not fetch the fragments past them.  lib.PLAN_FULL_PAD switches the trim off.

A product skipped is a product with an exact zero, so the two runs must agree BIT FOR BIT (torch.equal; +0 and -0 compare
equal, the only difference a skipped zero product can make):

  test 1  step scalars, every gradient, mu and v of ops.elbo_step, and ops.qf_moments, trimmed against PLAN_FULL_PAD, over every
          remainder class (MT, MR) = (1,5), (2,1), (2,4), (4,12), (7,4), (7,16), (8,16), behind both k_rows variants (16 and 10
          rows per wave), flow / closed-form / per-row likelihoods, and one case behind k_rows4
  test 2  what the trim relies on: L, L^T and -Dinv as the prepare launch leaves them in the workspace are the identity and zeros
          on the padding, exactly, both ways
  test 3  the device's jitter ladder with a failing pivot in the last block column: status and results equal the PLAN_FULL_PAD run

(The same trims of the row kernel's chains, of the last block column's pivots and of the slab reduction's loads passed these tests
and were taken out again because they did not pay: profiles/NOTES.md, round 9.)
"""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

MS = [5, 17, 20, 60, 100, 112, 128]       # (MT, MR) = (1,5), (2,1), (2,4), (4,12), (7,4), (7,16), (8,16)


@functools.lru_cache(maxsize=None)
def _problem(N, D, M, flow, S):
    """N rows of a seeded problem with M inducing points (the generator draws Z from its rows: at least M of them)."""
    from oracle import tgp_oracle as orc       # generator only
    prob = orc.synthetic_problem(max(N, 160), D, M, seed=31, flow=flow, S=S)
    prob["X"], prob["Y"] = prob["X"][:N].contiguous(), prob["Y"][:N].contiguous()
    if prob["rowp"] is not None:
        prob["rowp"] = prob["rowp"][:N].contiguous()
    return prob


def _step(key, plan):
    from tgp.pytorch_amd import ops
    dev = torch.device("cuda:0")
    N, D, M, flow, S = key
    prob = _problem(*key)
    p = {k: v.to(dev) for k, v in prob["params"].items()}
    rowp = prob["rowp"].to(dev) if prob["rowp"] is not None else None
    fs = ops.FlowSpec(prob["program"], p["theta"].numel(), 0 if rowp is None else rowp.shape[1], dev) if flow else None
    out, g, status, (mu, v) = ops.elbo_step(prob["X"].to(dev), prob["Y"].to(dev), p["Z"], p["raw_lengthscale"],
                                            p["raw_outputscale"], p["m"], p["Lam"], p["log_var_noise"], float(N), flow=fs,
                                            theta=p.get("theta"), rowp=rowp, S=S, plan=plan, want_moments=True)
    torch.cuda.synchronize()
    assert int(status[0]) == 0 and int(status[1]) == 0, (key, plan, status.tolist())
    res = {"out": out.cpu(), "mu": mu.cpu(), "v": v.cpu()}
    res.update({"g_" + k: t.cpu() for k, t in g.items()})
    return res


def _assert_same(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        assert torch.isfinite(a[k]).all(), (what, k, "not finite")
        diff = float((a[k] - b[k]).abs().max()) if a[k].numel() else 0.0
        print("pad trim", what, k, "max |trimmed - full| = %.3e" % diff, flush=True)
        assert torch.equal(a[k], b[k]), (what, k, diff)


def _check_step(key, plan):
    from tgp.pytorch_amd import lib
    _assert_same(_step(key, plan), _step(key, plan | lib.PLAN_FULL_PAD), (key, plan))


# ---- test 1 -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flow", ["tanh3x2", None, "idsal2"])
@pytest.mark.parametrize("M", MS)
def test_step_rw16_bit_equal(M, flow):
    """k_rows at 16 rows per wave, N = 77 (two workgroups, the second ragged): flow likelihood (S = 32), SVGP closed form,
    per-row flow parameters."""
    from tgp.pytorch_amd import lib
    _check_step((77, 4, M, flow, 32), lib.PLAN_ROWS_K16)


def test_step_rw16_bit_equal_d13():
    """D = 13: the DP = 16 instantiation."""
    from tgp.pytorch_amd import lib
    _check_step((77, 13, 100, "tanh3x2", 32), lib.PLAN_ROWS_K16)


@pytest.mark.parametrize("M", [60, 100])
def test_step_rw10_bit_equal(M):
    """N = 7 937 under PLAN_ROWS_K: the 10-rows-per-wave kernel, 198 full workgroups and one ragged one."""
    from tgp.pytorch_amd import lib
    _check_step((7937, 4, M, "tanh3x2", 32), lib.PLAN_ROWS_K)


@pytest.mark.parametrize("M", MS)
def test_moments_bit_equal(M):
    """The moments-only launch (no backward: the switch must change nothing)."""
    from tgp.pytorch_amd import lib, ops
    dev = torch.device("cuda:0")
    prob = _problem(77, 4, M, None, 32)
    p = {k: v.to(dev) for k, v in prob["params"].items()}
    res = []
    for plan in (0, lib.PLAN_FULL_PAD):
        mu, v = ops.qf_moments(prob["X"].to(dev), p["Z"], p["raw_lengthscale"], p["raw_outputscale"], p["m"], p["Lam"], plan=plan)
        torch.cuda.synchronize()
        res.append({"mu": mu.cpu(), "v": v.cpu()})
    _assert_same(res[0], res[1], ("moments", M))


def test_step_rows4_bit_equal():
    """The automatic plan at N = 77 runs k_rows4: the M x M backward behind its slabs."""
    _check_step((77, 4, 100, "tanh3x2", 32), 0)


# ---- test 2 -------------------------------------------------------------------------------------------------------------
def _plan_offsets(D, M, P):
    """Workspace offsets (doubles) of L, L^T and -Dinv as make_plan lays them out (csrc/tgp_dev.hpp)."""
    def rup(x, a):
        return (x + a - 1) // a * a
    MT = (M + 15) // 16
    MP = 16 * MT
    DP = 4 if D <= 4 else (8 if D <= 8 else 16)
    mm = MP * MP
    o = 64 + 16 + 16 + MP * DP + MP + MP + 2 * rup(P + 1, 16)      # hdr, ils, ls, Zs, mpad, w, tp, tg
    return {"MT": MT, "MP": MP, "L": o + mm, "LT": o + 3 * mm, "nD": o + 9 * mm}


def _lt_written(MP):
    """The part of L^T the prepare launch writes: the tiles on and above the diagonal (the transposes of L's lower tiles, which
    are all the row kernel reads).  The strictly-lower tiles of L^T belong to no launch -- the workspace is not initialised, so
    they hold whatever the allocation held before -- unlike the strictly-upper tiles of L, which the tile blocks zero."""
    t = torch.arange(MP) // 16
    return t[:, None] <= t[None, :]


@pytest.mark.parametrize("full", [False, True])
@pytest.mark.parametrize("M", [100, 17])
def test_prepare_leaves_identity_on_the_padding(M, full):
    from tgp.pytorch_amd import lib, ops
    dev = torch.device("cuda:0")
    plan = lib.PLAN_ROWS_K16 | (lib.PLAN_FULL_PAD if full else 0)
    key = (77, 4, M, None, 32)
    ops.workspace(77, 4, M, 1, 0, 0, 0, dev, lib.KERNELS["scale_rbf"], plan).fill_(12345.678)   # as a recycled allocation would be
    _step(key, plan)
    ws = ops.workspace(77, 4, M, 1, 0, 0, 0, dev, lib.KERNELS["scale_rbf"], plan).cpu()
    o = _plan_offsets(4, M, 0)
    MT, MP = o["MT"], o["MP"]
    MR = M - 16 * (MT - 1)
    Lm = ws[o["L"]:o["L"] + MP * MP].reshape(MP, MP)
    LT = ws[o["LT"]:o["LT"] + MP * MP].reshape(MP, MP)
    nD = ws[o["nD"]:o["nD"] + MT * 256].reshape(MT, 16, 16)
    eye = torch.eye(MP, dtype=torch.float64)
    wr = _lt_written(MP)
    assert torch.equal(LT[wr], Lm.t()[wr])        # with L below: identity and zeros on the padding of L^T too, wherever it is written
    assert torch.equal(Lm[M:, :], eye[M:, :]) and torch.equal(Lm[:, M:], eye[:, M:])      # identity rows and columns, exactly
    assert torch.equal(torch.triu(Lm, 1), torch.zeros_like(Lm))
    assert bool((torch.diagonal(Lm)[:M] > 0).all())
    e16 = torch.eye(16, dtype=torch.float64)
    last = nD[MT - 1]
    assert torch.equal(last[MR:, :], -e16[MR:, :]) and torch.equal(last[:, MR:], -e16[:, MR:])   # minus identity, exactly
    assert torch.equal(torch.triu(last, 1), torch.zeros_like(last))
    # -Dinv of the real part is the inverse of the real part of the last diagonal tile of L
    Ld = Lm[16 * (MT - 1):16 * (MT - 1) + MR, 16 * (MT - 1):16 * (MT - 1) + MR]
    err = float((Ld @ (-last[:MR, :MR]) - torch.eye(MR, dtype=torch.float64)).abs().max())
    print("pad trim prepare M=%d full=%s |L_dd Dinv - I| = %.2e" % (M, full, err), flush=True)
    assert err < 1e-9


def test_prepare_bit_equal_with_full_pad():
    """The whole of L and -Dinv and the written part of L^T, trimmed against PLAN_FULL_PAD (the two runs have workspaces of their
    own, filled with different garbage first)."""
    from tgp.pytorch_amd import lib, ops
    dev = torch.device("cuda:0")
    for M in (100, 17):
        got = []
        for plan in (lib.PLAN_ROWS_K16, lib.PLAN_ROWS_K16 | lib.PLAN_FULL_PAD):
            ops.workspace(77, 4, M, 1, 0, 0, 0, dev, lib.KERNELS["scale_rbf"], plan).fill_(1.0 + plan)
            _step((77, 4, M, None, 32), plan)
            ws = ops.workspace(77, 4, M, 1, 0, 0, 0, dev, lib.KERNELS["scale_rbf"], plan).cpu()
            o = _plan_offsets(4, M, 0)
            mm = o["MP"] ** 2
            got.append((ws[o["L"]:o["L"] + mm].clone(), ws[o["LT"]:o["LT"] + mm].clone(), ws[o["nD"]:o["nD"] + o["MT"] * 256].clone()))
        wr = _lt_written(o["MP"]).reshape(-1)
        for k, (a, b) in enumerate(zip(*got)):
            assert torch.equal(a[wr], b[wr]) if k == 1 else torch.equal(a, b), (M, k)


# ---- test 3 -------------------------------------------------------------------------------------------------------------
def test_jitter_ladder_with_a_padded_last_column():
    """The recipe of test_gpu_models.py::test_device_jitter_ladder_inside_the_captured_step at M = 100, the duplicated inducing
    points in the first tile and in the last block column: K_MM fails at level 0, the ladder inside k_prep_a
    recovers, and status and results equal the PLAN_FULL_PAD run."""
    from oracle import tgp_oracle as orc       # generator only
    from tgp.pytorch_amd import lib
    from tgp.pytorch_amd.engine import ElboEngine
    dev = torch.device("cuda:0")
    prob = orc.synthetic_problem(128, 3, 100, seed=1, flow=None, S=8)
    prob["params"]["Z"][1] = prob["params"]["Z"][0]
    prob["params"]["Z"][97:100] = prob["params"]["Z"][96]
    res = {}
    for name, plan, ladder in (("noladder", 0, 0.0), ("trim", 0, 1e-8), ("full", lib.PLAN_FULL_PAD, 1e-8)):
        e = ElboEngine(prob["X"], prob["Y"], prob["params"], 128.0, device=dev, jitter_ladder=ladder, plan=plan)
        e.elbo()
        torch.cuda.synchronize()
        res[name] = (e.status[:3].cpu().tolist(), e.fp.out[:3].cpu().clone(), e.fp.grad.cpu().clone())
        print("pad trim ladder", name, "status", res[name][0], "out", res[name][1].tolist(), flush=True)
    assert res["noladder"][0][0] > 0                        # K_MM fails at level 0
    st, out, grad = res["trim"]
    assert st[0] == 0 and st[1] == 0 and st[2] >= 1         # ... and the ladder recovers
    assert st == res["full"][0]
    assert torch.isfinite(out).all() and torch.isfinite(grad).all()
    assert torch.equal(out, res["full"][1]) and torch.equal(grad, res["full"][2])
