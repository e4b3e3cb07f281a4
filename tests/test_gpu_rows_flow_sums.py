"""GPU (-m gpu): the flow-parameter gradient sums of the 10-rows-per-wave row kernel.

At 10 rows per wave (k_rows<.., RW = 10>) the wave's (row, node) pairs make ONE trip through the flow, so every lane forms each
shared flow parameter's partial exactly once: the reverse sweep (flow_backward_store, PN) stores them lane-private in stack slots
it has just read, each wave sums its 64 lanes of every parameter once after the sweep (flow_param_wave_sums, a transposed LDS
read in a fixed order) and the tail adds the four waves in wave order.

  1. against oracle/tgp_oracle.py at the bars of tests/test_gpu_rows_sform.py (values 1e-9, gradients 1e-7, rel_err of conftest)
  2. the same step twice on differently filled workspaces, a step of another shape between them: torch.equal on every output
  3. against the 16-rows-per-wave kernel (PLAN_ROWS_K16) on the same inputs: another summation order only, so every output within
     the same bars of it; the gradient of theta asserted on its own, its figure printed
  4. one program of the extended kind set (the TGP_FLOWX unit) from a reference fixture, its first 4 003 rows, as in 3

N = 4 003 is the smallest N at which rows_rw() gives 10 rows per wave: 100 full workgroups and one of 3 rows, most of whose pairs
are invalid -- their lanes must still store zeros, not leave what the forward sweep put into those slots.  D = 4, S = 32.  Cases:
M = 100 (MT = 7, the odd dealing of the G row blocks) with tanh3x2 (four partials per step, P = 30), sal2 (two per block) and
idsal3 (per-row SAL blocks keep their own path through the stack; g_rowp is compared too), M = 128 (MT = 8, the even dealing)
and M = 5 (MT = 1).  Every step runs on a workspace filled with garbage first, another value per run."""
import functools

import pytest
import torch

from conftest import load_golden, rel_err

pytestmark = pytest.mark.gpu

TOL_VAL = 1e-9
TOL_GRAD = 1e-7
N, D, S = 4003, 4, 32
CASES = [(100, "tanh3x2"), (100, "sal2"), (100, "idsal3"), (128, "tanh3x2"), (5, "tanh3x2")]
IDS = ["M%d-%s" % c for c in CASES]
NAMES = {"Z": "Z", "raw_ls": "raw_lengthscale", "raw_os": "raw_outputscale", "m": "m", "Lam": "Lam", "lvn": "log_var_noise",
         "theta": "theta", "rowp": "rowp"}


@functools.lru_cache(maxsize=None)
def _problem(M, flow):
    from oracle import tgp_oracle as orc       # generator and checker only
    return orc.synthetic_problem(N, D, M, seed=41, flow=flow, S=S)


@functools.lru_cache(maxsize=None)
def _fixture_problem(name):
    g = load_golden(name)
    return {"X": g["X"][:N].contiguous(), "Y": g["Y"][:N].contiguous(), "params": g["params"], "program": g["program"],
            "rowp": None, "N_total": float(g["N_total"]), "S": int(g["xs"].numel())}


@functools.lru_cache(maxsize=None)
def _oracle_step(M, flow):
    from oracle import tgp_oracle as orc
    prob = _problem(M, flow)
    return orc.elbo_and_grads(prob["X"], prob["Y"], prob["params"], prob["N_total"], prob["program"], prob["xs"], prob["ws"],
                              prob["rowp"])


def _run(prob, plan, garbage, nodes=S):
    from tgp.pytorch_amd import ops
    dev = torch.device("cuda:0")
    p = {k: v.to(dev) for k, v in prob["params"].items()}
    rowp = prob["rowp"].to(dev) if prob["rowp"] is not None else None
    fs = ops.FlowSpec(prob["program"], p["theta"].numel(), 0 if rowp is None else rowp.shape[1], dev)
    cached = ops.workspace
    ops.workspace = lambda *a, **kw: cached(*a, **kw).fill_(garbage)       # as a recycled allocation would be
    try:
        out, g, status, (mu, v) = ops.elbo_step(prob["X"].to(dev), prob["Y"].to(dev), p["Z"], p["raw_lengthscale"],
                                                p["raw_outputscale"], p["m"], p["Lam"], p["log_var_noise"], prob["N_total"],
                                                flow=fs, theta=p["theta"], rowp=rowp, S=nodes, plan=plan, want_moments=True)
        torch.cuda.synchronize()
    finally:
        ops.workspace = cached
    assert int(status[0]) == 0 and int(status[1]) == 0, (plan, status.tolist())
    res = {"out": out.cpu(), "mu": mu.cpu(), "v": v.cpu()}
    res.update({"g_" + k: t.cpu() for k, t in g.items()})
    return res


@functools.lru_cache(maxsize=None)
def _step(M, flow, plan_name, garbage):
    """one step of a case; shared by the tests (the results are compared, never changed)"""
    from tgp.pytorch_amd import lib
    return _run(_problem(M, flow), getattr(lib, plan_name), garbage)


def _assert_close(a, b, what):
    """every output of `a` within the bars of `b`; the gradient of theta on its own"""
    assert a.keys() == b.keys()
    errs = {k: rel_err(a[k], b[k]) for k in a if a[k].numel()}
    print("rows flow sums", what, " ".join("%s=%.2e" % kv for kv in errs.items()), flush=True)
    for k, e in errs.items():
        if k != "g_theta":
            assert e < (TOL_GRAD if k.startswith("g_") else TOL_VAL), (what, k, e)
    print("rows flow sums", what, "g_theta relative difference = %.3e" % errs["g_theta"], flush=True)
    assert errs["g_theta"] < TOL_GRAD, (what, "g_theta", errs["g_theta"])


@pytest.mark.parametrize("M,flow", CASES, ids=IDS)
def test_rw10_matches_oracle(M, flow):
    from oracle import tgp_oracle as orc
    prob = _problem(M, flow)
    (elbo, ell, kld), og = _oracle_step(M, flow)
    r = _step(M, flow, "PLAN_ROWS_K", 12345.678)
    pc = prob["params"]
    mo, vo = orc.qf_moments(prob["X"], pc["Z"], pc["raw_lengthscale"], pc["raw_outputscale"], pc["m"], pc["Lam"])
    errs = {"ELBO": rel_err(r["out"][0], elbo), "ELL": rel_err(r["out"][1], ell), "KLD": rel_err(r["out"][2], kld),
            "mu": rel_err(r["mu"], mo.reshape(-1)), "v": rel_err(r["v"], vo.reshape(-1))}
    errs.update({k: rel_err(t, og[NAMES[k[2:]]]) for k, t in r.items() if k.startswith("g_")})
    print("rows flow sums oracle", (M, flow), " ".join("%s=%.2e" % kv for kv in errs.items()), flush=True)
    assert "g_theta" in errs and (flow != "idsal3" or "g_rowp" in errs)
    for k, e in errs.items():
        assert e < (TOL_GRAD if k.startswith("g_") else TOL_VAL), ((M, flow), k, e)


@pytest.mark.parametrize("M,flow", CASES, ids=IDS)
def test_rw10_twice_bit_equal(M, flow):
    from tgp.pytorch_amd import lib
    a = _step(M, flow, "PLAN_ROWS_K", 12345.678)
    _run(_problem(17, "sal2"), lib.PLAN_ROWS_K, 4.5e3)       # another shape: the LDS no longer holds the first run's contents
    b = _run(_problem(M, flow), lib.PLAN_ROWS_K, -8765.4321)
    assert a.keys() == b.keys()
    for k in a:
        assert torch.isfinite(a[k]).all(), ((M, flow), k, "not finite")
        diff = float((a[k] - b[k]).abs().max()) if a[k].numel() else 0.0
        print("rows flow sums twice", (M, flow), k, "max |difference| = %.3e" % diff, flush=True)
        assert torch.equal(a[k], b[k]), ((M, flow), k, diff)


@pytest.mark.parametrize("M,flow", CASES, ids=IDS)
def test_rw10_matches_rw16(M, flow):
    a = _step(M, flow, "PLAN_ROWS_K", 12345.678)
    b = _step(M, flow, "PLAN_ROWS_K16", 777.25)
    differs = any(not torch.equal(a[k], b[k]) for k in a)
    assert differs, ((M, flow), "PLAN_ROWS_K ran the 16-rows-per-wave kernel")
    _assert_close(a, b, ((M, flow), "10 against 16 rows per wave"))


def test_rw10_extended_kinds_match_rw16():
    """Box-Cox + affine + arcsinh + affine (P = 9) through the TGP_FLOWX unit: one, four and two partials per block."""
    from tgp.pytorch_amd import lib
    prob = _fixture_problem("flows_power_bcl_al1")
    a = _run(prob, lib.PLAN_ROWS_K, 31415.9, nodes=prob["S"])
    b = _run(prob, lib.PLAN_ROWS_K16, -2.5e6, nodes=prob["S"])
    assert any(not torch.equal(a[k], b[k]) for k in a), "PLAN_ROWS_K ran the 16-rows-per-wave kernel"
    _assert_close(a, b, ("flows_power_bcl_al1", "10 against 16 rows per wave"))
