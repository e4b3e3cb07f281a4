"""GPU (-m gpu): the row kernel's (S - I) A form (csrc/tgp_rows.hpp: C = (S - I) A, v = s2 + sum A o C,
Abar = m mubar^T + 2 C diag(vbar)) against oracle/tgp_oracle.py, for every variant of k_rows that carries it:

  moments only (tgp_qf_moments_f64; it keeps B = L_q^T A) mu 1e-9, v 1e-9 of the largest entry (test_gpu_models.py's bar)
  training, 16 rows per wave, 4 nodes in flight          values 1e-9, gradients 1e-7 (test_gpu_parity.py's bars), and the
                                                         (mu, v) the training launch writes at the moments' bar
  training, 16 rows per wave, one node in flight         (a flow stack too long for four nodes in LDS)
  training, 10 rows per wave                             (the library selects it for 7 936 < N <= 10 240 only, so its
                                                          "small ragged" problem is N = 7 937: 198 full workgroups and one of 17 rows)
  training, closed-form Gaussian likelihood (SVGP)

at MT = 1, 4, 7, 8 (M = 16, 60, 100, 128), one Power-shaped problem (N = 8 611, D = 4, S = 32) and one small ragged one each.
`plan` pins the kernel: PLAN_ROWS_K16 = k_rows at 16 rows per wave, PLAN_ROWS_K = k_rows with its own rows-per-wave rule
(without it a small training problem runs on k_rows4, which keeps the B form).

Two more cases sit at the two ends of the cancellation in sum A o C: Lam scaled until ||S|| >> 1, and Lam = I + 1e-6 noise
(S - I ~ 0).  Every figure is printed before it is asserted."""
import functools

import pytest
import torch

from conftest import rel_err

pytestmark = pytest.mark.gpu

TOL_VAL = 1e-9
TOL_GRAD = 1e-7
MS = [16, 60, 100, 128]            # MT = 1, 4, 7, 8


@functools.lru_cache(maxsize=None)
def _problem(N, D, M, flow, S, lam):
    from oracle import tgp_oracle as orc       # checker only
    prob = orc.synthetic_problem(N, D, M, seed=23, flow=flow, S=S)
    p = prob["params"]
    if lam == "big":            # ||S|| >> 1: entries of L_q of order 10, ||S|| of order 1e2 M
        p["Lam"] = 200.0 * p["Lam"]
    elif lam == "eye":          # S - I ~ 0: the whitened prior, perturbed so that the product is not exactly zero
        gen = torch.Generator().manual_seed(29)
        p["Lam"] = torch.eye(M, dtype=torch.float64) + 1e-6 * torch.randn(M, M, generator=gen, dtype=torch.float64)
    return prob


@functools.lru_cache(maxsize=None)
def _oracle_step(key):
    from oracle import tgp_oracle as orc
    prob = _problem(*key)
    return orc.elbo_and_grads(prob["X"], prob["Y"], prob["params"], prob["N_total"], prob["program"], prob["xs"], prob["ws"],
                              prob["rowp"])


def _check_step(key, plan, expect_rw10=None):
    from oracle import tgp_oracle as orc
    from tgp.pytorch_amd import lib, ops
    dev = torch.device("cuda:0")
    N, D, M, flow, S, lam = key
    prob = _problem(*key)
    (elbo, ell, kld), og = _oracle_step(key)
    p = {k: v.to(dev) for k, v in prob["params"].items()}
    rowp = prob["rowp"].to(dev) if prob["rowp"] is not None else None
    fs = ops.FlowSpec(prob["program"], p["theta"].numel(), 0 if rowp is None else rowp.shape[1], dev) if flow else None

    def run(pl):
        out, g, status, (mu, v) = ops.elbo_step(prob["X"].to(dev), prob["Y"].to(dev), p["Z"], p["raw_lengthscale"],
                                          p["raw_outputscale"], p["m"], p["Lam"], p["log_var_noise"], prob["N_total"],
                                          flow=fs, theta=p.get("theta"), rowp=rowp, S=S, plan=pl, want_moments=True)
        torch.cuda.synchronize()
        assert int(status[0]) == 0 and int(status[1]) == 0
        return out.cpu(), {k: t.cpu() for k, t in g.items()}, mu.cpu(), v.cpu()

    out, g, mu, v = run(plan)
    if expect_rw10 is not None:
        # the kernel under test really is the 10-rows-per-wave one: forcing 16 rows per wave gives other bits
        o16, g16, _, _ = run(lib.PLAN_ROWS_K16)
        differs = not torch.equal(out, o16) or any(not torch.equal(g[k], g16[k]) for k in g)
        assert differs == expect_rw10, (key, "10 rows per wave expected: %s" % expect_rw10)
    names = {"Z": "Z", "raw_ls": "raw_lengthscale", "raw_os": "raw_outputscale", "m": "m", "Lam": "Lam", "lvn": "log_var_noise",
             "theta": "theta", "rowp": "rowp"}
    pc = prob["params"]
    mo, vo = orc.qf_moments(prob["X"], pc["Z"], pc["raw_lengthscale"], pc["raw_outputscale"], pc["m"], pc["Lam"])
    errs = {"ELBO": rel_err(out[0], elbo), "ELL": rel_err(out[1], ell), "KLD": rel_err(out[2], kld),
            "mu": rel_err(mu, mo.reshape(-1)), "v": rel_err(v, vo.reshape(-1))}
    errs.update({"g_" + k: rel_err(t, og[names[k]]) for k, t in g.items()})
    print("sform step", key, "plan", plan, " ".join("%s=%.2e" % kv for kv in errs.items()), flush=True)
    for k, e in errs.items():
        assert e < (TOL_GRAD if k.startswith("g_") else TOL_VAL), (key, plan, k, e)


def _check_moments(key):
    from oracle import tgp_oracle as orc
    from tgp.pytorch_amd import ops
    dev = torch.device("cuda:0")
    prob = _problem(*key)
    pc = prob["params"]
    mo, vo = orc.qf_moments(prob["X"], pc["Z"], pc["raw_lengthscale"], pc["raw_outputscale"], pc["m"], pc["Lam"])
    p = {k: v.to(dev) for k, v in pc.items()}
    mu, v = ops.qf_moments(prob["X"].to(dev), p["Z"], p["raw_lengthscale"], p["raw_outputscale"], p["m"], p["Lam"])
    torch.cuda.synchronize()
    em, ev = rel_err(mu.cpu(), mo.reshape(-1)), rel_err(v.cpu(), vo.reshape(-1))
    print("sform moments", key, "mu=%.2e v=%.2e" % (em, ev), "min v = %.3g" % float(vo.min()), flush=True)
    assert em < 1e-9 and ev < 1e-9, (key, em, ev)


@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("N", [8611, 157])
def test_moments_match_oracle(N, M):
    _check_moments((N, 4, M, None, 32, "std"))


@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("N", [8611, 157])
def test_train_rw16_matches_oracle(N, M):
    from tgp.pytorch_amd import lib
    _check_step((N, 4, M, "tanh3x2", 32, "std"), lib.PLAN_ROWS_K16)


@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("N", [8611, 7937])
def test_train_rw10_matches_oracle(N, M):
    from tgp.pytorch_amd import lib
    _check_step((N, 4, M, "tanh3x2", 32, "std"), lib.PLAN_ROWS_K, expect_rw10=True)


@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("N", [8611, 157])
def test_train_closed_form_matches_oracle(N, M):
    from tgp.pytorch_amd import lib
    _check_step((N, 4, M, None, 32, "std"), lib.PLAN_ROWS_K16)


@pytest.mark.parametrize("N", [8611, 157])
def test_train_one_node_in_flight_matches_oracle(N):
    """tanh5x6 at M = 100, D = 8: 35 stack slots, four nodes in flight do not fit beside the tiles -> k_rows<.., MODE = 2>."""
    from tgp.pytorch_amd import lib
    _check_step((N, 8, 100, "tanh5x6", 32, "std"), lib.PLAN_ROWS_K16)


@pytest.mark.parametrize("lam", ["big", "eye"])
@pytest.mark.parametrize("rw", [10, 16])
def test_cancellation_ends_match_oracle(rw, lam):
    """||S|| >> 1 and S - I ~ 0 at Power shape, training and moments."""
    from tgp.pytorch_amd import lib
    key = (8611, 4, 100, "tanh3x2", 32, lam)
    if rw == 10:
        _check_step(key, lib.PLAN_ROWS_K, expect_rw10=True)
    else:
        _check_step(key, lib.PLAN_ROWS_K16)
        _check_moments(key)
