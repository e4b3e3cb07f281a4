"""GPU (-m gpu): greedy conditional-variance selection of inducing points in HIP (tgp_greedy_inducing_f64), through the C ABI,
against the float64 CPU recurrence of tests/greedy_model.py; then utils.GREEDY_VARIANCE into a model.

Largest shortfall of the greedy property seen on an MI355X, in units of the allowed 64 (j + 1) 2^-52 s2: see DESIGN.md §8."""
import functools
import math

import pytest
import torch

import greedy_model as gm

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F64 = torch.float64
TOL = 1e-9            # the project's tolerance for a float64 kernel against its restatement
KINDS = ("scale_rbf", "scale_matern32")
CASES = [s + (k,) for s in gm.GPU_SHAPES for k in KINDS]
EXACT = [c for c in CASES if c not in gm.NEAR_TIES]
ids = lambda c: "%d-%d-%d-%s" % c          # noqa: E731


@pytest.fixture(scope="module", autouse=True)
def f64():
    from tgp.pytorch_amd import config as cg
    old = torch.get_default_dtype()
    cg.set_maximum_precission()
    cg.device = DEV
    yield
    torch.set_default_dtype(old)


def run(p, M, min_var=gm.MIN_VAR, ws=None, ws_bytes=None, expect=0):
    """One call of tgp_greedy_inducing_f64: (idx (M,) int32, Z (M, D), trace (M + 1,), M_eff, the workspace), all M entries with
    their tails, on the host (one read-back); the outputs start as sentinels so that an entry never written shows."""
    from tgp.pytorch_amd import lib as L
    lib = L.load()
    N, D = p["X"].shape
    X, rl, ro = p["X"].to(DEV), p["raw_ls"].to(DEV), p["raw_os"].to(DEV)
    need = lib.tgp_greedy_inducing_workspace_bytes(N, D, M)
    if ws is None:
        ws = torch.empty(max(need, 8) // 8 + 1, dtype=F64, device=DEV)
    idx = torch.full((max(M, 1),), -7, dtype=torch.int32, device=DEV)
    Z = torch.full((max(M, 1), D), -7.0, dtype=F64, device=DEV)
    trace = torch.full((max(M, 1) + 1,), -7.0, dtype=F64, device=DEV)
    count = torch.full((1,), -7, dtype=torch.int32, device=DEV)
    rc = lib.tgp_greedy_inducing_f64(L.ptr(X), N, D, L.ptr(rl), L.ptr(ro), L.KERNELS.get(p["kernel"], p["kernel"]), M, min_var,
                                     L.ptr(idx), L.ptr(Z), L.ptr(trace), L.ptr(count), L.ptr(ws), need if ws_bytes is None else ws_bytes,
                                     L.stream_ptr())
    assert rc == expect, (rc, lib.tgp_last_error())
    torch.cuda.synchronize()
    return idx.cpu(), Z.cpu(), trace.cpu(), int(count.cpu()), ws


@functools.lru_cache(maxsize=None)
def _case(case):
    """(inputs, the device's outputs, C read from the workspace, the CPU recurrence along the DEVICE's sequence): once per case."""
    N, M, D, kind = case
    p = gm.make_case(*case)
    idx, Z, trace, m_eff, ws = run(p, M)
    C = ws[:M * N].reshape(M, N).cpu()        # the workspace's first section (torch allocations are 16-byte aligned)
    ok = m_eff == M and len(set(idx.tolist())) == M and 0 <= int(idx.min()) and int(idx.max()) < N
    return p, (idx, Z, trace, m_eff), C, gm.greedy(p, follow=idx.to(torch.int64)) if ok else None


@pytest.mark.parametrize("case", CASES, ids=ids)
def test_greedy_property_on_the_devices_own_sequence(case):
    """The CPU follows the device's idx and does not choose: at every step the row the device took has, in the CPU's arithmetic,
    a conditional variance within 64 (j + 1) 2^-52 s2 of the best one -- whichever way a near-tie fell.  The margin is a
    forward-error allowance (each of the j subtracted products is rounded to a few ulp of s2, exp_fast is within ulps of exp)."""
    p, (idx, _, _, m_eff), _, f = _case(case)
    assert m_eff == case[1] and f is not None, (m_eff, idx)
    assert int(idx[0]) == 0
    j = torch.arange(1, case[1] + 1, dtype=F64)
    short = (f["dmax"] - f["dpiv"]) / (64.0 * j * 2.0 ** -52 * p["s2"])
    print(case, "largest shortfall / allowance: %.3g" % float(short.max()))
    assert float(short.max()) <= 1.0


@pytest.mark.parametrize("case", EXACT, ids=ids)
def test_sequence_equals_the_cpus_where_no_step_is_a_near_tie(case):
    """The CPU's own best and second-best d are more than 1e-9 s2 apart at every step after step 0 (asserted here): idx must be
    the CPU's, p_0 = 0 included.  (The kept near-tie, RBF 1000 / 129 / 4, stays in CASES for the property test above;
    tests/test_greedy_host.py asserts on the CPU that its gap is under the line.)"""
    p, (idx, _, _, _), _, _ = _case(case)
    r = gm.greedy(p)
    assert bool((r["gap"][1:] > gm.GAP * p["s2"]).all())
    assert idx.tolist() == r["idx"].tolist()


@pytest.mark.parametrize("case", CASES, ids=ids)
def test_values_match_the_recurrence_along_the_same_sequence(case):
    """trace at 1e-9 of N s2, C (read from the workspace) at 1e-9 of s2, Z = X[idx] bit for bit."""
    p, (idx, Z, trace, m_eff), C, f = _case(case)
    assert f is not None
    N, s2 = p["N"], p["s2"]
    e_tr = float((trace - f["trace"]).abs().max()) / (N * s2)
    e_c = float((C - f["C"]).abs().max()) / s2
    print(case, "trace %.3g  C %.3g" % (e_tr, e_c))
    assert e_tr < TOL and e_c < TOL
    assert bool((trace[1:] <= trace[:-1]).all())
    assert torch.equal(Z, p["X"][idx.to(torch.int64)])


@pytest.mark.parametrize("kind", KINDS)
def test_early_stop_on_repeated_rows(kind):
    """R = 7 distinct rows at least 3.5 length-scales apart, each 50 times (two workgroups), M = 20 asked: M_eff = 7 exactly, the
    first copy of each distinct row, tails idx = -1 / trace = NaN / Z = NaN; all 20 step launches are enqueued, no error."""
    R, reps, M = 7, 50, 20
    p, group = gm.make_repeats(R, reps, 4, kind)
    idx, Z, trace, m_eff, _ = run(p, M)
    assert m_eff == R
    taken = idx[:R].to(torch.int64)
    assert sorted(group[taken].tolist()) == list(range(R))
    for i in taken.tolist():
        assert i == int(torch.nonzero(group == group[i])[0])          # ties go to the smallest index
    assert idx[R:].tolist() == [-1] * (M - R)
    assert bool(torch.isnan(trace[R + 1:]).all()) and bool(torch.isnan(Z[R:]).all()) and not bool(torch.isnan(trace[:R + 1]).any())
    assert torch.equal(Z[:R], p["X"][taken])
    r = gm.greedy(p, M=M)
    assert r["M_eff"] == R and r["idx"].tolist() == taken.tolist()
    assert float((trace[:R + 1] - r["trace"]).abs().max()) < TOL * p["N"] * p["s2"]


def _bits(t):
    return t.contiguous().view(torch.int64) if t.dtype == F64 else t


def test_repeats_are_bit_identical_and_a_stopped_call_leaves_nothing_behind():
    """Two calls: the same bits in idx, Z, trace.  Then an early-stopped call and the first problem again on the SAME workspace
    (same N, D, M: the stop word and the records sit where the stopped call left them): unaffected."""
    R, reps, M = 7, 50, 20
    p = gm.make_case(R * reps, M, 4, "scale_rbf")
    a = run(p, M)
    b = run(p, M)
    assert a[3] == b[3] == M
    for x, y in zip(a[:3], b[:3]):
        assert torch.equal(_bits(x), _bits(y))
    q, _ = gm.make_repeats(R, reps, 4, "scale_rbf")
    ws = a[4]
    assert run(q, M, ws=ws)[3] == R
    c = run(p, M, ws=ws)
    assert c[3] == M
    for x, y in zip(a[:3], c[:3]):
        assert torch.equal(_bits(x), _bits(y))


def test_refusals_name_the_entry_and_launch_nothing():
    from tgp.pytorch_amd import lib as L
    lib = L.load()
    p = gm.make_case(300, 10, 4, "scale_rbf")
    big = torch.empty(1 << 16, dtype=F64, device=DEV)
    for M in (0, 301, 4097):
        out = run(p, M, ws=big, ws_bytes=big.numel() * 8, expect=L.E_UNSUPPORTED)
        assert b"tgp_greedy_inducing_f64" in lib.tgp_last_error() and out[3] == -7
    for D in (0, 17):
        q = dict(p, X=torch.zeros(300, D, dtype=F64), raw_ls=torch.zeros(max(D, 1), dtype=F64))
        run(q, 10, ws=big, ws_bytes=big.numel() * 8, expect=L.E_UNSUPPORTED)
        assert b"tgp_greedy_inducing_f64" in lib.tgp_last_error()
    run(dict(p, kernel=2), 10, ws=big, ws_bytes=big.numel() * 8, expect=L.E_UNSUPPORTED)
    assert b"tgp_greedy_inducing_f64" in lib.tgp_last_error()
    need = lib.tgp_greedy_inducing_workspace_bytes(300, 4, 10)
    idx, Z, trace, count, _ = run(p, 10, ws=big, ws_bytes=need - 24, expect=L.E_WORKSPACE)        # (16 bytes are alignment slack)
    assert b"tgp_greedy_inducing_f64" in lib.tgp_last_error() and str(need).encode() in lib.tgp_last_error()
    assert count == -7 and idx.tolist() == [-7] * 10 and bool((trace == -7.0).all()) and bool((Z == -7.0).all())


def test_greedy_variance_into_a_model():
    """N = 1000, M = 64: a model built on GREEDY_VARIANCE's rows has a finite collapsed bound, and the package's own
    tr(K_XX) - tr(K_XZ K_ZZ^-1 K_ZX) (ops.kernel_matrix, float64 solve on the host) meets trace[M] at 1e-9 of N s2."""
    from tgp.pytorch_amd import ops
    from tgp.pytorch_amd.kernels import instance_kernel
    from tgp.pytorch_amd.likelihoods import GaussianLinearMean
    from tgp.pytorch_amd.models import sparse_MF_GP
    from tgp.pytorch_amd.utils import GREEDY_VARIANCE
    N, M, D = 1000, 64, 4
    p = gm.make_case(N, M, D, "scale_rbf")
    g = torch.Generator().manual_seed(3)
    Y = torch.sin(p["X"] @ torch.randn(D, dtype=F64, generator=g)) + 0.3 * torch.randn(N, dtype=F64, generator=g)
    K = instance_kernel("scale_rbf", ard_num_dim=D, num_multioutput=1, kernel_is_shared=False,
                        init_params={"length_scale": 1.0, "kernel_scale": 1.5})
    Z, info = GREEDY_VARIANCE(p["X"], M, K, return_info=True)
    idx, trace = info["idx"].cpu(), info["trace"].cpu()
    assert Z.shape == (M, D) and torch.equal(Z.cpu(), p["X"][idx]) and trace.shape == (M + 1,)
    model = sparse_MF_GP(["zero", K], p["X"], Z.cpu().clone(), N, GaussianLinearMean(1, 0.05, False), 1, True, False, False, False,
                         False, 0.0).to(DEV)
    assert torch.equal(model.Z.detach()[0].cpu(), p["X"][idx])
    bound = model.collapsed_bound(p["X"].to(DEV), Y.reshape(-1, 1).to(DEV))[0]
    assert math.isfinite(float(bound))
    rl, ro = K._params()
    rl, ro, Xd = rl.to(DEV), ro.to(DEV), p["X"].to(DEV)
    Kzz = ops.kernel_matrix(Z.to(DEV), None, rl, ro).cpu()
    Kzx = ops.kernel_matrix(Z.to(DEV), Xd, rl, ro).cpu()
    s2 = float(torch.nn.functional.softplus(ro))
    resid = N * s2 - float((Kzx * torch.linalg.solve(Kzz, Kzx)).sum())
    print("trace[M] %.12g  tr(K - Q) %.12g  of N s2 = %.6g" % (float(trace[-1]), resid, N * s2))
    assert abs(float(trace[-1]) - resid) < TOL * N * s2
