"""CPU: greedy conditional-variance selection of inducing points -- the recurrence restated in float64 (tests/greedy_model.py)
against a dense solve, the library's host-side refusals, and utils.GREEDY_VARIANCE / ops.greedy_inducing with the library stubbed."""
import ctypes as C
import math

import pytest
import torch

import greedy_model as gm
from tgp.pytorch_amd import lib as L
from tgp.pytorch_amd import ops

F64 = torch.float64


@pytest.fixture(scope="module", autouse=True)
def f64():
    from tgp.pytorch_amd import config as cg
    old = torch.get_default_dtype()
    cg.set_maximum_precission()
    cg.device = "cpu"
    yield
    torch.set_default_dtype(old)


# ---- the recurrence ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", gm.CPU_CASES, ids=lambda c: "%d-%d-%d-%s" % c)
def test_two_routes_agree_at_every_step(case):
    """d and the trace of the recurrence against diag / tr of K - K[:,S] K[S,S]^-1 K[S,:] by a dense solve, at every step.
    cond(K[S,S]) <= 1e5 bounds the dense route's own error by 1e5 x 2^-52 = 2e-11 of s2, so 1e-9 holds both; the figures stay
    where GREEDY_CPU recorded them (4 x: another BLAS may round differently; 1e-15: figures of a few ulp)."""
    assert set(gm.GREEDY_CPU) == set(gm.CPU_CASES)
    m, r = gm.measure(case)
    rec = gm.GREEDY_CPU[case]
    print(case, m)
    assert r["M_eff"] == case[1]
    assert m["cond"] <= 1e5 and 0.5 * rec["cond"] <= m["cond"] <= 2.0 * rec["cond"]
    assert m["d"] < 1e-9 and m["d"] <= 4.0 * rec["d"] + 1e-15
    assert m["trace"] < 1e-9 and m["trace"] <= 4.0 * rec["trace"] + 1e-15


@pytest.mark.parametrize("case", gm.CPU_CASES, ids=lambda c: "%d-%d-%d-%s" % c)
def test_trace_never_increases_and_rows_are_picked_once(case):
    p = gm.make_case(*case)
    r = gm.greedy(p)
    tr, idx = r["trace"], r["idx"]
    assert tr[0] == p["N"] * p["s2"] and bool((tr[1:] <= tr[:-1]).all()) and bool((tr >= 0).all())
    assert len(set(idx.tolist())) == len(idx) and int(idx[0]) == 0
    # (the restatement returns no Z, so Z == X[idx] has nothing to bite on here: test_ops_greedy_inducing_slices_to_m_eff checks
    # it of the host wrapper, tests/test_gpu_greedy.py of the device, bit for bit)
    # following its own sequence, the recurrence never finds a better row than the one it took
    f = gm.greedy(p, follow=idx)
    assert torch.equal(f["C"], r["C"]) and torch.equal(f["dpiv"], f["dmax"])


def test_step_zero_tie_goes_to_row_zero_and_duplicates_stop_the_selection():
    """R distinct rows, each repeated: M_eff = R, the first copy (smallest index) of each, and the trace ends at rounding level."""
    p, group = gm.make_repeats(5, 13, 4, "scale_rbf")
    r = gm.greedy(p, M=12)
    assert r["M_eff"] == 5 and sorted(group[r["idx"]].tolist()) == list(range(5))
    for i in r["idx"].tolist():
        assert i == int(torch.nonzero(group == group[i])[0])
    assert float(r["trace"][-1]) <= 1e-12 * p["N"] * p["s2"]


def test_the_gpu_cases_that_must_match_exactly_clear_the_gap():
    """The exact-sequence list of tests/test_gpu_greedy.py, on the CPU: every case outside NEAR_TIES keeps its best and
    second-best d more than 1e-9 s2 apart after step 0, the kept near-tie RBF 1000 / 129 / 4 does not."""
    for shape in gm.GPU_SHAPES:
        for kind in ("scale_rbf", "scale_matern32"):
            case = shape + (kind,)
            p = gm.make_case(*case)
            r = gm.greedy(p)
            assert r["M_eff"] == shape[1] and float(r["dpiv"].min()) > 2.0 * gm.MIN_VAR, case
            clear = bool((r["gap"][1:] > gm.GAP * p["s2"]).all())
            assert clear == (case not in gm.NEAR_TIES), (case, float(r["gap"][1:].min()) / p["s2"])


# ---- the library's refusals: host-only, nothing touches a device ----------------------------------------------------------
def test_library_refuses_outside_its_limits():
    lib = L.load()
    assert lib.tgp_greedy_inducing_workspace_bytes(8611, 4, 100) >= 8 * (100 * 8611 + 8611)
    fake = C.c_void_p(64)
    for N, D, M, kern in ((10, 4, 0, 0), (10, 4, 11, 0), (5000, 4, 4097, 0), (10, 0, 2, 0), (10, 17, 2, 0), (0, 4, 1, 0), (10, 4, 2, 2)):
        if kern == 0:
            assert lib.tgp_greedy_inducing_workspace_bytes(N, D, M) == 0
        rc = lib.tgp_greedy_inducing_f64(fake, N, D, fake, fake, kern, M, 1e-8, fake, fake, fake, fake, fake, 1 << 40, None)
        assert rc == L.E_UNSUPPORTED and b"tgp_greedy_inducing_f64" in lib.tgp_last_error(), (N, D, M, kern)
    need = lib.tgp_greedy_inducing_workspace_bytes(100, 4, 10)
    assert lib.tgp_greedy_inducing_workspace_bytes(5000, 16, 4096) > 0
    rc = lib.tgp_greedy_inducing_f64(fake, 100, 4, fake, fake, 0, 10, 1e-8, fake, fake, fake, fake, fake, need - 24, None)
    assert rc == L.E_WORKSPACE and b"tgp_greedy_inducing_f64" in lib.tgp_last_error() and str(need).encode() in lib.tgp_last_error()
    for bad in (-1e-8, math.nan):
        assert lib.tgp_greedy_inducing_f64(fake, 100, 4, fake, fake, 0, 10, bad, fake, fake, fake, fake, fake, need, None) == -8
    assert lib.tgp_greedy_inducing_f64(None, 100, 4, fake, fake, 0, 10, 1e-8, fake, fake, fake, fake, fake, need, None) == -1
    assert lib.tgp_greedy_inducing_f64(fake, 100, 4, fake, fake, 0, 10, 1e-8, None, fake, fake, fake, fake, need, None) == -9


# ---- host plumbing, the library stubbed -----------------------------------------------------------------------------------
class StubLib:
    """tgp_greedy_inducing_f64 on host tensors: records what it was handed and answers with the first `m_eff` rows."""

    def __init__(self, m_eff=None):
        self.m_eff, self.calls = m_eff, []

    def tgp_greedy_inducing_workspace_bytes(self, N, D, M):
        return 512

    def tgp_greedy_inducing_f64(self, X, N, D, rl, ro, kernel, M, min_var, idx, Z, trace, count, ws, nbytes, stream):
        ls = list((C.c_double * D).from_address(rl.value))
        self.calls.append(dict(N=N, D=D, M=M, kernel=kernel, min_var=min_var, nbytes=nbytes, raw_ls=ls,
                               raw_os=(C.c_double * 1).from_address(ro.value)[0]))
        m_eff = M if self.m_eff is None else self.m_eff
        x = (C.c_double * (N * D)).from_address(X.value)
        iv, zv = (C.c_int32 * M).from_address(idx.value), (C.c_double * (M * D)).from_address(Z.value)
        tv = (C.c_double * (M + 1)).from_address(trace.value)
        for i in range(M):
            iv[i] = 2 * i if i < m_eff else -1
            tv[i + 1] = float(N - i - 1) if i < m_eff else math.nan
            for k in range(D):
                zv[i * D + k] = x[2 * i * D + k] if i < m_eff else math.nan
        tv[0] = float(N)
        (C.c_int32 * 1).from_address(count.value)[0] = m_eff
        return 0


@pytest.fixture
def stub(monkeypatch):
    monkeypatch.setattr(L, "ptr", lambda t: None if t is None else C.c_void_p(t.data_ptr()))
    monkeypatch.setattr(L, "stream_ptr", lambda: None)
    from tgp.pytorch_amd import utils
    monkeypatch.setattr(utils, "_hip_device", lambda X, who: X.device)

    def make(m_eff=None):
        lib = StubLib(m_eff)
        monkeypatch.setattr(L, "load", lambda: lib)
        return lib
    return make


def _kernel(name, D, ls=1.5, ks=0.7):
    from tgp.pytorch_amd.kernels import instance_kernel
    return instance_kernel(name, ard_num_dim=D, num_multioutput=1, kernel_is_shared=False,
                           init_params={"length_scale": ls, "kernel_scale": ks})


def test_ops_greedy_inducing_slices_to_m_eff(stub):
    lib = stub(3)
    X = torch.randn(12, 2, dtype=F64, generator=torch.Generator().manual_seed(0))
    idx, Z, trace, m_eff = ops.greedy_inducing(X, 5, torch.zeros(2, dtype=F64), torch.zeros(1, dtype=F64), kernel="scale_matern32",
                                               min_var=1e-6)
    assert m_eff == 3 and idx.tolist() == [0, 2, 4] and idx.dtype == torch.int64
    assert torch.equal(Z, X[idx]) and trace.tolist() == [12.0, 11.0, 10.0, 9.0]
    assert lib.calls[-1]["kernel"] == L.KERNEL_SCALE_MATERN32 and lib.calls[-1]["min_var"] == 1e-6 and lib.calls[-1]["nbytes"] == 512
    with pytest.raises(ValueError, match="raw_ls"):
        ops.greedy_inducing(X, 5, torch.zeros(3, dtype=F64), torch.zeros(1, dtype=F64))
    with pytest.raises(L.TgpError, match="float64"):
        ops.greedy_inducing(X.float(), 5, torch.zeros(2, dtype=F64), torch.zeros(1, dtype=F64))


@pytest.mark.parametrize("name", ["scale_rbf", "scale_matern32"])
def test_greedy_variance_reads_the_kernel_and_returns_rows(stub, name):
    from tgp.pytorch_amd.utils import GREEDY_VARIANCE, inv_softplus
    lib = stub()
    X = torch.randn(12, 3, dtype=F64, generator=torch.Generator().manual_seed(1))
    K = _kernel(name, 3)
    Z = GREEDY_VARIANCE(X, 4, K)
    call = lib.calls[-1]
    assert call["kernel"] == L.KERNELS[name] and (call["N"], call["D"], call["M"], call["min_var"]) == (12, 3, 4, 1e-8)
    assert call["raw_ls"] == [float(inv_softplus(1.5))] * 3 and call["raw_os"] == float(inv_softplus(0.7))
    assert Z.shape == (4, 3) and torch.equal(Z, X[[0, 2, 4, 6]])
    Z2, info = GREEDY_VARIANCE(X, 4, K, min_var=1e-6, return_info=True)
    assert torch.equal(Z2, Z) and info["idx"].tolist() == [0, 2, 4, 6] and info["trace"].shape == (5,)
    assert lib.calls[-1]["min_var"] == 1e-6
    # one shared length-scale (ard_num_dims=None) serves every column
    Kiso = _kernel(name, None)
    GREEDY_VARIANCE(X, 2, Kiso)
    assert lib.calls[-1]["raw_ls"] == [float(inv_softplus(1.5))] * 3


def test_greedy_variance_argument_checks(stub):
    from tgp.pytorch_amd.utils import GREEDY_VARIANCE
    lib = stub(2)
    X = torch.randn(12, 3, dtype=F64, generator=torch.Generator().manual_seed(2))
    K = _kernel("scale_rbf", 3)
    with pytest.raises(ValueError, match="M_eff = 2"):
        GREEDY_VARIANCE(X, 4, K)
    n = len(lib.calls)
    with pytest.raises(TypeError, match="ScaleKernel"):
        GREEDY_VARIANCE(X, 4, "scale_rbf")
    with pytest.raises(ValueError, match="num_Z"):
        GREEDY_VARIANCE(X, 0, K)
    with pytest.raises(ValueError, match="num_Z"):
        GREEDY_VARIANCE(X, 13, K)
    with pytest.raises(ValueError, match="length-scales"):
        GREEDY_VARIANCE(X, 4, _kernel("scale_rbf", 2))
    with pytest.raises(ValueError, match="min_var"):
        GREEDY_VARIANCE(X, 4, K, min_var=-1.0)
    with pytest.raises(ValueError, match="X"):
        GREEDY_VARIANCE(X.reshape(-1), 4, K)
    assert len(lib.calls) == n                                     # refused before the library is asked


class _ModelReached(Exception):
    pass


@pytest.mark.parametrize("init", ["default", "kmeans", "greedy"])
def test_main_hands_the_chosen_rows_to_the_model(monkeypatch, capsys, init):
    """main([...]) run up to the model's construction, with the data set, both initialisers and the model stubbed: greedy selects
    with the kernel main.py builds (scale_rbf at length-scale 2, scale 2), after the likelihood is set up, prints
    trace[M] / trace[0], and its rows are the model's init_Z; the default and kmeans never ask the greedy selection."""
    from tgp.pytorch_amd import config as cg
    from tgp.pytorch_amd import main as M
    from tgp.pytorch_amd.kernels import ScaleKernel
    monkeypatch.setattr(cg, "device", "cpu")                        # (main sets it; restored after the test)
    X = torch.randn(20, 3, dtype=F64, generator=torch.Generator().manual_seed(4))
    dc = {"X_tr": X, "Y_tr": X[:, :1].clone(), "Dx": 3, "Dy": 1, "N_tr": 20, "Y_std": 1.0}
    monkeypatch.setattr(M, "return_dataset", lambda *a, **k: ([None, None, None], dc))
    asked = []

    def kmeans(Xa, num_Z, **kw):
        asked.append("kmeans")
        return Xa[:num_Z] + 0.5

    def greedy(Xa, num_Z, kernel, min_var=1e-8, return_info=False):
        asked.append("greedy")
        assert Xa is X and num_Z == 5 and return_info and isinstance(kernel, ScaleKernel) and kernel.hip_kernel == "scale_rbf"
        ls, os_ = kernel._params()
        assert torch.allclose(torch.nn.functional.softplus(ls), torch.full((3,), 2.0, dtype=ls.dtype))
        assert torch.allclose(torch.nn.functional.softplus(os_), torch.full((1,), 2.0, dtype=os_.dtype))
        idx = torch.arange(0, 10, 2)
        return Xa[idx], {"idx": idx, "trace": torch.tensor([40.0, 30.0, 20.0, 10.0, 5.0, 2.5], dtype=F64)}

    def model(**kw):
        raise _ModelReached(kw)

    monkeypatch.setattr(M, "KMEANS", kmeans)
    monkeypatch.setattr(M, "GREEDY_VARIANCE", greedy)
    monkeypatch.setattr(M, "sparse_MF_GP", model)
    argv = ["--model", "SVGP", "--dataset", "synthetic_power", "--train_test_seed_split", "1", "--num_inducing", "5"]
    if init != "default":
        argv += ["--init_Z", init]
    with pytest.raises(_ModelReached) as e:
        M.main(argv)
    kw = e.value.args[0]
    out = capsys.readouterr().out
    if init == "greedy":
        assert asked == ["greedy"] and torch.equal(kw["init_Z"], X[0:10:2])
        assert "init_Z greedy: trace[M]/trace[0] = 6.250000e-02" in out
    else:
        assert asked == ["kmeans"] and torch.equal(kw["init_Z"], X[:5] + 0.5) and "init_Z" not in out


def test_main_refuses_greedy_for_multiclass(capsys):
    from tgp.pytorch_amd import main as M
    with pytest.raises(SystemExit):
        M.main(["--model", "SVGP", "--dataset", M.MULTICLASS_DATASETS[0], "--train_test_seed_split", "1", "--num_inducing", "5",
                "--likelihood", "multiclass", "--init_Z", "greedy"])
    assert "--init_Z greedy" in capsys.readouterr().err
