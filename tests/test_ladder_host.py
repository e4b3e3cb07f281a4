"""CPU: psd_safe_cholesky's retry protocol as each operator runs it (ops.run_jitter_ladder is their only retry loop), with
the library stubbed: the stub "factorises" on CPU tensors, fails a scripted number of times and records the jitter of every
call.  ops.run_jitter_ladder itself: tests/test_unwhiten_host.py."""
import ctypes as C
import warnings

import pytest
import torch

from tgp.pytorch_amd import lib as L
from tgp.pytorch_amd import ops

LADDER = [0.0, 1e-8, 1e-7, 1e-6]            # the first try, then ops.jitter_ladder()
PIVOT = 3
N, D, M = 6, 2, 4


class StubLib:
    """The entry points the five operators launch through: the first `failures` calls report a failed pivot (`nan`: NaN in
    K_MM instead), every call records its jitter."""

    def __init__(self, failures, nan=False):
        self.failures, self.nan, self.seen = failures, nan, []

    def _factorise(self, jitter, status):
        self.seen.append(float(jitter))
        bad = len(self.seen) <= self.failures
        words = (C.c_int32 * 8).from_address(status.value)
        words[0], words[1] = (PIVOT if bad and not self.nan else 0), int(bad and self.nan)
        return 0

    def tgp_elbo_step_f64(self, md, X, Y, rowp, out, gs, mu, v, status, ws, nbytes, stream):
        return self._factorise(md.jitter, status)

    def tgp_qf_moments_f64(self, md, X, mu, v, status, ws, nbytes, stream):
        return self._factorise(md.jitter, status)

    def tgp_qf_cov_f64(self, md, X, mu, Sigma, status, ws, nbytes, stream):
        return self._factorise(md.jitter, status)

    def tgp_qf_joint_sample_f64(self, mu, Sigma, n, jitter, eps, S, F0, Ls, status, ws, nbytes, stream):
        return self._factorise(jitter, status)

    def tgp_qf_cov_workspace_bytes(self, *shape):
        return 64

    tgp_qf_joint_sample_workspace_bytes = tgp_qf_cov_workspace_bytes


@pytest.fixture
def stub(monkeypatch):
    """ops on CPU tensors: host addresses for device pointers, no stream, a fixed workspace; returns the StubLib factory."""
    monkeypatch.setattr(L, "ptr", lambda t: None if t is None else C.c_void_p(t.data_ptr()))
    monkeypatch.setattr(L, "stream_ptr", lambda: None)
    monkeypatch.setattr(ops, "workspace", lambda *a, **k: torch.empty(8, dtype=torch.float64))
    reads = []
    real = ops.raise_for_status
    monkeypatch.setattr(ops, "raise_for_status", lambda st: reads.append(1) or real(st))

    def make(failures, nan=False):
        lib = StubLib(failures, nan)
        lib.status_reads = reads
        del reads[:]
        monkeypatch.setattr(L, "load", lambda: lib)
        return lib
    return make


def _gp():
    g = torch.Generator().manual_seed(0)
    r = lambda *s: torch.randn(*s, dtype=torch.float64, generator=g)      # noqa: E731
    return r(N, D), r(M, D), r(D), r(1), r(M), r(M, M)                   # X, Z, raw_ls, raw_os, m, Lam


def run_elbo_step_safe(info, **kw):
    X, Z, rl, ro, m, Lam = _gp()
    ops.elbo_step_safe(X, torch.zeros(N, dtype=torch.float64), Z, rl, ro, m, Lam, torch.zeros(1, dtype=torch.float64), N)


def run_qf_moments(info, **kw):
    ops.qf_moments(*_gp(), info=info, **kw)


def run_qf_cov(info, **kw):
    ops.qf_cov(*_gp(), info=info, **kw)


def run_qf_joint_sample_safe(info, **kw):
    ops.qf_joint_sample_safe(torch.zeros(N, dtype=torch.float64), torch.eye(N, dtype=torch.float64),
                             torch.zeros(2, N, dtype=torch.float64), info=info)


# operator -> (runner, the matrix its NotPSDError names, whether the message carries the pivot, whether it fills `info`)
OPERATORS = {"elbo_step_safe": (run_elbo_step_safe, "K_MM", True, False), "qf_moments": (run_qf_moments, "K_MM", False, True),
             "qf_cov": (run_qf_cov, "K_MM", False, True), "qf_joint_sample_safe": (run_qf_joint_sample_safe, "Sigma", True, True)}


def check_protocol(run, seen, failures, what, pivot, info):
    """`failures` failed calls, then success: the jitters tried, info["jitter"], the one warning -- or the exhaustion."""
    want = LADDER[:failures + 1]
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        if failures >= len(LADDER):
            with pytest.raises(ops.NotPSDError) as err:
                run()
            msg = str(err.value)
            assert what in msg and ("%g" % LADDER[-1]) in msg and (("(pivot %d)" % PIVOT) in msg) == pivot
            want = LADDER
        else:
            run()
    assert seen() == pytest.approx(want, rel=1e-12, abs=0.0) and len(seen()) == len(want)
    hits = [x for x in w if issubclass(x.category, ops.NumericalWarning)]
    if 0 < failures < len(LADDER):
        assert len(hits) == 1 and str(hits[0].message) == "A not p.d., added jitter of %g to the diagonal" % want[-1]
    else:
        assert not hits
    if info is not None:         # the value it ended with; the start when every rung failed
        assert info["jitter"] == pytest.approx(want[-1] if failures < len(LADDER) else 0.0, rel=1e-12, abs=0.0)


@pytest.mark.parametrize("failures", (0, 1, 3, 4), ids=("clean", "fails_at_0", "through_second_rung", "never"))
@pytest.mark.parametrize("op", sorted(OPERATORS))
def test_operator_follows_the_ladder(stub, op, failures):
    run, what, pivot, fills = OPERATORS[op]
    lib, info = stub(failures), {}
    check_protocol(lambda: run(info), lambda: lib.seen, failures, what, pivot, info if fills else None)
    assert len(lib.status_reads) == len(lib.seen)        # one status read (one host sync) per attempt


@pytest.mark.parametrize("op", ("qf_moments", "qf_cov"))
def test_unchecked_call_is_one_launch_and_no_status_read(stub, op):
    lib, info = stub(4), {}
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        OPERATORS[op][0](info, check=False, jitter=1e-7)
    assert lib.seen == [1e-7] and lib.status_reads == [] and info["jitter"] == 1e-7


@pytest.mark.parametrize("op", sorted(OPERATORS))
def test_nan_is_raised_before_any_retry(stub, op):
    lib = stub(4, nan=True)
    with pytest.raises(ops.NanError):
        OPERATORS[op][0]({})
    assert lib.seen == [0.0]


A0 = (2.0, 3.0)


def _stub_cholesky(monkeypatch, A, failures):
    """ops.cholesky stubbed: the jitter of a call is what its matrix carries on the diagonal beyond A's."""
    seen, mats = [], []

    def cholesky(Ax, want_inverse=False):
        seen.append(float(Ax[0, 0]) - A0[0])
        mats.append(Ax)
        status = torch.zeros(8, dtype=torch.int32)
        status[0] = PIVOT if len(seen) <= failures else 0
        return Ax.clone(), None, status
    monkeypatch.setattr(ops, "cholesky", cholesky)
    return seen, mats


@pytest.mark.parametrize("failures", (0, 1, 3, 4), ids=("clean", "fails_at_0", "through_second_rung", "never"))
def test_psd_safe_cholesky_follows_the_ladder(monkeypatch, failures):
    A = torch.diag(torch.tensor(A0, dtype=torch.float64))
    seen, mats = _stub_cholesky(monkeypatch, A, failures)
    out = []
    check_protocol(lambda: out.extend(ops.psd_safe_cholesky(A)), lambda: [round(j, 12) for j in seen], failures, "matrix",
                   False, None)
    assert mats[0] is A and torch.equal(A, torch.diag(torch.tensor(A0, dtype=torch.float64)))    # the first try: A itself, untouched
    if failures < len(LADDER):
        assert out[1] is mats[-1] and float(out[1][1, 1]) - A0[1] == pytest.approx(LADDER[failures], rel=1e-6, abs=0.0)


def test_psd_safe_cholesky_takes_the_callers_base_jitter(monkeypatch):
    A = torch.diag(torch.tensor(A0, dtype=torch.float64))
    seen, _ = _stub_cholesky(monkeypatch, A, 2)
    with pytest.warns(ops.NumericalWarning, match="%g" % 1e-4):
        ops.psd_safe_cholesky(A, jitter=1e-5)
    assert seen == pytest.approx([0.0, 1e-5, 1e-4], rel=1e-6, abs=0.0)
