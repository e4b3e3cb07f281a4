"""GPU (-m gpu): every public Ell*Function name against the ops.ell_* launch it binds -- value, every input gradient under an
upstream gradient of 2.5, None for the inputs that are absent, the noise gradient in the noise's own shape -- bit for bit.  The
seven names share ONE autograd Function (ops.EllFunction) and one backward; an arity or order slip in it would otherwise show
only as a wrong number far downstream, in a model's ELBO.  N = 7 rows (no multiple of a wave or of 4), S = 8 nodes."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F64 = torch.float64
N, S, UP = 7, 8, 2.5
SAL, PER_ROW = 1, 4
# (theta, rowp) present: no flow parameters at all, one shared SAL block, one per-row SAL block, a shared and a per-row one
CASES = {"none": ([], 0, 0), "theta": ([(SAL, 0, 0, 0)], 2, 0), "rowp": ([(SAL, 0, 0, PER_ROW)], 0, 2),
         "theta_rowp": ([(SAL, 0, 0, 0), (SAL, 0, 0, PER_ROW)], 2, 2)}


@pytest.fixture(scope="module")
def data():
    """One set of inputs for every test, made once and left unchanged: (1, N) and (2, N) moments, targets of each kind."""
    g = torch.Generator().manual_seed(11)
    d = {"mu": 0.5 * torch.randn(2, N, generator=g, dtype=F64), "v": 0.05 + 0.3 * torch.rand(2, N, generator=g, dtype=F64),
         "real": torch.randn(N, generator=g, dtype=F64), "label": (torch.rand(N, generator=g) < 0.5).to(F64),
         "count": torch.poisson(2.0 * torch.rand(N, generator=g, dtype=F64)), "lvn": torch.full((1, 1), -1.2, dtype=F64),
         "theta": torch.tensor([0.2, 0.9], dtype=F64),
         "rowp": torch.stack([0.1 * torch.randn(N, generator=g, dtype=F64), 0.8 + 0.05 * torch.randn(N, generator=g, dtype=F64)], 1)}
    return {k: t.to(DEV).contiguous() for k, t in d.items()}


def _flow(case):
    from tgp.pytorch_amd import ops
    program, P, RP = CASES[case]
    return ops.FlowSpec(program, P, RP, DEV), P > 0, RP > 0


def _leaf(t):
    return t.clone().requires_grad_(True)


def _check(out, ref, ins):
    """`out` of an Ell*Function.apply against the launch's dict `ref`; `ins` = EllFunction's six tensor inputs (None: absent),
    each present one a leaf that requires a gradient."""
    from tgp.pytorch_amd import ops
    assert out.shape == (1,) and torch.equal(out.detach(), ref["ell"].reshape(1))
    up = torch.tensor([UP], dtype=F64, device=DEV)
    slots = ops.EllFunction.backward(out.grad_fn, up)       # one slot per forward argument, the launch description last
    assert len(slots) == 7 and slots[0] is None and slots[6] is None
    for slot, t in zip(slots[1:6], ins[1:]):
        assert (slot is None) == (t is None)
    out.backward(up)
    for key, t in zip(("g_mu", "g_v", "g_lvn", "g_theta", "g_rowp"), ins[1:]):
        if t is not None:
            assert t.grad.shape == t.shape, key
            assert torch.equal(t.grad, (UP * ref[key]).reshape(t.shape)), key
    assert ins[0].grad is None


def test_gauss(data):
    from tgp.pytorch_amd import ops
    Y, mu, v, lvn = data["real"], _leaf(data["mu"][0]), _leaf(data["v"][0]), _leaf(data["lvn"])
    ell, g_lvn, g_mu, g_v = ops.ell_gauss(Y, data["mu"][0], data["v"][0], data["lvn"])
    out = ops.EllGaussFunction.apply(Y, mu, v, lvn)
    _check(out, {"ell": ell, "g_lvn": g_lvn, "g_mu": g_mu, "g_v": g_v}, (Y, mu, v, lvn, None, None))
    assert lvn.grad.shape == (1, 1)


@pytest.mark.parametrize("case", ["none", "theta"])
def test_warp(data, case):
    from tgp.pytorch_amd import ops
    flow, has_theta, _ = _flow(case)
    Y, mu, v, lvn = data["real"], _leaf(data["mu"][0]), _leaf(data["v"][0]), _leaf(data["lvn"])
    theta = _leaf(data["theta"]) if has_theta else None
    ref = ops.ell_warp(Y, data["mu"][0], data["v"][0], data["lvn"], flow, data["theta"] if has_theta else None)
    out = ops.EllWarpFunction.apply(Y, mu, v, lvn, theta, flow)
    _check(out, ref, (Y, mu, v, lvn, theta, None))
    assert lvn.grad.shape == (1, 1)


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("name", ["flow", "bernoulli", "poisson", "student", "hetero"])
def test_quadrature(data, name, case):
    from tgp.pytorch_amd import ops
    flow, has_theta, has_rowp = _flow(case)
    rows = slice(0, 2) if name == "hetero" else 0             # the heteroscedastic moments are the (2, N) pairs
    mu0, v0 = data["mu"][rows], data["v"][rows]
    th0, rp0 = data["theta"] if has_theta else None, data["rowp"] if has_rowp else None
    mu, v, lvn = _leaf(mu0), _leaf(v0), _leaf(data["lvn"])
    theta, rowp = _leaf(th0) if has_theta else None, _leaf(rp0) if has_rowp else None
    df = torch.tensor([4.0], dtype=F64, device=DEV)
    if name == "flow":
        Y = data["real"]
        ref = ops.ell_flow(Y, mu0, v0, data["lvn"], flow, th0, S, rp0)
        out = ops.EllFlowFunction.apply(Y, mu, v, lvn, theta, rowp, flow, S)
    elif name == "bernoulli":
        Y, lvn = data["label"], None
        ref = ops.ell_bernoulli(Y, mu0, v0, flow, th0, S, rp0)
        out = ops.EllBernoulliFunction.apply(Y, mu, v, theta, rowp, flow, S)
    elif name == "poisson":
        Y, lvn = data["count"], None
        ref = ops.ell_poisson(Y, mu0, v0, flow, th0, S, rp0)
        out = ops.EllPoissonFunction.apply(Y, mu, v, theta, rowp, flow, S)
    elif name == "student":
        Y = data["real"]
        ref = ops.ell_student(Y, mu0, v0, data["lvn"], df, flow, th0, S, rp0)
        out = ops.EllStudentFunction.apply(Y, mu, v, lvn, df, theta, rowp, flow, S)
    else:
        Y = data["real"]
        ref = ops.ell_hetero(Y, mu0, v0, data["lvn"], flow, th0, S, rp0, scale=1.75)
        assert ref["g_mu"].shape == (N,) and ref["g_mu_h"].shape == (N,)      # the dict's own entries: row 0 and row 1
        ref = dict(ref, g_mu=torch.stack((ref["g_mu"], ref["g_mu_h"])), g_v=torch.stack((ref["g_v"], ref["g_v_h"])))
        out = ops.EllHeteroFunction.apply(Y, mu, v, lvn, theta, rowp, flow, S, 1.75)
    assert "g_lvn" in ref or lvn is None
    _check(out, ref, (Y, mu, v, lvn, theta, rowp))
    if lvn is not None:
        assert lvn.grad.shape == (1, 1)
