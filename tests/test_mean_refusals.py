"""CPU: what the mean functions refuse.  The C entries tgp_mean_forward_f64 / tgp_mean_backward_f64 with their codes (nothing is
launched: every row ends in a refusal, the pointers only have to be non-NULL, as in tests/test_api_refusals.py), and the
NotImplementedErrors of the models and the engines, each naming the mean."""
import ctypes as C

import pytest
import torch

from tgp.pytorch_amd import lib as L

PTR = C.c_void_p(8)             # non-NULL, never dereferenced
UNSUP, WSP = L.E_UNSUPPORTED, L.E_WORKSPACE
BIG = 1 << 30

FWD = [("X", PTR), ("N", 64), ("D", 4), ("a", PTR), ("b", None), ("alpha", 1.0), ("in", None), ("out", PTR), ("ld", 2), ("col", 1),
       ("one_col", 0), ("stream", None)]
BWD = [("X", PTR), ("N", 64), ("D", 4), ("a", PTR), ("g", PTR), ("ldg", 2), ("colg", 1), ("g_a", PTR), ("g_b", PTR), ("g_X", PTR),
       ("workspace", PTR), ("workspace_bytes", BIG), ("stream", None)]
ROWS = [
    ("tgp_mean_forward_f64", dict(X=None), -1),
    ("tgp_mean_forward_f64", dict(N=0), -2),
    ("tgp_mean_forward_f64", dict(D=0), UNSUP),
    ("tgp_mean_forward_f64", dict(D=17), UNSUP),
    ("tgp_mean_forward_f64", dict(a=None), -4),
    ("tgp_mean_forward_f64", dict(out=None), -8),
    ("tgp_mean_forward_f64", dict(ld=0), -9),
    ("tgp_mean_forward_f64", dict(col=2), -10),
    ("tgp_mean_forward_f64", dict(col=-1), -10),
    ("tgp_mean_forward_f64", dict(one_col=2), -11),
    ("tgp_mean_forward_f64", dict(one_col=1), -11),          # one_col == col
    ("tgp_mean_backward_f64", dict(X=None), -1),
    ("tgp_mean_backward_f64", dict(N=-3), -2),
    ("tgp_mean_backward_f64", dict(D=17), UNSUP),
    ("tgp_mean_backward_f64", dict(a=None), -4),             # g_X wanted: a is needed
    ("tgp_mean_backward_f64", dict(g=None), -5),
    ("tgp_mean_backward_f64", dict(ldg=0), -6),
    ("tgp_mean_backward_f64", dict(colg=2), -7),
    ("tgp_mean_backward_f64", dict(g_a=None), -8),
    ("tgp_mean_backward_f64", dict(workspace=None), -11),
    ("tgp_mean_backward_f64", dict(workspace_bytes=8), WSP),
    ("tgp_mean_backward_f64", dict(N=1025, workspace_bytes=17 * 8), WSP),      # two workgroups: 2 x 17 partial sums
]


@pytest.mark.parametrize("entry,over,code", ROWS, ids=["%s-%s" % (e[9:], "-".join("%s=%s" % kv for kv in o.items())) for e, o, _ in ROWS])
def test_refused(entry, over, code):
    lib = L.load()
    args = [over.get(k, v) for k, v in (FWD if "forward" in entry else BWD)]
    rc = getattr(lib, entry)(*args)
    assert rc == code
    if code in (UNSUP, WSP):
        assert entry.encode() in lib.tgp_last_error()


def test_workspace_bytes():
    lib = L.load()
    f = lib.tgp_mean_backward_workspace_bytes
    assert f(1, 1) == 17 * 8 and f(1024, 16) == 17 * 8 and f(1025, 4) == 2 * 17 * 8 and f(8611, 4) == 9 * 17 * 8
    assert f(0, 4) == 0 and f(10, 0) == 0 and f(10, 17) == 0
    # the grid is a function of N alone: the same for every D
    assert len({f(4133, D) for D in range(1, 17)}) == 1


@pytest.fixture
def f64():
    from tgp.pytorch_amd import config as cg
    old = torch.get_default_dtype()
    cg.set_maximum_precission()
    yield cg
    torch.set_default_dtype(old)


def _common(D=3, N=24, M=5):
    from tgp.pytorch_amd.kernels import instance_kernel
    X = torch.randn(N, D, dtype=torch.float64)
    return X, M, lambda Dy=1: instance_kernel("scale_rbf", ard_num_dim=D, num_multioutput=Dy, kernel_is_shared=False)


@pytest.mark.parametrize("mean", ("linear", "identity"))
def test_models_refuse(f64, mean):
    from tgp.pytorch_amd.flows import SAL
    from tgp.pytorch_amd.likelihoods import GaussianNonLinearMean, MulticlassCategorical, WarpedGaussianLinearMean
    from tgp.pytorch_amd.models import sparse_MF_GP, sparse_MF_SP
    X, M, kern = _common()
    N, D = X.shape
    with pytest.raises(NotImplementedError, match="'%s' mean function.*multi-class" % mean):
        sparse_MF_GP([mean, kern(3)], X, X[:M].clone(), float(N), MulticlassCategorical(3), 3, True, False, False, False, False, 0.0)
    lik = WarpedGaussianLinearMean(out_dim=1, noise_init=0.05, noise_is_shared=False, flow=SAL(1), quad_points=8)
    with pytest.raises(NotImplementedError, match="'%s' mean function.*warped" % mean):
        sparse_MF_GP([mean, kern()], X, X[:M].clone(), float(N), lik, 1, True, False, False, False, False, 0.0)
    ident = SAL(1, input_dependent=True, input_dim=D, num_hidden_layers=1, batch_norm=0, dropout=0.5, hidden_dim=8,
                hidden_activation="tanh", inference="MC_dropout")
    with pytest.raises(NotImplementedError, match="'%s' mean function.*input-dependent" % mean):
        sparse_MF_SP([mean, kern()], X, X[:M].clone(), float(N), GaussianNonLinearMean(1, 0.05, False, quadrature_points=8), 1, True,
                     False, False, False, False, [ident], "single", 0.0)
    # the same three with the zero mean build
    sparse_MF_GP(["zero", kern()], X, X[:M].clone(), float(N), lik, 1, True, False, False, False, False, 0.0)


@pytest.mark.parametrize("mean", ("linear", "identity"))
def test_engines_refuse(f64, mean):
    from tgp.pytorch_amd.engine import ElboEngine, MinibatchEngine
    from conftest import load_golden
    g = load_golden("mean_tiny_sal1_lin")
    spec = (mean, g["mean_a"], g["mean_b"] if mean == "linear" else None)
    args = (g["X"], g["Y"], g["params"], float(g["N_total"]))
    with pytest.raises(NotImplementedError, match="'%s' mean function.*single-rank" % mean):
        ElboEngine(*args, flow_blocks=g["program"], S=8, world_size=2, mean=spec)
    with pytest.raises(NotImplementedError, match="'%s' mean function.*minibatch" % mean):
        MinibatchEngine(*args, 16, flow_blocks=g["program"], S=8, mean=spec)
    with pytest.raises(NotImplementedError, match="'%s' mean function.*warped" % mean):
        ElboEngine(*args, flow_blocks=g["program"], S=8, likelihood="warped", mean=spec)
    with pytest.raises(ValueError, match="mean must be"):
        ElboEngine(*args, flow_blocks=g["program"], S=8, mean=("quadratic", None, None))


def test_mean_needs_the_gpu(f64):
    from tgp.pytorch_amd.means import Linear
    with pytest.raises(L.TgpError, match="GPU only"):
        Linear(3, 1)(torch.zeros(1, 4, 3, dtype=torch.float64))
    with pytest.raises(NotImplementedError, match="one output"):
        Linear(3, 2)(torch.zeros(2, 4, 3, dtype=torch.float64))
