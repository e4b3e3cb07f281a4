"""No GPU: the host side of the Matern-5/2 and rational-quadratic kernels -- the ids, the range of alpha, the packing behind the
raw output scale, the RQ spectral sampler, the command line, the engines' refusal and the CPU twin of the greedy test's margin."""
import ctypes as C
import os
import re

import pytest
import torch

import kernel_family_model as kfm
from tgp.pytorch_amd import lib as L
from tgp.pytorch_amd import ops
from tgp.pytorch_amd import pathwise as pw

F64 = torch.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(autouse=True)
def f64():
    from tgp.pytorch_amd import config as cg
    old, dev = torch.get_default_dtype(), cg.device
    cg.set_maximum_precission()
    cg.device = "cpu"
    yield
    cg.device = dev
    torch.set_default_dtype(old)


def test_header_ids_are_the_packages():
    text = open(os.path.join(ROOT, "include", "tgp_hip.h")).read()
    ids = {m.group(1).lower(): int(m.group(2)) for m in re.finditer(r"#define TGP_KERNEL_(SCALE_\w+) (\d+)", text)}
    assert ids == L.KERNELS == {"scale_rbf": 0, "scale_matern32": 1, "scale_rq": 3, "scale_matern52": 5}
    lim = {m.group(1): float(m.group(2)) for m in re.finditer(r"#define TGP_RQ_(M\w+)_ALPHA (\S+)", text)}
    assert (lim["MIN"], lim["MAX"]) == (L.RQ_MIN_ALPHA, L.RQ_MAX_ALPHA) == (1e-2, 1e4)


def test_an_unknown_kernel_id_is_refused_before_a_pointer_is_read():
    """Ids 2 and 4 (the two the header leaves unassigned below its largest), 6 and -1 with pointers that cannot be read: TGP_E_UNSUPPORTED and a text that
    names the entry and the four kernels."""
    lib = L.load()
    fake = C.c_void_p(64)
    md = L.TgpModel()
    md.Z = md.raw_ls = md.raw_os = md.m = md.Lam = fake
    md.N, md.D, md.M = 10, 4, 5
    for kern in (2, 4, 6, -1):
        md.kernel = kern
        calls = {
            "tgp_greedy_inducing_f64": lambda: lib.tgp_greedy_inducing_f64(fake, 10, 4, fake, fake, kern, 2, 1e-8, fake, fake, fake,
                                                                           fake, fake, 1 << 40, None),
            "tgp_pathwise_coeff_f64": lambda: lib.tgp_pathwise_coeff_f64(md, fake, 8, fake, fake, 2, fake, fake, fake, 1 << 40, None),
            "tgp_pathwise_eval_f64": lambda: lib.tgp_pathwise_eval_f64(kern, fake, 10, 4, fake, 5, fake, fake, fake, 8, fake, 2, fake,
                                                                       None),
        }
        for entry, call in calls.items():
            assert call() == L.E_UNSUPPORTED, (entry, kern)
            text = lib.tgp_last_error()
            assert entry.encode() in text and b"_MATERN52" in text and b"_RQ" in text, text


def test_alpha_outside_its_range_is_a_value_error():
    from tgp.pytorch_amd.kernels import RQKernel, instance_kernel
    ro = torch.zeros(1, dtype=F64)
    for bad in (0.0, 9.9e-3, 1.0001e4, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="alpha"):
            ops.rq_scale(ro, bad)
        with pytest.raises(ValueError, match="alpha"):
            RQKernel(alpha=bad)
        with pytest.raises(ValueError, match="alpha"):
            instance_kernel("scale_rq", 3, 1, False, init_params={"alpha": bad})
        with pytest.raises(ValueError, match="alpha"):
            pw.spectral_frequencies("scale_rq", 8, 3, alpha=bad)
    for good in (1e-2, 0.5, 2.0, 1e4):
        assert ops.rq_scale(ro, good).tolist() == [0.0, good]
    with pytest.raises(L.TgpError, match="alpha"):
        ops.rq_scale(ro, None)
    with pytest.raises(L.TgpError, match="alpha"):
        pw.spectral_frequencies("scale_rq", 8, 3)


def test_kernel_classes_names_and_packing():
    from tgp.pytorch_amd.kernels import MaternKernel, RQKernel, ScaleKernel, instance_kernel
    assert MaternKernel(nu=2.5, ard_num_dims=3).nu == 2.5
    with pytest.raises(NotImplementedError, match="nu"):
        MaternKernel(nu=0.5)
    names = {}
    for name in L.KERNELS:
        K = instance_kernel(name, 3, 1, False, init_params={"length_scale": 2.0, "kernel_scale": 3.0, "alpha": 0.75})
        assert isinstance(K, ScaleKernel) and K.hip_kernel == name
        names[name] = type(K.base_kernel).__name__
        rl, ro = K._params()
        assert torch.allclose(torch.nn.functional.softplus(rl), torch.full((3,), 2.0, dtype=F64))
        assert torch.allclose(torch.nn.functional.softplus(ro[:1]), torch.full((1,), 3.0, dtype=F64))
        assert ro.tolist()[1:] == ([0.75] if name == "scale_rq" else [])
        assert sorted(n for n, _ in K.named_parameters()) == ["base_kernel.raw_lengthscale", "raw_outputscale"]
    assert names == {"scale_rbf": "RBFKernel", "scale_matern32": "MaternKernel", "scale_matern52": "MaternKernel", "scale_rq": "RQKernel"}
    K = instance_kernel("scale_rq", 3, 1, False)
    assert isinstance(K.base_kernel, RQKernel) and K.base_kernel.alpha.tolist() == [2.0] and "base_kernel.alpha" in K.state_dict()
    # the packed output scale carries the gradient to raw_outputscale and nothing to alpha
    packed = K.packed_outputscale()
    assert packed.shape == (2,) and packed.requires_grad
    (packed * torch.tensor([3.0, 5.0], dtype=F64)).sum().backward()
    assert K.raw_outputscale.grad.tolist() == [3.0] and not K.base_kernel.alpha.requires_grad
    with pytest.raises(NotImplementedError, match="scale_rq"):
        instance_kernel("scale_periodic", 3, 1, False)


def test_rq_calls_without_alpha_behind_the_output_scale_are_refused():
    """The library reads raw_os[1] for 'scale_rq': every host entry checks the length before it asks the library."""
    X, Z = torch.zeros(4, 2, dtype=F64), torch.zeros(3, 2, dtype=F64)
    rl, one, two = torch.zeros(2, dtype=F64), torch.zeros(1, dtype=F64), torch.tensor([0.0, 2.0], dtype=F64)
    m, Lam, w = torch.zeros(3, dtype=F64), torch.eye(3, dtype=F64), torch.ones(4, dtype=F64)
    calls = [lambda ro, k: ops.kernel_matrix(X, Z, rl, ro, kernel=k), lambda ro, k: ops.kxxk(X, Z, rl, ro, kernel=k),
             lambda ro, k: ops.kxwxk(X, Z, rl, ro, w, kernel=k), lambda ro, k: ops.greedy_inducing(X, 2, rl, ro, kernel=k),
             lambda ro, k: ops.qf_moments(X, Z, rl, ro, m, Lam, kernel=k), lambda ro, k: ops.unwhiten(Z, rl, ro, m, Lam, kernel=k),
             lambda ro, k: ops.elbo_step(X, w, Z, rl, ro, m, Lam, one, 4.0, kernel=k)]
    for call in calls:
        with pytest.raises(ValueError, match="raw_os"):
            call(one, "scale_rq")
        for k in ("scale_rbf", "scale_matern32", "scale_matern52"):
            with pytest.raises(ValueError, match="raw_os"):
                call(two, k)


@pytest.mark.parametrize("alpha", (0.5, 2.0))
def test_rq_spectral_frequencies(alpha):
    """Seeded and reproducible; Phi Phi^T -> K: the error at R2 = 2048 is below the one at 256 and below 0.12 s2 (a Monte-Carlo
    mean of 2048 terms bounded by s2: 5 standard errors of 1 / sqrt(2048) = 0.022)."""
    a = pw.spectral_frequencies("scale_rq", 7, 3, torch.Generator().manual_seed(5), alpha=alpha)
    assert a.shape == (7, 3) and a.dtype == F64
    assert torch.equal(a, pw.spectral_frequencies("scale_rq", 7, 3, torch.Generator().manual_seed(5), alpha=alpha))
    assert not torch.equal(a, pw.spectral_frequencies("scale_rq", 7, 3, torch.Generator().manual_seed(6), alpha=alpha))
    err = {}
    for R2 in (256, 2048):
        om = pw.spectral_frequencies("scale_rq", R2, 4, torch.Generator().manual_seed(0), alpha=alpha)
        err[R2] = kfm.spectral_error("scale_rq@%g" % alpha, R2, om)
        print("alpha", alpha, "R2", R2, "spectral error / s2 = %.3e" % err[R2])
    assert err[2048] < err[256] and err[2048] < 0.12


def test_matern52_has_no_spectral_sampler_yet():
    from tgp.pytorch_amd.kernels import instance_kernel
    from tgp.pytorch_amd.likelihoods import GaussianLinearMean
    from tgp.pytorch_amd.models import sparse_MF_GP
    assert set(pw.SPECTRAL_KERNELS) == set(L.KERNELS) - {"scale_matern52"}
    X = torch.randn(12, 3, dtype=F64, generator=torch.Generator().manual_seed(1))
    K = instance_kernel("scale_matern52", ard_num_dim=3, num_multioutput=1, kernel_is_shared=False)
    model = sparse_MF_GP(["zero", K], X, X[:5].clone(), 12.0, GaussianLinearMean(1, 0.05, False), 1, True, False, False, False,
                         False, 0.0)
    with pytest.raises(L.TgpError, match="spectral"):
        model.posterior_paths(2, num_frequencies=4, generator=torch.Generator().manual_seed(9))


class _ModelReached(Exception):
    pass


@pytest.mark.parametrize("argv,name,alpha", [([], "scale_rbf", None), (["--kernel", "rbf"], "scale_rbf", None),
                                             (["--kernel", "matern32"], "scale_matern32", None),
                                             (["--kernel", "matern52"], "scale_matern52", None),
                                             (["--kernel", "rq"], "scale_rq", 2.0),
                                             (["--kernel", "rq", "--rq_alpha", "0.5"], "scale_rq", 0.5),
                                             (["--rq_alpha", "0.5"], "scale_rbf", None)])
def test_main_builds_the_chosen_kernel(monkeypatch, argv, name, alpha):
    """main([...]) up to the model's construction with the data set, the initialiser and the model stubbed: --kernel and --rq_alpha
    reach instance_kernel, and a command line without them asks for 'scale_rbf' with the initial values it always had."""
    from tgp.pytorch_amd import config as cg
    from tgp.pytorch_amd import kernels
    from tgp.pytorch_amd import main as M
    monkeypatch.setattr(cg, "device", "cpu")
    X = torch.randn(20, 3, dtype=F64, generator=torch.Generator().manual_seed(4))
    dc = {"X_tr": X, "Y_tr": X[:, :1].clone(), "Dx": 3, "Dy": 1, "N_tr": 20, "Y_std": 1.0}
    monkeypatch.setattr(M, "return_dataset", lambda *a, **k: ([None, None, None], dc))
    asked = []

    def instance_kernel(kname, **kw):
        asked.append((kname, kw))
        return kernels.instance_kernel(kname, **kw)

    def model(**kw):
        raise _ModelReached(kw)

    monkeypatch.setattr(M, "instance_kernel", instance_kernel)
    monkeypatch.setattr(M, "KMEANS", lambda Xa, num_Z, **kw: Xa[:num_Z] + 0.5)
    monkeypatch.setattr(M, "sparse_MF_GP", model)
    with pytest.raises(_ModelReached) as e:
        M.main(["--model", "SVGP", "--dataset", "synthetic_power", "--train_test_seed_split", "1", "--num_inducing", "5"] + argv)
    (kname, kw), = asked
    assert kname == name and (kw["ard_num_dim"], kw["num_multioutput"], kw["kernel_is_shared"]) == (3, 1, False)
    want = {"length_scale": 2.0, "kernel_scale": 2.0, "noisy_variance": 1e-6}
    if alpha is not None:
        want["alpha"] = alpha
    assert kw["init_params"] == want
    K = e.value.args[0]["model_specs"][1]
    assert K.hip_kernel == name and (alpha is None or K.base_kernel.alpha.tolist() == [alpha])


def test_main_refuses_an_alpha_outside_the_range(capsys):
    from tgp.pytorch_amd import main as M
    base = ["--model", "SVGP", "--dataset", "synthetic_power", "--train_test_seed_split", "1", "--num_inducing", "5"]
    for bad in ("0", "1e5"):
        with pytest.raises(SystemExit):
            M.main(base + ["--kernel", "rq", "--rq_alpha", bad])
        assert "--rq_alpha" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        M.main(base + ["--kernel", "matern12"])


def test_engines_refuse_the_rq_kernel_with_a_reason():
    from tgp.pytorch_amd import engine
    why = engine.engine_refusal(kernel="scale_rq")
    assert "rational-quadratic" in why and "one slot behind raw_os" in why and "eager" in why
    for k in (None, "scale_rbf", "scale_matern32", "scale_matern52"):
        assert engine.engine_refusal(kernel=k) is None and engine.engine_refusal(kernel=k, minibatch=True) is None
    assert engine.engine_refusal(kernel="scale_rq", minibatch=True) == why
    # an earlier reason keeps its text
    assert engine.engine_refusal(kernel="scale_rq", is_whiten=False) == engine.engine_refusal(is_whiten=False)
    X, Y = torch.zeros(4, 2, dtype=F64), torch.zeros(4, 1, dtype=F64)
    with pytest.raises(NotImplementedError, match=re.escape(why)):          # (before the library or the device is touched)
        engine.ElboEngine(X, Y, {}, 4.0, device="cpu", kernel="scale_rq")
    with pytest.raises(NotImplementedError, match=re.escape(why)):
        engine.MinibatchEngine(X, Y, {}, 4.0, 2, device="cpu", kernel="scale_rq")


@pytest.mark.parametrize("kind", kfm.K4)
@pytest.mark.parametrize("N,D,M", kfm.GREEDY_CASES)
def test_greedy_cases_have_a_clear_runner_up(N, D, M, kind):
    """The CPU recurrence on the cases of the GPU test: every pick leads the runner-up by more than 1e-6 of its own d, ten orders
    above the recurrence's rounding (greedy_model.GREEDY_CPU: d agrees with the dense route to 1e-15 s2) -- so the GPU test may
    ask for the same indices."""
    r = kfm.greedy(kfm.greedy_case(N, D, M, kind))
    print(kind, (N, D, M), "margin %.3e" % r["margin"], "trace[M]/trace[0] %.3e" % float(r["trace"][-1] / r["trace"][0]))
    assert r["M_eff"] == M and r["margin"] > kfm.GREEDY_MARGIN


@pytest.mark.parametrize("kind", kfm.K4)
def test_restated_gradient_weight_is_autograds(kind):
    """k_g = -2 dk/d(d2) of the table against autograd through k(d2), from d2 = 0 (finite there) to 40.  Autograd forms the
    Matern derivative through r = sqrt(d2) as a difference of terms of size sqrt5 / (2 r), so its own rounding is
    2^-52 sqrt5 / (2 r) per term: the bound is 1e-12 plus eight of those."""
    d2 = torch.cat((torch.zeros(1, dtype=F64), torch.logspace(-12, 1.6, 60, dtype=F64))).requires_grad_(True)
    kfm.from_d2(d2, 1.3, kind).sum().backward()
    kg = kfm.gweight(d2.detach(), 1.3, kind)
    tol = 1e-12 + (8.0 * 2.0 ** -52 * kfm.SQRT5 / (2.0 * d2.detach().clamp_min(1e-30).sqrt()) if kind == "scale_matern52" else 0.0)
    assert bool(torch.isfinite(kg).all()) and bool(((kg + 2.0 * d2.grad).abs() <= 1.3 * tol)[1:].all())
    assert float(kg[0]) == pytest.approx(1.3 * (5.0 / 3.0 if kind == "scale_matern52" else 1.0), rel=1e-12)
