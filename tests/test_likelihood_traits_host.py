"""CPU: the likelihoods describe themselves.  Every class carries the whole trait table of likelihoods.Likelihood, the traits are
no parameters or buffers (the names of every model's state are the ones recorded before the table existed), engine_name keys
engine.engine_refusal as the trainer's class ladder did, models.py knows no likelihood class by name, and the one autograd
Function behind the Ell*Function names hands each gradient to its own input."""
import pytest
import torch

F64 = torch.float64
CLASSES = ("GaussianLinearMean", "GaussianNonLinearMean", "WarpedGaussianLinearMean", "Bernoulli", "Poisson", "StudentT",
           "HeteroscedasticGaussian", "MulticlassCategorical")
FLAGS = ("has_noise", "has_flow", "flow_on_targets", "compiles_flows", "one_launch_logp")
REFUSALS = ("outputs_refusal", "extra_flow_refusal", "refuses_input_dependent", "refuses_mean", "refuses_full_cov",
            "refuses_full_cov_predictive", "refuses_paths", "refuses_optimal_qu", "refuses_optimal_qu_id", "refuses_cdf",
            "refuses_crps")
# what the trainer's class -> name ladder gave engine.engine_refusal, and what it answered
ENGINE = {"GaussianLinearMean": (None, None), "GaussianNonLinearMean": (None, None), "WarpedGaussianLinearMean": ("warped", None),
          "Bernoulli": ("bernoulli", "the step engines have no Bernoulli likelihood: it trains on the eager path (ops.ElboFunction)"),
          "MulticlassCategorical": ("multiclass", "the step engines have no multi-class likelihood: its C latent GPs train on the "
                                                  "eager path's composed step"),
          "Poisson": ("poisson", "the step engines have no Poisson likelihood: it trains on the eager path (ops.ElboFunction)"),
          "StudentT": ("studentt", "the step engines have no Student-t likelihood: it trains on the eager path (ops.ElboFunction)"),
          "HeteroscedasticGaussian": ("hetero", "the step engines have no heteroscedastic likelihood: its two latent GPs train on "
                                                "the eager path's composed step, on one rank")}
GP = ["Z", "covariance_function.base_kernel.raw_lengthscale", "covariance_function.raw_outputscale", "q_U.chol_variational_covar",
      "q_U.variational_mean"]
NOISE = ["likelihood.log_var_noise"]
WARP = ["likelihood.flow.0.flow_arr.%d.%s" % (k, ab) for k in range(4) for ab in "ab"]
SAL1 = ["G_matrix.0.flow_arr.%d.%s" % (k, ab) for k in range(2) for ab in "ab"]
# sorted names of a model of each likelihood, recorded before the trait table: (state_dict, parameters, buffers)
NAMES = {"GaussianLinearMean": (GP + NOISE, GP + NOISE, []),
         "GaussianNonLinearMean": (SAL1 + GP + NOISE, SAL1 + GP + NOISE, []),
         "WarpedGaussianLinearMean": (GP + WARP + NOISE, GP + WARP + NOISE, []),
         "Bernoulli": (GP, GP, ["_bern_lvn"]),
         "Poisson": (GP, GP, ["_bern_lvn"]),
         "StudentT": (GP + ["likelihood.df"] + NOISE, GP + NOISE, ["likelihood.df"]),
         "HeteroscedasticGaussian": (GP + NOISE, GP + NOISE, []),
         "MulticlassCategorical": (GP, GP, [])}
# the likelihood's own (state_dict, buffers)
OWN = {"GaussianLinearMean": (["log_var_noise"], []), "GaussianNonLinearMean": (["log_var_noise"], []),
       "WarpedGaussianLinearMean": ([w[len("likelihood."):] for w in WARP] + ["log_var_noise"], []), "Bernoulli": ([], []),
       "Poisson": ([], []), "StudentT": (["df", "log_var_noise"], ["df"]), "HeteroscedasticGaussian": (["log_var_noise"], []),
       "MulticlassCategorical": ([], [])}


@pytest.fixture(autouse=True)
def _f64():
    from tgp.pytorch_amd import config as cg
    old = torch.get_default_dtype()
    cg.set_maximum_precission()
    yield
    torch.set_default_dtype(old)


def _likelihood(name):
    """(instance, num_outputs) with the constructor arguments of the host tests."""
    from tgp.pytorch_amd import likelihoods as LK
    from tgp.pytorch_amd.flows import SAL
    return {"GaussianLinearMean": lambda: (LK.GaussianLinearMean(1, 0.05, False), 1),
            "GaussianNonLinearMean": lambda: (LK.GaussianNonLinearMean(1, 0.05, False, 20), 1),
            "WarpedGaussianLinearMean": lambda: (LK.WarpedGaussianLinearMean(1, 0.05, False, SAL(2), 20), 1),
            "Bernoulli": lambda: (LK.Bernoulli(), 1), "Poisson": lambda: (LK.Poisson(), 1),
            "StudentT": lambda: (LK.StudentT(1, 0.05, False, 20, df=4.0), 1),
            "HeteroscedasticGaussian": lambda: (LK.HeteroscedasticGaussian(0.05, 20), 2),
            "MulticlassCategorical": lambda: (LK.MulticlassCategorical(3), 3)}[name]()


def _model(name, N=30, M=5, D=3):
    from tgp.pytorch_amd.flows import SAL
    from tgp.pytorch_amd.kernels import instance_kernel
    from tgp.pytorch_amd.models import sparse_MF_GP, sparse_MF_SP
    lik, dy = _likelihood(name)
    X = torch.randn(N, D, dtype=F64)
    K = instance_kernel("scale_rbf", ard_num_dim=D, num_multioutput=dy, kernel_is_shared=False,
                        init_params={"length_scale": 2.0, "kernel_scale": 2.0, "noisy_variance": 1e-6})
    if name != "GaussianNonLinearMean":
        return sparse_MF_GP(["zero", K], X, X[:M].clone(), N, lik, dy, True, False, False, False, False, 0.0)
    return sparse_MF_SP(["zero", K], X, X[:M].clone(), N, lik, dy, True, False, False, False, False, [SAL(1)], "single", 0.0)


@pytest.mark.parametrize("name", CLASSES)
def test_every_trait_is_defined(name):
    from tgp.pytorch_amd import lib as L
    from tgp.pytorch_amd import likelihoods as LK
    cls = getattr(LK, name)
    assert issubclass(cls, LK.Likelihood) and issubclass(cls, torch.nn.Module)
    lik, dy = _likelihood(name)
    for flag in FLAGS:
        assert isinstance(getattr(cls, flag), bool), flag
    for r in REFUSALS:
        text = getattr(cls, r)
        assert text is None or (isinstance(text, str) and text.strip()), r
    assert cls.kind in ("regression", "classifier", "count")
    assert cls.lik_id in (None, L.LIK_WARPED, L.LIK_BERNOULLI, L.LIK_POISSON, L.LIK_STUDENT)
    assert cls.engine_name is None or isinstance(cls.engine_name, str)
    assert lik.num_latent == dy and lik.composed == (dy > 1)
    assert 1 <= lik.flow_outputs <= dy and 1 <= lik.observed_outputs <= dy
    assert set(lik.lik_kwargs()) == {"lik", "df"} and lik.lik_kwargs()["lik"] == cls.lik_id
    assert (lik.noise() is None) == (not cls.has_noise)
    assert lik.check_targets(torch.zeros(3, 1, dtype=F64)) is None
    # where a flag is off, the text that says so is there
    if dy > 1:
        assert cls.outputs_refusal and cls.refuses_full_cov and cls.refuses_paths and cls.refuses_mean
    assert (cls.refuses_optimal_qu is None) == (name in ("GaussianLinearMean", "WarpedGaussianLinearMean"))
    assert (cls.refuses_cdf is not None) == (name in ("Poisson", "StudentT", "HeteroscedasticGaussian"))
    assert cls.refuses_cdf is None or "%s" in cls.refuses_cdf
    assert cls.refuses_crps is None or "%s" in cls.refuses_crps


def test_what_each_likelihood_says_of_itself():
    from tgp.pytorch_amd import lib as L
    from tgp.pytorch_amd import likelihoods as LK
    assert [getattr(LK, n).lik_id for n in CLASSES] == [None, None, L.LIK_WARPED, L.LIK_BERNOULLI, L.LIK_POISSON, L.LIK_STUDENT,
                                                        None, None]
    assert [getattr(LK, n).kind for n in CLASSES] == ["regression"] * 3 + ["classifier", "count", "regression", "regression",
                                                                             "classifier"]
    assert [n for n in CLASSES if not getattr(LK, n).has_noise] == ["Bernoulli", "Poisson", "MulticlassCategorical"]
    assert [n for n in CLASSES if not getattr(LK, n).has_flow] == ["GaussianLinearMean"]
    assert [n for n in CLASSES if getattr(LK, n).flow_on_targets] == ["WarpedGaussianLinearMean"]
    assert [n for n in CLASSES if getattr(LK, n).refuses_input_dependent] == ["Poisson", "StudentT", "HeteroscedasticGaussian"]
    assert LK.Poisson.refuses_input_dependent == ("the Poisson likelihood is built for SVGP and TGP: input-dependent flows "
                                                  "(ID_TGP) are not")
    assert LK.StudentT.refuses_optimal_qu == "the Student-t likelihood is not Gaussian in f: q(u) has no closed-form optimum"
    assert float(LK.StudentT(1, 0.05, False, 20, df=6.0).lik_kwargs()["df"]) == 6.0
    with pytest.raises(ValueError, match="counts"):
        LK.Poisson.check_targets(torch.tensor([[0.5]], dtype=F64))
    hetero = LK.HeteroscedasticGaussian(0.05, 20)
    assert (hetero.num_latent, hetero.flow_outputs, hetero.observed_outputs) == (2, 1, 1)
    multi = LK.MulticlassCategorical(4)
    assert (multi.num_latent, multi.flow_outputs, multi.observed_outputs) == (4, 4, 4)


@pytest.mark.parametrize("name", CLASSES)
def test_engine_name_keys_engine_refusal(name):
    from tgp.pytorch_amd import likelihoods as LK
    from tgp.pytorch_amd.engine import engine_refusal
    key, answer = ENGINE[name]
    assert getattr(LK, name).engine_name == key
    assert engine_refusal(likelihood=getattr(LK, name).engine_name) == answer


@pytest.mark.parametrize("name", CLASSES)
def test_state_names_are_the_recorded_ones(name):
    model = _model(name)
    state, params, buffers = NAMES[name]
    assert sorted(model.state_dict()) == sorted(state)
    assert sorted(n for n, _ in model.named_parameters()) == sorted(params)
    assert sorted(n for n, _ in model.named_buffers()) == sorted(buffers)
    own_state, own_buffers = OWN[name]
    assert sorted(model.likelihood.state_dict()) == sorted(own_state)
    assert sorted(n for n, _ in model.likelihood.named_buffers()) == sorted(own_buffers)
    assert model._lik_id == model.likelihood.lik_id and model._is_composed == model.likelihood.composed


def test_models_names_no_likelihood_class():
    from tgp.pytorch_amd import models
    for name in CLASSES + ("Likelihood",):
        assert not hasattr(models, name), name
    for gone in ("_is_bernoulli", "_is_poisson", "_is_student", "_is_warped", "_is_multiclass", "_is_hetero"):
        assert not hasattr(models.sparse_MF_SP, gone), gone


@pytest.mark.parametrize("present", [(True, True, True), (False, False, False), (True, False, True), (False, True, False)])
def test_one_backward_hands_each_gradient_to_its_input(present):
    """ops.EllFunction on a stand-in launch (no device): every present input gets upstream x its own entry, absent ones None."""
    from tgp.pytorch_amd import ops
    N, up = 7, torch.tensor([2.5], dtype=F64)
    g = torch.Generator().manual_seed(0)
    ref = {"ell": torch.tensor(1.5, dtype=F64), "g_lvn": torch.tensor(3.0, dtype=F64), "g_mu": torch.randn(N, generator=g, dtype=F64),
           "g_v": torch.randn(N, generator=g, dtype=F64), "g_theta": torch.randn(2, generator=g, dtype=F64),
           "g_rowp": torch.randn(N, 2, generator=g, dtype=F64)}

    def launch(Y, mu, v, lvn, theta, rowp):
        assert not any(t.requires_grad for t in (Y, mu, v, lvn, theta, rowp) if t is not None)
        return dict(ref, g_theta=ref["g_theta"] if theta is not None else ref["g_theta"][:0],
                    g_rowp=ref["g_rowp"] if rowp is not None else None)

    Y = torch.zeros(N, dtype=F64)
    mu, v = (torch.zeros(N, dtype=F64, requires_grad=True) for _ in range(2))
    lvn, theta, rowp = (torch.zeros(*shape, dtype=F64, requires_grad=True) if has else None
                        for shape, has in zip(((1, 1), (2,), (N, 2)), present))
    out = ops.EllFunction.apply(Y, mu, v, lvn, theta, rowp, launch)
    assert out.shape == (1,) and float(out.detach()) == 1.5
    slots = ops.EllFunction.backward(out.grad_fn, up)
    assert [s is None for s in slots] == [True, False, False] + [not has for has in present] + [True]
    out.backward(up)
    for key, t in zip(("g_mu", "g_v", "g_lvn", "g_theta", "g_rowp"), (mu, v, lvn, theta, rowp)):
        if t is not None:
            assert t.grad.shape == t.shape and torch.equal(t.grad, (2.5 * ref[key]).reshape(t.shape)), key
