"""Likelihood classes with the reference's constructor signatures and attribute names
(code/dsp/likelihoods/GaussianLinearMean.py, GaussianNonLinearMean.py).  They hold `log_var_noise`
(observation noise, positive transform = exp) and evaluate their moments on the GPU; the expected
log-likelihood used in training lives inside the fused ELBO kernel (ops.ElboFunction).

A likelihood says what it is: `Likelihood` lists the traits the models and the trainer read (they never ask for a class), each
class below sets the ones in which it differs.  A new likelihood is a class here, its traits and its `ops.ell_*`."""
import torch
import torch.nn as nn
import torch.distributions as td

from . import config as cg
from . import ops
from .flow import compile_flow, nets_rowp, stack_theta
from .utils import inverse_positive_transform, positive_transform

# refusal texts several likelihoods share, %s the likelihood's `display` name
NOT_GAUSSIAN_IN_F = "the %s likelihood is not Gaussian in f: q(u) has no closed-form optimum"
NO_INPUT_DEPENDENT = "the %s likelihood is built for SVGP and TGP: input-dependent flows (ID_TGP) are not"


class Likelihood(nn.Module):
    """The base of every likelihood and the table of its traits: plain class attributes and properties, none a parameter or a
    buffer.  A `refuses_*` trait is None where the likelihood covers the thing and the refusal's text where it does not."""

    display = None                  # the name the shared refusal texts and the trainer's fall-back sentences use
    lik_id = None                   # lib.LIK_* of the step and of ops.predict; None: told by the flow's presence, or composed
    engine_name = None              # the `likelihood=` key of engine.engine_refusal
    kind = "regression"             # | "classifier" (class probabilities, no quantiles, no CRPS) | "count" (a pmf)
    has_noise = True                # a trained scalar sits behind the ABI's noise pointer and noise() returns it (log_var_noise,
                                    # or one of another name: log_dispersion); False: the pointer gets a zero that no kernel reads
    has_flow = True                 # False: the Gaussian closed form, no flow program at all
    flow_on_targets = False         # the flow is the likelihood's own (`self.flow`) and warps the targets, not f
    compiles_flows = False          # _flow_inputs is the likelihood's own: shared flow parameters only
    one_launch_logp = False         # predict_rows gives the moments AND the exact log density of the targets, one launch
    outputs_refusal = None          # said when num_outputs is not `num_latent`
    extra_flow_refusal = None       # said of a flow on a latent GP past `flow_outputs`
    refuses_input_dependent = None  # input-dependent flows (ID_TGP)
    refuses_mean = None             # a non-zero mean function: what it is not built for
    refuses_full_cov = None         # marginal_variational_qf_parameters(diagonal=False)
    refuses_full_cov_predictive = None      # predictive_distribution(diagonal=False)
    refuses_paths = None            # posterior_paths
    refuses_optimal_qu = None       # not Gaussian in f: no closed-form optimal q(u) (None: Gaussian in f)
    refuses_optimal_qu_id = None    # the same, said instead when the model's flows are input-dependent
    refuses_cdf = None              # exact predictive CDF / quantiles; %s: the method asked for
    refuses_crps = None             # exact CRPS; %s: the class name

    @property
    def num_latent(self):
        """Latent GPs behind one observed output: 1, C (multi-class) or 2 (heteroscedastic)."""
        return 1

    @property
    def composed(self):
        """Several latent GPs: the step is composed per GP from the stand-alone pieces."""
        return self.num_latent > 1

    @property
    def flow_outputs(self):
        """The first so many latent GPs carry a flow."""
        return self.num_latent

    @property
    def observed_outputs(self):
        """Outputs sample_from_output draws, each from all latent rows."""
        return self.num_latent

    def noise(self):
        """What the ABI's noise pointer reads, one element with the graph to the parameter; None without a noise parameter."""
        return self.log_var_noise.reshape(-1)[:1] if self.has_noise else None

    def lik_kwargs(self):
        """The likelihood's keyword arguments of the step (ops.elbo_step) and of ops.predict."""
        return {"lik": self.lik_id, "df": None}

    @staticmethod
    def check_targets(Y):
        """ValueError for targets the likelihood cannot take; the kernels do not look."""

    def _flow_inputs(self, flow, X, dev, with_grad=False):
        """(FlowSpec, theta, rowp) of flow[0] for the quadrature kernels; `with_grad` keeps the graph to the flow's parameters
        (expected_log_prob)."""
        spec, theta_list, nets = compile_flow(flow[0])
        rowp = None
        if nets:
            rowp = nets_rowp(nets, X[0] if X.dim() == 3 else X, with_grad=with_grad)      # the HIP MLP kernel (dropout follows the layers)
        return spec, stack_theta(theta_list, dev, with_grad), rowp

    def predict_rows(self, mu, v, lvn, spec, theta, rowp, Y=None, Y_std=1.0, want_moments=True):
        """(m1, m2, logp) of the rows from ONE predictive launch: mu, v the q(f) moments (num_latent, N) or flat, `lvn` what
        `noise()` gives, detached (a zero where it gives None)."""
        return ops.predict(mu.reshape(-1).contiguous(), v.reshape(-1).contiguous(), lvn, spec, theta,
                           getattr(self, "quad_points", None), rowp, Y=Y, Y_std=Y_std, want_moments=want_moments,
                           **self.lik_kwargs())

    def _moments(self, gauss_mean, gauss_cov, flow, X):
        """m1, m2 of predict_rows on the likelihood's own flow inputs, each of gauss_mean's shape."""
        spec, theta, rowp = self._flow_inputs(flow, X, gauss_mean.device)
        lvn = self.noise()
        lvn = torch.zeros(1, dtype=torch.float64, device=gauss_mean.device) if lvn is None else lvn.detach().contiguous()
        m1, m2, _ = self.predict_rows(gauss_mean, gauss_cov, lvn, spec, theta, rowp)
        return m1.reshape(gauss_mean.shape), m2.reshape(gauss_mean.shape)


class _GaussianBase(Likelihood):
    def __init__(self, out_dim, noise_init, noise_is_shared):
        super().__init__()
        self.out_dim = out_dim
        self.noise_is_shared = noise_is_shared
        n = 1 if noise_is_shared else out_dim
        init = inverse_positive_transform(torch.tensor(noise_init, dtype=cg.dtype))
        self.log_var_noise = nn.Parameter(torch.ones(n, 1, dtype=cg.dtype) * init)

    def _lvn(self):
        return self.log_var_noise.expand(self.out_dim, 1) if self.noise_is_shared else self.log_var_noise

    def sample_from_output(self, f, i, **kwargs):
        var = positive_transform(self._lvn()[i])
        return td.Normal(f, torch.ones_like(f) * torch.sqrt(var)).sample()


class GaussianLinearMean(_GaussianBase):
    """p(y|f) = N(y|f, s2): closed-form ELL (GaussianLinearMean.py:60-87) and moments (:89-118)."""

    has_flow = False

    def expected_log_prob(self, Y, gauss_mean, gauss_cov, **kwargs):
        # differentiable in the moments and the noise like the reference's torch code (gradients from the same launch)
        return ops.EllGaussFunction.apply(Y.reshape(-1), gauss_mean.reshape(-1).contiguous(), gauss_cov.reshape(-1).contiguous(),
                                          self._lvn().reshape(-1)[:1].contiguous())

    def marginal_moments(self, gauss_mean, gauss_cov, diagonal=True, **kwargs):
        assert diagonal, "only diagonal covariances on this path"
        C_Y = positive_transform(self._lvn()).detach().expand(-1, gauss_mean.size(1)) + gauss_cov
        return gauss_mean.clone(), C_Y


class GaussianNonLinearMean(_GaussianBase):
    """p(y|G(f)) with Gauss-Hermite integration over q(f) (GaussianNonLinearMean.py:64-203)."""

    refuses_optimal_qu = "a flow on f (TGP) makes the likelihood non-Gaussian in f: q(u) has no closed-form optimum (SVGP and WGP have one)"
    refuses_optimal_qu_id = "input-dependent flows (ID_TGP) act on f: the likelihood is not Gaussian in f and q(u) has no closed-form optimum"

    def __init__(self, out_dim, noise_init, noise_is_shared, quadrature_points):
        super().__init__(out_dim, noise_init, noise_is_shared)
        self.quad_points = quadrature_points

    def expected_log_prob(self, Y, gauss_mean, gauss_cov, flow, X, **kwargs):
        assert len(flow) == self.out_dim == 1, "one flow per output; Dy = 1 on this path"
        # differentiable in the moments, the noise and the flow's parameters like the reference's torch code
        spec, theta, rowp = self._flow_inputs(flow, X, gauss_mean.device, with_grad=True)
        return ops.EllFlowFunction.apply(Y.reshape(-1), gauss_mean.reshape(-1).contiguous(), gauss_cov.reshape(-1).contiguous(),
                                         self._lvn().reshape(-1)[:1].contiguous(), theta, rowp, spec, self.quad_points)

    def marginal_moments(self, gauss_mean, gauss_cov, flow, X, **kwargs):
        assert len(flow) == self.out_dim == 1
        return self._moments(gauss_mean, gauss_cov, flow, X)


class WarpedGaussianLinearMean(GaussianLinearMean):
    """Warped GP: the flow T acts on the targets, p(y|f) = N(T(y)|f, s2) T'(y) (likelihoods/WarpedGaussianLinearMean.py).
    Constructor signature and attribute names of the reference (`flow` a ModuleList of one, `quad_points`,
    `log_var_noise`).  The flow has shared parameters only (it never sees X)."""

    lik_id = ops.L.LIK_WARPED
    engine_name = "warped"
    has_flow = flow_on_targets = compiles_flows = True
    refuses_mean = "the warped likelihood"
    refuses_crps = "the warped predictive (%s) is not a Gaussian mixture in y, so it has no closed pair term"

    def __init__(self, out_dim, noise_init, noise_is_shared, flow, quad_points):
        super().__init__(out_dim, noise_init, noise_is_shared)
        from .flow import instance_flow
        self.flow = nn.ModuleList([instance_flow(flow) if isinstance(flow, list) else flow])
        from .flow import ExpFlow, NormalCDFFlow, SoftplusFlow
        for fl in getattr(self.flow[0], "flow_arr", [self.flow[0]]):
            if isinstance(fl, (NormalCDFFlow, ExpFlow, SoftplusFlow)):
                raise ValueError("WarpedGaussianLinearMean: a {} block cannot warp the targets: the warp must map onto the real "
                                 "line, so that every Gaussian latent value is the image of a target".format(type(fl).__name__))
        self.quad_points = quad_points

    def _flow_inputs(self, flow=None, X=None, dev=None, with_grad=False):
        """Of the likelihood's own flow, whatever `flow` and `X` are."""
        spec, theta_list, nets = compile_flow(self.flow[0])
        if nets:
            raise ops.L.TgpError("a warped likelihood takes shared flow parameters only (no input-dependent blocks)")
        return spec, stack_theta(theta_list, dev, with_grad), None

    def expected_log_prob(self, Y, gauss_mean, gauss_cov, **kwargs):
        """Gaussian closed-form ELL at T(Y) plus sum_n log T'(y_n) (:65-85), differentiable in the moments, the noise and
        the flow's parameters (tgp_ell_warp_f64: value and every gradient in one launch)."""
        spec, theta, _ = self._flow_inputs(dev=gauss_mean.device, with_grad=True)
        return ops.EllWarpFunction.apply(Y.reshape(-1), gauss_mean.reshape(-1).contiguous(), gauss_cov.reshape(-1).contiguous(),
                                         self._lvn().reshape(-1)[:1].contiguous(), theta, spec)

    def unwarped_marginal_moments(self, gauss_mean, gauss_cov, diagonal=True):
        return super().marginal_moments(gauss_mean, gauss_cov, diagonal)

    def marginal_moments(self, gauss_mean, gauss_cov, diagonal=True, **kwargs):
        """Gauss-Hermite moments of T^-1(f), f ~ N(mean, cov + s2): (m1, E[.^2] - m1^2) (:93-148)."""
        assert diagonal, "only diagonal covariances on this path"
        return self._moments(gauss_mean, gauss_cov, None, None)

    def sample_from_output(self, f, i, **kwargs):
        """T^-1(f + s eps) (:44-63)."""
        var = positive_transform(self._lvn()[i]).detach()
        fs = td.Normal(f, torch.ones_like(f) * torch.sqrt(var)).sample()
        return self.flow[0].inverse(fs)

    def log_marginal(self, Y, gauss_mean, gauss_cov):
        """log N(T(Y) | mean, cov + s2 I) + sum log T'(Y) for a full covariance (:151-168, with its `sel.flow` typo fixed).
        Y, gauss_mean (Dy, MB), gauss_cov (Dy, MB, MB); plain torch on the GPU apart from the flow pass (not a hot path)."""
        spec, theta, _ = self._flow_inputs(dev=Y.device)
        ld, t = ops.flow_logdet(Y.reshape(-1).contiguous(), spec, theta, want_G=True) if spec.nblk else (Y.new_zeros(()), Y.reshape(-1))
        t = t.reshape(Y.shape)
        C = gauss_cov + torch.diag_embed(positive_transform(self._lvn()).detach().expand(-1, Y.size(1)))
        return td.MultivariateNormal(gauss_mean, covariance_matrix=C).log_prob(t) + ld


class Bernoulli(Likelihood):
    """p(y|G(f)) = Phi(G(f))^y Phi(-G(f))^(1-y), probit link, for binary classification (likelihoods/Bernoulli.py).
    No parameters.  The quadrature over q(f0) runs in float64 on the GPU (tgp_ell_flow_f64 / tgp_predict_f64 with
    TGP_LIK_BERNOULLI), with log Phi evaluated in the tails instead of through Phi."""

    display = "Bernoulli"
    lik_id = ops.L.LIK_BERNOULLI
    engine_name = "bernoulli"
    kind = "classifier"
    has_noise = False
    refuses_optimal_qu = NOT_GAUSSIAN_IN_F % display

    def __init__(self):
        super().__init__()
        self.C = 2
        self.quad_points = cg.quad_points

    def sample_from_output(self, f, i, **kwargs):
        probs = torch.special.ndtr(f)
        return td.Bernoulli(probs=probs).sample().to(cg.dtype)

    def _checks(self, gauss_mean, flow, X):
        assert len(flow) == 1, "Flow list must be size 1 for Bernoulli likelihood"
        assert gauss_mean.size(0) == 1, "Binary classification just require one GP for both classes"
        assert len(X.shape) == 3, 'Bad input X, expected (n_class,MB*S,Dx)'

    def expected_log_prob(self, Y, gauss_mean, gauss_cov, flow, X, **kwargs):
        """sum_n E_q(f0)[y_n log Phi(G(f0)) + (1 - y_n) log Phi(-G(f0))]; Y (1, MB) labels in [0, 1], moments (1, MB)."""
        self._checks(gauss_mean, flow, X)
        spec, theta, rowp = self._flow_inputs(flow, X, gauss_mean.device, with_grad=True)
        return ops.EllBernoulliFunction.apply(Y.reshape(-1).to(gauss_mean.dtype), gauss_mean.reshape(-1).contiguous(),
                                              gauss_cov.reshape(-1).contiguous(), theta, rowp, spec, self.quad_points)

    def marginal_moments(self, gauss_mean, gauss_cov, flow, X, **kwargs):
        """P(y = 1) of shape (MB, 1): Phi(mu / sqrt(1 + v)) for the identity flow, else each row's own quadrature."""
        self._checks(gauss_mean, flow, X)
        return self._moments(gauss_mean, gauss_cov, flow, X)[0].reshape(-1, 1)


class Poisson(Likelihood):
    """p(y|G(f)) = Poisson(y | exp(G(f))) for count targets: the flow of the latent GP is the log-rate (the identity flow
    gives the log-Gaussian Cox / Poisson GP model, a learned flow learns the link).  No parameters.  The quadrature over q(f0)
    runs in float64 on the GPU (tgp_ell_flow_f64 / tgp_predict_f64 with TGP_LIK_POISSON); the predictive log-pmf is a
    log-sum-exp over the nodes.  The reference has no such class; the interface is Bernoulli's."""

    display = "Poisson"
    lik_id = ops.L.LIK_POISSON
    engine_name = "poisson"
    kind = "count"
    has_noise = False
    one_launch_logp = True
    refuses_input_dependent = NO_INPUT_DEPENDENT % display
    refuses_optimal_qu = NOT_GAUSSIAN_IN_F % display
    refuses_cdf = ("%s: the predictive of a Poisson model is discrete; predictive_pmf(X, kmax) gives its pmf "
                   "(cumsum: the CDF) and posterior_quantiles the quantiles of the log-rate")

    def __init__(self):
        super().__init__()
        self.quad_points = cg.quad_points

    def sample_from_output(self, f, i, **kwargs):
        return torch.poisson(torch.exp(f))

    @staticmethod
    def check_targets(Y):
        """ValueError unless every target is a count: an integer >= 0 (the kernels take any real >= 0 and do not look)."""
        Yd = Y.detach()
        if not bool(((Yd >= 0) & (Yd == torch.round(Yd))).all()):     # (a NaN fails both comparisons)
            raise ValueError("the Poisson likelihood takes counts: every target must be an integer >= 0")

    def _checks(self, gauss_mean, flow, X):
        assert len(flow) == 1, "Flow list must be size 1 for Poisson likelihood"
        assert gauss_mean.size(0) == 1, "Count regression on this path has one output GP"
        assert len(X.shape) == 3, 'Bad input X, expected (1,MB,Dx)'

    def expected_log_prob(self, Y, gauss_mean, gauss_cov, flow, X, **kwargs):
        """sum_n E_q(f0)[y_n G(f0) - exp(G(f0))] - lgamma(y_n + 1); Y (1, MB) counts, moments (1, MB)."""
        self.check_targets(Y)
        self._checks(gauss_mean, flow, X)
        spec, theta, rowp = self._flow_inputs(flow, X, gauss_mean.device, with_grad=True)
        return ops.EllPoissonFunction.apply(Y.reshape(-1).to(gauss_mean.dtype), gauss_mean.reshape(-1).contiguous(),
                                            gauss_cov.reshape(-1).contiguous(), theta, rowp, spec, self.quad_points)

    def marginal_moments(self, gauss_mean, gauss_cov, flow, X, **kwargs):
        """(m1, m2) = (E[y], Var[y]) of the predictive, in counts, each of gauss_mean's shape (1, MB)."""
        self._checks(gauss_mean, flow, X)
        return self._moments(gauss_mean, gauss_cov, flow, X)


class NegativeBinomial(Poisson):
    """p(y|G(f)) = NB(y | mean = exp(G(f)), dispersion r) for over-dispersed counts: Var[y | f] = mean + mean^2 / r, and r -> inf is
    the Poisson likelihood.  One parameter, `log_dispersion` = log r (one element, initialised at log `dispersion_init`), which
    sits where the Gaussian classes' log_var_noise sits in the ABI and is trained through the same gradient slot.  Supported
    range 1e-3 <= r <= 1e3 (past it the terms of d/dlog r cancel and Poisson is the model to take; nothing looks at the value
    during training).  The quadrature over q(f0) runs in float64 on the GPU (tgp_ell_flow_f64 / tgp_predict_f64 with
    TGP_LIK_NEGBIN).  The reference has no such class; the interface is Poisson's."""

    display = "negative-binomial"
    lik_id = ops.L.LIK_NEGBIN
    engine_name = "negbinomial"
    has_noise = True
    outputs_refusal = "the negative-binomial likelihood is built for one output (num_outputs = 1)"
    refuses_input_dependent = NO_INPUT_DEPENDENT % display
    refuses_optimal_qu = NOT_GAUSSIAN_IN_F % display
    refuses_cdf = ("%s: the predictive of a negative-binomial model is discrete; predictive_pmf(X, kmax) gives its pmf "
                   "(cumsum: the CDF) and posterior_quantiles the quantiles of the log-mean")

    def __init__(self, dispersion_init=1.0):
        super().__init__()
        r = float(dispersion_init)
        if not r > 0.0:
            raise ValueError("the dispersion of the negative-binomial likelihood must be > 0, got %g" % r)
        self.log_dispersion = nn.Parameter(torch.log(torch.tensor([r], dtype=cg.dtype)))

    def noise(self):
        """log r, the one element behind the ABI's noise pointer, with the graph to the parameter."""
        return self.log_dispersion.reshape(-1)[:1]

    @property
    def dispersion(self):
        """r = exp(log_dispersion), detached."""
        return torch.exp(self.log_dispersion.detach())

    @staticmethod
    def check_targets(Y):
        """ValueError unless every target is a count: an integer >= 0 (the kernels take any real >= 0 and do not look)."""
        Yd = Y.detach()
        if not bool(((Yd >= 0) & (Yd == torch.round(Yd))).all()):     # (a NaN fails both comparisons)
            raise ValueError("the negative-binomial likelihood takes counts: every target must be an integer >= 0")

    def sample_from_output(self, f, i, **kwargs):
        """A Gamma-Poisson draw: Poisson(exp(f) Gamma(r, r))."""
        r = self.dispersion.to(f.device, f.dtype).reshape(())
        return torch.poisson(torch.exp(f) * td.Gamma(r, r).sample(f.shape).reshape(f.shape))

    def expected_log_prob(self, Y, gauss_mean, gauss_cov, flow, X, **kwargs):
        """sum_n E_q(f0)[log NB(y_n | exp(G(f0)), r)], differentiable in the moments, log_dispersion and the flow's parameters;
        Y (1, MB) counts, moments (1, MB)."""
        self.check_targets(Y)
        self._checks(gauss_mean, flow, X)
        spec, theta, rowp = self._flow_inputs(flow, X, gauss_mean.device, with_grad=True)
        return ops.EllNegBinFunction.apply(Y.reshape(-1).to(gauss_mean.dtype), gauss_mean.reshape(-1).contiguous(),
                                           gauss_cov.reshape(-1).contiguous(), self.noise().contiguous(), theta, rowp, spec,
                                           self.quad_points)


class Gamma(Likelihood):
    """p(y|G(f)) = Gamma(y | shape a, mean exp(G(f))) for positive, skewed targets (durations, claim sizes, rainfall, prices):
    the rate is a exp(-G(f)) and Var[y | f] = exp(2 G(f)) / a, the variance proportional to the squared mean.  One parameter,
    `log_shape` = log a (one element, initialised at log `shape_init`), which sits where the Gaussian classes' log_var_noise sits
    in the ABI and is trained through the same gradient slot.  Supported range lib.GAMMA_MIN_SHAPE <= a <= lib.GAMMA_MAX_SHAPE
    (below it the extreme quantiles leave the double range; nothing looks at the value during training, the exact CDF and
    quantiles of the model refuse a shape that has left it).  The quadrature over q(f0) runs in float64 on the GPU
    (tgp_ell_flow_f64 / tgp_predict_f64 with TGP_LIK_GAMMA); the predictive is a mixture of Gammas, a location family in log y,
    whose exact CDF and quantiles tgp_predict_cdf_f64 / tgp_predict_quantile_f64 serve.  kind = "regression": the
    log density is that of the raw target (-log Y_std included: the targets may be scaled, not centred).  The reference has no
    such class."""

    display = "gamma"
    lik_id = ops.L.LIK_GAMMA
    engine_name = "gamma"
    kind = "regression"
    has_noise = True
    one_launch_logp = True
    outputs_refusal = "the gamma likelihood is built for one output (num_outputs = 1)"
    refuses_input_dependent = NO_INPUT_DEPENDENT % display
    refuses_optimal_qu = NOT_GAUSSIAN_IN_F % display
    refuses_cdf = None
    refuses_crps = "the predictive of a gamma model (%s) is a mixture of Gammas, which has no closed pair term"

    def __init__(self, shape_init=1.0, quadrature_points=None):
        super().__init__()
        a = float(shape_init)
        if not ops.L.GAMMA_MIN_SHAPE <= a <= ops.L.GAMMA_MAX_SHAPE:
            raise ValueError("the shape of the gamma likelihood must lie in [%g, %g], got %g"
                             % (ops.L.GAMMA_MIN_SHAPE, ops.L.GAMMA_MAX_SHAPE, a))
        self.quad_points = cg.quad_points if quadrature_points is None else quadrature_points
        self.log_shape = nn.Parameter(torch.log(torch.tensor([a], dtype=cg.dtype)))

    def noise(self):
        """log a, the one element behind the ABI's noise pointer, with the graph to the parameter."""
        return self.log_shape.reshape(-1)[:1]

    @property
    def shape(self):
        """a = exp(log_shape), detached."""
        return torch.exp(self.log_shape.detach())

    def check_shape(self):
        """ValueError, naming the range, if the trained shape has left [lib.GAMMA_MIN_SHAPE, lib.GAMMA_MAX_SHAPE] (one sync)."""
        a = float(self.shape.reshape(-1)[0])
        if not ops.L.GAMMA_MIN_SHAPE <= a <= ops.L.GAMMA_MAX_SHAPE:      # (a NaN fails both comparisons)
            raise ValueError("the shape of the gamma likelihood is %g: the exact CDF and quantiles cover [%g, %g]"
                             % (a, ops.L.GAMMA_MIN_SHAPE, ops.L.GAMMA_MAX_SHAPE))

    @staticmethod
    def check_targets(Y):
        """ValueError unless every target is finite and > 0 (the kernels take log y and do not look)."""
        Yd = Y.detach()
        if not bool(((Yd > 0) & torch.isfinite(Yd)).all()):     # (a NaN fails the comparison)
            raise ValueError("the gamma likelihood takes positive targets: every target must be finite and > 0")

    def sample_from_output(self, f, i, **kwargs):
        """exp(f) Gamma(a, rate a): mean exp(f), shape a."""
        a = self.shape.to(f.device, f.dtype).reshape(())
        return torch.exp(f) * td.Gamma(a, a).sample(f.shape).reshape(f.shape)

    def _checks(self, gauss_mean, flow, X):
        assert len(flow) == 1, "Flow list must be size 1 for the gamma likelihood"
        assert gauss_mean.size(0) == 1, "Gamma regression on this path has one output GP"
        assert len(X.shape) == 3, 'Bad input X, expected (1,MB,Dx)'

    def expected_log_prob(self, Y, gauss_mean, gauss_cov, flow, X, **kwargs):
        """sum_n E_q(f0)[log Gamma(y_n | a, a exp(-G(f0)))], differentiable in the moments, log_shape and the flow's parameters;
        Y (1, MB) positive targets, moments (1, MB)."""
        self.check_targets(Y)
        self._checks(gauss_mean, flow, X)
        spec, theta, rowp = self._flow_inputs(flow, X, gauss_mean.device, with_grad=True)
        return ops.EllGammaFunction.apply(Y.reshape(-1).to(gauss_mean.dtype), gauss_mean.reshape(-1).contiguous(),
                                          gauss_cov.reshape(-1).contiguous(), self.noise().contiguous(), theta, rowp, spec,
                                          self.quad_points)

    def marginal_moments(self, gauss_mean, gauss_cov, flow, X, **kwargs):
        """(m1, m2) = (E[y], Var[y]) of the predictive, m2 = (1 + 1/a) E[exp(2 G(f))] - m1^2, each of gauss_mean's shape (1, MB)."""
        self._checks(gauss_mean, flow, X)
        return self._moments(gauss_mean, gauss_cov, flow, X)


class Beta(Likelihood):
    """p(y|G(f)) = Beta(y | mu phi, (1 - mu) phi), mu = sigmoid(G(f)), for proportions and rates strictly inside (0, 1)
    (conversion rates, fractions, percentages, probabilities as data): the flow's value is the log-odds of the mean, phi the
    precision, Var[y | f] = mu (1 - mu) / (1 + phi) -- it shrinks towards both ends of the interval.  The link is fixed; the
    monotone flow of a TGP learns what the link function should have been.  One parameter, `log_precision` = log phi (one
    element, initialised at log `precision_init`), which sits where the Gaussian classes' log_var_noise sits in the ABI and is
    trained through the same gradient slot.  Supported range lib.BETA_MIN_PRECISION <= phi <= lib.BETA_MAX_PRECISION (nothing
    looks at the value during training; the exact CDF and quantiles of the model refuse a precision that has left it).  The
    quadrature over q(f0) runs in float64 on the GPU (tgp_ell_flow_f64 / tgp_predict_f64 with TGP_LIK_BETA); the predictive is a
    mixture of Betas whose exact CDF and quantiles tgp_predict_cdf_f64 / tgp_predict_quantile_f64 serve through a regularised
    incomplete beta function.  kind = "regression"; the targets are never standardised (Y_std is ignored).  The
    reference has no such class."""

    display = "beta"
    lik_id = ops.L.LIK_BETA
    engine_name = "beta"
    kind = "regression"
    has_noise = True
    one_launch_logp = True
    outputs_refusal = "the beta likelihood is built for one output (num_outputs = 1)"
    refuses_input_dependent = NO_INPUT_DEPENDENT % display
    refuses_optimal_qu = NOT_GAUSSIAN_IN_F % display
    refuses_cdf = None
    refuses_crps = "the predictive of a beta model (%s) is a mixture of Betas, which has no closed pair term"

    def __init__(self, precision_init=10.0, quadrature_points=None):
        super().__init__()
        phi = float(precision_init)
        if not ops.L.BETA_MIN_PRECISION <= phi <= ops.L.BETA_MAX_PRECISION:
            raise ValueError("the precision of the beta likelihood must lie in [%g, %g], got %g"
                             % (ops.L.BETA_MIN_PRECISION, ops.L.BETA_MAX_PRECISION, phi))
        self.quad_points = cg.quad_points if quadrature_points is None else quadrature_points
        self.log_precision = nn.Parameter(torch.log(torch.tensor([phi], dtype=cg.dtype)))

    def noise(self):
        """log phi, the one element behind the ABI's noise pointer, with the graph to the parameter."""
        return self.log_precision.reshape(-1)[:1]

    @property
    def precision(self):
        """phi = exp(log_precision), detached."""
        return torch.exp(self.log_precision.detach())

    def check_precision(self):
        """ValueError, naming the range, if the trained precision has left [lib.BETA_MIN_PRECISION, lib.BETA_MAX_PRECISION]
        (one sync)."""
        phi = float(self.precision.reshape(-1)[0])
        if not ops.L.BETA_MIN_PRECISION <= phi <= ops.L.BETA_MAX_PRECISION:      # (a NaN fails both comparisons)
            raise ValueError("the precision of the beta likelihood is %g: the exact CDF and quantiles cover [%g, %g]"
                             % (phi, ops.L.BETA_MIN_PRECISION, ops.L.BETA_MAX_PRECISION))

    @staticmethod
    def check_targets(Y):
        """ValueError unless every target is finite and strictly inside (0, 1) (the kernels take log y and log(1 - y) and do
        not look)."""
        Yd = Y.detach()
        if not bool(((Yd > 0) & (Yd < 1)).all()):     # (a NaN fails both comparisons)
            raise ValueError("the beta likelihood takes proportions: every target must be finite and strictly inside (0, 1)")

    def sample_from_output(self, f, i, **kwargs):
        """Beta(mu phi, (1 - mu) phi) at mu = sigmoid(f)."""
        phi = self.precision.to(f.device, f.dtype).reshape(())
        return td.Beta(torch.sigmoid(f) * phi, torch.sigmoid(-f) * phi).sample().reshape(f.shape)

    def _checks(self, gauss_mean, flow, X):
        assert len(flow) == 1, "Flow list must be size 1 for the beta likelihood"
        assert gauss_mean.size(0) == 1, "Beta regression on this path has one output GP"
        assert len(X.shape) == 3, 'Bad input X, expected (1,MB,Dx)'

    def expected_log_prob(self, Y, gauss_mean, gauss_cov, flow, X, **kwargs):
        """sum_n E_q(f0)[log Beta(y_n | mu phi, (1 - mu) phi)], mu = sigmoid(G(f0)), differentiable in the moments, log_precision
        and the flow's parameters; Y (1, MB) proportions, moments (1, MB)."""
        self.check_targets(Y)
        self._checks(gauss_mean, flow, X)
        spec, theta, rowp = self._flow_inputs(flow, X, gauss_mean.device, with_grad=True)
        return ops.EllBetaFunction.apply(Y.reshape(-1).to(gauss_mean.dtype), gauss_mean.reshape(-1).contiguous(),
                                         gauss_cov.reshape(-1).contiguous(), self.noise().contiguous(), theta, rowp, spec,
                                         self.quad_points)

    def marginal_moments(self, gauss_mean, gauss_cov, flow, X, **kwargs):
        """(m1, m2) = (E[y], Var[y]) of the predictive, m2 = E[mu (1 - mu)] / (1 + phi) + Var[mu], each of gauss_mean's shape
        (1, MB)."""
        self._checks(gauss_mean, flow, X)
        return self._moments(gauss_mean, gauss_cov, flow, X)


class Ordinal(Likelihood):
    """p(y = k | G(f)) = Phi((b_{k+1} - G(f)) / sigma) - Phi((b_k - G(f)) / sigma) for ORDERED categories y in {0, .., K-1}
    (ratings, grades, severity levels): the cumulative-probit likelihood with K - 1 fixed bin edges b_1 < .. < b_{K-1}, b_0 = -inf,
    b_K = +inf.  `bin_edges` is a buffer, not a parameter (no optimiser moves it); the default is b_j = j - K / 2, unit spacing,
    centred.  With the edges fixed the monotone flow G of a TGP learns the spacing of the levels, which is ordinal regression
    with learned cut-points; SVGP keeps the spacing the edges give.  One parameter, `log_var_noise` = log sigma^2 (the Gaussian
    classes' name, shape (1, 1)); `noise_init` is sigma^2.  2 <= num_classes <= 64.  The quadrature over q(f0) runs in float64 on
    the GPU (tgp_ell_flow_f64 / tgp_predict_f64 with TGP_LIK_ORDINAL).  kind = "count": predictive_pmf(X, K - 1) is
    the class probabilities, predictive_crps(kmax=K - 1) the ranked probability score.  The reference has no such class."""

    display = "ordinal"
    lik_id = ops.L.LIK_ORDINAL
    engine_name = "ordinal"
    kind = "count"
    has_noise = True
    one_launch_logp = True
    outputs_refusal = "the ordinal likelihood is built for one output (num_outputs = 1)"
    refuses_input_dependent = NO_INPUT_DEPENDENT % display
    refuses_optimal_qu = NOT_GAUSSIAN_IN_F % display
    refuses_cdf = ("%s: the predictive of an ordinal model is discrete; predictive_pmf(X, num_classes - 1) gives its class "
                   "probabilities (cumsum: the CDF, from which the median class is read) and posterior_quantiles the quantiles "
                   "of G(f)")

    def __init__(self, num_classes, bin_edges=None, noise_init=1.0, quadrature_points=None):
        super().__init__()
        K = int(num_classes)
        if K != num_classes or not 2 <= K <= ops.L.ORDINAL_MAX_K:
            raise ValueError("the ordinal likelihood takes 2 <= num_classes <= %d, got %s" % (ops.L.ORDINAL_MAX_K, num_classes))
        if bin_edges is None:
            bin_edges = [j - K / 2.0 for j in range(1, K)]
        edges = ops.check_ordinal_edges(bin_edges).clone().to(cg.dtype)
        if edges.numel() != K - 1:
            raise ValueError("the ordinal likelihood of %d classes takes %d bin edges, got %d" % (K, K - 1, edges.numel()))
        if not float(noise_init) > 0.0:
            raise ValueError("the noise variance of the ordinal likelihood must be > 0, got %g" % float(noise_init))
        self.num_classes = K
        self.quad_points = cg.quad_points if quadrature_points is None else quadrature_points
        self.register_buffer("bin_edges", edges)
        self.log_var_noise = nn.Parameter(torch.ones(1, 1, dtype=cg.dtype) *
                                          inverse_positive_transform(torch.tensor(noise_init, dtype=cg.dtype)))

    def lik_kwargs(self):
        """The bin edges ride beside the noise: ops.ordinal_noise puts {log sigma^2, K, b_1, .., b_{K-1}} behind the ABI's noise
        pointer (the `df` key is the slot for what rides there)."""
        return {"lik": self.lik_id, "df": self.bin_edges}

    def check_targets(self, Y):
        """ValueError unless every target is a class: an integer in [0, num_classes - 1] (the kernels clamp and do not look)."""
        Yd = Y.detach()
        if not bool(((Yd >= 0) & (Yd <= self.num_classes - 1) & (Yd == torch.round(Yd))).all()):     # (a NaN fails all three)
            raise ValueError("the ordinal likelihood takes classes: every target must be an integer in [0, %d]"
                             % (self.num_classes - 1))

    def sample_from_output(self, f, i, **kwargs):
        """The number of bin edges below f + sigma eps."""
        sd = torch.sqrt(positive_transform(self.log_var_noise.detach().reshape(())))
        z = f + sd * torch.randn_like(f)
        return (z.unsqueeze(-1) > self.bin_edges.to(f.device, f.dtype)).sum(-1).to(cg.dtype)

    def _checks(self, gauss_mean, flow, X):
        assert len(flow) == 1, "Flow list must be size 1 for the ordinal likelihood"
        assert gauss_mean.size(0) == 1, "Ordinal regression on this path has one output GP"
        assert len(X.shape) == 3, 'Bad input X, expected (1,MB,Dx)'

    def expected_log_prob(self, Y, gauss_mean, gauss_cov, flow, X, **kwargs):
        """sum_n E_q(f0)[log p(y_n | G(f0))], differentiable in the moments, log_var_noise and the flow's parameters (none in
        bin_edges); Y (1, MB) classes, moments (1, MB)."""
        self.check_targets(Y)
        self._checks(gauss_mean, flow, X)
        spec, theta, rowp = self._flow_inputs(flow, X, gauss_mean.device, with_grad=True)
        return ops.EllOrdinalFunction.apply(Y.reshape(-1).to(gauss_mean.dtype), gauss_mean.reshape(-1).contiguous(),
                                            gauss_cov.reshape(-1).contiguous(), self.noise().contiguous(), self.bin_edges, theta,
                                            rowp, spec, self.quad_points)

    def marginal_moments(self, gauss_mean, gauss_cov, flow, X, **kwargs):
        """(m1, m2) = (E[y], Var[y]) of the predictive, in classes, each of gauss_mean's shape (1, MB)."""
        self._checks(gauss_mean, flow, X)
        return self._moments(gauss_mean, gauss_cov, flow, X)


class StudentT(_GaussianBase):
    """p(y|G(f)) = StudentT(y | df, loc = G(f), scale = sigma) for regression with gross errors in the targets: heavy tails keep
    a few outliers from inflating the noise and with it every predictive interval.  `log_var_noise` (the Gaussian classes' name
    and shape) holds log sigma^2, the log of the squared SCALE -- the noise variance is sigma^2 df / (df - 2); `noise_init` is
    sigma^2.  `df`, the degrees of freedom, is a fixed hyper-parameter kept as a buffer: it is not in parameters(), so no
    optimiser or weight decay moves it.  Supported range 2 < df <= 1e4 (ValueError outside): at or below 2 there is no variance,
    far above the Gaussian likelihood is the model to take.  The quadrature over q(f0) runs in float64 on the GPU
    (tgp_ell_flow_f64 / tgp_predict_f64 with TGP_LIK_STUDENT).  The reference has no such class."""

    display = "Student-t"
    lik_id = ops.L.LIK_STUDENT
    engine_name = "studentt"
    one_launch_logp = True
    outputs_refusal = "the Student-t likelihood is built for one output (num_outputs = 1)"
    refuses_input_dependent = NO_INPUT_DEPENDENT % display
    refuses_optimal_qu = NOT_GAUSSIAN_IN_F % display
    refuses_cdf = ("%s: the CDF of a Student-t predictive needs the incomplete beta function, which is not "
                   "built; use the sampled intervals (sample_from_predictive_distribution), or "
                   "posterior_quantiles for the quantiles of G(f)")
    refuses_crps = "the Student-t likelihood (%s) has no closed pair term E|Y - Y'| for a mixture of t densities"

    def __init__(self, out_dim, noise_init, noise_is_shared, quadrature_points, df=4.0):
        super().__init__(out_dim, noise_init, noise_is_shared)
        self.quad_points = quadrature_points
        self.register_buffer("df", torch.tensor([ops.check_student_df(df)], dtype=cg.dtype))

    def lik_kwargs(self):
        """`df` rides beside the noise: ops.student_noise puts {log sigma^2, nu} behind the ABI's noise pointer."""
        return {"lik": self.lik_id, "df": self.df}

    def sample_from_output(self, f, i, **kwargs):
        """G(f) + sigma t, t a Student-t draw of df degrees of freedom."""
        sd = torch.sqrt(positive_transform(self._lvn()[i])).detach()
        t = td.StudentT(self.df.to(f.device, f.dtype)).sample(f.shape).reshape(f.shape)
        return f + sd * t

    def expected_log_prob(self, Y, gauss_mean, gauss_cov, flow, X, **kwargs):
        """sum_n E_q(f0)[log StudentT(y_n | df, G(f0), sigma)], differentiable in the moments, log_var_noise and the flow's
        parameters; Y (1, MB), moments (1, MB)."""
        assert len(flow) == self.out_dim == 1, "one flow per output; Dy = 1 on this path"
        assert len(X.shape) == 3, 'Bad input X, expected (1,MB,Dx)'
        spec, theta, rowp = self._flow_inputs(flow, X, gauss_mean.device, with_grad=True)
        return ops.EllStudentFunction.apply(Y.reshape(-1).to(gauss_mean.dtype), gauss_mean.reshape(-1).contiguous(),
                                            gauss_cov.reshape(-1).contiguous(), self._lvn().reshape(-1)[:1].contiguous(),
                                            self.df, theta, rowp, spec, self.quad_points)

    def marginal_moments(self, gauss_mean, gauss_cov, flow, X, **kwargs):
        """(m1, m2) = mean and variance of the predictive in standardised units, each of gauss_mean's shape (1, MB); m2 holds
        the Student-t's own variance sigma^2 df / (df - 2)."""
        assert len(flow) == self.out_dim == 1
        return self._moments(gauss_mean, gauss_cov, flow, X)


class HeteroscedasticGaussian(Likelihood):
    """p(y | f, h) = N(y | G(f), exp(c + h)) for regression with input-dependent noise: f is latent GP 0 (with the model's
    flow), h latent GP 1 (no flow) and c = `log_var_noise`, the one parameter: the prior mean of the log noise variance,
    initialised at log `noise_init`.  The moments arrive as (2, MB): row 0 those of q(f), row 1 those of q(h).  h integrates out
    of the expected log-likelihood in closed form (tgp_ell_hetero_f64); the predictive density is an S x S product rule
    (tgp_predict_hetero_f64); DESIGN.md 8.  The reference has no such class."""

    display = "heteroscedastic"
    engine_name = "hetero"
    one_launch_logp = True
    num_latent = 2
    flow_outputs = observed_outputs = 1      # f carries the flow; one observed output, drawn from both latent rows
    outputs_refusal = "HeteroscedasticGaussian needs num_outputs = 2: latent GP 0 is f, latent GP 1 the log-noise h"
    extra_flow_refusal = "the heteroscedastic likelihood takes no flow on h, the log-noise GP: flow_specs[1] must be empty"
    refuses_input_dependent = NO_INPUT_DEPENDENT % display
    refuses_mean = "the heteroscedastic likelihood"
    refuses_full_cov = ("diagonal=False is not built for the heteroscedastic likelihood (HeteroscedasticGaussian: "
                        "two latent GPs)")
    refuses_full_cov_predictive = "diagonal=False is not built for the heteroscedastic likelihood (two latent GPs)"
    refuses_paths = ("posterior_paths is not built for the heteroscedastic likelihood (HeteroscedasticGaussian: "
                     "two latent GPs)")
    refuses_optimal_qu = ("the heteroscedastic likelihood (HeteroscedasticGaussian) has two coupled latent GPs: neither q(u) has a "
                          "closed-form optimum")
    refuses_cdf = ("%s: the exact CDF and quantiles of the heteroscedastic likelihood's double mixture "
                   "(HeteroscedasticGaussian) are not built; use the sampled intervals "
                   "(sample_from_predictive_distribution), posterior_quantiles for G(f) or "
                   "predictive_noise_std for the noise level")
    refuses_crps = ("the heteroscedastic likelihood (%s) is a double mixture with unequal variances, whose pair term is not "
                    "built")

    def __init__(self, noise_init, quadrature_points):
        super().__init__()
        self.out_dim = 2
        self.quad_points = quadrature_points
        self.log_var_noise = nn.Parameter(torch.ones(1, 1, dtype=cg.dtype) *
                                          inverse_positive_transform(torch.tensor(noise_init, dtype=cg.dtype)))

    def _checks(self, gauss_mean, gauss_cov, flow):
        assert gauss_mean.dim() == 2 and gauss_mean.size(0) == 2 and gauss_cov.shape == gauss_mean.shape, \
            "the heteroscedastic likelihood takes the moments of two latent GPs, shape (2, MB)"
        assert len(flow) >= 1, "Flow list must hold the flow of f (output 0)"

    def expected_log_prob(self, Y, gauss_mean, gauss_cov, flow, X, scale=1.0, **kwargs):
        """scale sum_n E_q(f) q(h)[log N(y_n | G(f), exp(c + h))], differentiable in both pairs of moments, c and the flow's
        parameters; Y (1, MB), moments (2, MB)."""
        self._checks(gauss_mean, gauss_cov, flow)
        spec, theta, rowp = self._flow_inputs(flow, X, gauss_mean.device, with_grad=True)
        return ops.EllHeteroFunction.apply(Y.reshape(-1).to(gauss_mean.dtype), gauss_mean.contiguous(), gauss_cov.contiguous(),
                                           self.log_var_noise.reshape(-1)[:1].contiguous(), theta, rowp, spec, self.quad_points,
                                           float(scale))

    def predict_rows(self, mu, v, lvn, spec, theta, rowp, Y=None, Y_std=1.0, want_moments=True):
        """tgp_predict_hetero_f64 on the (2, N) moments: m1, m2 of shape (1, N) and the per-row exact log density (N,)."""
        m1, m2, lp = ops.predict_hetero(mu.detach().contiguous(), v.detach().contiguous(), lvn, spec, theta, self.quad_points,
                                        rowp, Y=Y, Y_std=Y_std)
        return m1.reshape(1, -1), m2.reshape(1, -1), lp

    def marginal_moments(self, gauss_mean, gauss_cov, flow, X, Y=None, Y_std=1.0, **kwargs):
        """(m1, m2) = mean and variance of the predictive in standardised units, each (1, MB); m2 holds the mean noise variance
        exp(c + mu_h + v_h / 2).  With Y also the per-row exact log predictive density (MB,) as a third value, same launch."""
        self._checks(gauss_mean, gauss_cov, flow)
        spec, theta, rowp = self._flow_inputs(flow, X, gauss_mean.device)
        res = self.predict_rows(gauss_mean, gauss_cov, self.noise().detach().contiguous(), spec, theta, rowp, Y=Y, Y_std=Y_std)
        return res[:2] if Y is None else res

    def noise_std(self, gauss_mean_h, gauss_cov_h, probs):
        """Quantiles of the noise standard deviation exp((c + h) / 2) under q(h) = N(mean, cov), closed form (h -> exp is
        increasing): exp((c + mean + z_p sqrt(cov)) / 2), shape (Q, MB) for probs of length Q."""
        _, zq = ops.quantile_probs(probs, gauss_mean_h.device)
        mu, sd = gauss_mean_h.detach().reshape(1, -1), torch.sqrt(gauss_cov_h.detach().clamp_min(0.0)).reshape(1, -1)
        return torch.exp(0.5 * (self.log_var_noise.detach().reshape(()) + mu + zq.reshape(-1, 1) * sd))

    def sample_from_output(self, f, i, **kwargs):
        """G(f) + exp((c + h) / 2) eps for f of shape (2, n): row 0 the draws of G(f), row 1 those of h."""
        assert f.size(0) == 2, "Bad specified input"
        sd = torch.exp(0.5 * (self.log_var_noise.detach().reshape(()) + f[1]))
        return f[0] + sd * torch.randn_like(f[0])


class MulticlassCategorical(Likelihood):
    """p(y|G(f)) = softmax(G_1(f_1), ..., G_C(f_C))[y] over C latent GPs (likelihoods/MulticlassCategorical.py): every integral
    is a Monte-Carlo mean over `SMC` joint draws of the C latents of a row (tgp_ell_softmax_f64 / tgp_predict_softmax_f64).
    The draws: `eps` (S, C, MB) standard normals the caller fixes -- here (also (calls, S, C, MB): one set per training call)
    or per call -- or, by default, the kernels' own
    counter-based ones, a function of (`seed`, the number of training calls so far, sample, class, row): nothing of size
    S x C x MB is allocated, and every training call draws afresh."""

    EVAL_SALT = 0x6576616C     # prediction draws come from a stream of their own

    display = "multi-class (softmax)"
    engine_name = "multiclass"
    kind = "classifier"
    has_noise = False
    compiles_flows = one_launch_logp = True
    outputs_refusal = "MulticlassCategorical needs num_outputs = its number of classes"
    refuses_mean = "the multi-class model"
    refuses_full_cov = "diagonal=False is not built for multi-class models (num_outputs = C latent GPs)"
    refuses_paths = "posterior_paths is not built for multi-class models (num_outputs = C latent GPs)"
    refuses_optimal_qu = NOT_GAUSSIAN_IN_F % display

    def __init__(self, num_classes: int, eps=None, seed=None):
        super().__init__()
        assert num_classes > 2, "If you have a binary classification problem use the Bernouilli"
        self.C = num_classes
        self.SMC = cg.quad_points
        self.eps = eps
        self.seed = int(cg.config_seed if seed is None else seed)
        self._step = None            # device int32 counter of the training calls (the draws' step word)
        self._calls = 0              # training calls served from a 4-d `eps`

    @property
    def quad_points(self):
        return self.SMC

    @property
    def num_latent(self):
        return self.C

    def sample_from_output(self, f, i, **kwargs):
        assert f.size(0) == self.C, "Bad specified input"
        return td.Categorical(probs=torch.softmax(f.t(), dim=1)).sample().to(cg.dtype)

    def _flow_inputs(self, flow, X, dev, with_grad=False):
        """(SoftmaxSpec of the C flows, their shared parameters one after the other, None)."""
        specs, theta = [], []
        for fl in flow:
            spec, theta_list, nets = compile_flow(fl)
            if nets:
                raise ops.L.TgpError("the multi-class likelihood takes shared flow parameters only (no input-dependent blocks)")
            specs.append(spec)
            theta += theta_list
        return ops.SoftmaxSpec(specs), stack_theta(theta, dev, with_grad), None

    def _checks(self, gauss_mean, flow, X):
        assert len(flow) == self.C, "Flow list must be size {} for MultiClass likelihood".format(self.C)
        assert gauss_mean.size(0) == self.C, "Multiclass classification requires {} GPs, got {}".format(self.C, gauss_mean.size(0))
        assert len(X.shape) == 3, 'Bad input X, expected (n_class,MB*S,Dx)'
        assert X.size(0) == self.C, 'Wrong first dimension in X, expected n_classes'

    def _next_step(self, dev):
        if self._step is None or self._step.device != dev:
            self._step = torch.zeros(1, dtype=torch.int32, device=dev)
        self._step += 1
        return self._step.clone()     # snapshot: a later call must not change the draws this call's graph refers to

    def expected_log_prob(self, Y, gauss_mean, gauss_cov, flow, X, eps=None, seed=None, row0=0, scale=1.0, **kwargs):
        """1/S sum_s sum_n log softmax(G(f0_s))[y_n]; Y (1, MB) class indices, moments (C, MB).  Differentiable in the
        moments and the flows' parameters; `scale` multiplies value and gradients inside the launch."""
        self._checks(gauss_mean, flow, X)
        dev = gauss_mean.device
        spec, theta, _ = self._flow_inputs(flow, X, dev, with_grad=True)
        eps = self.eps if eps is None else eps
        if eps is not None and eps.dim() == 4:       # (calls, S, C, MB): one set of draws per training call, in order
            eps, self._calls = eps[self._calls], self._calls + 1
        step = None if eps is not None else self._next_step(dev)
        return ops.SoftmaxEllFunction.apply(Y.reshape(-1).to(gauss_mean.dtype), gauss_mean.contiguous(), gauss_cov.contiguous(),
                                            theta, spec, self.SMC, eps, self.seed if seed is None else int(seed), step,
                                            int(row0), float(scale))

    def predict_rows(self, mu, v, lvn, spec, theta, rowp, Y=None, Y_std=1.0, want_moments=True, eps=None, seed=None, row0=0):
        """tgp_predict_softmax_f64 on the (C, N) moments: (P (N, C), None, log P[n, y_n] or None); no noise, no scale."""
        P, logp = ops.predict_softmax(mu.detach().contiguous(), v.detach().contiguous(), spec, theta, self.SMC,
                                      eps=eps, seed=(self.seed if seed is None else int(seed)) ^ self.EVAL_SALT,
                                      step_dev=self._step, row0=row0, Y=Y)
        return P, None, logp

    def marginal_moments(self, gauss_mean, gauss_cov, flow, X, eps=None, seed=None, row0=0, Y=None, **kwargs):
        """P (MB, C) = 1/S sum_s softmax(G(f0_s)); with Y also log P[n, y_n] as a second return value.  The draws are `eps`
        (S, C, MB) when given here, else counter-based (the constructor's `eps` belongs to the training rows)."""
        self._checks(gauss_mean, flow, X)
        spec, theta, _ = self._flow_inputs(flow, X, gauss_mean.device)
        P, _, logp = self.predict_rows(gauss_mean, gauss_cov, None, spec, theta, None, Y=Y, eps=eps, seed=seed, row0=row0)
        return P if Y is None else (P, logp)
