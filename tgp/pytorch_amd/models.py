"""Drop-in model classes: `sparse_MF_SP` (TGP / ID_TGP) and `sparse_MF_GP` (SVGP).

Same constructor signatures, attribute and nn.Parameter names, method names, argument meaning and return
shapes as the reference (code/dsp/models/sparse_MF_SP.py:47, sparse_MF_GP.py:40), so the reference's
main.py / trainer idiom works unchanged:

    ELBO, ELL, KLD = model.ELBO(x, y);  (-ELBO).backward();  optimizer.step()

What differs is underneath: every number is produced by the HIP kernels of libtgp_hip.so (fused row kernel,
blocked Cholesky, hand-derived adjoints, the MLP kernel for the input-dependent flows' networks in training AND in
every evaluation method).  There is NO CPU fallback: calling these methods with CPU tensors
raises (the oracle in oracle/ is the CPU restatement, and it is test infrastructure only).
Restrictions of this build (asserted): one output GP (Dy = 1, all BASELINE configs; C latent GPs with MulticlassCategorical, two
-- f and the log-noise h -- with HeteroscedasticGaussian), 'scale_rbf' / 'scale_matern32' kernel, float64.  Mean functions
'zero', 'linear' and 'identity' (means.py; a non-zero mean with the multi-class, heteroscedastic, warped and input-dependent
models raises NotImplementedError).  Both q(u) parameterisations: with is_whiten=False the parameters (m, L_q) describe
q(u) = N(m, L_q L_q^T) and every method runs the whitened kernels at m_w = L^-1 m, Lam_w = L^-1 tril(L_q) (tgp_unwhiten_f64).
"""
from typing import List

import numpy
import torch
import torch.nn as nn

from . import config as cg
from . import ops
from .flow import CompositeFlow, IdentityFlow, compile_flow, instance_flow
from .means import MEAN_NAMES, ZeroMean, return_mean, return_projection_matrix
from .likelihoods import (Bernoulli, GaussianLinearMean, GaussianNonLinearMean, HeteroscedasticGaussian, MulticlassCategorical,
                          Poisson, StudentT, WarpedGaussianLinearMean)
from .utils import positive_transform

DEFAULT_INIT = {"variational_distribution": {"variance_scale": 1.0, "mean_scale": 0.0}}


class CholeskyVariationalDistribution(nn.Module):
    """Parameter holder with gpytorch's names (the reference uses it as such, sparse_MF_SP.py:158-177)."""

    def __init__(self, num_inducing_points, batch_shape=torch.Size([])):
        super().__init__()
        self.variational_mean = nn.Parameter(torch.zeros(*batch_shape, num_inducing_points, dtype=cg.dtype))
        eye = torch.eye(num_inducing_points, dtype=cg.dtype).repeat(*batch_shape, 1, 1)
        self.chol_variational_covar = nn.Parameter(eye)


def enable_eval_dropout(modules):
    """code/dsp/models/utils_models.py:358-364."""
    found = False
    for module in modules:
        if "Dropout" in type(module).__name__:
            module.train()
            found = True
    return found


class sparse_MF_SP(nn.Module):
    def __init__(self, model_specs: list, X: torch.tensor, init_Z: torch.tensor, N: float, likelihood: nn.Module,
                 num_outputs: int, is_whiten: bool, K_is_shared: bool, mean_is_shared: bool, Z_is_shared: bool,
                 q_U_is_shared: bool, flow_specs: list, flow_connection: str, add_noise_inducing: float,
                 be_fully_bayesian: bool = False, init_params: dict = {}) -> None:
        super().__init__()
        assert len(model_specs) == 2, "Parameter model_specs should be len 2: mean name and kernel instance"
        if isinstance(likelihood, StudentT) and int(num_outputs) != 1:
            raise NotImplementedError("the Student-t likelihood is built for one output (num_outputs = 1)")
        # C outputs only as the C latent GPs of the multi-class likelihood, 2 only as (f, h) of the heteroscedastic one (composed
        # step)
        assert int(num_outputs) == 1 or (isinstance(likelihood, MulticlassCategorical) and int(num_outputs) == likelihood.C) or \
            (isinstance(likelihood, HeteroscedasticGaussian) and int(num_outputs) == 2), \
            "this build implements the single-output path (Dy = 1, every BASELINE config)"
        assert not isinstance(likelihood, HeteroscedasticGaussian) or int(num_outputs) == 2, \
            "HeteroscedasticGaussian needs num_outputs = 2: latent GP 0 is f, latent GP 1 the log-noise h"
        assert not isinstance(likelihood, MulticlassCategorical) or int(num_outputs) == likelihood.C, \
            "MulticlassCategorical needs num_outputs = its number of classes"
        assert model_specs[0] in MEAN_NAMES, "mean function must be one of %s, got %r" % (", ".join(MEAN_NAMES), model_specs[0])
        assert not (K_is_shared or Z_is_shared or q_U_is_shared), "sharing flags are False in main.py"
        assert not mean_is_shared or model_specs[0] == "linear", \
            "mean_is_shared = True only with Linear mean function, got {}".format(model_specs[0])
        self.out_dim = int(num_outputs)
        self.inp_dim = int(init_Z.size(1))
        self.kernel_is_shared, self.mean_is_shared = K_is_shared, mean_is_shared
        self.Z_is_shared, self.q_U_is_shared = Z_is_shared, q_U_is_shared
        self.N = float(N)
        self.M = init_Z.size(0)
        self.likelihood = likelihood
        self.fully_bayesian = be_fully_bayesian
        ip = dict(DEFAULT_INIT)
        ip.update(init_params)
        self.init_params = ip
        self.standard_sampler = None        # the reference re-creates a td.MultivariateNormal here; sampling uses torch.randn
        self.is_training = True
        self.quad_points = likelihood.quad_points if isinstance(likelihood, (GaussianNonLinearMean, Bernoulli, Poisson, StudentT, WarpedGaussianLinearMean, MulticlassCategorical, HeteroscedasticGaussian)) else cg.quad_points
        if isinstance(likelihood, (Bernoulli, Poisson)):
            # the ABI's noise pointer: read by no Bernoulli or Poisson kernel, gradient 0; a buffer, so model.parameters() is the
            # reference's (Bernoulli) and holds no noise parameter (Poisson)
            self.register_buffer("_bern_lvn", torch.zeros(1, dtype=cg.dtype), persistent=False)
        self.is_whiten = bool(is_whiten)

        # inducing points (sparse_MF_SP.py:140-156)
        Z = torch.zeros(self.out_dim, self.M, self.inp_dim, dtype=cg.dtype)
        for l in range(self.out_dim):
            aux = init_Z.clone().to(cg.dtype)
            if add_noise_inducing > 0.0:
                aux = init_Z * torch.tensor(add_noise_inducing * numpy.random.randn(self.M, self.inp_dim), dtype=cg.dtype)
            Z[l, :] = aux
        self.Z = nn.Parameter(Z)
        # q(u) (sparse_MF_SP.py:158-177)
        q_U = CholeskyVariationalDistribution(self.M, batch_shape=torch.Size([self.out_dim]))
        vs = ip["variational_distribution"]["variance_scale"]
        ms = ip["variational_distribution"]["mean_scale"]
        q_U.chol_variational_covar.data = torch.eye(self.M, dtype=cg.dtype).view(1, self.M, self.M).repeat(self.out_dim, 1, 1) * numpy.sqrt(vs)
        q_U.variational_mean.data = torch.ones(self.out_dim, self.M, dtype=cg.dtype) * ms
        self.q_U = q_U
        self.covariance_function = model_specs[1]
        # flows (sparse_MF_SP.py:232-266)
        assert flow_connection == "single", "flow_connection must be 'single'"
        assert len(flow_specs) == self.out_dim
        G = []
        for fl in flow_specs:
            G.append(instance_flow(fl) if isinstance(fl, list) else fl)
        self.G_matrix = nn.ModuleList(G)
        self.G_flow_connection = flow_connection
        if self._is_poisson and any(getattr(fl, "input_dependent", False) for g in self.G_matrix
                                    for fl in getattr(g, "flow_arr", [])):
            raise NotImplementedError("the Poisson likelihood is built for SVGP and TGP: input-dependent flows (ID_TGP) are not")
        if self._is_student and any(getattr(fl, "input_dependent", False) for g in self.G_matrix
                                    for fl in getattr(g, "flow_arr", [])):
            raise NotImplementedError("the Student-t likelihood is built for SVGP and TGP: input-dependent flows (ID_TGP) are not")
        if self._is_hetero:
            if any(not isinstance(fl, IdentityFlow) for fl in getattr(self.G_matrix[1], "flow_arr", [self.G_matrix[1]])):
                raise NotImplementedError("the heteroscedastic likelihood takes no flow on h, the log-noise GP: flow_specs[1] must be empty")
            if any(getattr(fl, "input_dependent", False) for fl in getattr(self.G_matrix[0], "flow_arr", [])):
                raise NotImplementedError("the heteroscedastic likelihood is built for SVGP and TGP: input-dependent flows (ID_TGP) are not")
            if model_specs[0] != "zero":
                raise NotImplementedError("the '%s' mean function is not built for the heteroscedastic likelihood: use the 'zero' mean"
                                          % model_specs[0])
        # mean function (sparse_MF_SP.py:184-206); mean_is_shared: one mean for all outputs, at Dy = 1 the same object
        name = model_specs[0]
        if name != "zero":
            what = ("the multi-class model" if self._is_multiclass else "the warped likelihood" if self._is_warped else
                    "input-dependent flows (ID_TGP)" if any(getattr(fl, "input_dependent", False) for g in self.G_matrix
                                                             for fl in getattr(g, "flow_arr", [])) else None)
            if what is not None:
                raise NotImplementedError("the '%s' mean function is not built for %s: use the 'zero' mean" % (name, what))
        W = return_projection_matrix(self.inp_dim, self.out_dim, X.reshape(-1, self.inp_dim)) if name == "identity" else None
        self.mean_function = return_mean(name, self.inp_dim, 1 if mean_is_shared else self.out_dim, W)
        self.l2_regularize = False
        self._cfg = {}

    # ---- configuration -----------------------------------------------------------------------------
    def be_fully_bayesian(self, mode):
        self.fully_bayesian = mode

    def set_is_training(self, mode):
        self.is_training = mode

    # ---- helpers ---------------------------------------------------------------------------------
    def _require_gpu(self, t):
        if not t.is_cuda:
            raise ops.L.TgpError("tgp.pytorch_amd models run on the GPU only (got a %s tensor); there is no CPU "
                                 "fallback in the product path" % t.device)
        if t.dtype != torch.float64:
            raise ops.L.TgpError("float64 only: call config.set_maximum_precission() before building the model "
                                 "(code/main.py:124)")

    @property
    def _has_mean(self):
        return not isinstance(self.mean_function, ZeroMean)

    @property
    def _is_bernoulli(self):
        return isinstance(self.likelihood, Bernoulli)

    @property
    def _is_poisson(self):
        return isinstance(self.likelihood, Poisson)

    @property
    def _is_student(self):
        return isinstance(self.likelihood, StudentT)

    @property
    def _lik_id(self):
        """The `lik` of the ops calls: a lib.LIK_* for the likelihoods that are not told by the presence of a flow, else None."""
        return (ops.L.LIK_BERNOULLI if self._is_bernoulli else ops.L.LIK_POISSON if self._is_poisson else
                ops.L.LIK_STUDENT if self._is_student else ops.L.LIK_WARPED if self._is_warped else None)

    @property
    def _is_warped(self):
        return isinstance(self.likelihood, WarpedGaussianLinearMean)

    @property
    def _is_multiclass(self):
        return isinstance(self.likelihood, MulticlassCategorical)

    @property
    def _is_hetero(self):
        return isinstance(self.likelihood, HeteroscedasticGaussian)

    @property
    def _is_composed(self):
        """Several latent GPs: the step is composed per GP from the stand-alone pieces (_qf_per_class, per-GP KL)."""
        return self._is_multiclass or self._is_hetero

    def _gp_params(self, c=None, jitter=0.0, ladder=None, info=None):
        """What the whitened kernels consume: (Z, raw_ls, raw_os, m, Lam, lvn).  Whitened: the parameters themselves.
        Unwhitened (sparse_MF_SP.py:357-360, :386-391): m_w = L^-1 m, Lam_w = L^-1 tril(L_q) with L L^T = K_ZZ + jitter I, the
        factorisation under psd_safe_cholesky's ladder (or `ladder`); differentiable in Z, the kernel parameters, m and L_q
        when one of them needs it.  `info["jitter"]` receives the jitter the transform ended with."""
        p = self._raw_params(c)
        if self.is_whiten:
            if info is not None:
                info["jitter"] = 0.0
            return p
        Z, rl, ro, m, Lq, lvn = p
        kern = self.covariance_function.hip_kernel
        if ladder is None and cg.global_jitter is not None:      # config.global_jitter: the ladder's base, as for the step
            ladder = ops.jitter_ladder(jitter=cg.global_jitter)
        if self._has_mean:
            # m - m(Z): the mean of q(u) against the prior mean m(Z) (sparse_MF_SP.py:359) -- and the KL against
            # p(u) = N(m(Z), K_ZZ) (:446) depends on m - m(Z) only, so the same transform serves it.  The gradient reaches the
            # mean's parameters and Z through MeanFunction on Z (tgp_mean_backward_f64's g_X).
            if torch.is_grad_enabled():
                m = m - self.mean_function.vector(Z)
            else:
                m = self.mean_function.vector(Z, alpha=-1.0, inp=m.detach().contiguous())
        if torch.is_grad_enabled() and any(t.requires_grad for t in (Z, rl, ro, m, Lq)):
            m_w, Lam_w = ops.UnwhitenFunction.apply(Z, rl, ro, m, Lq, kern, float(jitter), ladder, info)
        else:
            m_w, Lam_w, _, _ = ops.unwhiten(*(t.detach() for t in (Z, rl, ro, m, Lq)), jitter=float(jitter), kernel=kern,
                                            info=info, ladder=ladder)
        return Z, rl, ro, m_w, Lam_w, lvn

    def _raw_params(self, c=None):
        k = self.covariance_function
        if c is not None:            # latent GP c of a multi-class model: slice c of the batched parameters, no noise
            D = self.inp_dim
            return (self.Z[c], k.base_kernel.raw_lengthscale.reshape(-1, D)[c], k.raw_outputscale.reshape(-1)[c:c + 1],
                    self.q_U.variational_mean[c], self.q_U.chol_variational_covar[c], None)
        lvn = self._bern_lvn if self._is_bernoulli or self._is_poisson else self.likelihood.log_var_noise.reshape(-1)[:1]
        return (self.Z[0], k.base_kernel.raw_lengthscale.reshape(-1), k.raw_outputscale.reshape(-1),
                self.q_U.variational_mean[0], self.q_U.chol_variational_covar[0], lvn)

    def _qf_per_class(self, X2):
        """(mu, v) of shape (C, MB): one tgp_qf_moments_f64 per latent GP, in class order on the current stream;
        differentiable (tgp_qf_moments_bwd_f64) when a parameter needs it."""
        mus, vs = [], []
        for c in range(self.out_dim):
            info = {}
            Z, rl, ro, m, Lam, _ = self._gp_params(c, info=info)
            if torch.is_grad_enabled() and any(t.requires_grad for t in (Z, rl, ro, m, Lam)):
                mu, v = ops.QfMomentsFunction.apply(X2.detach(), Z, rl, ro, m, Lam, self.covariance_function.hip_kernel)
            else:
                mu, v = ops.qf_moments(X2, *(t.detach() for t in (Z, rl, ro, m, Lam)), jitter=info["jitter"],
                                       kernel=self.covariance_function.hip_kernel)
            mus.append(mu)
            vs.append(v)
        return torch.stack(mus), torch.stack(vs)

    def _elbo_multiclass(self, X2, Y, eps=None):
        """ELL - sum_c KL_c (sparse_MF_SP.py:590-593) composed from the stand-alone differentiable pieces: per class the
        q(f) moments and the KL, then ONE softmax likelihood launch over all classes.  Each class's row kernel runs twice,
        once for the moments and once for their adjoint (the known cost of the composed step)."""
        mu, v = self._qf_per_class(X2)
        KLD = self.KLD()
        X3 = X2.unsqueeze(0).expand(self.out_dim, -1, -1)
        ELL = self.likelihood.expected_log_prob(Y.t(), mu, v, flow=self.G_matrix, X=X3, eps=eps, scale=self.N / Y.size(0)).sum()
        KLD = KLD.sum()
        return ELL - KLD, ELL, KLD

    def _elbo_hetero(self, X2, Y):
        """ELL - KL_f - KL_h composed as _elbo_multiclass: the q(f) and q(h) moments and the two KL terms from the stand-alone
        differentiable pieces, then ONE heteroscedastic likelihood launch (tgp_ell_hetero_f64) that returns the adjoints of all
        four moment vectors, c and the flow's parameters."""
        mu, v = self._qf_per_class(X2)
        KLD = self.KLD().sum()
        ELL = self.likelihood.expected_log_prob(Y.t(), mu, v, flow=self.G_matrix, X=X2.unsqueeze(0),
                                                scale=self.N / Y.size(0)).sum()
        return ELL - KLD, ELL, KLD

    def _hetero_predict(self, X2, Y=None, Y_std=1.0):
        """Eval-mode q(f), q(h) moments at the rows of X2 and ONE tgp_predict_hetero_f64 launch on them:
        (m1 (1, N), m2 (1, N), logp (N,) or None, mean_q_f (2, N, 1), cov_q_f (2, N, 1)); no autograd."""
        self._require_gpu(X2)
        self._eval_mode()
        with torch.no_grad():
            mean_q_f, cov_q_f = self.marginal_variational_qf_parameters(X2, diagonal=True, is_duvenaud=False)
            res = self.likelihood.marginal_moments(mean_q_f.squeeze(2), cov_q_f.squeeze(2), flow=self.G_matrix, X=X2.unsqueeze(0),
                                                   Y=None if Y is None else Y.reshape(-1).to(mean_q_f.dtype), Y_std=Y_std)
        self.train()
        return res[0], res[1], (res[2] if Y is not None else None), mean_q_f, cov_q_f

    def predictive_noise_std(self, X, probs):
        """Quantiles of the noise standard deviation sqrt(exp(c + h(x))) under q(h) at the rows of X, shape (Q, N), in the
        model's standardised units: exp((c + mu_h + z_p sqrt(v_h)) / 2), closed form.  probs 0.5: the median noise level."""
        if not self._is_hetero:
            raise NotImplementedError("predictive_noise_std: the heteroscedastic likelihood only; %s has one noise level"
                                      % type(self.likelihood).__name__)
        X2 = X[0] if X.dim() == 3 else X
        self._require_gpu(X2)
        self._eval_mode()
        with torch.no_grad():
            mean_q_f, cov_q_f = self.marginal_variational_qf_parameters(X2, diagonal=True, is_duvenaud=False)
            q = self.likelihood.noise_std(mean_q_f[1].reshape(-1), cov_q_f[1].reshape(-1), probs)
        self.train()
        return q

    def _flow_inputs(self, X2d, with_grad, samples=1):
        """(FlowSpec or None, theta, rowp): shared scalars stacked into one vector, per-row parameters from the MLPs on the
        HIP kernel (dropout follows the nets' Dropout layers, as in the reference).  `samples` > 1 (fully Bayesian
        evaluation): the rows are evaluated `samples` times in ONE launch, rowp row s * N + n, every (sample, row) with
        its own dropout mask -- the reference's X.repeat to (S_MC, N, Dx), models/sparse_MF_SP.py:753-758."""
        if self._is_warped:          # the likelihood's own flow, applied to the targets: shared parameters only
            ctx = torch.enable_grad() if with_grad else torch.no_grad()
            with ctx:
                spec, theta = self.likelihood._flow_inputs(X2d.device, with_grad=with_grad)
            return spec, theta, None
        if isinstance(self.likelihood, GaussianLinearMean):
            return None, None, None
        spec, theta_list, nets = compile_flow(self.G_matrix[0])
        ctx = torch.enable_grad() if with_grad else torch.no_grad()
        with ctx:
            theta = torch.stack([p.reshape(()) for p in theta_list]) if theta_list else None
            rowp = None
            if nets:
                if "mlp" not in self._cfg:
                    from .flow import mlp_spec
                    self._cfg["mlp"] = mlp_spec(nets, seed=cg.config_seed)
                    self._cfg["mlp_step"] = torch.zeros(2, dtype=torch.int32, device=X2d.device)
                mspec = self._cfg["mlp"]
                if mspec is None:
                    raise ops.L.TgpError("the flow's parameter networks are outside the HIP MLP kernel's coverage (one "
                                         "architecture D -> H x L -> 1, H <= 64, 1 <= L <= 3, relu/tanh, dropout); this "
                                         "package has no torch.nn fallback for them")
                # all nets in one HIP launch (tgp_mlp_forward/backward_f64); a fresh dropout mask per call, the same
                # one for this call's backward (the counter moves before the forward, not after it)
                self._cfg["mlp_step"][0] += 1
                W = torch.cat([p.reshape(-1) for net in nets for p in net.parameters()])
                # dropout is on when the nets' Dropout layers are in train mode: in training, and in the fully
                # Bayesian evaluation, where enable_eval_dropout() re-enables ONLY those layers after eval()
                # (models/utils_models.py:358-364) -- the container's own .training flag is False there
                drop_on = any(mod.training for mod in nets[0].modules() if "Dropout" in type(mod).__name__)
                # the counter is snapshotted per call: a second forward before this call's backward (loss accumulated
                # over minibatches, an evaluation between ELBO() and backward()) must not change the mask the
                # backward recomputes
                Xs = X2d.contiguous() if samples == 1 else X2d.repeat(samples, 1)
                # evaluation draws from a mask stream of its own: the resident engine counts its training steps from 0
                # too, and MC-dropout samples at test time must not replay the masks of training step k
                mcall = mspec if with_grad else mspec.salted(ops.MASK_SALT_EVAL)
                rowp = ops.MlpFunction.apply(Xs, W, mcall, bool(drop_on), self._cfg["mlp_step"].clone())
        return spec, theta, rowp

    # ---- model computations ------------------------------------------------------------------------
    def marginal_variational_qf_parameters(self, X, diagonal: bool, is_duvenaud: bool, init_Z=None):
        """q(f) marginals (sparse_MF_SP.py:274-396): returns mu of shape (Dy, MB, 1) and cov of shape (Dy, MB, 1), or
        (Dy, MB, MB) with diagonal=False -- the full covariance K_xx - K_xz K_zz^-1 K_zx + rhs^T S rhs (:384), from
        tgp_qf_cov_f64.  The full covariance is evaluated WITHOUT autograd and both tensors come back detached; when
        gradients are enabled and a parameter requires them the call raises (diagonal=True is the differentiable path).
        MB <= 4096, single-output models only."""
        assert not is_duvenaud, "is_duvenaud=False on this path"
        if not diagonal and self._is_hetero:
            raise NotImplementedError("diagonal=False is not built for the heteroscedastic likelihood (HeteroscedasticGaussian: "
                                      "two latent GPs)")
        X2 = X[0] if X.dim() == 3 else X
        self._require_gpu(X2)
        if not diagonal:
            if self._is_multiclass:
                raise NotImplementedError("diagonal=False is not built for multi-class models (num_outputs = C latent GPs)")
            info = {}
            Z, rl, ro, m, Lam, _ = self._gp_params(info=info)
            if torch.is_grad_enabled() and any(t.requires_grad for t in (Z, rl, ro, m, Lam)):
                raise NotImplementedError("the full covariance (diagonal=False) has no backward: call it under torch.no_grad(); "
                                          "diagonal=True is the differentiable path")
            if self._has_mean and torch.is_grad_enabled() and any(q.requires_grad for q in self.mean_function.parameters()):
                raise NotImplementedError("the full covariance (diagonal=False) has no backward: call it under torch.no_grad(); "
                                          "diagonal=True is the differentiable path")
            # (unwhitened: the factor behind Sigma starts at the jitter the transform ended with; whitened: 0)
            mu, cov = ops.qf_cov(X2.detach(), *(t.detach() for t in (Z, rl, ro, m, Lam)), jitter=info["jitter"],
                                 kernel=self.covariance_function.hip_kernel)
            if self._has_mean:       # mu + m(X) (sparse_MF_SP.py:355,360), in place
                mu = self.mean_function.vector(X2.detach(), inp=mu).detach()
            return mu.reshape(1, -1, 1), cov.unsqueeze(0)
        if self._is_composed:
            mu, v = self._qf_per_class(X2)
            return mu.unsqueeze(2), v.unsqueeze(2)
        info = {}
        Z, rl, ro, m, Lam, _ = self._gp_params(info=info)
        if torch.is_grad_enabled() and any(t.requires_grad for t in (Z, rl, ro, m, Lam)):
            # differentiable like the reference's (autograd through :274-396): tgp_qf_moments_bwd_f64 in the backward
            # (its own ladder from jitter 0: with an unwhitened q(u) it ends where the transform's did, same matrix, same ladder)
            mu, v = ops.QfMomentsFunction.apply(X2.detach(), Z, rl, ro, m, Lam, self.covariance_function.hip_kernel)
        else:
            mu, v = ops.qf_moments(X2, *(t.detach() for t in (Z, rl, ro, m, Lam)), jitter=info["jitter"],
                                   kernel=self.covariance_function.hip_kernel)
        if self._has_mean:           # mu + m(X) (sparse_MF_SP.py:355,360): every method downstream of (mu, v) gets it from here
            if torch.is_grad_enabled() and (mu.requires_grad or any(q.requires_grad for q in self.mean_function.parameters())):
                mu = mu + self.mean_function.vector(X2.detach())
            else:
                mu = self.mean_function.vector(X2.detach(), inp=mu)
        return mu.reshape(1, -1, 1), v.reshape(1, -1, 1)

    def _kld_unwhitened(self, c=None):
        """KL(q(u) || p(u)) of sparse_MF_SP.py:433-453: p(u) = N(0, K_ZZ + j I) from add_jitter_MultivariateNormal, which adds
        at least 1e-8 (ladder 1e-8 * 10^i, i < 5).  Equal to the whitened KL at unwhiten(m, L_q; j); differentiable in Z,
        the kernel parameters, m and L_q."""
        Z, rl, ro, m_w, Lam_w, _ = self._gp_params(c, jitter=ops.KL_PRIOR_JITTERS[0], ladder=ops.KL_PRIOR_JITTERS)
        if torch.is_grad_enabled() and (m_w.requires_grad or Lam_w.requires_grad):
            return ops.KlFunction.apply(m_w, Lam_w).reshape(())
        return ops.kl_whitened(m_w.detach(), Lam_w.detach())[0].reshape(()).clone()

    def KLD(self):
        """KL(q(u) || p(u)), shape (Dy,): the whitened form (sparse_MF_SP.py:406-431), differentiable in (m, L_q) like the
        reference's, or with is_whiten=False the KL against N(0, K_ZZ + j I) (:433-453), differentiable in Z and the kernel
        parameters too."""
        if not self.is_whiten:
            if self._is_composed:
                return torch.stack([self._kld_unwhitened(c) for c in range(self.out_dim)])
            return self._kld_unwhitened().reshape(1)
        if self._is_composed:
            kls = []
            for c in range(self.out_dim):
                m, Lam = self.q_U.variational_mean[c], self.q_U.chol_variational_covar[c]
                if torch.is_grad_enabled() and (m.requires_grad or Lam.requires_grad):
                    kls.append(ops.KlFunction.apply(m, Lam).reshape(()))
                else:
                    kls.append(ops.kl_whitened(m.detach(), Lam.detach())[0].reshape(()).clone())
            return torch.stack(kls)
        m, Lam = self.q_U.variational_mean[0], self.q_U.chol_variational_covar[0]
        if torch.is_grad_enabled() and (m.requires_grad or Lam.requires_grad):
            return ops.KlFunction.apply(m, Lam).reshape(1)
        kl, _, _ = ops.kl_whitened(m.detach(), Lam.detach())
        return kl.reshape(1)

    def ELBO(self, X, Y, _qu_jitter=None):
        """Returns (ELBO, ELL, KLD): positive ELBO with autograd, the trainer negates (sparse_MF_SP.py:552-598).
        `_qu_jitter` (collapsed_bound only): q(u) enters as a constant and the step starts at this jitter."""
        X2 = X[0] if X.dim() == 3 else X
        self._require_gpu(X2)
        assert Y.dim() == 2 and Y.shape[1] == 1, "Y must be (MB, 1)"
        if self._is_multiclass:
            return self._elbo_multiclass(X2, Y)
        if self._is_hetero:
            assert _qu_jitter is None
            return self._elbo_hetero(X2, Y)
        if self._is_poisson:
            self.likelihood.check_targets(Y)      # counts only (ValueError); the kernels themselves take any real >= 0
        info = {}
        Z, rl, ro, m, Lam, lvn = self._gp_params(info=info)
        if _qu_jitter is not None:
            m, Lam = m.detach(), Lam.detach()
        spec, theta, rowp = self._flow_inputs(X2, with_grad=True)
        cfg = self._cfg
        cfg.update(N_total=self.N, flow=spec, S=self.quad_points, check_status=(cg.status_check == "always"),
                   global_jitter=cg.global_jitter, kernel=self.covariance_function.hip_kernel,
                   lik=self._lik_id, df=self.likelihood.df if self._is_student else None,
                   grad_Y=False)
        if self._has_mean:
            if spec is None:
                # Gaussian likelihood: the unchanged closed-form step on Y - m(X); the step hands back the targets' adjoint
                # -scale e^-eta (Y - m(X) - mu), which MeanFunction (alpha = -1) turns into the mean's
                Y = self.mean_function.vector(X2, alpha=-1.0, inp=Y.detach().reshape(-1).contiguous()).reshape(-1, 1)
                cfg["grad_Y"] = True
            else:
                # flow likelihoods: a per-row affine block (a_n, b_n) = (1, m(x_n)) at the head of the program turns G(f) into
                # G(f + m(x_n)); the step's g_rowp[:, 1] is dELBO/dm(x_n)
                rowp = self.mean_function.rowp(X2)
                spec = ops.FlowSpec([(ops.L.FLOW_AFFINE, 0, 0, ops.L.FLAG_PER_ROW)] + list(spec.blocks), spec.P, 2, X2.device)
                cfg["flow"] = spec
        if not self.is_whiten:
            # the step's likelihood term at (m_w, Lam_w) and the jitter their factor was formed with (0 unless the ladder
            # raised it), its own KL switched off; the KL against the reference's jittered prior is added apart
            cfg["jitter"] = info["jitter"]
            ell = ops.EllStepFunction.apply(X2, Y, Z, rl, ro, m, Lam, lvn, theta, rowp, cfg)
            kld = self.KLD().sum()
            return ell - kld, ell, kld
        if _qu_jitter is not None:
            cfg["jitter"] = float(_qu_jitter)
            try:
                return ops.ElboFunction.apply(X2, Y, Z, rl, ro, m, Lam, lvn, theta, rowp, cfg)
            finally:
                del cfg["jitter"]
        elbo, ell, kld = ops.ElboFunction.apply(X2, Y, Z, rl, ro, m, Lam, lvn, theta, rowp, cfg)
        return elbo, ell, kld

    # ---- closed-form optimal q(u): the collapsed bound ----------------------------------------------
    def _qu_refusal(self):
        """Why this model has no closed-form optimal q(u), or None.  The closed form needs a likelihood that is Gaussian in f
        (on the targets themselves, on Y - m(X), or on the warped targets T(Y)) and the whitened parameterisation."""
        if self._is_multiclass:
            return "the multi-class (softmax) likelihood is not Gaussian in f: q(u) has no closed-form optimum"
        if self._is_bernoulli:
            return "the Bernoulli likelihood is not Gaussian in f: q(u) has no closed-form optimum"
        if self._is_poisson:
            return "the Poisson likelihood is not Gaussian in f: q(u) has no closed-form optimum"
        if self._is_student:
            return "the Student-t likelihood is not Gaussian in f: q(u) has no closed-form optimum"
        if self._is_hetero:
            return ("the heteroscedastic likelihood (HeteroscedasticGaussian) has two coupled latent GPs: neither q(u) has a "
                    "closed-form optimum")
        if not isinstance(self.likelihood, GaussianLinearMean):
            if any(getattr(fl, "input_dependent", False) for g in self.G_matrix for fl in getattr(g, "flow_arr", [])):
                return "input-dependent flows (ID_TGP) act on f: the likelihood is not Gaussian in f and q(u) has no closed-form optimum"
            return "a flow on f (TGP) makes the likelihood non-Gaussian in f: q(u) has no closed-form optimum (SVGP and WGP have one)"
        if not self.is_whiten:
            return "is_whiten=False: the closed form is built for the whitened q(u) only"
        return None

    def set_optimal_qu(self, X, Y):
        """Write the maximiser of the ELBO over q(u), at the current hyper-parameters and for these rows, into q_U
        (ops.optimal_qu / tgp_optimal_qu_f64; no autograd).  The targets are Y for the Gaussian likelihood, Y - m(X) with a linear
        or identity mean and T(Y) for the warped likelihood -- what the unchanged Gaussian step is run on.  Returns the `info`
        dict of the factorisation (info["jitter"]).  NotImplementedError, naming the reason, where no closed form exists."""
        why = self._qu_refusal()
        if why is not None:
            raise NotImplementedError("set_optimal_qu: " + why)
        X2 = X[0] if X.dim() == 3 else X
        self._require_gpu(X2)
        info = {}
        with torch.no_grad():
            Z, rl, ro, _, _, lvn = self._raw_params()
            t = Y.detach().reshape(-1).contiguous()
            if self._is_warped:
                spec, theta, _ = self._flow_inputs(X2, with_grad=False)
                if spec.nblk > 0:
                    t = ops.flow_eval(t, spec, None if theta is None else theta.detach(), want=("G",))["G"]
            elif self._has_mean:
                t = self.mean_function.vector(X2.detach(), alpha=-1.0, inp=t)
            m, Lam = ops.optimal_qu(X2.detach(), t, Z.detach(), rl.detach(), ro.detach(), lvn.detach(), self.N,
                                    kernel=self.covariance_function.hip_kernel, info=info,
                                    ladder=ops.jitter_ladder(jitter=cg.global_jitter))
            self.q_U.variational_mean.data[0].copy_(m)
            self.q_U.chol_variational_covar.data[0].copy_(Lam)
        return info

    def collapsed_bound(self, X, Y):
        """(ELBO, ELL, KLD) at the optimal q(u) of the current hyper-parameters: Titsias' collapsed bound as a differentiable
        function of Z, the kernel parameters, the noise and (where present) the mean's and the warp's parameters.  Forward:
        set_optimal_qu, then the unchanged step at the jitter the optimum ended with.  Backward: the step's gradients for the
        hyper-parameters; d ELBO / d q(u) vanishes at the optimum, so these ARE the collapsed bound's gradients (envelope
        theorem) and q_U, a constant of the step here, receives none.  q_U holds the optimum afterwards."""
        info = self.set_optimal_qu(X, Y)
        return self.ELBO(X, Y, _qu_jitter=info["jitter"])

    def check_status(self):
        """Lazy Cholesky status check (cg.status_check = 'lazy'): raises like psd_safe_cholesky would have."""
        st = self._cfg.get("last_status")
        if st is not None and ops.raise_for_status(st.cpu()):
            raise ops.NotPSDError("K_MM was not positive definite in the last ELBO call (pivot %d)" % int(st[0]))

    def ELL(self, X, Y, mean, cov):
        """N/MB * E_q(f)[log p(y|G(f))] from given moments (sparse_MF_SP.py:601-626); no autograd."""
        MB = Y.size(0)
        if self._is_multiclass and X.dim() == 2:
            X = X.unsqueeze(0).expand(self.out_dim, -1, -1)
        ell = self.likelihood.expected_log_prob(Y.t(), mean.squeeze(dim=2), cov.squeeze(dim=2), flow=self.G_matrix, X=X)
        return self.N / MB * ell

    def _eval_mode(self):
        self.eval()
        if self.fully_bayesian:
            assert enable_eval_dropout(self.modules()), "fully bayesian mode needs dropout layers in the flow"

    def predictive_distribution(self, X, diagonal: bool = True, S_MC_NNet: int = None):
        """m1, m2 (Dy, MB) + q(f) moments (sparse_MF_SP.py:457-540)."""
        assert not self.is_training, "This method only works in eval mode"
        if self._is_hetero:
            if not diagonal:
                raise NotImplementedError("diagonal=False is not built for the heteroscedastic likelihood (two latent GPs)")
            m1, m2, _, mean_q_f, cov_q_f = self._hetero_predict(X[0] if X.dim() == 3 else X)
            return m1, m2, mean_q_f, cov_q_f
        assert diagonal
        X3 = X.repeat(self.out_dim, 1, 1) if X.dim() == 2 else X
        self._eval_mode()
        with torch.no_grad():
            mean_q_f, cov_q_f = self.marginal_variational_qf_parameters(X3, diagonal=True, is_duvenaud=False)
            if self.fully_bayesian:
                assert S_MC_NNet is not None
                # all S_MC dropout samples in ONE pass, as the reference does by expanding X to (S_MC, N, Dx)
                # (sparse_MF_SP.py:753-758): one MLP launch over S_MC * N rows (a mask per sample and row), one
                # tgp_predict_f64 launch, then the mixture moments (:516-531)
                S, MB = int(S_MC_NNet), X3.shape[1]
                spec, theta, rowp = self._flow_inputs(X3[0], with_grad=False, samples=S)
                if self._is_bernoulli:
                    # P of every (sample, row) in one tgp_predict_f64 launch, the MC mean per row (sparse_MF_SP.py:521-525)
                    P, _, _ = ops.predict(mean_q_f.reshape(-1).repeat(S), cov_q_f.reshape(-1).repeat(S), self._bern_lvn, spec,
                                          theta.detach() if theta is not None else None, self.quad_points, rowp,
                                          lik=ops.L.LIK_BERNOULLI)
                    self.train()
                    return P.reshape(S, MB, 1).mean(0), None, mean_q_f, cov_q_f
                lvn = self.likelihood.log_var_noise.detach().reshape(-1)[:1].contiguous()
                mY, cY, _ = ops.predict(mean_q_f.reshape(-1).repeat(S), cov_q_f.reshape(-1).repeat(S), lvn, spec,
                                        theta.detach() if theta is not None else None, self.quad_points, rowp)
                mY, cY = mY.reshape(1, S, MB), cY.reshape(1, S, MB)       # (Dy, S, MB)
                m1 = mY.mean(1)
                m2 = (cY + mY ** 2).mean(1) - m1 ** 2
            elif self._is_bernoulli or self._is_multiclass:      # P(y = 1) of shape (MB, 1) / P of shape (MB, C)
                m1, m2 = self.likelihood.marginal_moments(mean_q_f.squeeze(2), cov_q_f.squeeze(2), flow=self.G_matrix, X=X3), None
            else:
                m1, m2 = self.likelihood.marginal_moments(mean_q_f.squeeze(2), cov_q_f.squeeze(2), diagonal=True,
                                                          flow=self.G_matrix, X=X3)
        self.train()
        return m1, m2, mean_q_f, cov_q_f

    def test_log_likelihood(self, X, Y, return_moments: bool, Y_std, S_MC_NNet: int = None):
        """log p(Y*|X*) summed over the batch, shape (Dy,), and optionally [m1, m2] (sparse_MF_SP.py:637-825)."""
        assert not self.is_training, "This method only works in eval mode"
        MB = X.size(0)
        X3 = X.repeat(self.out_dim, 1, 1) if X.dim() == 2 else X
        self._require_gpu(X3)
        if self._is_hetero:
            # sum_n log p(y_n | x_n), the exact log predictive density of the raw targets under the S x S product rule (every
            # constant, -log Y_std), with [m1, m2] from the same tgp_predict_hetero_f64 launch
            m1, m2, lp, _, _ = self._hetero_predict(X3[0], Y, float(Y_std.reshape(-1)[0]))
            return lp.sum().reshape(1), ([m1, m2] if return_moments else None)
        if self._is_multiclass:
            # sum_n log P[n, y_n] in float64, P and its logarithm from one tgp_predict_softmax_f64 launch (the reference goes
            # through float32 and compute_calibration_measures)
            self._eval_mode()
            with torch.no_grad():
                mean_q_f, cov_q_f = self.marginal_variational_qf_parameters(X3, diagonal=True, is_duvenaud=False)
                P, lp = self.likelihood.marginal_moments(mean_q_f.squeeze(2), cov_q_f.squeeze(2), flow=self.G_matrix, X=X3,
                                                         Y=Y.reshape(-1).to(mean_q_f.dtype))
            assert torch.isfinite(lp).all(), "Got saturated probabilities"
            self.train()
            return lp.sum().reshape(1), ([P] if return_moments else None)
        if self._is_bernoulli:
            # sum_n y log P + (1 - y) log(1 - P) in float64 (the reference takes it through float32 and
            # compute_calibration_measures), P as predictive_distribution returns it (MC mean when fully Bayesian)
            P, _, _, _ = self.predictive_distribution(X3, diagonal=True, S_MC_NNet=S_MC_NNet)
            assert torch.isfinite(P).all(), "Got saturated probabilities"
            P = P.reshape(-1)
            y = Y.reshape(-1).to(P.dtype)
            with torch.no_grad():
                lp = torch.where(y != 0, y * torch.log(P), torch.zeros_like(P)) + \
                    torch.where(y != 1, (1 - y) * torch.log1p(-P), torch.zeros_like(P))
            self.train()
            return lp.sum().reshape(1), ([torch.stack((1.0 - P, P), dim=1)] if return_moments else None)
        if self._is_poisson:
            # sum_n log p(y_n | x_n), the log predictive pmf of the observed counts, with [m1, m2] from the same launch; counts
            # have no scale: Y_std is not used (no log Y_std is subtracted)
            lp, m1, m2 = self._poisson_predict(X3[0], Y.reshape(-1), want_moments=return_moments)
            return lp.sum().reshape(1), ([m1.reshape(1, MB), m2.reshape(1, MB)] if return_moments else None)
        if self._is_student:
            # sum_n log p(y_n | x_n), the exact log predictive density of the raw targets (every constant, -log Y_std), with
            # [m1, m2] from the same tgp_predict_f64 launch
            self._eval_mode()
            with torch.no_grad():
                mean_q_f, cov_q_f = self.marginal_variational_qf_parameters(X3, diagonal=True, is_duvenaud=False)
                spec, theta, rowp = self._flow_inputs(X3[0], with_grad=False)
                m1, m2, lp = ops.predict(mean_q_f.reshape(-1).contiguous(), cov_q_f.reshape(-1).contiguous(),
                                         self.likelihood.log_var_noise.detach().reshape(-1)[:1].contiguous(), spec,
                                         theta.detach() if theta is not None else None, self.quad_points, rowp,
                                         Y=Y.reshape(-1).to(mean_q_f.dtype), Y_std=float(Y_std.reshape(-1)[0]),
                                         lik=ops.L.LIK_STUDENT, df=self.likelihood.df, want_moments=return_moments)
            self.train()
            return lp.sum().reshape(1), ([m1.reshape(1, MB), m2.reshape(1, MB)] if return_moments else None)
        predictive_params = None
        if return_moments:
            m1, m2, mean_q_f, cov_q_f = self.predictive_distribution(X3, diagonal=True, S_MC_NNet=S_MC_NNet)
            predictive_params = [m1, m2]
        else:
            self._eval_mode()
            with torch.no_grad():
                mean_q_f, cov_q_f = self.marginal_variational_qf_parameters(X3, diagonal=True, is_duvenaud=False)
        self._eval_mode()
        ystd = float(Y_std.reshape(-1)[0])
        mu, v = mean_q_f.reshape(-1).contiguous(), cov_q_f.reshape(-1).contiguous()
        lvn = self.likelihood.log_var_noise.detach().reshape(-1)[:1].contiguous()
        with torch.no_grad():
            if self._is_warped:
                # the exact warped predictive density log N(T(y) | mu, v + s2) + log T'(y) - log Y_std, summed over the rows
                # (the reference's branch for this class would give log N(y | m1, m2): DESIGN.md 8)
                spec, theta, _ = self._flow_inputs(X3[0], with_grad=False)
                _, _, lp = ops.predict(mu, v, lvn, spec, theta, self.quad_points, Y=Y, Y_std=ystd, lik=ops.L.LIK_WARPED,
                                       want_moments=False)
                log_p_y = lp.sum().reshape(1)
            elif isinstance(self.likelihood, GaussianLinearMean):
                _, _, lp = ops.predict(mu, v, lvn, Y=Y, Y_std=ystd)
                log_p_y = lp.sum().reshape(1)
            else:
                # S_MC dropout samples (fully Bayesian) in ONE pass: the nets over S_MC * N rows, one tgp_predict_f64
                # launch over the same rows (sparse_MF_SP.py:753-768 expands X, Y the same way)
                n_mc = int(S_MC_NNet) if self.fully_bayesian else 1
                spec, theta, rowp = self._flow_inputs(X3[0], with_grad=False, samples=n_mc)
                rep = (lambda t: t.repeat(n_mc)) if n_mc > 1 else (lambda t: t)
                _, _, lp = ops.predict(rep(mu), rep(v), lvn, spec, theta.detach() if theta is not None else None,
                                       self.quad_points, rowp, Y=rep(Y.reshape(-1)), Y_std=ystd)
                # kernel: logsumexp_s[log(w_s/sqrt(pi)) + logN]; the reference sums log w_s + logN and subtracts
                # 0.5*log(pi) where cg.pi is a float32 tensor (sparse_MF_SP.py:768-776): rebuild exactly that
                lp = lp.reshape(n_mc, MB) + 0.5 * float(numpy.log(numpy.pi))
                # float32 arithmetic of the reference's constant, with the correctly rounded float32 log(pi) (a host
                # torch.log in float32 differs by 1 ulp between CPU ISAs, which would make the result host-dependent)
                log_pi32 = numpy.log(numpy.float32(numpy.pi))
                if self.fully_bayesian:
                    stack = lp - float(numpy.float32(0.5) * log_pi32)
                    log_p_y = (torch.logsumexp(stack, 0).sum() - MB * numpy.log(n_mc)).reshape(1)
                else:
                    log_p_y = (lp[0].sum() - float(numpy.float32(0.5 * MB) * log_pi32)).reshape(1)
        self.train()
        return log_p_y, predictive_params

    # ---- count models: the predictive pmf -----------------------------------------------------------------
    def _poisson_predict(self, X2, Y, want_moments=True):
        """ONE tgp_predict_f64 launch of a Poisson model over B blocks of the N rows of X2, block b with the counts
        Y[b * N:(b + 1) * N] (the q(f) moments repeated B times): (logp (B * N,), m1 (N,), m2 (N,)), the moments None unless
        asked for.  Eval mode, no autograd.  A Poisson model has no input-dependent flow, so there are no per-row parameters
        (a mean function is part of mu) and no MC-dropout mixture."""
        if self.fully_bayesian:
            raise NotImplementedError("a Poisson model has no input-dependent flows, so no fully Bayesian (MC-dropout) mode")
        self._require_gpu(X2)
        N = X2.shape[0]
        B = Y.numel() // N
        assert B * N == Y.numel(), "Y must hold a whole number of blocks of X's rows"
        self._eval_mode()
        with torch.no_grad():
            mean_q_f, cov_q_f = self.marginal_variational_qf_parameters(X2.unsqueeze(0), diagonal=True, is_duvenaud=False)
            spec, theta, rowp = self._flow_inputs(X2, with_grad=False)
            assert rowp is None
            m1, m2, lp = ops.predict(mean_q_f.reshape(-1).repeat(B), cov_q_f.reshape(-1).repeat(B), self._bern_lvn, spec,
                                     theta.detach() if theta is not None else None, self.quad_points, None,
                                     Y=Y.to(mean_q_f.dtype), lik=ops.L.LIK_POISSON, want_moments=want_moments)
        self.train()
        return (lp, m1[:N], m2[:N]) if want_moments else (lp, None, None)

    def predictive_pmf(self, X, kmax: int):
        """The predictive pmf of a count model at the rows of X (N, Dx): P of shape (N, kmax + 1), P[n, k] = p(y_n = k | x_n),
        the exponential of tgp_predict_f64's log pmf from one launch over N (kmax + 1) rows (block k asks for the count k).
        Rows sum to 1 once kmax is past the mass; P.cumsum(1) is the predictive CDF, from which count intervals are read."""
        if not self._is_poisson:
            raise NotImplementedError("predictive_pmf: a count likelihood (Poisson) only; %s models have predictive_quantiles "
                                      "or class probabilities" % type(self.likelihood).__name__)
        assert X.dim() == 2, "Invalid input X.shape"
        kmax = int(kmax)
        assert kmax >= 0, "kmax must be >= 0"
        N = X.shape[0]
        k = torch.arange(kmax + 1, dtype=X.dtype, device=X.device).repeat_interleave(N)
        lp, _, _ = self._poisson_predict(X, k, want_moments=False)
        return torch.exp(lp).reshape(kmax + 1, N).t().contiguous()

    # ---- exact quantiles and CDF of the predictive / posterior marginals -----------------------------------
    def _quantile_inputs(self, X, what):
        """Eval-mode q(f) moments (mu, v of shape (N,)), the noise and the flow inputs of the rows of X, under no_grad."""
        if what == "predictive_crps":        # (its own reasons; the existing values of `what` below are unchanged)
            name = type(self.likelihood).__name__
            if self._is_bernoulli or self._is_multiclass:
                raise NotImplementedError("predictive_crps: a %s model predicts classes, which have no CRPS" % name)
            why = None
            if self._is_student:
                why = "the Student-t likelihood (%s) has no closed pair term E|Y - Y'| for a mixture of t densities" % name
            elif self._is_hetero:
                why = ("the heteroscedastic likelihood (%s) is a double mixture with unequal variances, whose pair term is not "
                       "built" % name)
            elif self._is_warped:
                why = "the warped predictive (%s) is not a Gaussian mixture in y, so it has no closed pair term" % name
            elif self.fully_bayesian:
                why = "the fully Bayesian model is an MC-dropout mixture over parameter draws, which the kernel does not sum"
            if why is not None:
                raise NotImplementedError("predictive_crps: %s; pass samples=S for the sampled estimator "
                                          "(ops.crps_from_samples of S predictive draws)" % why)
        if self._is_bernoulli or self._is_multiclass:
            raise NotImplementedError("%s: a %s model has no quantiles" % (what, type(self.likelihood).__name__))
        if self._is_poisson and what != "posterior_quantiles":
            raise NotImplementedError("%s: the predictive of a Poisson model is discrete; predictive_pmf(X, kmax) gives its pmf "
                                      "(cumsum: the CDF) and posterior_quantiles the quantiles of the log-rate" % what)
        if self._is_student and what != "posterior_quantiles":
            raise NotImplementedError("%s: the CDF of a Student-t predictive needs the incomplete beta function, which is not "
                                      "built; use the sampled intervals (sample_from_predictive_distribution), or "
                                      "posterior_quantiles for the quantiles of G(f)" % what)
        if self._is_hetero and what != "posterior_quantiles":
            raise NotImplementedError("%s: the exact CDF and quantiles of the heteroscedastic likelihood's double mixture "
                                      "(HeteroscedasticGaussian) are not built; use the sampled intervals "
                                      "(sample_from_predictive_distribution), posterior_quantiles for G(f) or "
                                      "predictive_noise_std for the noise level" % what)
        if self.fully_bayesian:
            raise NotImplementedError("%s: the fully Bayesian model (an MC-dropout mixture over parameter draws) is out of "
                                      "scope; use the sampled intervals" % what)
        assert X.dim() == 2, "Invalid input X.shape"
        self._eval_mode()
        with torch.no_grad():
            mean_q_f, cov_q_f = self.marginal_variational_qf_parameters(X.repeat(self.out_dim, 1, 1), diagonal=True,
                                                                        is_duvenaud=False)
            if self._is_hetero:      # output 0: f, the latent GP that goes through the flow
                mean_q_f, cov_q_f = mean_q_f[:1], cov_q_f[:1]
            spec, theta, rowp = self._flow_inputs(X, with_grad=False)
        lvn = self._raw_params()[5].detach().reshape(-1)[:1].contiguous()
        theta = theta.detach() if theta is not None else None
        return mean_q_f.reshape(-1).contiguous(), cov_q_f.reshape(-1).contiguous(), lvn, spec, theta, rowp

    def predictive_quantiles(self, X, probs):
        """Exact quantiles of p(y* | x*) at the rows of X, shape (Dy, Q, N), in the model's standardised units: the roots of
        the Gauss-Hermite predictive CDF (ops.predict_quantiles); the Gaussian likelihood's closed form; a warped model's
        T^-1(mu + zq sqrt(v + noise)).  probs: any order, each strictly inside (0, 1)."""
        mu, v, lvn, spec, theta, rowp = self._quantile_inputs(X, "predictive_quantiles")
        with torch.no_grad():
            if self._is_warped:
                _, zq = ops.quantile_probs(probs, mu.device)
                t = mu.unsqueeze(0) + zq.unsqueeze(1) * torch.sqrt(v.clamp_min(0.0) + torch.exp(lvn)).unsqueeze(0)
                q, _ = ops.flow_inverse(t, spec, theta)
            else:
                q = ops.predict_quantiles(mu, v, lvn, probs, spec, theta, self.quad_points, rowp)
        self.train()
        return q.unsqueeze(0)

    def posterior_quantiles(self, X, probs):
        """Quantiles of G(f0) under q(f0) at the rows of X, shape (Dy, Q, N): exact, G is increasing, so they are
        G(mu + zq sqrt(v)).  (A warped model's latent function carries no flow: mu + zq sqrt(v).)"""
        mu, v, lvn, spec, theta, rowp = self._quantile_inputs(X, "posterior_quantiles")
        with torch.no_grad():
            _, zq = ops.quantile_probs(probs, mu.device)
            f = mu.unsqueeze(0) + zq.unsqueeze(1) * torch.sqrt(v.clamp_min(0.0)).unsqueeze(0)
            if spec is not None and spec.nblk > 0 and not self._is_warped:
                f = ops.flow_eval(f.contiguous(), spec, theta, rowp, want=("G",))["G"]
        self.train()
        return f.unsqueeze(0)

    def predictive_cdf(self, X, Y):
        """The predictive CDF at the targets Y (N,1), standardised units: the PIT values of a calibration plot, shape (Dy, N).
        A warped model's is Phi((T(y) - mu) / sqrt(v + noise))."""
        mu, v, lvn, spec, theta, rowp = self._quantile_inputs(X, "predictive_cdf")
        with torch.no_grad():
            y = Y.reshape(-1).to(mu.dtype)
            if self._is_warped:
                t = ops.flow_eval(y.contiguous(), spec, theta, want=("G",))["G"] if spec.nblk > 0 else y
                cdf, _ = ops.predict_cdf(mu, v, lvn, t)
            else:
                cdf, _ = ops.predict_cdf(mu, v, lvn, y, spec, theta, self.quad_points, rowp)
        self.train()
        return cdf.unsqueeze(0)

    def predictive_crps(self, X, Y, Y_std=None, samples=None, kmax=None):
        """The continuous ranked probability score of p(y* | x*) at the targets Y (N,1), shape (Dy, N), in the model's
        standardised units -- or times Y_std when that is given (the CRPS has the units of the target).  Exact through
        ops.predict_crps for whatever predictive_cdf serves through the Gauss-Hermite mixture (Gaussian and flow likelihoods).
        A Poisson model: sum_k (cdf_k - 1{k >= y})^2 over k = 0..kmax from predictive_pmf(X, kmax); kmax is the caller's, as
        for predictive_pmf (past the mass the terms are 0).  samples=S: ops.crps_from_samples of S draws of
        sample_from_predictive_distribution, for any regression model.  Without it Student-t, heteroscedastic, warped and fully
        Bayesian models raise NotImplementedError; Bernoulli and multi-class models always do."""
        exact = samples is None and not self._is_poisson
        if exact or self._is_bernoulli or self._is_multiclass:
            ins = self._quantile_inputs(X, "predictive_crps")       # (the refusals; classifiers are refused on every route)
        y = Y.reshape(-1)
        if samples is not None:
            was = self.is_training
            self.set_is_training(False)
            try:
                draws, _, _ = self.sample_from_predictive_distribution(X, int(samples))       # (Dy,S,N,1)
            finally:
                self.set_is_training(was)
            out = ops.crps_from_samples(draws[0, :, :, 0], y.to(draws.dtype)).unsqueeze(0)
        elif self._is_poisson:
            if kmax is None:
                raise ValueError("predictive_crps of a Poisson model needs kmax, the last count of the sum (predictive_pmf's)")
            cdf = self.predictive_pmf(X, kmax).cumsum(1)                                       # (N, kmax + 1)
            k = torch.arange(int(kmax) + 1, dtype=cdf.dtype, device=cdf.device).unsqueeze(0)
            out = ((cdf - (k >= y.to(cdf.dtype).unsqueeze(1)).to(cdf.dtype)) ** 2).sum(1).unsqueeze(0)
        else:
            mu, v, lvn, spec, theta, rowp = ins
            with torch.no_grad():
                out = ops.predict_crps(mu, v, lvn, y.to(mu.dtype), spec, theta, self.quad_points, rowp).unsqueeze(0)
            self.train()
        if Y_std is not None:
            out = out * float(torch.as_tensor(Y_std).reshape(-1)[0])
        return out

    def predictive_interval_score(self, X, Y, alpha=0.05, Y_std=None):
        """The interval score of the central (1 - alpha) predictive interval at the targets Y (N,1), shape (Dy, N):
        ops.interval_score of predictive_quantiles(X, [alpha / 2, 1 - alpha / 2]) -- the same models, the same refusals.
        Standardised units, or times Y_std when that is given."""
        q = self.predictive_quantiles(X, [0.5 * alpha, 1.0 - 0.5 * alpha])[0]                  # (2,N)
        out = ops.interval_score(q[0], q[1], Y.reshape(-1).to(q.dtype), alpha).unsqueeze(0)
        if Y_std is not None:
            out = out * float(torch.as_tensor(Y_std).reshape(-1)[0])
        return out

    # ---- sampling (sparse_MF_SP.py:837-992) --------------------------------------------------------
    def sample_from_variational_marginal_base(self, X, diagonal: bool, is_duvenaud: bool, init_Z=None, S: int = 1):
        """diagonal=True: one independent draw per row of X (the caller has repeated the rows S times).  diagonal=False:
        S JOINT draws over the MB rows of X (not repeated): Sigma is formed once, eps = randn(S, MB) on the device, the draw
        kernel gives f0 = mu + eps chol(Sigma + jitter I)^T under psd_safe_cholesky's jitter ladder (first try: jitter 0).
        Returns f0 of shape (Dy, S * MB) in the diagonal path's sample-major layout, mean (Dy, MB, 1), cov (Dy, MB, MB)."""
        X3 = X.repeat(self.out_dim, 1, 1) if X.dim() == 2 else X
        Dy, SMB, _ = X3.shape
        if not diagonal:
            with torch.no_grad():
                mean_q_f, cov_q_f = self.marginal_variational_qf_parameters(X3, diagonal=False, is_duvenaud=is_duvenaud)
                e = torch.randn(int(S), SMB, dtype=mean_q_f.dtype, device=mean_q_f.device)
                f0 = ops.qf_joint_sample_safe(mean_q_f.reshape(-1), cov_q_f[0], e, jitter=cg.global_jitter)
            return f0.reshape(1, -1), mean_q_f, cov_q_f
        mean_q_f, cov_q_f = self.marginal_variational_qf_parameters(X3, diagonal=True, is_duvenaud=is_duvenaud)
        e = torch.randn(Dy, SMB, 1, dtype=mean_q_f.dtype, device=mean_q_f.device)
        f = (e * cov_q_f.sqrt() + mean_q_f).squeeze(dim=2)
        return f, mean_q_f, cov_q_f

    def sample_from_variational_marginal(self, X, S: int, diagonal: bool, is_duvenaud: bool, init_Z=None):
        """S function samples on the rows of X: f (Dy, S * MB) after the flows, the q(f0) moments and f0.  diagonal=False
        draws each sample jointly over the rows (coherent functions) and returns cov_q_f0 of shape (Dy, MB, MB)."""
        X3 = X.repeat(self.out_dim, 1, 1) if X.dim() == 2 else X
        X1 = X3
        X3 = X3.repeat(1, S, 1)
        if self.is_training:
            self.train()
        else:
            self._eval_mode()
        with torch.no_grad():
            if diagonal:
                f0, mean_q_f0, cov_q_f0 = self.sample_from_variational_marginal_base(X3, diagonal, is_duvenaud, init_Z)
            else:
                f0, mean_q_f0, cov_q_f0 = self.sample_from_variational_marginal_base(X1, diagonal, is_duvenaud, init_Z, S=S)
            f = torch.stack([g(f0[i], X3[i]) for i, g in enumerate(self.G_matrix)], 0)
        self.train()
        return f, mean_q_f0, cov_q_f0, f0

    def posterior_paths(self, S: int, num_frequencies: int = 1024, generator=None):
        """S coherent posterior function draws as a pathwise.PosteriorPaths (Wilson et al. 2020): `paths.f0(X)` and `paths(X)`
        evaluate the SAME S functions on any rows, in any batches, in O(N (num_frequencies + M) S) -- no N x N covariance and no
        4096-row cap.  The draw is fixed at the current parameters (detached copies).  `generator`: a seeded CPU torch.Generator
        behind the frequencies and the normals.  Unwhitened models go through the transform of `_gp_params`, as for the full
        covariance."""
        if self._is_multiclass:
            raise NotImplementedError("posterior_paths is not built for multi-class models (num_outputs = C latent GPs)")
        if self._is_hetero:
            raise NotImplementedError("posterior_paths is not built for the heteroscedastic likelihood (HeteroscedasticGaussian: "
                                      "two latent GPs)")
        if self.fully_bayesian:
            raise NotImplementedError("posterior_paths is not built for be_fully_bayesian models: the MC-dropout flows have "
                                      "no fixed per-row parameters, so a draw would not be one function")
        from .pathwise import draw_paths
        with torch.no_grad():
            info = {}
            Z, rl, ro, m, Lam, _ = self._gp_params(info=info)
            return draw_paths(*(t.detach() for t in (Z, rl, ro, m, Lam)), self.covariance_function.hip_kernel, S,
                              num_frequencies=num_frequencies, generator=generator, jitter=info["jitter"],
                              mean_function=self.mean_function if self._has_mean else None, flow=self.G_matrix[0])

    def sample_from_predictive_distribution(self, X, S: int, diagonal: bool = True) -> List[torch.tensor]:
        """diagonal=False: the likelihood's noise is added to JOINT function draws (one coherent function per sample)."""
        assert not self.is_training, "This method only works in eval mode"
        assert X.dim() == 2, "Invalid input X.shape"
        N, _ = X.shape
        with torch.no_grad():
            f_k, _, _, f_0 = self.sample_from_variational_marginal(X, S, diagonal=diagonal, is_duvenaud=False)
            # (the heteroscedastic likelihood has ONE observed output, drawn from both latent rows of f_k)
            samples = [self.likelihood.sample_from_output(f_k, i).view(S, N, 1) for i in range(1 if self._is_hetero else self.out_dim)]
        self.train()
        return torch.stack(samples, dim=0), f_k, f_0


class sparse_MF_GP(sparse_MF_SP):
    """SVGP (Hensman et al.): the same class with identity flows (sparse_MF_GP.py:40-64)."""

    def __init__(self, model_specs: list, X, init_Z, N: float, likelihood: nn.Module, num_outputs: int,
                 is_whiten: bool, K_is_shared: bool, mean_is_shared: bool, Z_is_shared: bool, q_U_is_shared: bool,
                 add_noise_inducing: float, init_params: dict = {}) -> None:
        flow_specs = [[("identity", [])] for _ in range(num_outputs)]
        super().__init__(model_specs, X, init_Z, N, likelihood, num_outputs, is_whiten, K_is_shared, mean_is_shared,
                         Z_is_shared, q_U_is_shared, flow_specs, "single", add_noise_inducing,
                         be_fully_bayesian=False, init_params=init_params)

    def sample_from_variational_marginal(self, X, S: int, diagonal: bool, is_duvenaud: bool, init_Z=None):
        X3 = X.repeat(self.out_dim, 1, 1) if X.dim() == 2 else X
        with torch.no_grad():
            if diagonal:
                f, mean_q_f, cov_q_f = self.sample_from_variational_marginal_base(X3.repeat(1, S, 1), diagonal, is_duvenaud, init_Z)
            else:
                f, mean_q_f, cov_q_f = self.sample_from_variational_marginal_base(X3, diagonal, is_duvenaud, init_Z, S=S)
        return f, mean_q_f, cov_q_f, f
