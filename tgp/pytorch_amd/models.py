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
from .flow import IdentityFlow, compile_flow, instance_flow, stack_theta
from .means import MEAN_NAMES, ZeroMean, return_mean, return_projection_matrix

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
        if int(num_outputs) != likelihood.num_latent:
            if likelihood.num_latent == 1 and likelihood.outputs_refusal is not None:
                raise NotImplementedError(likelihood.outputs_refusal)
            # C outputs only as the C latent GPs of the multi-class likelihood, 2 only as (f, h) of the heteroscedastic one (composed
            # step)
            assert int(num_outputs) == 1, "this build implements the single-output path (Dy = 1, every BASELINE config)"
            raise AssertionError(likelihood.outputs_refusal)
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
        self.quad_points = getattr(likelihood, "quad_points", cg.quad_points)
        if not likelihood.has_noise and not likelihood.composed:
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
        if any(not isinstance(fl, IdentityFlow) for g in self.G_matrix[likelihood.flow_outputs:] for fl in getattr(g, "flow_arr", [g])):
            raise NotImplementedError(likelihood.extra_flow_refusal)
        if self._input_dependent and likelihood.refuses_input_dependent is not None:
            raise NotImplementedError(likelihood.refuses_input_dependent)
        # mean function (sparse_MF_SP.py:184-206); mean_is_shared: one mean for all outputs, at Dy = 1 the same object
        name = model_specs[0]
        if name != "zero":
            what = likelihood.refuses_mean or ("input-dependent flows (ID_TGP)" if self._input_dependent else None)
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
    def _input_dependent(self):
        """A flow of the model has per-row parameters from a network on X (ID_TGP)."""
        return any(getattr(fl, "input_dependent", False) for g in self.G_matrix for fl in getattr(g, "flow_arr", []))

    @property
    def _noise(self):
        """What the ABI's noise pointer reads: the likelihood's noise, else the zero that no kernel reads (None: no such call)."""
        return self.likelihood.noise() if self.likelihood.has_noise else getattr(self, "_bern_lvn", None)

    @property
    def _lik_id(self):
        """The `lik` of the ops calls: a lib.LIK_* for the likelihoods that are not told by the presence of a flow, else None."""
        return self.likelihood.lik_id

    @property
    def _is_composed(self):
        """Several latent GPs: the step is composed per GP from the stand-alone pieces (_qf_per_class, per-GP KL)."""
        return self.likelihood.composed

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
            return (self.Z[c], k.base_kernel.raw_lengthscale.reshape(-1, D)[c], k.packed_outputscale(c),
                    self.q_U.variational_mean[c], self.q_U.chol_variational_covar[c], None)
        return (self.Z[0], k.base_kernel.raw_lengthscale.reshape(-1), k.packed_outputscale(),
                self.q_U.variational_mean[0], self.q_U.chol_variational_covar[0], self._noise)

    def _qf_one(self, X2, c=None):
        """(mu, v) of q(f) at the rows of X2 for latent GP c (None: the only one): tgp_qf_moments_f64, differentiable like the
        reference's autograd through sparse_MF_SP.py:274-396 (tgp_qf_moments_bwd_f64, its own ladder from jitter 0: with an
        unwhitened q(u) it ends where the transform's did, same matrix, same ladder) when a parameter needs it -- and in the
        rows of X2 themselves when X2 requires grad (tgp_qf_input_grad_f64); X2 is handed over undetached in that case only."""
        info = {}
        Z, rl, ro, m, Lam, _ = self._gp_params(c, info=info)
        x_grad = torch.is_grad_enabled() and X2.requires_grad
        if x_grad or (torch.is_grad_enabled() and any(t.requires_grad for t in (Z, rl, ro, m, Lam))):
            return ops.QfMomentsFunction.apply(X2 if x_grad else X2.detach(), Z, rl, ro, m, Lam,
                                               self.covariance_function.hip_kernel)
        return ops.qf_moments(X2, *(t.detach() for t in (Z, rl, ro, m, Lam)), jitter=info["jitter"],
                              kernel=self.covariance_function.hip_kernel)

    def _qf_per_class(self, X2):
        """(mu, v) of shape (C, MB): one _qf_one per latent GP, in class order on the current stream."""
        mus, vs = zip(*(self._qf_one(X2, c) for c in range(self.out_dim)))
        return torch.stack(mus), torch.stack(vs)

    def _elbo_composed(self, X2, Y):
        """ELL - sum_c KL_c (sparse_MF_SP.py:590-593) of a model of several latent GPs (multi-class: C, heteroscedastic: f and h)
        composed from the stand-alone differentiable pieces: per GP the q(f) moments and the KL, then ONE likelihood launch
        over all of them (tgp_ell_softmax_f64 / tgp_ell_hetero_f64) that returns the adjoints of every moment vector, the
        noise and the flows' parameters.  Each GP's row kernel runs twice, once for the moments and once for their adjoint
        (the known cost of the composed step)."""
        mu, v = self._qf_per_class(X2)
        KLD = self.KLD().sum()
        X3 = X2.unsqueeze(0).expand(self.likelihood.flow_outputs, -1, -1)
        ELL = self.likelihood.expected_log_prob(Y.t(), mu, v, flow=self.G_matrix, X=X3, scale=self.N / Y.size(0)).sum()
        return ELL - KLD, ELL, KLD

    def _predict_rows(self, X2, Y=None, Y_std=1.0, want_moments=True, qf=None):
        """The ONE predictive launch of the likelihood (ops.predict / predict_hetero / predict_softmax, by its predict_rows) at
        the rows of X2: eval mode -> q(f) moments (or `qf`, already there) -> flow inputs -> launch -> train(); no autograd.
        (m1, m2, logp or None, mean_q_f, cov_q_f), the first three as the likelihood shapes them.  A count model takes Y of
        B * N entries: block b of the launch holds the counts Y[b * N:(b + 1) * N] against the same N rows, their moments
        repeated B times (predictive_pmf); it has no input-dependent flow, so no MC-dropout mixture.  The likelihood's
        lik_kwargs() carry, in their `df` key, what rides beside the noise (ops.noise_slot): degrees of freedom or bin edges."""
        count = self.likelihood.kind == "count"
        if count and self.fully_bayesian:
            raise NotImplementedError("a %s model has no input-dependent flows, so no fully Bayesian (MC-dropout) mode"
                                      % self.likelihood.display)
        self._require_gpu(X2)
        self._eval_mode()
        with torch.no_grad():
            mean_q_f, cov_q_f = qf if qf is not None else self.marginal_variational_qf_parameters(X2, diagonal=True,
                                                                                                  is_duvenaud=False)
            spec, theta, rowp = self._flow_inputs(X2, with_grad=False)
            mu, v = mean_q_f.squeeze(2), cov_q_f.squeeze(2)
            if count and Y is not None:
                B = Y.numel() // X2.shape[0]
                assert B * X2.shape[0] == Y.numel(), "Y must hold a whole number of blocks of X's rows"
                mu, v = mu.reshape(-1).repeat(B), v.reshape(-1).repeat(B)
            lvn = self._noise
            res = self.likelihood.predict_rows(mu, v, None if lvn is None else lvn.detach().contiguous(), spec,
                                               theta.detach() if theta is not None else None, rowp,
                                               Y=None if Y is None else Y.reshape(-1).to(mu.dtype), Y_std=Y_std,
                                               want_moments=want_moments)
        self.train()
        return (*res, mean_q_f, cov_q_f)

    def predictive_noise_std(self, X, probs):
        """Quantiles of the noise standard deviation sqrt(exp(c + h(x))) under q(h) at the rows of X, shape (Q, N), in the
        model's standardised units: exp((c + mu_h + z_p sqrt(v_h)) / 2), closed form.  probs 0.5: the median noise level."""
        if not hasattr(self.likelihood, "noise_std"):
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
        ctx = torch.enable_grad() if with_grad else torch.no_grad()
        if self.likelihood.compiles_flows:     # the warp on the targets, the C flows of a multi-class model: shared parameters only
            with ctx:
                return self.likelihood._flow_inputs(self.G_matrix, X2d, X2d.device, with_grad=with_grad)
        if not self.likelihood.has_flow:
            return None, None, None
        spec, theta_list, nets = compile_flow(self.G_matrix[0])
        with ctx:
            theta = stack_theta(theta_list, None, with_grad)
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
        tgp_qf_cov_f64.  diagonal=True is differentiable in the parameters and, when X requires grad, in X (each row's moments
        in that row: tgp_qf_input_grad_f64 plus the mean function's slope).  The full covariance is evaluated WITHOUT autograd and both tensors come back detached; when
        gradients are enabled and a parameter requires them the call raises (diagonal=True is the differentiable path).
        MB <= 4096, single-output models only."""
        assert not is_duvenaud, "is_duvenaud=False on this path"
        if not diagonal and self.likelihood.refuses_full_cov is not None:
            raise NotImplementedError(self.likelihood.refuses_full_cov)
        X2 = X[0] if X.dim() == 3 else X
        self._require_gpu(X2)
        if not diagonal:
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
        mu, v = self._qf_one(X2)
        if self._has_mean:           # mu + m(X) (sparse_MF_SP.py:355,360): every method downstream of (mu, v) gets it from here
            if torch.is_grad_enabled() and X2.requires_grad:       # (the mean's slope reaches X through MeanFunction's g_X)
                mu = mu + self.mean_function.vector(X2)
            elif torch.is_grad_enabled() and (mu.requires_grad or any(q.requires_grad for q in self.mean_function.parameters())):
                mu = mu + self.mean_function.vector(X2.detach())
            else:
                mu = self.mean_function.vector(X2.detach(), inp=mu)
        return mu.reshape(1, -1, 1), v.reshape(1, -1, 1)

    def _kl_one(self, c=None):
        """KL(q(u) || p(u)) of latent GP c (None: the only one), 0-d.  Whitened (sparse_MF_SP.py:406-431): differentiable in
        (m, L_q) like the reference's.  Unwhitened (:433-453): p(u) = N(0, K_ZZ + j I) from add_jitter_MultivariateNormal, which
        adds at least 1e-8 (ladder 1e-8 * 10^i, i < 5); equal to the whitened KL at unwhiten(m, L_q; j) and differentiable in Z
        and the kernel parameters too."""
        if self.is_whiten:
            m, Lam = self.q_U.variational_mean[c or 0], self.q_U.chol_variational_covar[c or 0]
        else:
            _, _, _, m, Lam, _ = self._gp_params(c, jitter=ops.KL_PRIOR_JITTERS[0], ladder=ops.KL_PRIOR_JITTERS)
        if torch.is_grad_enabled() and (m.requires_grad or Lam.requires_grad):
            return ops.KlFunction.apply(m, Lam).reshape(())
        return ops.kl_whitened(m.detach(), Lam.detach())[0].reshape(())

    def KLD(self):
        """KL(q(u) || p(u)), shape (Dy,): one _kl_one per latent GP."""
        if self._is_composed:
            return torch.stack([self._kl_one(c) for c in range(self.out_dim)])
        return self._kl_one().reshape(1)

    def ELBO(self, X, Y, _qu_jitter=None):
        """Returns (ELBO, ELL, KLD): positive ELBO with autograd, the trainer negates (sparse_MF_SP.py:552-598).
        `_qu_jitter` (collapsed_bound and the trainer's natgrad loop): q(u) enters as a constant and the step starts at this jitter."""
        X2 = X[0] if X.dim() == 3 else X
        self._require_gpu(X2)
        assert Y.dim() == 2 and Y.shape[1] == 1, "Y must be (MB, 1)"
        if self._is_composed:
            assert _qu_jitter is None
            return self._elbo_composed(X2, Y)
        self.likelihood.check_targets(Y)          # (a count model: counts only; the kernels themselves take any real >= 0)
        info = {}
        Z, rl, ro, m, Lam, lvn = self._gp_params(info=info)
        if _qu_jitter is not None:
            m, Lam = m.detach(), Lam.detach()
        spec, theta, rowp = self._flow_inputs(X2, with_grad=True)
        cfg = self._cfg
        cfg.update(N_total=self.N, flow=spec, S=self.quad_points, check_status=(cg.status_check == "always"),
                   global_jitter=cg.global_jitter, kernel=self.covariance_function.hip_kernel,
                   grad_Y=False, **self.likelihood.lik_kwargs())
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
        lik = self.likelihood
        if lik.refuses_optimal_qu is not None:
            return lik.refuses_optimal_qu_id if lik.refuses_optimal_qu_id is not None and self._input_dependent else lik.refuses_optimal_qu
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
            if self.likelihood.flow_on_targets:
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

    # ---- natural-gradient steps of q(u): any likelihood of one latent GP -----------------------------------
    def _natgrad_refusal(self):
        """Why this model has no natural-gradient step of q(u), or None.  The step is built for one whitened latent GP with a
        zero prior mean whose likelihood sees f through shared parameters only."""
        lik = self.likelihood
        if lik.num_latent > 1:
            return ("a likelihood of %d coupled latent GPs (%s): the step is built for one latent GP"
                    % (lik.num_latent, type(lik).__name__))
        if lik.flow_on_targets:
            return ("the warped likelihood is Gaussian in f on the warped targets: set_optimal_qu gives the exact optimum of "
                    "q(u) in one step")
        if not self.is_whiten:
            return "is_whiten=False: the step is built for the whitened q(u) only"
        if self.fully_bayesian:
            return "be_fully_bayesian: the step needs the flow's parameters without dropout noise"
        if self._input_dependent:
            return "input-dependent flows (ID_TGP): the step is built for shared flow parameters"
        if self._has_mean:
            return "a non-zero mean function: the step is built for the zero prior mean"
        return None

    def natgrad_step_qu(self, X, Y, lr=1.0, site_floor=0.0):
        """One natural-gradient step of q(u) at the current hyper-parameters and for these rows, step size `lr` in (0, 1], written
        into q_U (no autograd): ops.qf_moments -> the likelihood's own ops.ell_* launch at scale N / MB, whose g_mu, g_v are the
        per-row adjoints -> ops.natgrad_qu at the jitter the moments ended with.  With the Gaussian likelihood and lr = 1 it is
        set_optimal_qu; for the others a damped Newton step on q(u) that needs no learning rate for m and Lam.  `site_floor`
        clamps the per-row precisions from below (0.0 keeps P' positive definite for every likelihood; None: no floor, and a
        likelihood that is not log-concave may raise ops.NotPSDError -- q_U is left as it was then).  The `df` key of the
        likelihood's lik_kwargs() is the slot for what rides beside the noise (ops.noise_slot): the Student-t's degrees of
        freedom, the ordinal likelihood's bin edges.  Returns the `info` dict
        (info["jitter"]).  NotImplementedError, naming the reason, for the models the step is not built for."""
        why = self._natgrad_refusal()
        if why is not None:
            raise NotImplementedError("natgrad_step_qu: " + why)
        X2 = X[0] if X.dim() == 3 else X
        self._require_gpu(X2)
        self.likelihood.check_targets(Y)
        info = {}
        kern = self.covariance_function.hip_kernel
        ladder = ops.jitter_ladder(jitter=cg.global_jitter)
        with torch.no_grad():
            Z, rl, ro, m, Lam, lvn = (None if t is None else t.detach().contiguous() for t in self._raw_params())
            X2 = X2.detach()
            spec, theta, rowp = self._flow_inputs(X2, with_grad=False)
            theta = None if theta is None else theta.detach()
            y = Y.detach().reshape(-1).to(Z.dtype).contiguous()
            jit = 0.0
            while True:
                # moments, sites and the step share one factor of K_ZZ: where the step's ladder climbs past the jitter the moments
                # ended with, they are formed again there (a finite ladder: the jitter only rises)
                mu, v = ops.qf_moments(X2, Z, rl, ro, m, Lam, jitter=jit, kernel=kern, info=info)
                jit = info["jitter"]
                res = ops._ell_rows(y, mu, v, lvn if self.likelihood.has_noise else None, spec, theta, self.quad_points, rowp,
                                    scale=self.N / y.numel(), **self.likelihood.lik_kwargs())
                m_new, Lam_new = ops.natgrad_qu(X2, Z, rl, ro, m, Lam, mu, res["g_mu"], res["g_v"], rho=float(lr),
                                                site_floor=site_floor, jitter=jit, kernel=kern, info=info, ladder=ladder)
                if info["jitter"] == jit:
                    break
                jit = info["jitter"]
            self.q_U.variational_mean.data[0].copy_(m_new)
            self.q_U.chol_variational_covar.data[0].copy_(Lam_new)
        return info

    def check_status(self):
        """Lazy Cholesky status check (cg.status_check = 'lazy'): raises like psd_safe_cholesky would have."""
        st = self._cfg.get("last_status")
        if st is not None and ops.raise_for_status(st.cpu()):
            raise ops.NotPSDError("K_MM was not positive definite in the last ELBO call (pivot %d)" % int(st[0]))

    def ELL(self, X, Y, mean, cov):
        """N/MB * E_q(f)[log p(y|G(f))] from given moments (sparse_MF_SP.py:601-626); no autograd."""
        MB = Y.size(0)
        if self._is_composed and X.dim() == 2:
            X = X.unsqueeze(0).expand(self.likelihood.flow_outputs, -1, -1)
        ell = self.likelihood.expected_log_prob(Y.t(), mean.squeeze(dim=2), cov.squeeze(dim=2), flow=self.G_matrix, X=X)
        return self.N / MB * ell

    def _eval_mode(self):
        self.eval()
        if self.fully_bayesian:
            assert enable_eval_dropout(self.modules()), "fully bayesian mode needs dropout layers in the flow"

    def predictive_distribution(self, X, diagonal: bool = True, S_MC_NNet: int = None):
        """m1, m2 (Dy, MB) + q(f) moments (sparse_MF_SP.py:457-540)."""
        assert not self.is_training, "This method only works in eval mode"
        lik = self.likelihood
        if not diagonal and lik.refuses_full_cov_predictive is not None:
            raise NotImplementedError(lik.refuses_full_cov_predictive)
        assert diagonal
        if lik.composed:             # the moments of all latent GPs into the likelihood's one launch
            m1, m2, _, mean_q_f, cov_q_f = self._predict_rows(X[0] if X.dim() == 3 else X)
            return m1, m2, mean_q_f, cov_q_f
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
                mY, cY, _ = ops.predict(mean_q_f.reshape(-1).repeat(S), cov_q_f.reshape(-1).repeat(S),
                                        self._noise.detach().contiguous(), spec, theta.detach() if theta is not None else None,
                                        self.quad_points, rowp, **lik.lik_kwargs())
                if lik.kind == "classifier":     # P of every (sample, row), the MC mean per row (sparse_MF_SP.py:521-525)
                    self.train()
                    return mY.reshape(S, MB, 1).mean(0), None, mean_q_f, cov_q_f
                mY, cY = mY.reshape(1, S, MB), cY.reshape(1, S, MB)       # (Dy, S, MB)
                m1 = mY.mean(1)
                m2 = (cY + mY ** 2).mean(1) - m1 ** 2
            else:                    # (a classifier gives P(y = 1) of shape (MB, 1) alone)
                res = lik.marginal_moments(mean_q_f.squeeze(2), cov_q_f.squeeze(2), diagonal=True, flow=self.G_matrix, X=X3)
                m1, m2 = (res, None) if lik.kind == "classifier" else res
        self.train()
        return m1, m2, mean_q_f, cov_q_f

    def test_log_likelihood(self, X, Y, return_moments: bool, Y_std, S_MC_NNet: int = None):
        """log p(Y*|X*) summed over the batch, shape (Dy,), and optionally [m1, m2] (sparse_MF_SP.py:637-825)."""
        assert not self.is_training, "This method only works in eval mode"
        MB = X.size(0)
        X3 = X.repeat(self.out_dim, 1, 1) if X.dim() == 2 else X
        self._require_gpu(X3)
        lik = self.likelihood
        if lik.one_launch_logp:
            # sum_n log p(y_n | x_n) with [m1, m2] from the same launch: the exact log predictive density of the raw targets,
            # every constant and -log Y_std (Student-t; heteroscedastic: under the S x S product rule), the log predictive pmf
            # of the observed counts (Poisson: counts have no scale, Y_std is not used), log P[n, y_n] in float64 (multi-class:
            # the reference goes through float32 and compute_calibration_measures)
            ystd = float(Y_std.reshape(-1)[0]) if lik.kind == "regression" else 1.0
            m1, m2, lp, _, _ = self._predict_rows(X3[0], Y, ystd, want_moments=return_moments)
            assert lik.kind != "classifier" or torch.isfinite(lp).all(), "Got saturated probabilities"
            if not return_moments:
                return lp.sum().reshape(1), None
            return lp.sum().reshape(1), ([m1] if m2 is None else [m1.reshape(1, MB), m2.reshape(1, MB)])
        if lik.kind == "classifier":
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
        predictive_params, qf = None, None
        if return_moments:
            m1, m2, *qf = self.predictive_distribution(X3, diagonal=True, S_MC_NNet=S_MC_NNet)
            predictive_params = [m1, m2]
        ystd = float(Y_std.reshape(-1)[0])
        if lik.refuses_optimal_qu is None:
            # Gaussian in f, on the targets or on the warped ones: log N(y | mu, v + s2), or the exact warped predictive density
            # log N(T(y) | mu, v + s2) + log T'(y), - log Y_std, summed over the rows (the reference's branch for the warped class
            # would give log N(y | m1, m2): DESIGN.md 8; its moments cost S flow inversions per row and are not asked for again)
            lp = self._predict_rows(X3[0], Y, ystd, want_moments=not lik.flow_on_targets, qf=qf)[2]
            return lp.sum().reshape(1), predictive_params
        self._eval_mode()
        with torch.no_grad():
            mean_q_f, cov_q_f = qf if qf is not None else self.marginal_variational_qf_parameters(X3, diagonal=True,
                                                                                                  is_duvenaud=False)
            mu, v = mean_q_f.reshape(-1).contiguous(), cov_q_f.reshape(-1).contiguous()
            lvn = self.likelihood.log_var_noise.detach().reshape(-1)[:1].contiguous()
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
    def predictive_pmf(self, X, kmax: int):
        """The predictive pmf of a count or ordinal model at the rows of X (N, Dx): P of shape (N, kmax + 1), P[n, k] =
        p(y_n = k | x_n), the exponential of tgp_predict_f64's log pmf from one launch over N (kmax + 1) rows (block k asks for the
        count, or class, k).  Rows sum to 1 once kmax is past the mass (an ordinal model of K classes: kmax = K - 1); P.cumsum(1)
        is the predictive CDF, from which count intervals and the median class are read."""
        if self.likelihood.kind != "count":
            raise NotImplementedError("predictive_pmf: a count (Poisson, negative-binomial) or ordinal likelihood only; %s models "
                                      "have predictive_quantiles or class probabilities" % type(self.likelihood).__name__)
        assert X.dim() == 2, "Invalid input X.shape"
        kmax = int(kmax)
        assert kmax >= 0, "kmax must be >= 0"
        N = X.shape[0]
        k = torch.arange(kmax + 1, dtype=X.dtype, device=X.device).repeat_interleave(N)
        lp = self._predict_rows(X, k, want_moments=False)[2]       # block k of the launch asks for the count k
        return torch.exp(lp).reshape(kmax + 1, N).t().contiguous()

    # ---- exact quantiles and CDF of the predictive / posterior marginals -----------------------------------
    def _quantile_inputs(self, X, what):
        """Eval-mode q(f) moments (mu, v of shape (N,)), the noise and the flow inputs of the rows of X, under no_grad."""
        lik, name = self.likelihood, type(self.likelihood).__name__
        if what == "predictive_crps":        # (its own reasons; the other values of `what` have theirs below)
            if lik.kind == "classifier":
                raise NotImplementedError("predictive_crps: a %s model predicts classes, which have no CRPS" % name)
            why = lik.refuses_crps % name if lik.refuses_crps is not None else None
            if why is None and self.fully_bayesian:
                why = "the fully Bayesian model is an MC-dropout mixture over parameter draws, which the kernel does not sum"
            if why is not None:
                raise NotImplementedError("predictive_crps: %s; pass samples=S for the sampled estimator "
                                          "(ops.crps_from_samples of S predictive draws)" % why)
        if lik.kind == "classifier":
            raise NotImplementedError("%s: a %s model has no quantiles" % (what, name))
        if lik.refuses_cdf is not None and what != "posterior_quantiles":
            raise NotImplementedError(lik.refuses_cdf % what)
        if self.fully_bayesian:
            raise NotImplementedError("%s: the fully Bayesian model (an MC-dropout mixture over parameter draws) is out of "
                                      "scope; use the sampled intervals" % what)
        assert X.dim() == 2, "Invalid input X.shape"
        if what != "posterior_quantiles" and hasattr(lik, "check_shape"):
            lik.check_shape()     # (a Gamma model: ValueError once the trained shape has left the range the root rule covers)
        if what != "posterior_quantiles" and hasattr(lik, "check_precision"):
            lik.check_precision()     # (a Beta model: the same of its precision)
        self._eval_mode()
        with torch.no_grad():
            mean_q_f, cov_q_f = self.marginal_variational_qf_parameters(X.repeat(self.out_dim, 1, 1), diagonal=True,
                                                                        is_duvenaud=False)
            # (of two latent GPs, output 0: f, the one that goes through the flow)
            mean_q_f, cov_q_f = mean_q_f[:lik.flow_outputs], cov_q_f[:lik.flow_outputs]
            spec, theta, rowp = self._flow_inputs(X, with_grad=False)
        lvn = self._noise.detach().reshape(-1)[:1].contiguous()
        theta = theta.detach() if theta is not None else None
        return mean_q_f.reshape(-1).contiguous(), cov_q_f.reshape(-1).contiguous(), lvn, spec, theta, rowp

    def predictive_quantiles(self, X, probs):
        """Exact quantiles of p(y* | x*) at the rows of X, shape (Dy, Q, N), in the model's standardised units: the roots of
        the Gauss-Hermite predictive CDF (ops.predict_quantiles); the Gaussian likelihood's closed form; a warped model's
        T^-1(mu + zq sqrt(v + noise)); a Gamma model's are those of its mixture of Gammas (ValueError if the trained shape has
        left [lib.GAMMA_MIN_SHAPE, lib.GAMMA_MAX_SHAPE]); a Beta model's those of its mixture of Betas, inside (0, 1) (ValueError if
        the trained precision has left [lib.BETA_MIN_PRECISION, lib.BETA_MAX_PRECISION]).  probs: any order, each strictly inside (0, 1)."""
        mu, v, lvn, spec, theta, rowp = self._quantile_inputs(X, "predictive_quantiles")
        with torch.no_grad():
            if self.likelihood.flow_on_targets:
                _, zq = ops.quantile_probs(probs, mu.device)
                t = mu.unsqueeze(0) + zq.unsqueeze(1) * torch.sqrt(v.clamp_min(0.0) + torch.exp(lvn)).unsqueeze(0)
                q, _ = ops.flow_inverse(t, spec, theta)
            else:
                q = ops.predict_quantiles(mu, v, lvn, probs, spec, theta, self.quad_points, rowp, lik=self._lik_id)
        self.train()
        return q.unsqueeze(0)

    def posterior_quantiles(self, X, probs):
        """Quantiles of G(f0) under q(f0) at the rows of X, shape (Dy, Q, N): exact, G is increasing, so they are
        G(mu + zq sqrt(v)).  (A warped model's latent function carries no flow: mu + zq sqrt(v).)"""
        mu, v, lvn, spec, theta, rowp = self._quantile_inputs(X, "posterior_quantiles")
        with torch.no_grad():
            _, zq = ops.quantile_probs(probs, mu.device)
            f = mu.unsqueeze(0) + zq.unsqueeze(1) * torch.sqrt(v.clamp_min(0.0)).unsqueeze(0)
            if spec is not None and spec.nblk > 0 and not self.likelihood.flow_on_targets:
                f = ops.flow_eval(f.contiguous(), spec, theta, rowp, want=("G",))["G"]
        self.train()
        return f.unsqueeze(0)

    def posterior_input_gradients(self, X):
        """(dmu, dv), each (Dy, N, D): the derivatives of the q(f) marginals mu_c(x_n), v_c(x_n) that
        marginal_variational_qf_parameters reports in the row x_n, one tgp_qf_input_grad_f64 call per latent GP (a multi-class
        model: Dy = C; a heteroscedastic one: f and h) -- the unwhitened q(u) through its transform, the mean function's own
        slope (linear: a, identity: W) added to dmu.  Eval mode, no autograd, then train(), as every prediction."""
        X2 = X[0] if X.dim() == 3 else X
        self._require_gpu(X2)
        self._eval_mode()
        kern = self.covariance_function.hip_kernel
        with torch.no_grad():
            Xd = X2.detach().contiguous()
            parts = []
            for c in (range(self.out_dim) if self._is_composed else (None,)):
                info = {}
                Z, rl, ro, m, Lam, _ = self._gp_params(c, info=info)
                parts.append(ops.qf_input_grad(Xd, *(t.detach() for t in (Z, rl, ro, m, Lam)), jitter=info["jitter"], kernel=kern))
            dmu, dv = torch.stack([p[0] for p in parts]), torch.stack([p[1] for p in parts])
            if self._has_mean:
                dmu = dmu + self.mean_function._ab()[0].detach().reshape(1, 1, -1)
        self.train()
        return dmu, dv

    def posterior_derivative(self, X):
        """(mean, var), each (Dy, N, D): the moments under q(f) of the derivative process d f_c(x_n) / d x_nd.  `mean` is
        posterior_input_gradients' dmu (the mean function's slope included); `var` is Var_q[d_d f_c(x_n)] = k_g(0) / l_d^2 +
        J_d^T L^-T W L^-1 J_d, one tgp_qf_input_grad_var_f64 call per latent GP through the same parameters -- the unwhitened
        q(u) through its transform, a multi-class model's C latents, a heteroscedastic one's (f, h).  var is stored as computed
        (rounding can leave a tiny negative): clamp at 0 where a square root is taken.  Eval mode, no autograd, then train()."""
        X2 = X[0] if X.dim() == 3 else X
        mean = self.posterior_input_gradients(X2)[0]
        self._eval_mode()
        kern = self.covariance_function.hip_kernel
        with torch.no_grad():
            Xd = X2.detach().contiguous()
            parts = []
            for c in (range(self.out_dim) if self._is_composed else (None,)):
                info = {}
                Z, rl, ro, m, Lam, _ = self._gp_params(c, info=info)
                parts.append(ops.qf_input_grad_var(Xd, *(t.detach() for t in (Z, rl, ro, m, Lam)), jitter=info["jitter"],
                                                   kernel=kern))
            var = torch.stack(parts)
        self.train()
        return mean, var

    def predictive_input_gradients(self, X, Y_std=None):
        """{"m1": (N, D), "m2": (N, D)}: the gradients in x_n of the predictive mean and variance predictive_distribution reports
        at the rows of X -- the chain rule of ops.predict_moment_grads (the partials of the moments in mu and v, through the
        flow) with posterior_input_gradients -- in the model's standardised units, or scaled by Y_std and Y_std^2 when Y_std is
        given.  The Gaussian and flow regression likelihoods only."""
        lik = self.likelihood
        if lik.lik_id is not None or lik.composed:
            raise NotImplementedError("predictive_input_gradients: the Gaussian and flow regression likelihoods only; the "
                                      "predictive moments of the %s likelihood are not a Gaussian's around the flow, and "
                                      "tgp_predict_moment_grads_f64 has no partials for them"
                                      % (lik.display or type(lik).__name__))
        if self._input_dependent:
            raise NotImplementedError("predictive_input_gradients: the model has input-dependent flows -- their per-row "
                                      "parameters depend on x through the networks, and that path has no input gradient")
        if self.fully_bayesian:
            raise NotImplementedError("predictive_input_gradients: the fully Bayesian model is an MC-dropout mixture over "
                                      "parameter draws, which has no input gradient here")
        X2 = X[0] if X.dim() == 3 else X
        dmu, dv = self.posterior_input_gradients(X2)
        mu, v, lvn, spec, theta, rowp = self._quantile_inputs(X2.detach(), "predictive_input_gradients")
        with torch.no_grad():
            dm1, dm2 = ops.predict_moment_grads(mu, v, lvn, spec, theta, self.quad_points, rowp)
            out = {"m1": dm1[0].unsqueeze(1) * dmu[0] + dm1[1].unsqueeze(1) * dv[0],
                   "m2": dm2[0].unsqueeze(1) * dmu[0] + dm2[1].unsqueeze(1) * dv[0]}
            if Y_std is not None:
                s = float(Y_std)
                out = {"m1": out["m1"] * s, "m2": out["m2"] * (s * s)}
        self.train()
        return out

    ACQUISITION_KINDS = ("ei", "log_ei", "pi", "ucb")

    def acquisition(self, X, kind="log_ei", best=None, maximize=True, beta=2.0, return_grad=False):
        """An acquisition function of Bayesian optimisation at the rows of X (N, D), in the model's standardised units: (N,), or
        ((N,), (N, D)) with return_grad, the second its gradient in x_n.  With c = +1 when `maximize`, else -1, and the incumbent
        `best` (the best target seen so far, standardised; the model does not keep its training targets, so it must be given):
          "ei"      the expected improvement E[(c (y - best))_+] under the predictive predictive_distribution reports
          "log_ei"  its logarithm, finite (and with a useful gradient) where EI underflows
          "pi"      the probability of improvement P(c (y - best) > 0)
          "ucb"     m1 + c beta sqrt(m2), the confidence bound of the predictive moments (needs no `best`)
        The first three are one tgp_predict_acquisition_f64 launch, the gradient formed in it from posterior_input_gradients'
        Jacobians; "ucb" is composed from ops.predict and ops.predict_moment_grads.  The Gaussian and flow regression
        likelihoods, one output; with return_grad neither input-dependent flows nor the fully Bayesian mode.  Eval mode, no
        autograd, then train(), as every prediction."""
        lik = self.likelihood
        if kind not in self.ACQUISITION_KINDS:
            raise ValueError("acquisition: kind must be one of %s, got %r" % (", ".join(map(repr, self.ACQUISITION_KINDS)), kind))
        if best is None and kind != "ucb":
            raise ValueError("acquisition: kind=%r needs best=, the incumbent target in standardised units (the model does "
                             "not keep its training targets)" % kind)
        if lik.lik_id is not None or lik.composed:
            raise NotImplementedError("acquisition: the Gaussian and flow regression likelihoods only; the predictive of the %s "
                                      "likelihood is not a Gaussian's around the flow, and tgp_predict_acquisition_f64 has no "
                                      "improvement terms for it" % (lik.display or type(lik).__name__))
        if self.out_dim != 1:
            raise NotImplementedError("acquisition: one output only (the model has %d): an improvement is that of one target"
                                      % self.out_dim)
        if return_grad and self._input_dependent:
            raise NotImplementedError("acquisition: the model has input-dependent flows -- their per-row parameters depend "
                                      "on x through the networks, and that path has no input gradient (values: "
                                      "return_grad=False)")
        if return_grad and self.fully_bayesian:
            raise NotImplementedError("acquisition: the fully Bayesian model is an MC-dropout mixture over parameter draws, "
                                      "which has no input gradient here")
        X2 = X[0] if X.dim() == 3 else X
        c = 1.0 if maximize else -1.0
        dmu = dv = None
        if return_grad:
            dmu, dv = self.posterior_input_gradients(X2)
            dmu, dv = dmu[0].contiguous(), dv[0].contiguous()
        mu, v, lvn, spec, theta, rowp = self._quantile_inputs(X2.detach(), "acquisition")
        S = self.quad_points
        with torch.no_grad():
            if kind == "ucb":
                m1, m2, _ = ops.predict(mu, v, lvn, spec, theta, S, rowp)
                sd = torch.sqrt(m2)
                out = m1 + (c * float(beta)) * sd
                if return_grad:
                    dm1, dm2 = ops.predict_moment_grads(mu, v, lvn, spec, theta, S, rowp)
                    a = dm1 + (0.5 * c * float(beta)) * dm2 / sd.unsqueeze(0)
                    out = (out, a[0].unsqueeze(1) * dmu + a[1].unsqueeze(1) * dv)
            else:
                out = ops.predict_acquisition(mu, v, lvn, kind, float(best), spec, theta, S, rowp, maximize=maximize,
                                              jac=(dmu, dv) if return_grad else None)
        self.train()
        return out

    def predictive_cdf(self, X, Y):
        """The predictive CDF at the targets Y (N,1), standardised units: the PIT values of a calibration plot, shape (Dy, N).
        A warped model's is Phi((T(y) - mu) / sqrt(v + noise))."""
        mu, v, lvn, spec, theta, rowp = self._quantile_inputs(X, "predictive_cdf")
        with torch.no_grad():
            y = Y.reshape(-1).to(mu.dtype)
            if self.likelihood.flow_on_targets:
                t = ops.flow_eval(y.contiguous(), spec, theta, want=("G",))["G"] if spec.nblk > 0 else y
                cdf, _ = ops.predict_cdf(mu, v, lvn, t)
            else:
                cdf, _ = ops.predict_cdf(mu, v, lvn, y, spec, theta, self.quad_points, rowp, lik=self._lik_id)
        self.train()
        return cdf.unsqueeze(0)

    def predictive_crps(self, X, Y, Y_std=None, samples=None, kmax=None):
        """The continuous ranked probability score of p(y* | x*) at the targets Y (N,1), shape (Dy, N), in the model's
        standardised units -- or times Y_std when that is given (the CRPS has the units of the target).  Exact through
        ops.predict_crps for whatever predictive_cdf serves through the Gauss-Hermite mixture (Gaussian and flow likelihoods).
        A Poisson model: sum_k (cdf_k - 1{k >= y})^2 over k = 0..kmax from predictive_pmf(X, kmax); kmax is the caller's, as
        for predictive_pmf (past the mass the terms are 0).  samples=S: ops.crps_from_samples of S draws of
        sample_from_predictive_distribution, for any regression model.  Without it Student-t, heteroscedastic, Gamma, Beta, warped and fully
        Bayesian models raise NotImplementedError; Bernoulli and multi-class models always do."""
        count = self.likelihood.kind == "count"
        exact = samples is None and not count
        if exact or self.likelihood.kind == "classifier":
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
        elif count:
            if kmax is None:
                raise ValueError("predictive_crps of a %s model needs kmax, the last count of the sum (predictive_pmf's)"
                                 % self.likelihood.display)
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
        if self.likelihood.refuses_paths is not None:
            raise NotImplementedError(self.likelihood.refuses_paths)
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
            samples = [self.likelihood.sample_from_output(f_k, i).view(S, N, 1) for i in range(self.likelihood.observed_outputs)]
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
