/*
 * tgp_hip.h -- C ABI of libtgp_hip.so: the MI355X (gfx950) implementation of the TGP
 * sparse-variational ELBO hot path (jmaronas/TGP.pytorch, `sparse_MF_SP.ELBO` and below).
 *
 * The reference has no FFI of its own (it is pure Python on ATen); the boundary it offers is the
 * model-class API.  This header is the plain-C surface that sits directly underneath that API:
 * every entry point names the reference call site(s) it replaces (file:line relative to
 * /root/reference/code).  The Python mirror of the reference classes (tgp/pytorch_amd) binds these
 * with ctypes; INTEGRATION.md shows the stub a reference maintainer would add.
 *
 * Conventions
 *   - all matrices row-major, contiguous, float64 (`_f64`; the reference's main.py runs in float64,
 *     dsp/config.py:37-46);
 *   - every pointer is a DEVICE pointer owned by the caller (e.g. torch tensor.data_ptr()), with ONE exception:
 *     tgp_model.program (a few int32 describing the flow) is a HOST array, read during the call;
 *     outputs and the workspace are pre-allocated by the caller, nothing is allocated inside;
 *   - `stream` is a hipStream_t passed as void*; calls are asynchronous and stream-ordered, safe
 *     to capture into a hipGraph, and re-entrant when callers use distinct streams + workspaces + status buffers
 *     (status[4..7] are hand-off words of the launches in flight: two concurrent calls that shared them would pass each
 *     other's waits early);
 *     the general-M path (M > 128 or a non-RBF kernel) forks independent phases onto helper streams that the
 *     library creates at a host thread's first such call and joins before the call returns (event record / wait:
 *     valid under capture of `stream`, where they become parallel branches of the graph) -- make a thread's first
 *     call outside a capture; the helper streams and events are per host thread, so threads never share them;
 *   - return value: 0 = launched; <0 = -(index of the offending argument) or TGP_E_*;
 *     numerical failure is reported ASYNCHRONOUSLY through `status` (device int32[8], ZERO before its first use):
 *       status[0] = LAPACK-style info of the Cholesky of K_MM (0 ok, j>0 = pivot j not positive;
 *                   TGP_STATUS_SYNC_TIMEOUT: a workgroup of the prepare or of the M x M backward launch gave up waiting for a hand-off word --
 *                   the hand-off words were not zero, or its producers never became resident; results invalid),
 *       status[1] = 1 if K_MM contained a NaN (the reference raises NanError, dsp/utils.py:241-254),
 *       status[2] = level of the on-device jitter ladder that succeeded (tgp_model.jitter_ladder),
 *       status[3] = STICKY count of expired hand-off waits: incremented by the launch whose wait expired, never cleared by the
 *                   library (status[0] is rewritten by the next call's prepare launch, so inside a replayed graph of several
 *                   steps a timeout shows only here); a fused-update call (tgp_elbo_step_adam_f64) whose backward launch sees
 *                   the timeout skips the update outside Lam and the step counter and returns NaN scalars; the caller
 *                   zeroes the word after it has handled the event,
 *       status[4..7] = hand-off words between workgroups of ONE launch (M <= 128: the tile blocks of the prepare
 *                   launch count themselves in status[4] once their tile of K_MM is in global memory, status[5] counts
 *                   the blocks that have left; the M x M backward launch counts its finished column blocks in bits 16-23
 *                   and its finished row-block halves in bits 24-31 of status[6], and the blocks that have left in status[7];
 *                   M > 128: the workgroups that produce the diagonal block a factorising workgroup of the same launch
 *                   waits for -- the first block of K_MM, then the trailing update's tiles -- count themselves in status[4]);
 *                   the library leaves them zero at the end of every
 *                   call, the caller must not touch them while a call is in flight.  A caller built against the
 *                   int32[4] status of ABI versions <= 100 must grow the buffer: check tgp_version() >= 101,
 *     so the host can replay with the reference's jitter ladder (dsp/utils.py:256-269) without a
 *     device sync per step.  No exception crosses the ABI.
 */
#ifndef TGP_HIP_H
#define TGP_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TGP_VERSION 104
#define TGP_FUSED_MAX_M 128 /* up to here the whole step is 4 fused kernel launches (operators resident in LDS/registers) */
#define TGP_BIG_MAX_M 4096  /* above: chunked path built on a tiled float64 MFMA GEMM                             */

/* error codes (negative return values below -64 are generic) */
#define TGP_E_UNSUPPORTED (-100) /* shape outside this build's limits (M > 4096, D > 16, ...) */
#define TGP_E_WORKSPACE (-101)   /* workspace too small                                        */
#define TGP_E_LDS (-102)         /* flow program too large for one CU's LDS                    */
#define TGP_E_LAUNCH (-103)      /* hipLaunchKernel failed; see tgp_last_error()               */
#define TGP_E_COMM (-104)        /* RCCL not loaded / an RCCL call failed; see tgp_last_error() */
/* value of status[0] (not a return value): a hand-off wait inside a launch expired (see Conventions) */
#define TGP_STATUS_SYNC_TIMEOUT (-77)

/* ---- flow program (models/flow.py CompositeFlow.forward :155-158) -------------------------------
 * A flow is a sequence of `nblk` blocks; block b is four int32: {kind, K, poff, flags}.
 *   kind   TGP_FLOW_AFFINE   g = a f + b                                   (flow.py:330-340)
 *          TGP_FLOW_SAL      g = sinh(b asinh(f) - a), asinh = log(f+sqrt(f^2+1)) (flow.py:904-905,936-977)
 *          TGP_FLOW_STEPTANH g = [f +] sum_k a_k + sp(b_k) tanh((f-c_k)/sp(d_k)) (flow.py:1096-1103,760-771)
 *          TGP_FLOW_ARCSINH  g = a + b asinh((f-c)/d) [+ f], asinh = log(x+sqrt(x^2+1)) (flow.py:495-521)
 *          TGP_FLOW_BOXCOX   g = (sgn(f)|f|^lam - 1)/lam [+ f]; lam == 0 is taken as 1e-11 (flow.py:377-417)
 *          TGP_FLOW_INV_BOXCOX g = sgn(w)|w|^(1/lam) [+ f], w = lam f + 1 (flow.py:424-443)
 *          (6 is unassigned and refused)
 *          TGP_FLOW_SINH     g = a + b sinh(x) [+ f], x = (f-c)/d; dg/df = (b/d) cosh(x) [+ 1] (flow.py:566-609)
 *          TGP_FLOW_NORMCDF  g = a + b Phi(x) [+ f], x = (f-c)/d; dg/df = (b/d) phi(x) [+ 1], phi = exp(-x^2/2)/sqrt(2 pi)
 *                            (flow.py:1006-1037 with is_learnable=True).  Bounded unless ADD_F0 is set.
 *          TGP_FLOW_TUKEY    g = (e^{gam f} - 1)/gam e^{h f^2/2} (Tukey g-and-h, flow.py:451-492);
 *                            dg/df = e^{h f^2/2} (e^{gam f} + h f (e^{gam f} - 1)/gam); gam == 0 is taken as 1e-11
 *          TGP_FLOW_EXP      g = dg/df = e^f (flow.py:283-294)
 *          TGP_FLOW_SOFTPLUS g = log(1 + e^f), dg/df = e^f/(1 + e^f); g = f, dg/df = 1 for f > 20 (torch's threshold; flow.py:262-276)
 *   K      number of tanh steps (STEPTANH only)
 *   poff   offset of the block's parameters in `theta` (shared scalars: AFFINE {a,b}, SAL {a,b},
 *          STEPTANH {a_k,b_k,c_k,d_k}_k, ARCSINH / SINH / NORMCDF {a,b,c,d}, BOXCOX / INV_BOXCOX {lam}, TUKEY {gam,h},
 *          EXP / SOFTPLUS none) or first column in `rowp` when TGP_FLAG_PER_ROW is set (AFFINE and SAL only; the other
 *          kinds refuse it)
 *   flags  TGP_FLAG_RESTRICT  set_restrictions=True: softplus on AFFINE.a / SAL.b / b and d of ARCSINH, SINH and NORMCDF;
 *                             TUKEY: gam = softplus(raw) (tukey_right); TUKEY's h = softplus(raw) with or without the flag
 *          TGP_FLAG_ADD_F0    add_init_f0=True (refused on TUKEY, EXP and SOFTPLUS: the reference never adds f there)
 *          TGP_FLAG_PER_ROW   input-dependent parameters, one value per data row (flow.py:949-965)
 *          TGP_FLAG_NEGATE    TUKEY only, and only with TGP_FLAG_RESTRICT: gam = -softplus(raw) (tukey_left); refused elsewhere
 * NORMCDF, EXP and SOFTPLUS do not map onto the real line: the warped likelihood (TGP_LIK_WARPED) and tgp_flow_inverse_f64
 * refuse a program that holds one (TGP_E_UNSUPPORTED).
 */
#define TGP_FLOW_AFFINE 0
#define TGP_FLOW_SAL 1
#define TGP_FLOW_STEPTANH 2
#define TGP_FLOW_ARCSINH 3
#define TGP_FLOW_BOXCOX 4
#define TGP_FLOW_INV_BOXCOX 5
#define TGP_FLOW_SINH 7
#define TGP_FLOW_NORMCDF 8
#define TGP_FLOW_TUKEY 9
#define TGP_FLOW_EXP 10
#define TGP_FLOW_SOFTPLUS 11
#define TGP_FLAG_RESTRICT 1
#define TGP_FLAG_ADD_F0 2
#define TGP_FLAG_PER_ROW 4
#define TGP_FLAG_NEGATE 8

/* likelihood selector */
#define TGP_LIK_GAUSS 0 /* GaussianLinearMean.expected_log_prob, likelihoods/GaussianLinearMean.py:60-87       */
#define TGP_LIK_FLOW 1  /* GaussianNonLinearMean.expected_log_prob, likelihoods/GaussianNonLinearMean.py:64-150 */
#define TGP_LIK_ADJOINT 2 /* internal to tgp_qf_moments_bwd_f64: no likelihood, the adjoints of mu, v are inputs */
/* Bernoulli.expected_log_prob / marginal_moments, likelihoods/Bernoulli.py: probit link through the flow,
 * log p(y | f0) = y log Phi(G(f0)) + (1 - y) log Phi(-G(f0)), y in [0, 1], Gauss-Hermite over q(f0) (S, xs, wn required).
 * log_var_noise stays a required pointer; its value is ignored and its gradient is written as 0.  The training step always
 * takes the general-M path.  tgp_predict_f64: m1 = P(y = 1), m2 = P (1 - P), logp = y log P + (1 - y) log(1 - P). */
#define TGP_LIK_BERNOULLI 3
/* WarpedGaussianLinearMean (likelihoods/WarpedGaussianLinearMean.py): the flow T is applied to the TARGETS,
 * log p(y | f) = log N(T(y) | f, exp(log_var_noise)) + log T'(y).  model->program / theta describe T (shared parameters only:
 * RP must be 0 in the training and likelihood entries, TGP_E_UNSUPPORTED otherwise); S, xs, wn serve prediction only.  The
 * training step is [t = T(Y)] -> the unchanged Gaussian step on t (either path) -> [theta's gradient, + scale sum log T'(y) on
 * out[0], out[1]]; tgp_elbo_step_adam_f64 applies the update in ONE separate launch after them.  An empty program gives
 * TGP_LIK_GAUSS's results bit for bit. */
#define TGP_LIK_WARPED 4
/* MulticlassCategorical (likelihoods/MulticlassCategorical.py): softmax over C latent GPs, each through its own flow, Monte
 * Carlo over all C latents of a row.  A documented constant only: the training-step entries are single-output and return
 * TGP_E_UNSUPPORTED for it (tgp_last_error() names the entry to use).  The likelihood is the stand-alone tgp_ell_softmax_f64;
 * a C-output step composes it with tgp_qf_moments_f64 / tgp_qf_moments_bwd_f64 / tgp_kl_whitened_f64 per class. */
#define TGP_LIK_SOFTMAX 5
/* Poisson counts with the flow as the log-rate, y ~ Poisson(exp(G(f0))):
 * log p(y | f0) = y G(f0) - exp(G(f0)) - lgamma(y + 1), y any real >= 0 (the library does not ask for integers), Gauss-Hermite
 * over q(f0) (S, xs, wn required); v <= 0 counts as 0 and its adjoint is 0.  log_var_noise stays a required pointer; its value
 * is ignored and its gradient is written as 0.  The training step always takes the general-M path.  G is not clamped: the
 * results are the float64 formula, and a node whose exp overflows gives -inf as it would in torch.
 * tgp_predict_f64: m1 = E[y] = sum_s wn_s exp(g_s), m2 = Var[y] = m1 + sum_s wn_s exp(2 g_s) - m1^2 (the empty program: the
 * log-normal closed forms), logp = log sum_s wn_s Poisson(y | exp(g_s)), the log predictive pmf, formed as a log-sum-exp so
 * that it stays finite where every term underflows; Y_std is ignored.  The predictive is discrete: the quantile and CDF
 * entries refuse it (TGP_E_UNSUPPORTED). */
#define TGP_LIK_POISSON 6
/* Student-t noise around the flow for robust regression, y | f0 ~ StudentT(nu, loc = G(f0), scale = sigma).  For this likelihood
 * model->log_var_noise points to TWO doubles {eta = log sigma^2, nu}: eta is the log of the squared SCALE (not of the variance,
 * which is sigma^2 nu / (nu - 2)), nu the degrees of freedom, a fixed hyper-parameter.  Supported range 2 < nu <= 1e4 (past it
 * the two lgamma of the constant cancel to ~1e-9 and the Gaussian likelihood is the model to take); the library does not look
 * at nu, which lives on the device.  With r = y - g:
 *   log p(y | g) = lgamma((nu+1)/2) - lgamma(nu/2) - log(nu pi)/2 - eta/2 - (nu+1)/2 log1p(r^2 / (nu sigma^2))
 *   d log p / dg = (nu+1) r / (nu sigma^2 + r^2),   d log p / d eta = -1/2 + (nu+1) r^2 / (2 (nu sigma^2 + r^2)),
 * double-precision pi, g not clamped, Gauss-Hermite over q(f0) (S, xs, wn required); v <= 0 counts as 0 and its adjoint is 0.
 * Gradients: grads->log_var_noise stays ONE double, d/d eta (as out[1] of tgp_ell_flow_f64); nu has no gradient and nothing is
 * written for it.  The training step always takes the general-M path.
 * tgp_predict_f64, in the standardised units of the other regression likelihoods: m1 = sum_s wn_s g_s, m2 = sum_s wn_s g_s^2 -
 * m1^2 + sigma^2 nu / (nu - 2) (+inf for nu <= 2), logp = log sum_s wn_s t_nu(y | g_s, sigma) - log Y_std, the exact log
 * predictive density of the raw target WITH every constant, formed as a log-sum-exp.  The empty program runs the same sum.
 * The quantile and CDF entries refuse it (TGP_E_UNSUPPORTED): the CDF needs the incomplete beta function. */
#define TGP_LIK_STUDENT 7
/* Heteroscedastic Gaussian noise around the flow, y ~ N(G(f), exp(c + h)): f is latent GP 0 (through the flow), h latent GP 1 (no
 * flow), c = log_var_noise[0] the prior mean of the log-variance.  A documented constant only, like TGP_LIK_SOFTMAX: every
 * single-output entry (tgp_elbo_step_f64 and its phases / Adam variants, tgp_optimal_qu_f64, tgp_ell_flow_f64, tgp_predict_f64,
 * tgp_predict_quantile_f64, tgp_predict_cdf_f64) returns TGP_E_UNSUPPORTED for it and tgp_last_error() names the entries to use:
 * tgp_ell_hetero_f64, composed with tgp_qf_moments_f64 / tgp_qf_moments_bwd_f64 / tgp_kl_whitened_f64 per latent GP, and
 * tgp_predict_hetero_f64. */
#define TGP_LIK_HETERO 8
/* Negative-binomial counts with the flow as the log-mean, y ~ NB(mean = exp(G(f0)), dispersion r): Var[y | f0] = mean + mean^2 / r,
 * r -> inf the Poisson.  log_var_noise[0] = lambda = log r, a TRAINED parameter in the noise slot.  Supported range
 * 1e-3 <= r <= 1e3: the terms of d/dlambda cancel as r grows (relative error of the float64 formula 1e-11 at r = 50, 2e-10 at
 * 1e3, 2e-7 at 1e4), and past 1e3 TGP_LIK_POISSON is the model to take; the library does not look at r, which lives on the
 * device.  With g = G(f0), u = g - lambda and sp(u) = log(1 + e^u), evaluated as u > 0 ? u + log1p(e^-u) : log1p(e^u):
 *   log p(y | g)      = lgamma(y + r) - lgamma(r) - lgamma(y + 1) + y u - (y + r) sp(u)
 *   d log p / dg      = y - (y + r) sigmoid(u)                     ( = r (y - mean) / (r + mean) )
 *   d log p / dlambda = r [psi(y + r) - psi(r)] - r sp(u) - d log p / dg,      psi the digamma function,
 * y any real >= 0 (the library does not ask for integers), g not clamped, Gauss-Hermite over q(f0) (S, xs, wn required); v <= 0
 * counts as 0 and its adjoint is 0.  Gradients: grads->log_var_noise is ONE double, d/dlambda (as out[1] of tgp_ell_flow_f64).
 * The training step always takes the general-M path.
 * tgp_predict_f64: m1 = E[y] = sum_s wn_s exp(g_s), m2 = Var[y] = m1 + (1 + 1/r) sum_s wn_s exp(2 g_s) - m1^2 (the empty program:
 * the log-normal closed forms E[mean] = exp(mu + v/2), E[mean^2] = exp(2 mu + 2 v)), logp = log sum_s wn_s NB(y | exp(g_s), r),
 * the log predictive pmf, formed as a log-sum-exp so that it stays finite where every term underflows; Y_std is ignored.  The
 * predictive is discrete: the quantile, CDF and CRPS entries refuse it (TGP_E_UNSUPPORTED). */
#define TGP_LIK_NEGBIN 9
/* Ordered categories through the flow (cumulative probit), y in {0, .., K-1}, 2 <= K <= 64, with K-1 strictly increasing FIXED bin
 * edges b_1 < .. < b_{K-1} (b_0 = -inf, b_K = +inf) and noise of scale sigma on the latent side: for this likelihood
 * model->log_var_noise points to K+1 doubles {eta = log sigma^2, K, b_1, .., b_{K-1}}; eta is trained, K and the edges are fixed
 * hyper-parameters.  The library does not look at them (they live on the device): the host layer checks that the edges are finite
 * and increasing and that 2 <= K <= 64.  With g = G(f0), u = (b_{y+1} - g) / sigma and l = (b_y - g) / sigma:
 *   log p(y | g)     = log(Phi(u) - Phi(l))
 *   d log p / dg     = (phi(l) - phi(u)) / (sigma (Phi(u) - Phi(l)))
 *   d log p / d eta  = (l phi(l) - u phi(u)) / (2 (Phi(u) - Phi(l)))           (the terms of an infinite edge are 0),
 * formed on the side where both tails are small and through erfcx, so that all three stay finite however far g is from the bin.
 * The class is y clamped into [0, K-1]; a y that is not >= 0 (NaN included) counts as 0: no target makes a kernel read past the
 * K-1 edges.  Gauss-Hermite over q(f0) (S, xs, wn required); v <= 0 counts as 0 and its adjoint is 0.  Gradients:
 * grads->log_var_noise stays ONE double, d/d eta (as out[1] of tgp_ell_flow_f64); K and the edges have no gradient and nothing
 * is written for them.  The training step always takes the general-M path.
 * tgp_predict_f64: m1 = E[y] = sum_s wn_s sum_j (1 - Phi_j(g_s)), m2 = Var[y] = sum_s wn_s sum_j (2j - 1)(1 - Phi_j(g_s)) - m1^2 with
 * Phi_j(g) = Phi((b_j - g) / sigma), j = 1 .. K-1; logp = log sum_s wn_s p(y | g_s), the log predictive pmf, formed as a
 * log-sum-exp.  The empty program is closed: P(y <= k) = Phi((b_{k+1} - mu) / sqrt(sigma^2 + max(v, 0))).  Y_std is ignored (classes
 * have no units).  The predictive is discrete: the quantile, CDF and CRPS entries refuse it (TGP_E_UNSUPPORTED). */
#define TGP_LIK_ORDINAL 10
/* Gamma noise with a log link for positive targets, y > 0, y | f0 ~ Gamma(shape a, mean exp(G(f0))): rate a exp(-g), Var[y | f0] =
 * exp(2 g) / a, the variance proportional to the squared mean.  log_var_noise[0] = lambda = log a, a TRAINED parameter in the
 * noise slot.  Supported range TGP_GAMMA_MIN_SHAPE <= a <= TGP_GAMMA_MAX_SHAPE: below it the extreme quantiles leave the double
 * range (a = 0.01, p = 1e-6: log t ~ -1377); the library does not look at a, which lives on the device.  With g = G(f0),
 * l = log y and z = l - g:
 *   log p(y | g)      = [a log a - lgamma(a) - l] + a (z - e^z)
 *   d log p / dg      = a (e^z - 1)
 *   d log p / dlambda = a (log a + 1 - psi(a)) + a (z - e^z),      psi the digamma function,
 * g not clamped (a node whose e^z overflows gives -inf, as the float64 formula does), Gauss-Hermite over q(f0) (S, xs, wn
 * required); v <= 0 counts as 0 and its adjoint is 0.  The library does not check y > 0 (log y of such a target is -inf or
 * NaN).  Gradients: grads->log_var_noise is ONE double, d/dlambda (as out[1] of tgp_ell_flow_f64).  The training step always
 * takes the general-M path.
 * tgp_predict_f64: m1 = E[y] = sum_s wn_s exp(g_s), m2 = Var[y] = (1 + 1/a) sum_s wn_s exp(2 g_s) - m1^2 (the empty program: the
 * log-normal closed forms E[mean] = exp(mu + v/2), E[mean^2] = exp(2 mu + 2 v)), logp = log sum_s wn_s Gamma(y | a, a e^-g_s)
 * - log Y_std, formed as a log-sum-exp: a Gamma family is closed under scaling, so this is the density of the raw target when
 * the targets were divided by Y_std and not centred.
 * The predictive is a location family in log y: tgp_predict_cdf_f64 and tgp_predict_quantile_f64 serve it (below);
 * tgp_predict_crps_f64 refuses it (a mixture of Gammas has no closed pair term). */
#define TGP_LIK_GAMMA 11
#define TGP_GAMMA_MIN_SHAPE 0.1
#define TGP_GAMMA_MAX_SHAPE 1e3
/* most terms of the power series / continued fraction of the regularised incomplete gamma function (tgp_quantile.hip) */
#define TGP_GAMMA_PQ_MAXIT 2048
/* Beta noise with a logit link for proportions, 0 < y < 1, y | f0 ~ Beta(mu phi, (1 - mu) phi) with mu = sigmoid(G(f0)): the flow's
 * value is the log-odds of the mean, phi the precision, Var[y | f0] = mu (1 - mu) / (1 + phi).  log_var_noise[0] = lambda =
 * log phi, a TRAINED parameter in the noise slot.  Supported range TGP_BETA_MIN_PRECISION <= phi <= TGP_BETA_MAX_PRECISION; the
 * library does not look at phi, which lives on the device.  With g = G(f0), ly = log y, l1 = log1p(-y), y* = ly - l1,
 * a = mu phi and b = (1 - mu) phi, 1 - mu formed as sigmoid(-g) so that neither a nor b loses digits at large |g|:
 *   log p(y | g)      = lgamma(phi) - lgamma(a) - lgamma(b) + a y* + phi l1 - ly - l1
 *   d log p / dg      = mu (1 - mu) phi [y* - psi(a) + psi(b)]
 *   d log p / dlambda = phi [psi(phi) - mu psi(a) - (1 - mu) psi(b) + mu y* + l1],      psi the digamma function,
 * g not clamped, Gauss-Hermite over q(f0) (S, xs, wn required); v <= 0 counts as 0 and its adjoint is 0.  The library does not
 * check 0 < y < 1 (the logs of such a target are -inf or NaN).  Gradients: grads->log_var_noise is ONE double, d/dlambda (as
 * out[1] of tgp_ell_flow_f64).  The training step always takes the general-M path.
 * tgp_predict_f64: m1 = E[y] = sum_s wn_s mu_s, m2 = Var[y] = sum_s wn_s mu_s (1 - mu_s) / (1 + phi) + sum_s wn_s mu_s^2 - m1^2
 * (the last two from 1 - mu_s where m1 > 1/2: the same variance, without the cancellation next to 1),
 * logp = log sum_s wn_s Beta(y | a_s, b_s), formed as a log-sum-exp; the empty program runs the same sweep.  The targets are
 * never standardised: Y_std is ignored.
 * tgp_predict_cdf_f64 and tgp_predict_quantile_f64 serve the mixture of Betas (below); tgp_predict_crps_f64 refuses it (a
 * mixture of Betas has no closed pair term). */
#define TGP_LIK_BETA 12
#define TGP_BETA_MIN_PRECISION 0.5
#define TGP_BETA_MAX_PRECISION 1e3
/* most steps of the continued fraction of the regularised incomplete beta function (tgp_quantile.hip): twice the 87 that the
 * covered box needs (tests/test_beta_host.py) */
#define TGP_BETA_CF_MAXIT 174

/* covariance function: instance_kernel(name, ...) of models/utils_models.py:145-204 (gpytorch kernels, ARD, softplus
 * parameters).  With d2 = |(x - z)/l|^2, l = softplus(raw_ls), s2 = softplus(raw_os[0]) and r = sqrt(max(d2, 1e-30)) as gpytorch's
 * covar_dist clamps it:
 *   RBF       s2 exp(-d2/2)
 *   MATERN32  s2 (1 + sqrt3 r) exp(-sqrt3 r)
 *   MATERN52  s2 (1 + sqrt5 r + 5/3 d2) exp(-sqrt5 r)
 *   RQ        s2 (1 + d2 / (2 alpha))^(-alpha)        the rational quadratic, a scale mixture of RBFs over the length-scale
 * Every kernel but the RBF runs on the general (tiled-GEMM) path at every M.
 * TGP_KERNEL_SCALE_RQ: `raw_os` addresses TWO doubles, {raw_outputscale, alpha}, in every entry that takes (kernel, raw_ls,
 * raw_os) or a tgp_model (the device that log_var_noise -> {eta, nu} is for TGP_LIK_STUDENT_T).  alpha is a fixed hyper-parameter,
 * supported for TGP_RQ_MIN_ALPHA <= alpha <= TGP_RQ_MAX_ALPHA (beyond the upper end the kernel is the RBF to O(1/alpha)); the
 * library trusts the pointer and the value -- the host layer checks the range.  grads->raw_os and raw_os_bar receive ONE value,
 * d/d raw_outputscale, for every kernel: the gradient with respect to alpha needs a third weighted pass over K_NM (weight
 * dk/dalpha beside k and k_g) and is left to a later ABI.
 * There is no Matern-1/2: its gradient weight s2 exp(-r)/r is unbounded at coincident points, and the gradients of Z and of the
 * length-scales are formed from expanded statistics that cancel there. */
#define TGP_KERNEL_SCALE_RBF 0      /* 'scale_rbf'      utils_models.py:188-193 (what main.py:229 uses) */
#define TGP_KERNEL_SCALE_MATERN32 1 /* 'scale_matern32' utils_models.py:199-204                          */
/* (2 and 4 are not assigned and stay refused: callers and tests of ABI <= 103 use 2 as THE unknown kernel id) */
#define TGP_KERNEL_SCALE_RQ 3       /* 'scale_rq'       gpytorch RQKernel under a ScaleKernel, alpha fixed */
#define TGP_KERNEL_SCALE_MATERN52 5 /* 'scale_matern52' gpytorch MaternKernel(nu=2.5) under a ScaleKernel */
#define TGP_RQ_MIN_ALPHA 1e-2
#define TGP_RQ_MAX_ALPHA 1e4

/* tgp_model.plan: which of the library's equivalent implementations a call runs (results agree to rounding; speed differs).
 * The library's own choice (0) depends on the shape only.  A workspace sized by tgp_workspace_bytes[_kernel] holds every
 * row-kernel variant; a forced chunk size needs tgp_workspace_bytes_plan.
 *   bits 0-3  row kernel of the fused path (M <= 128):
 *     TGP_PLAN_ROWS_AUTO  library's choice        TGP_PLAN_ROWS_K16  k_rows, 16 data rows per wave
 *     TGP_PLAN_ROWS_K     k_rows, rows per wave by the library's rule (16 or 10): never k_rows4
 *     TGP_PLAN_ROWS4_NW4 / TGP_PLAN_ROWS4_NW8  k_rows4 with 4 / 8 waves per workgroup (ignored where its LDS plan or the
 *                          workspace's slab count does not allow it)
 *   bit 4     TGP_PLAN_NO_CHUNK_OVERLAP  general-M path: one set of chunk buffers, forward and backward of the chunks in line
 *   bit 5     TGP_PLAN_FULL_PAD  fused path (M <= 128): the M x M backward launch contracts over all MP / 4 k-steps of M padded
 *             to the next multiple of 16 instead of the ceil(M / 4) that carry data.  Same results bit for bit (the padding
 *             holds exact zeros); exists for A/B timing and for the tests that compare the two.  The workspace size does not
 *             depend on it.
 *   bits 8-23 TGP_PLAN_CHUNK_ROWS(n)     general-M path: row chunks of at most n rows (rounded up to 128; 0 = 16 384) */
#define TGP_PLAN_ROWS_AUTO 0
#define TGP_PLAN_ROWS_K16 1
#define TGP_PLAN_ROWS_K 2
#define TGP_PLAN_ROWS4_NW4 3
#define TGP_PLAN_ROWS4_NW8 4
#define TGP_PLAN_ROWS_MASK 15
#define TGP_PLAN_NO_CHUNK_OVERLAP 16
#define TGP_PLAN_FULL_PAD 32
#define TGP_PLAN_CHUNK_ROWS(n) (((((n) + 127) / 128) & 0xffff) << 8)
#define TGP_PLAN_CHUNK_OF(plan) ((((plan) >> 8) & 0xffff) * 128)

typedef struct tgp_model {
  int32_t N;       /* rows in this call (this rank's shard of the minibatch)            */
  int32_t D;       /* input dimension (<= 16)                                           */
  int32_t M;       /* inducing points: <= 128 fused path, <= TGP_BIG_MAX_M tiled-GEMM path */
  int32_t S;       /* quadrature nodes (TGP_LIK_FLOW)                                   */
  int32_t nblk;    /* flow blocks                                                       */
  int32_t P;       /* shared flow scalars in theta                                      */
  int32_t RP;      /* per-row flow parameter columns in rowp                            */
  int32_t lik;     /* TGP_LIK_*                                                         */
  int32_t kernel;  /* TGP_KERNEL_*                                                      */
  int32_t plan;    /* kernel-selection overrides of THIS call, TGP_PLAN_* below; 0 = automatic (what every caller but
                      an A/B measurement or a test of a specific kernel passes).  Was `reserved0` up to ABI 102.  */
  double scale;    /* N_total / MB_global: sparse_MF_SP.ELL, models/sparse_MF_SP.py:623-626 */
  double jitter;   /* added to diag(K_MM) before the Cholesky (0 unless retrying)       */
  double kl_scale; /* weight of the KL gradient in this call: 1/world_size so that an
                      all-reduce(sum) over row shards counts it once                    */
  double jitter_ladder; /* > 0: psd_safe_cholesky's retry ladder (dsp/utils.py:256-269) runs ON THE DEVICE -- a failed
                      factorisation is repeated with jitter_ladder * 10^i, i = 0..2, added to diag(K_MM); status[2] = the
                      level that succeeded (1..3) or 0.  0: no retry, status[0] reports the pivot (host ladder:
                      ops.elbo_step_safe).  Fused path: inside k_prep_a; general-M path: one extra launch that returns
                      at once unless the blocked factorisation failed (then a single-workgroup refactorisation).  */
  /* parameters (reference nn.Parameter names in brackets) */
  const double* Z;             /* (M,D)   [Z]                                               */
  const double* raw_ls;        /* (D)     [covariance_function.base_kernel.raw_lengthscale] */
  const double* raw_os;        /* (1)     [covariance_function.raw_outputscale]; (2) {raw_outputscale, alpha} for TGP_KERNEL_SCALE_RQ */
  const double* m;             /* (M)     [q_U.variational_mean]                            */
  const double* Lam;           /* (M,M)   [q_U.chol_variational_covar] dense, tril at use   */
  const double* log_var_noise; /* (1)     [likelihood.log_var_noise]                        */
  const double* theta;         /* (P)     [G_matrix.0.flow_arr.*] or NULL                   */
  const int32_t* program;      /* (nblk,4) HOST array (copied into the kernel arguments), NULL if none; nblk <= 64 */
  const double* xs;            /* (S) Gauss-Hermite nodes                                   */
  const double* wn;            /* (S) weights / sqrt(pi)                                    */
} tgp_model;

typedef struct tgp_grads {
  double* Z;
  double* raw_ls;
  double* raw_os;
  double* m;
  double* Lam;
  double* log_var_noise;
  double* theta; /* (P) or NULL     */
  double* rowp;  /* (N,RP) or NULL  */
} tgp_grads;

int tgp_version(void);
const char* tgp_last_error(void);
/* sha256 (first 16 hex digits) of the kernel sources this library was compiled from (csrc Makefile SRC_HASH): the
   Python binding recomputes it from the tree and refuses a stale binary. */
const char* tgp_source_hash(void);

/* Bytes of workspace the calls below need for a problem of this shape (training is the maximum). */
size_t tgp_workspace_bytes(int32_t N, int32_t D, int32_t M, int32_t S, int32_t nblk, int32_t P, int32_t RP);
/* Same for a given covariance function (tgp_workspace_bytes == TGP_KERNEL_SCALE_RBF). */
size_t tgp_workspace_bytes_kernel(int32_t N, int32_t D, int32_t M, int32_t S, int32_t nblk, int32_t P, int32_t RP,
                                  int32_t kernel);
/* Same for a call that passes tgp_model.plan = `plan` (a forced chunk size changes the general-M path's buffers). */
size_t tgp_workspace_bytes_plan(int32_t N, int32_t D, int32_t M, int32_t S, int32_t nblk, int32_t P, int32_t RP,
                                int32_t kernel, int32_t plan);

/* Same for a call with likelihood `lik` (TGP_LIK_*): a TGP_LIK_BERNOULLI, TGP_LIK_POISSON, TGP_LIK_STUDENT, TGP_LIK_NEGBIN,
 * TGP_LIK_ORDINAL, TGP_LIK_GAMMA or TGP_LIK_BETA training step runs on the general-M path at every M. */
size_t tgp_workspace_bytes_lik(int32_t N, int32_t D, int32_t M, int32_t S, int32_t nblk, int32_t P, int32_t RP,
                               int32_t kernel, int32_t plan, int32_t lik);

/* One fused ELBO evaluation with gradients: replaces sparse_MF_SP.ELBO (models/sparse_MF_SP.py:552-598)
 * + loss.backward() (trainers/trainer_base.py:341) for one minibatch shard.
 *   X (N,D), Y (N), rowp (N,RP) or NULL
 *   out[0..3] = {ELBO_shard = ELL_shard - KL, ELL_shard, KL, 0}; gradients are d(ELL_shard - kl_scale*KL).
 *   mu, v: optional per-row q(f) moments (NULL to skip). */
int tgp_elbo_step_f64(const tgp_model* model, const double* X, const double* Y, const double* rowp, double* out,
                      const tgp_grads* grads, double* mu, double* v, int32_t* status, void* workspace,
                      size_t workspace_bytes, void* stream);

/* Same call restricted to some of its phases (profiling / roofline measurement: bench.py brackets one phase with
 * HIP events).  phases: bit0 = M x M prepare (K_MM, Cholesky, L^-1, KL), bit1 = fused row kernel,
 * bit2 = slab reduction + M x M adjoint + gradient assembly.  Phases must have run in order at least once on the
 * same workspace; tgp_elbo_step_f64 == phases 7. */
#define TGP_PHASE_PREPARE 1u
#define TGP_PHASE_ROWS 2u
#define TGP_PHASE_BACKWARD 4u
int tgp_elbo_step_phases_f64(const tgp_model* model, const double* X, const double* Y, const double* rowp,
                             double* out, const tgp_grads* grads, double* mu, double* v, int32_t* status,
                             void* workspace, size_t workspace_bytes, uint32_t phases, void* stream);

/* The whole training step of one rank in one call: tgp_elbo_step_f64 followed by tgp_adam_dev_f64 over a flat parameter
 * buffer (trainers/trainer_base.py:337-342: ELBO, backward, optimizer.step()).  `adam` describes the flat buffers; the
 * pointers of `grads` must point INTO adam->grads (the engine's layout: every gradient a view of one buffer), no weight
 * decay.  On the fused path (M <= 128) the update is applied inside the last two backward launches (the q(u) factor's
 * 10^4 entries by passenger workgroups beside the K_MM adjoint, the rest where the gradients are assembled): one launch
 * and one dependent pass over the buffers less than the two calls.  Same arithmetic, same results.  Single rank only: a
 * data-parallel step has its all-reduce between the gradients and the update and keeps the two calls. */
typedef struct tgp_adam_args {
  double* params;      /* (n) */
  double* grads;       /* (n) written by this call */
  double* exp_avg;     /* (n) */
  double* exp_avg_sq;  /* (n) */
  int64_t n;
  double lr, beta1, beta2, eps;
  int32_t* step_dev;   /* device int32[2] {step, ticket}, as tgp_adam_dev_f64 */
  int32_t maximize;    /* != 0: ascend (the gradients are of +ELBO) */
  uint32_t phases;     /* 0: the whole step; else a TGP_PHASE_* mask as in tgp_elbo_step_phases_f64 -- the update is applied
                          with TGP_PHASE_BACKWARD (an engine that runs the phases apart, e.g. the two-stream ID_TGP step) */
} tgp_adam_args;
int tgp_elbo_step_adam_f64(const tgp_model* model, const double* X, const double* Y, const double* rowp, double* out,
                           const tgp_grads* grads, double* mu, double* v, int32_t* status, void* workspace,
                           size_t workspace_bytes, const tgp_adam_args* adam, void* stream);

/* q(f) marginals only: sparse_MF_SP.marginal_variational_qf_parameters (models/sparse_MF_SP.py:274-396,
 * whitened, diagonal=True).  mu, v: (N). */
int tgp_qf_moments_f64(const tgp_model* model, const double* X, double* mu, double* v, int32_t* status,
                       void* workspace, size_t workspace_bytes, void* stream);

/* Full-covariance q(f): sparse_MF_SP.marginal_variational_qf_parameters, models/sparse_MF_SP.py:274-396, whitened,
 * diagonal=False (:384).  With A = L^-1 K(Z, X), L L^T = K_MM + jitter I, L_q = tril(Lam):
 *   mu = A^T m,   Sigma = K(X, X) + A^T (L_q L_q^T - I) A      (N x N, dense, no padding; Sigma[i][j] == Sigma[j][i] bit for bit)
 * Uses model->{N,D,M,kernel,jitter,Z,raw_ls,raw_os,m,Lam}; lik / flow fields ignored.  mu (N), Sigma (N,N) symmetric.
 * status[0] is tgp_cholesky_f64's (pivot of K_MM; the host runs the jitter ladder as for tgp_qf_moments_f64).
 * Limits: 1 <= N <= TGP_BIG_MAX_M, 1 <= M <= TGP_BIG_MAX_M, 1 <= D <= 16, else TGP_E_UNSUPPORTED; a workspace below
 * tgp_qf_cov_workspace_bytes gives TGP_E_WORKSPACE (tgp_last_error() names the entry in both cases).  No float atomics,
 * fixed reduction orders: two calls on the same input return the same bits. */
size_t tgp_qf_cov_workspace_bytes(int32_t N, int32_t D, int32_t M);
int tgp_qf_cov_f64(const tgp_model* model, const double* X, double* mu, double* Sigma, int32_t* status,
                   void* workspace, size_t workspace_bytes, void* stream);

/* Input gradients of the q(f) marginals: d mu_n / d x_nd and d v_n / d x_nd of tgp_qf_moments_f64's mu (N), v (N) at the rows
 * X (N,D), whitened q(u).  A stationary kernel is k(d2), d2 = |(x - z) / l|^2, with the weight k_g = -2 dk/d(d2) (the table of
 * kernels above); with K_ZZ + jitter I = L L^T, W = tril(Lam) tril(Lam)^T - I, a = L^-T m and U = L^-T W L^-1 K(Z, X) (M x N):
 *   J[n,m,d] = dk(x_n, z_m) / dx_nd = -k_g(d2_nm) (x_nd - z_md) / l_d^2
 *   mu_n = sum_m k_nm a_m                 dmu[n,d] = sum_m J[n,m,d] a_m
 *   v_n  = s2 + sum_m k_nm U_mn           dv[n,d]  = 2 sum_m J[n,m,d] U_mn
 * Each row's mu and v depend on that row's x only, so the Jacobians are the adjoint too: g_X = g_mu dmu + g_v dv, row by row.
 * The difference (x_nd - z_md) is formed directly from the scaled rows, never from expanded statistics: a row of X equal to a row
 * of Z bit for bit contributes an exact zero (every k_g is finite at d2 = 0, MATERN32's too).
 * Uses model->{N,D,M,kernel,jitter,Z,raw_ls,raw_os,m,Lam}; lik / flow fields ignored.  dmu, dv: (N,D) row-major.
 * status[0] is tgp_cholesky_f64's (pivot of K_ZZ; the host runs the jitter ladder as for tgp_qf_moments_f64).
 * Rows are processed in passes of TGP_XGRAD_PASS_ROWS rows (fixed: never a function of N), and the workspace is sized for
 * min(N, TGP_XGRAD_PASS_ROWS) rows; a row's result does not depend on the pass it falls in.
 * Limits: N >= 1, 1 <= M <= TGP_BIG_MAX_M, 1 <= D <= 16, else TGP_E_UNSUPPORTED; a workspace below
 * tgp_qf_input_grad_workspace_bytes gives TGP_E_WORKSPACE (tgp_last_error() names the entry in both cases).  The kernel id is
 * checked before any pointer is read (-1); a null model or model array, X, dmu, dv, status, workspace: -1, -2, -3, -4, -5, -6.
 * No float atomics, fixed summation orders: two calls on the same input return the same bits. */
#define TGP_XGRAD_PASS_ROWS 16384
size_t tgp_qf_input_grad_workspace_bytes(int32_t N, int32_t D, int32_t M);
int tgp_qf_input_grad_f64(const tgp_model* model, const double* X, double* dmu /* (N,D) */, double* dv /* (N,D) */,
                          int32_t* status, void* workspace, size_t workspace_bytes, void* stream);

/* The variance of the derivative process under q(f), the error bar of dmu above.  The posterior covariance is
 * Sigma(x, x') = k(x, x') + k(x, Z) B k(Z, x') with the symmetric B = L^-T W L^-1; its mixed derivative in x_d and x'_d at
 * x' = x is
 *   dvar[n,d] = k_g(0) / l_d^2 + sum_{m,m'} J[n,m,d] B[m,m'] J[n,m',d]
 * with k_g(0) = s2 (RBF), 3 s2 (MATERN32), 5/3 s2 (MATERN52), s2 (RQ).  Per pass of TGP_XGRAD_PASS_ROWS rows and per dimension
 * d: A_d = L^-1 J_d^T (the tiles of J_d generated on chip, never stored), C_d = W A_d on the fp64 matrix cores, and
 * dvar[n,d] = k_g(0) / l_d^2 + sum_m A_d[m,n] C_d[m,n] with m ascending.  The value is stored as computed and never clamped
 * (rounding can leave a tiny negative where the posterior pins the slope; clamp where a square root is taken).  (x - z) is
 * formed directly from the scaled rows.  Model fields, status[0], passes and the workspace rule as for tgp_qf_input_grad_f64;
 * dvar: (N,D) row-major.  A row's result depends on that row only, not on N or its pass; no float atomics, same input, same bits.
 * Limits: N >= 1, 1 <= M <= TGP_BIG_MAX_M, 1 <= D <= 16, a known kernel id, else TGP_E_UNSUPPORTED; a workspace below
 * tgp_qf_input_grad_var_workspace_bytes gives TGP_E_WORKSPACE (tgp_last_error() names the entry in all three cases).  A null
 * model or model array, X, dvar, status, workspace: -1, -2, -3, -4, -5.  Every refusal happens before any launch. */
size_t tgp_qf_input_grad_var_workspace_bytes(int32_t N, int32_t D, int32_t M);
int tgp_qf_input_grad_var_f64(const tgp_model* model, const double* X, double* dvar /* (N,D) */, int32_t* status,
                              void* workspace, size_t workspace_bytes, void* stream);

/* Joint draws from N(mu, Sigma): L_Sigma = chol(Sigma + jitter I) (tgp_cholesky_f64's status convention: status[0] = pivot),
 * F0 (S,N) = mu + eps L_Sigma^T for the caller's standard normals eps (S,N) -- sample-major, the layout X.repeat(1, S, 1)
 * gives on the diagonal path.  Lsig (N,N): optional output (NULL to skip).  1 <= N <= TGP_BIG_MAX_M, 1 <= S <= 4096. */
size_t tgp_qf_joint_sample_workspace_bytes(int32_t N, int32_t S);
int tgp_qf_joint_sample_f64(const double* mu, const double* Sigma, int32_t N, double jitter, const double* eps, int32_t S,
                            double* F0, double* Lsig, int32_t* status, void* workspace, size_t workspace_bytes, void* stream);

/* Adjoint of tgp_cholesky_f64 (what autograd replays for torch.cholesky inside psd_safe_cholesky, dsp/utils.py:239, when a
 * caller differentiates through the factor outside ELBO()): given L, Linv = L^-1 (both as tgp_cholesky_f64 returns them)
 * and L_bar (M x M; its part on and below the diagonal counts) it writes the SYMMETRIC
 *   A_bar = 1/2 L^-T (Phi(L^T L_bar) + Phi(L^T L_bar)^T) L^-1,   Phi = lower triangle with the diagonal halved
 * -- torch's cholesky backward.  Any M <= TGP_BIG_MAX_M: operands are padded to a multiple of 128 and run through the
 * three products of the general-M backward chain; workspace tgp_cholesky_bwd_workspace_bytes(M). */
size_t tgp_cholesky_bwd_workspace_bytes(int32_t M);
int tgp_cholesky_bwd_f64(const double* L, const double* Linv, const double* L_bar, int32_t M, double* A_bar, void* workspace,
                         size_t workspace_bytes, void* stream);

/* Unwhitened q(u) (is_whiten=False, models/sparse_MF_SP.py:352-391 and :433-453): the caller's (m, L_q) describe
 * q(u) = N(m, L_q L_q^T) on the inducing values.  With L L^T = K_ZZ + jitter I and the zero mean function
 *   m_w = L^-1 m,   Lam_w = L^-1 tril(L_q)        (lower x lower = lower; the strict upper triangle of Lam_w is exact zeros,
 *                                                  the strict upper triangle of L_q is never read)
 * is the whitened model with the same q(f) and the same KL against N(0, L L^T): every whitened entry of this header then
 * serves the unwhitened model at (m_w, Lam_w).  Z (M,D), m (M), L_q (M,M); outputs m_w (M), Lam_w, L, Linv (M,M);
 * status[0] is tgp_cholesky_f64's (the host runs the jitter ladder).
 * tgp_unwhiten_bwd_f64: given the forward's L, Linv, m_w, Lam_w and the cotangents m_w_bar (M), Lam_w_bar (M,M; its part on
 * and below the diagonal counts) it writes
 *   m_bar = L^-T m_w_bar,   L_q_bar = tril(L^-T Lam_w_bar),   L_bar = -tril(L^-T (m_w_bar m_w^T + Lam_w_bar Lam_w^T)),
 *   K_bar = tgp_cholesky_bwd_f64(L_bar),  and  Z_bar (M,D), raw_ls_bar (D), raw_os_bar (1) = K_bar + K_bar^T contracted with
 *   the derivative of the kernel matrix (the jitter and the diagonal carry no gradient with respect to Z).
 * Limits: 1 <= M <= TGP_BIG_MAX_M, 1 <= D <= 16, else TGP_E_UNSUPPORTED; a workspace below the *_workspace_bytes value gives
 * TGP_E_WORKSPACE (tgp_last_error() names the entry).  No float atomics, fixed reduction orders: same input, same bits. */
size_t tgp_unwhiten_workspace_bytes(int32_t M, int32_t D);
int tgp_unwhiten_f64(int32_t kernel, const double* Z, const double* raw_ls, const double* raw_os, int32_t M, int32_t D,
                     double jitter, const double* m, const double* L_q, double* m_w, double* Lam_w, double* L, double* Linv,
                     int32_t* status, void* workspace, size_t workspace_bytes, void* stream);
size_t tgp_unwhiten_bwd_workspace_bytes(int32_t M, int32_t D);
int tgp_unwhiten_bwd_f64(int32_t kernel, const double* Z, const double* raw_ls, const double* raw_os, int32_t M, int32_t D,
                         const double* L, const double* Linv, const double* m_w, const double* Lam_w, const double* m_w_bar,
                         const double* Lam_w_bar, double* m_bar, double* L_q_bar, double* Z_bar, double* raw_ls_bar,
                         double* raw_os_bar, void* workspace, size_t workspace_bytes, void* stream);

/* Closed-form optimal q(u) of the Gaussian likelihood (the maximiser behind Titsias' collapsed bound), whitened, zero prior
 * mean.  With K = K_ZZ + jitter I = L L^T, sigma^2 = exp(log_var_noise[0]) and c = model->scale:
 *   C = K_ZX K_XZ (M,M),   b = K_ZX y (M)        one pass over the rows, K_ZX generated on chip and never stored
 *   B = I + (c / sigma^2) L^-1 C L^-T,   S* = B^-1 = Lam* Lam*^T (Lam* lower, positive diagonal),   m* = (c / sigma^2) S* L^-1 b
 * (m*, Lam*) maximise what tgp_elbo_step_f64 computes for TGP_LIK_GAUSS over (m, Lam); at c = 1 its value there is the collapsed
 * bound log N(y | 0, Q + sigma^2 I) - tr(K_XX - Q) / (2 sigma^2), Q = K_XZ K^-1 K_ZX.  Lam* comes from ONE factorisation: the
 * index-reversed J B J = L' L'^T gives Lam* = J L'^-T J.
 * Uses model->{N,D,M,kernel,scale,jitter,Z,raw_ls,raw_os,log_var_noise}; m, Lam, lik and the flow fields are ignored.
 * X (N,D), Y (N); outputs m_out (M) and Lam_out (M,M; exact zeros above the diagonal) -- they may be the model's own m / Lam.
 * status[0] is tgp_cholesky_f64's for K (the host runs the jitter ladder); a failure of the second factorisation (B is
 * I + a positive semi-definite matrix: NaNs only) is reported there as well when K's succeeded.
 * tgp_kxxk_f64 is the first stage alone: C (M,M; C[i][j] == C[j][i] bit for bit) and b (M); Y == NULL or b == NULL skips b.
 * The rows are split into groups whose size depends on N and M only; the groups are summed in order by a second launch.  No
 * float atomics: two calls on the same input return the same bits on any device.
 * Limits: 1 <= M <= TGP_BIG_MAX_M, 1 <= D <= 16, N >= 1, else TGP_E_UNSUPPORTED; a workspace below the *_workspace_bytes value
 * gives TGP_E_WORKSPACE (tgp_last_error() names the entry in both cases). */
size_t tgp_optimal_qu_workspace_bytes(int32_t N, int32_t D, int32_t M);
int tgp_optimal_qu_f64(const tgp_model* model, const double* X, const double* Y, double* m_out, double* Lam_out,
                       int32_t* status, void* workspace, size_t workspace_bytes, void* stream);
size_t tgp_kxxk_workspace_bytes(int32_t N, int32_t M);
int tgp_kxxk_f64(int32_t kernel, const double* X, int32_t N, const double* Z, int32_t M, int32_t D, const double* raw_ls,
                 const double* raw_os, const double* Y, double* C, double* b, void* workspace, size_t workspace_bytes,
                 void* stream);

/* Natural-gradient step of the whitened q(u) = N(m, Lam Lam^T) for any likelihood, in its conjugate-computation form (Khan & Lin
 * 2017; Salimbeni et al. 2018): the closed-form optimum above with per-row pseudo-observations.  With K = K_ZZ + jitter I = L L^T,
 * a_n = L^-1 k_Z(x_n), mu_n = a_n^T m, and the adjoints mu_bar_n = d(c ELL)/d mu_n, v_bar_n = d(c ELL)/d v_n that tgp_ell_gauss_f64 /
 * tgp_ell_flow_f64 write as g_mu, g_v at scale c (they already hold c):
 *   lambda_n = -2 v_bar_n, lambda_n <- max(lambda_n, site_floor) (a NaN site_floor: no floor), r_n = mu_bar_n + lambda_n mu_n
 *   C = K_ZX diag(lambda) K_XZ,  b = K_ZX r        one pass over the rows, the sites formed per row, K_ZX never stored
 *   B = I + L^-1 C L^-T,  h = L^-1 b,  P = (Lam Lam^T)^-1
 *   P' = (1 - rho) P + rho B,  h' = (1 - rho) P m + rho h,  Lam' Lam'^T = P'^-1 (Lam' lower, positive diagonal),  m' = P'^-1 h'
 * rho in (0, 1] is the step size in natural parameters; with the Gaussian likelihood's adjoints and rho = 1 the step is
 * tgp_optimal_qu_f64's optimum.  At rho = 1 model->m and model->Lam are not read.  Lam's diagonal may have any sign.
 * Uses model->{N,D,M,kernel,jitter,Z,raw_ls,raw_os,m,Lam}; lik, scale and the flow fields are ignored.  X (N,D); mu, mu_bar,
 * v_bar (N); outputs m_out (M), Lam_out (M,M; exact zeros above the diagonal) -- they may be the model's own m / Lam.
 * status[0] is tgp_cholesky_f64's for K (the host runs the jitter ladder) and status[1] == 1 its NaN flag.  When K's factorisation
 * succeeded and met no NaN, status[1] reports the q(u) side: -(pivot) when Lam Lam^T is not positive definite, 1 + pivot when P' is
 * not (sites of a likelihood that is not log-concave, without a floor); NaNs without a failing pivot count as pivot M + 1 -- more
 * jitter does not help there.  When status[0] or status[1] is not zero the outputs are not written.  One stream, no host synchronisation, fixed summation orders: same input, same bits.
 * tgp_kxwxk_f64 is the weighted first stage alone: C = K_ZX diag(w) K_XZ (M,M; C[i][j] == C[j][i] bit for bit), b = K_ZX r (M);
 * w of any sign; r == NULL or b == NULL skips b.  With w = 1 it returns tgp_kxxk_f64's bits.
 * Limits and error codes are tgp_kxxk_f64's / tgp_optimal_qu_f64's; rho outside (0, 1] or an unknown kernel gives
 * TGP_E_UNSUPPORTED before any pointer is read. */
size_t tgp_kxwxk_workspace_bytes(int32_t N, int32_t M);
int tgp_kxwxk_f64(int32_t kernel, const double* X, int32_t N, const double* Z, int32_t M, int32_t D, const double* raw_ls,
                  const double* raw_os, const double* w, const double* r, double* C, double* b, void* workspace,
                  size_t workspace_bytes, void* stream);
size_t tgp_natgrad_qu_workspace_bytes(int32_t N, int32_t D, int32_t M);
int tgp_natgrad_qu_f64(const tgp_model* model, const double* X, const double* mu, const double* mu_bar, const double* v_bar,
                       double rho, double site_floor, double* m_out, double* Lam_out, int32_t* status, void* workspace,
                       size_t workspace_bytes, void* stream);

/* Greedy conditional-variance selection of inducing points: the pivoted Cholesky factorisation of K_XX (Burt, Rasmussen, van der
 * Wilk 2020, "Convergence of sparse variational inference in Gaussian processes regression").  It picks the M rows of X that most
 * reduce tr(K_XX - Q_XX), Q_XX = K_XZ K_ZZ^-1 K_ZX, and returns that residual trace after every pick.  With s2 the kernel's
 * variance, start with d_n = s2 for all rows and no picked rows.  For j = 0 .. M-1:
 *   1. p_j = argmax_n d_n over rows not yet picked; ties go to the smallest index (step 0 is an exact tie: p_0 = 0)
 *   2. if d_{p_j} <= min_var, stop: M_eff = j
 *   3. c_n = (k(x_n, x_{p_j}) - sum_{l<j} C[l,n] C[l,p_j]) / sqrt(d_{p_j}), the sum in the order of l
 *   4. C[j,n] = c_n
 *   5. d_n <- max(d_n - c_n^2, 0)
 *   6. row p_j is marked picked: it never competes again and adds nothing to the trace
 *   7. trace[j+1] = sum_{n not picked} d_n;  trace[0] = N s2
 * Outputs: idx (M, int32), Z (M,D) = X[idx] bit for bit, trace (M+1), count[0] = M_eff; the unused tails idx[M_eff..] = -1,
 * trace[M_eff+1..] = NaN, Z[M_eff..] = NaN.  X (N,D), raw_ls (D), raw_os (1), kernel TGP_KERNEL_*.
 * M + 1 launches on the stream (one per step, one closing), nothing read back; a stop is sticky: the later launches return at
 * once.  The arg-max and the trace reduce in a fixed order (wave butterfly, the waves in order, the workgroups' records in order),
 * the grid depends on N only, no float atomics: same input, same bits on any device.
 * workspace: tgp_greedy_inducing_workspace_bytes(N, D, M) bytes = C (M,N), d (N), two sets of workgroup records and the stop
 * word, each section a whole number of 64 doubles, + 16; C starts at the first 16-byte aligned address of the workspace.
 * Limits: 1 <= M <= min(N, TGP_BIG_MAX_M), 1 <= D <= 16, a known kernel, else TGP_E_UNSUPPORTED; a workspace below the sizer's
 * value gives TGP_E_WORKSPACE before any launch (tgp_last_error() names the entry in both cases); min_var < 0 or NaN: -8. */
size_t tgp_greedy_inducing_workspace_bytes(int32_t N, int32_t D, int32_t M);
int tgp_greedy_inducing_f64(const double* X, int32_t N, int32_t D, const double* raw_ls, const double* raw_os, int32_t kernel,
                            int32_t M, double min_var, int32_t* idx, double* Z, double* trace, int32_t* count, void* workspace,
                            size_t workspace_bytes, void* stream);

/* Pathwise posterior function draws (Wilson et al. 2020, "Efficiently sampling functions from Gaussian process posteriors") of the
 * whitened sparse GP: a draw is a weight vector over 2 R2 random Fourier features of the prior and the M kernel columns at the
 * inducing points, and can then be evaluated on any rows, in any batches, consistently, in O(N (R2 + M) S).  With
 * l = softplus(raw_ls), s2 = softplus(raw_os), K = K_ZZ + jitter I = L L^T, Lam = tril(Lam), amp = sqrt(s2 / R2) and
 * a_j(x) = sum_d omega[j,d] x_d / l_d (in the order of d):
 *   phi_j(x) = amp cos a_j(x),   phi_{R2+j}(x) = amp sin a_j(x)      (j < R2; sum_j phi_j(x)^2 = s2 at every x)
 *   nu_s     = L^-T (m + Lam eps_s - L^-1 Phi_Z W_s^T)               (the inducing-point update is exact)
 *   f0_s(x)  = sum_{j < 2 R2} phi_j(x) W[s,j] + sum_{i < M} k(x, z_i) nu_s[i]
 * The kernels draw no random numbers: omega (R2,D) are frequencies of the unit-length-scale kernel (N(0, I) for the RBF, the
 * multivariate Student-t with 3 degrees of freedom for Matern-3/2), W (S, 2 R2) and eps (S,M) standard normals.
 * tgp_pathwise_coeff_f64: coef (2 R2 + M, S) row-major; rows [0, 2 R2) = amp W[s,j], rows [2 R2, 2 R2 + M) = nu_s[i].  Uses
 *   model->{D,M,kernel,jitter,Z,raw_ls,raw_os,m,Lam}; status[0] is tgp_cholesky_f64's (the host runs the jitter ladder, as for
 *   tgp_qf_cov_f64).  Phi_Z is generated on chip and never stored.  workspace: tgp_pathwise_workspace_bytes(N, D, M, R2, S) bytes
 *   (N any value >= 1: it does not change the size), sections of whole 64 doubles, + 16.
 * tgp_pathwise_eval_f64: F0 (S,N) = the draws of coef on the rows X (N,D).  A value of F0 depends on its row of X and on coef
 *   only (fixed contraction order): X evaluated in one call or in pieces gives the same bits.  S * N may exceed 2^31.
 * No float atomics, fixed summation orders: two calls on the same input return the same bits.
 * Limits: N >= 1, 1 <= D <= 16, 1 <= M <= TGP_BIG_MAX_M, 1 <= R2 <= TGP_PATHWISE_MAX_R2, 1 <= S <= TGP_PATHWISE_MAX_S, one of
 * the two kernels, else TGP_E_UNSUPPORTED; a workspace below the sizer's value gives TGP_E_WORKSPACE (tgp_last_error() names the
 * entry in both cases); a null pointer gives the negative index of its argument.  Every refusal happens before any launch. */
#define TGP_PATHWISE_MAX_R2 8192
#define TGP_PATHWISE_MAX_S 256
size_t tgp_pathwise_workspace_bytes(int32_t N, int32_t D, int32_t M, int32_t R2, int32_t S);
int tgp_pathwise_coeff_f64(const tgp_model* model, const double* omega, int32_t R2, const double* W, const double* eps, int32_t S,
                           double* coef, int32_t* status, void* workspace, size_t workspace_bytes, void* stream);
int tgp_pathwise_eval_f64(int32_t kernel, const double* X, int32_t N, int32_t D, const double* Z, int32_t M, const double* raw_ls,
                          const double* raw_os, const double* omega, int32_t R2, const double* coef, int32_t S, double* F0,
                          void* stream);

/* Input gradients of the draws: dF0 (D,S,N), plane d in F0's layout, dF0[d][s][n] = d f0_s(x_n) / d x_nd.  With
 * w_jd = omega[j,d] / l_d and k_g = -2 dk/d(d2) (the table of kernels above; finite at d2 = 0):
 *   d f0_s(x) / d x_d = sum_{j < R2} w_jd [ -amp sin a_j(x) W[s,j] + amp cos a_j(x) W[s,R2+j] ]
 *                       - sum_{i < M} k_g(d2(x, z_i)) (x_d - z_id) / l_d^2 nu_s[i]
 * coef is tgp_pathwise_coeff_f64's; the features' derivatives are generated on chip and never stored, and (x_d - z_id) is formed
 * directly from the scaled rows (a row of X equal to a row of Z bit for bit: an exact zero in that term).  The contraction walks
 * the rows of coef in tgp_pathwise_eval_f64's order, one set of accumulators per dimension: an element depends on its row of X,
 * its d and coef only, so X in one call, in pieces, below or above the row count at which the row tiling changes gives the same
 * bits.  No float atomics.  D * S * N may exceed 2^31.  Limits, refusals and their order: tgp_pathwise_eval_f64's, with dF0 in
 * the place of F0 (-13); tgp_last_error() names this entry. */
int tgp_pathwise_grad_f64(int32_t kernel, const double* X, int32_t N, int32_t D, const double* Z, int32_t M, const double* raw_ls,
                          const double* raw_os, const double* omega, int32_t R2, const double* coef, int32_t S,
                          double* dF0 /* (D,S,N) */, void* stream);

/* Mean functions (models/means.py, chosen by model_specs[0], models/utils_models.py:285-294): 'linear' m(x) = x a + b with a (D)
 * and b (1) trainable, 'identity' m(x) = x W with W (D) fixed (b = NULL).  One output GP: a is a vector.  The reference adds
 * m(X) to the q(f) mean (models/sparse_MF_SP.py:314,355,360), subtracts m(Z) from the unwhitened variational mean (:359) and uses
 * it as the prior mean of the unwhitened KL (:446).
 * tgp_mean_forward_f64:   out[n ld + col] = alpha (sum_d X[n,d] a[d] + b[0]) + (in ? in[n] : 0),  n < N, the sum in the order
 *   d = 0 .. D-1; b == NULL counts as 0; one_col >= 0 also writes 1.0 to out[n ld + one_col].  No other element of out is
 *   touched.  With ld = 2, col = 1, one_col = 0 it fills the (N, 2) rowp columns (a_n, b_n) = (1, m(x_n)) of a per-row
 *   TGP_FLOW_AFFINE block at the head of a flow program, which turns G(f) into G(f + m(x_n)); with alpha = -1, in = Y it forms
 *   Y - m(X); with in = mu it forms mu + m(X).  in may alias out when ld = 1.
 * tgp_mean_backward_f64:  with g_n = g[n ldg + colg] (read in place from a column of g_rowp, or a vector with ldg = 1, colg = 0)
 *   g_a[d] = sum_n g_n X[n,d],   g_b[0] = sum_n g_n (g_b == NULL: skipped),   g_X[n,d] = g_n a[d] (g_X == NULL: skipped, and a
 *   may then be NULL).  Summation order, fixed: a lane sums rows 1024 w + t + 256 i (i = 0 .. 3) of workgroup w, the wave
 *   butterfly, the four waves in order, the workgroups in order by a second launch.  The grid depends on N only.  No float
 *   atomics: same input, same bits on any device.  workspace: tgp_mean_backward_workspace_bytes(N, D) bytes, 8-byte aligned.
 * Limits: N >= 1, 1 <= D <= 16 (else TGP_E_UNSUPPORTED, tgp_last_error() names the entry), 0 <= col < ld, one_col < ld and
 * != col, 0 <= colg < ldg: otherwise the negative index of the offending argument; a small workspace gives TGP_E_WORKSPACE. */
int tgp_mean_forward_f64(const double* X, int32_t N, int32_t D, const double* a, const double* b, double alpha, const double* in,
                         double* out, int32_t ld, int32_t col, int32_t one_col, void* stream);
size_t tgp_mean_backward_workspace_bytes(int32_t N, int32_t D);
int tgp_mean_backward_f64(const double* X, int32_t N, int32_t D, const double* a, const double* g, int32_t ldg, int32_t colg,
                          double* g_a, double* g_b, double* g_X, void* workspace, size_t workspace_bytes, void* stream);

/* Adjoint of tgp_qf_moments_f64 (what autograd replays for models/sparse_MF_SP.py:274-396 when a caller differentiates
 * the q(f) marginals outside ELBO(): predictive moments with respect to the inducing points, hyper-parameters or q(u)).
 * Given mu_bar, v_bar (N) it writes d(sum_n mu_bar_n mu_n + v_bar_n v_n)/d{Z, raw_ls, raw_os, m, Lam} into `grads`
 * (grads->log_var_noise receives 0; theta / rowp are not touched).  Same kernels as the training step -- the row
 * kernel takes the adjoints instead of forming them from a likelihood, the M x M chain runs with KL weight 0 -- on
 * either path (fused for M <= 128, general-M above); workspace as tgp_workspace_bytes for S = 1, no flow. */
int tgp_qf_moments_bwd_f64(const tgp_model* model, const double* X, const double* mu_bar, const double* v_bar,
                           const tgp_grads* grads, int32_t* status, void* workspace, size_t workspace_bytes,
                           void* stream);

/* K_MM assembly: gpytorch ScaleKernel(RBFKernel(ard)) as built by instance_kernel('scale_rbf'),
 * models/utils_models.py:188-193, called at models/sparse_MF_SP.py:316.  K (M,M). */
int tgp_kmm_f64(const double* Z, const double* raw_ls, const double* raw_os, int32_t M, int32_t D, double jitter,
                double* K, void* stream);
/* Same with the covariance function selected (TGP_KERNEL_*); X2 == NULL: K(X1, X1) + jitter I (N2 ignored),
 * else K(X1, X2) of shape (N1, N2). */
int tgp_kernel_matrix_f64(int32_t kernel, const double* X1, int32_t N1, const double* X2, int32_t N2, int32_t D,
                          const double* raw_ls, const double* raw_os, double jitter, double* K, void* stream);

/* K_NM assembly (models/sparse_MF_SP.py:319); K (N,M).  Diagnostic/next-row use: the training path
 * never materialises K_NM. */
int tgp_knm_f64(const double* X, const double* Z, const double* raw_ls, const double* raw_os, int32_t N, int32_t M,
                int32_t D, double* K, void* stream);

/* Lower Cholesky with LAPACK-style info: torch.cholesky inside psd_safe_cholesky, dsp/utils.py:239.
 * A (M,M) symmetric, L (M,M) lower (strict upper zeroed); Linv (M,M) = L^-1 or NULL. */
int tgp_cholesky_f64(const double* A, int32_t M, double* L, double* Linv, int32_t* status, void* workspace,
                     size_t workspace_bytes, void* stream);
/* Workspace of tgp_cholesky_f64: 0 for M <= 128 (factorised in one CU's LDS), the blocked multi-kernel path above. */
size_t tgp_cholesky_workspace_bytes(int32_t M);

/* Dense float64 contraction on the matrix cores, the building block of the M > 128 path (the reference's
 * torch.bmm / triangular_solve calls at models/sparse_MF_SP.py:354,376-382 on (M,M)x(M,N) operands):
 *   C = alpha * op(A) op(B) + beta * C, row-major, op = transpose when trans_* != 0.
 * m, n multiples of 128, k a multiple of 16, lda/ldb even, A and B 16-byte aligned (callers pad).  `tri` declares triangular operands so that the k range
 * is trimmed per output tile: 1 op(A) lower, 2 op(A) upper, 4 op(B) lower, 8 op(B) upper, 16 compute only the
 * lower block triangle of C (flags OR-ed; 0 = general).  A misaligned A / B, and a leading dimension that is odd (lda, ldb)
 * or shorter than the row it strides (lda, ldb, ldc), are refused with that argument's code. */
int tgp_gemm_f64(int32_t trans_a, int32_t trans_b, int32_t tri, int32_t m, int32_t n, int32_t k, double alpha,
                 const double* A, int32_t lda, const double* B, int32_t ldb, double beta, double* C, int32_t ldc,
                 void* stream);

/* The same contraction with everything the tiled kernels can fuse into it, as one descriptor:
 *   x = alpha * (op(A) o a_mul * diag(k_scale)) op(B) + gamma * add;  x *= col_scale[j] * row_scale[i];
 *   x += rowv[i] * colv[j];  C = x + beta * C
 * Fields 1-14 are tgp_gemm_f64's arguments in its order, so that a refusal carries the same code from both entries:
 * the return value of tgp_gemm_ex_f64 / tgp_gemm_route is -(number of the offending FIELD, counted from 1 as numbered
 * below); -1 also stands for a NULL descriptor.  Every optional pointer is NULL when unused.
 *   a_mul     matrix with A's shape and leading dimension, multiplied into A element by element (16-byte aligned)
 *   k_scale   (k) scales of the contraction index (16-byte aligned)
 *   add       (m, n) with leading dimension ldadd >= n; excludes beta != 0 (the epilogue reads one extra matrix)
 *   rowv, colv  the rank-one term: both or neither
 *   ksplit    >= 1: the k range of every output tile is cut into ksplit slabs of whole 16-wide stages; slab z is written,
 *             epilogue included, to C + z * cz (cz >= (m - 1) * ldc + n doubles) and the CALLER adds the slabs
 *   xcd       workgroup -> tile order: 0 natural, 1 the column tiles of a tile row share an XCD, 2 the tiles of a k slab
 *             share an XCD (ksplit a multiple of 8, natural otherwise).  A pure speed choice: results do not depend on it
 *   scratch   NULL: one launch, as above.  Otherwise ksplit must be 1 and the product takes the route of the M x M
 *             products of the training step: split-K (min(8, 256 / tiles, k / 64) slabs, fewer than 2 = no split) into
 *             m * n-double slabs in `scratch`, then a fixed-order reduction C = sum of the slabs + beta * C.  When
 *             scratch_doubles is too small for the slabs, or add / col_scale / row_scale / rowv is given, it is the unsplit launch. */
typedef struct tgp_gemm_ex {
  int32_t trans_a, trans_b, tri; /*  1  2  3 */
  int32_t m, n, k;               /*  4  5  6 */
  double alpha;                  /*  7       */
  const double* A;               /*  8       */
  int32_t lda;                   /*  9: >= the row length of A as stored (k, or m when trans_a), even */
  const double* B;               /* 10       */
  int32_t ldb;                   /* 11: >= the row length of B as stored (n, or k when trans_b), even */
  double beta;                   /* 12       */
  double* C;                     /* 13       */
  int32_t ldc;                   /* 14: >= n */
  const double* a_mul;           /* 15       */
  const double* k_scale;         /* 16       */
  const double* add;             /* 17       */
  int32_t ldadd;                 /* 18       */
  double gamma;                  /* 19       */
  const double* col_scale;       /* 20: (n)  */
  const double* row_scale;       /* 21: (m)  */
  const double* rowv;            /* 22: (m)  */
  const double* colv;            /* 23: (n)  */
  int32_t ksplit;                /* 24       */
  size_t cz;                     /* 25       */
  int32_t xcd;                   /* 26       */
  double* scratch;               /* 27       */
  size_t scratch_doubles;        /* 28       */
} tgp_gemm_ex;
int tgp_gemm_ex_f64(const tgp_gemm_ex* d, void* stream);
/* Two independent products in one launch, as the blocked factorisation issues them: a with op(B) transposed (trans_a = 0,
 * trans_b = 1), b plain (trans_a = trans_b = 0).  Fused when neither has a_mul / k_scale, both or neither have an
 * epilogue, and ksplit = 1; two launches otherwise.  scratch must be NULL.  Codes: a's field numbers, b's plus 32. */
int tgp_gemm_pair_ex_f64(const tgp_gemm_ex* a, const tgp_gemm_ex* b, void* stream);
/* Host only, no pointer is looked at but for its alignment: the kernel and workgroup order the launcher chooses for `d`
 * (scratch ignored), or the refusal code of tgp_gemm_ex_f64. */
#define TGP_GEMM_ROUTE_128 0          /* 128 x 128 tiles, natural order (or the caller's xcd 1 / 2)                   */
#define TGP_GEMM_ROUTE_128_PAIRED 1   /* ... triangular op(B): column tiles j and n/128-1-j share a workgroup          */
#define TGP_GEMM_ROUTE_128_HEAVY 2    /* ... triangular op(B), unpaired: per-XCD heaviest-column-first order            */
#define TGP_GEMM_ROUTE_128_TRIANGLE 3 /* ... TRI_C_LOWER with split-K: compact enumeration of the lower block triangle  */
#define TGP_GEMM_ROUTE_64 4           /* 64 x 64 tiles, 8 waves                                                        */
int tgp_gemm_route(const tgp_gemm_ex* d);

/* Whitened KL and its gradients: sparse_MF_SP.KLD, models/sparse_MF_SP.py:406-431. out[0] = KL. */
int tgp_kl_whitened_f64(const double* m, const double* Lam, int32_t M, double* out, double* g_m, double* g_Lam,
                        void* stream);

/* Workspace of the two stand-alone likelihood entries below (per-workgroup partial sums; the workgroup count depends on
 * N: the flow kernel gives small problems 16 lanes per row instead of 4). */
size_t tgp_ell_workspace_bytes(int32_t N, int32_t P, int32_t RP);

/* SVGP closed-form expected log-likelihood (likelihoods/GaussianLinearMean.py:60-87 + dsp/utils.py:164-195),
 * summed over rows and multiplied by `scale`.  out[0] = ELL, out[1] = dELL/dlog_var_noise; g_mu, g_v: (N). */
int tgp_ell_gauss_f64(const double* Y, const double* mu, const double* v, int32_t N, const double* log_var_noise,
                      double scale, double* out, double* g_mu, double* g_v, void* workspace, size_t workspace_bytes,
                      void* stream);

/* TGP Gauss-Hermite expected log-likelihood through the flow (likelihoods/GaussianNonLinearMean.py:64-150),
 * with gradients w.r.t. mu, v, theta, rowp, log_var_noise.  out[0] = ELL, out[1] = dELL/dlog_var_noise.
 * model->lik == TGP_LIK_BERNOULLI: Bernoulli.expected_log_prob (likelihoods/Bernoulli.py) instead, out[1] = 0.
 * model->lik == TGP_LIK_POISSON: the Poisson expected log-likelihood of its #define, out[1] = 0.
 * model->lik == TGP_LIK_STUDENT: the Student-t one of its #define (log_var_noise = {log sigma^2, nu}), out[1] = dELL/dlog sigma^2.
 * model->lik == TGP_LIK_NEGBIN: the negative-binomial one of its #define (log_var_noise = log r), out[1] = dELL/dlog r.
 * model->lik == TGP_LIK_ORDINAL: the cumulative-probit one of its #define (log_var_noise = {log sigma^2, K, b_1, .., b_{K-1}}),
 * out[1] = dELL/dlog sigma^2.
 * model->lik == TGP_LIK_GAMMA: the Gamma one of its #define (log_var_noise = log a), out[1] = dELL/dlog a.
 * model->lik == TGP_LIK_BETA: the Beta one of its #define (log_var_noise = log phi), out[1] = dELL/dlog phi. */
int tgp_ell_flow_f64(const tgp_model* model, const double* Y, const double* mu, const double* v, const double* rowp,
                     double* out, double* g_mu, double* g_v, double* g_theta, double* g_rowp, void* workspace,
                     size_t workspace_bytes, void* stream);

/* Heteroscedastic Gaussian expected log-likelihood (TGP_LIK_HETERO).  mu, v, mu_bar, v_bar are (2,N): row 0 belongs to f,
 * q(f_n) = N(mu1, v1), row 1 to the log-noise GP, q(h_n) = N(mu2, v2), independent.  h integrates out in closed form; with
 * c = log_var_noise[0], a_n = c + mu2_n, p_n = exp(-a_n + v2_n / 2) and A_n = sum_s wn_s (y_n - G(mu1_n + sqrt(2 v1_n) xs_s))^2:
 *   out[0] = scale sum_n (-log(2 pi) / 2 - a_n / 2 - p_n A_n / 2)        (the constant: tgp_ell_flow_f64's)
 *   out[1] = d out[0] / d c = sum_n mu_bar[1][n];   mu_bar[1][n] = scale (-1/2 + p_n A_n / 2),   v_bar[1][n] = -scale p_n A_n / 4;
 *   mu_bar[0], v_bar[0], g_theta, g_rowp: those of tgp_ell_flow_f64 with exp(-log_var_noise) replaced by the row's p_n.
 * Every output pointer is optional.  v1 <= 0 and v2 <= 0 count as 0 and their adjoint is written as 0; p_n is not clamped.
 * Model fields: those tgp_ell_flow_f64 reads (model->lik is ignored); workspace: tgp_ell_workspace_bytes(N, P, RP).  Fixed
 * summation order, no float atomics: same input, same bits. */
int tgp_ell_hetero_f64(const tgp_model* model, const double* Y, const double* mu /* (2,N) */, const double* v /* (2,N) */,
                       const double* rowp, double* out, double* mu_bar /* (2,N) */, double* v_bar /* (2,N) */, double* g_theta,
                       double* g_rowp, void* workspace, size_t workspace_bytes, void* stream);

/* Flow evaluation G(f), dG/df, log dG/df for f of shape (S,N) (row n uses rowp[n,:]):
 * CompositeFlow.forward (models/flow.py:155-158) and Flow.forward_grad (:101-104); serves prediction and the
 * WGP-style log-Jacobian (likelihoods/WarpedGaussianLinearMean.py:65-85).  Any output may be NULL. */
int tgp_flow_eval_f64(const tgp_model* model, const double* f, int32_t S, int32_t N, const double* rowp, double* G,
                      double* dG, double* logdG, void* stream);

/* Fused flow + log-Jacobian accumulation: out[0] = sum over the (S,N) array of log dG/df (fixed summation order,
 * bit-reproducible), G (optional) = the warped values -- the two quantities of a warped-GP likelihood term
 * (likelihoods/WarpedGaussianLinearMean.py:65-85: log p(y) = log N(G(y) | ...) + sum log G'(y)) in one pass over f,
 * nothing of size S x N written unless G is asked for. */
size_t tgp_flow_logdet_workspace_bytes(int32_t S, int32_t N);
int tgp_flow_logdet_f64(const tgp_model* model, const double* f, int32_t S, int32_t N, const double* rowp, double* G,
                        double* out, void* workspace, size_t workspace_bytes, void* stream);

/* Warped-GP likelihood (likelihoods/WarpedGaussianLinearMean.py:65-85) with gradients, one launch:
 *   out[0] = scale sum_n [Gaussian closed form at t_n = T(y_n)] + scale sum_n log T'(y_n),
 *   out[1] = d out[0] / d log_var_noise,   out[2] = scale sum_n log T'(y_n);
 *   g_mu, g_v (N), g_theta (P), t_out (N) = T(Y): each optional (NULL to skip).  Fixed summation order (per-workgroup partials
 *   added by the last workgroup to arrive): bit-reproducible.  model: N, nblk, P, program, theta, log_var_noise, scale. */
size_t tgp_ell_warp_workspace_bytes(int32_t N, int32_t P);
int tgp_ell_warp_f64(const tgp_model* model, const double* Y, const double* mu, const double* v, double* out, double* g_mu,
                     double* g_v, double* g_theta, double* t_out, void* workspace, size_t workspace_bytes, void* stream);

/* Inverse of a flow, x = T^-1(t) for t of shape (S,N) (row n uses rowp[n,:]; CompositeFlow.inverse, models/flow.py:160-170):
 * blocks are inverted last to first, in closed form where there is one (AFFINE, SAL, ARCSINH, BOXCOX <-> INV_BOXCOX, all
 * without TGP_FLAG_ADD_F0), else by a bracketed Newton iteration on that block (bracket grown by doubling, Newton steps,
 * bisection whenever a step leaves the bracket, at most 128 evaluations per phase).  status (device int32[1], zeroed by the
 * caller): the call ADDS the number of elements that did not reach the stopping rule. */
int tgp_flow_inverse_f64(const tgp_model* model, const double* t, int32_t S, int32_t N, const double* rowp, double* x,
                         int32_t* status, void* stream);

/* ---- multi-class likelihood (likelihoods/MulticlassCategorical.py:60-133): C latent GPs, one flow program per class ----
 *   f0[s,c,n] = mu[c,n] + sqrt(max(v[c,n], 0)) eps[s,c,n],   g[s,c,n] = G_c(f0[s,c,n]),
 *   ELL = scale/S sum_n sum_s (g[s,y_n,n] - logsumexp_c g[s,c,n])        (max-subtracted: torch's CrossEntropyLoss)
 * Limits (TGP_E_UNSUPPORTED otherwise): 3 <= C <= TGP_SOFTMAX_MAX_C, 1 <= S <= TGP_SOFTMAX_MAX_S, at most 64 blocks over all
 * programs, shared flow parameters only (a block with TGP_FLAG_PER_ROW is refused).
 * eps: the caller's standard normals, (S,C,N) -- the reference's F0 layout -- or NULL: every lane derives its draws from a
 * splitmix64 hash of (seed, *step_dev, s, c, row0 + n) followed by Box-Muller (exact recipe: csrc/tgp_softmax.hip), nothing of
 * size S x C x N exists in memory; a row keeps its draws when the rows are sharded over calls (row0 = first row of the shard).
 * mu, v: (C,N);  Y: (N) float64 holding the class index 0..C-1;  P: (N,C). */
#define TGP_SOFTMAX_MAX_C 32
#define TGP_SOFTMAX_MAX_S 256
typedef struct tgp_softmax {
  int32_t N;                /* rows in this call                                                              */
  int32_t C;                /* classes = latent GPs                                                           */
  int32_t S;                /* Monte-Carlo samples per row                                                    */
  int32_t reserved0;
  const int32_t* program;   /* HOST (blk_off[C],4): the C programs one after the other; poff is relative to the
                               class's own parameters theta + theta_off[c]; NULL if no class has a block      */
  const int32_t* blk_off;   /* HOST (C+1): blocks of class c are [blk_off[c], blk_off[c+1])                   */
  const double* theta;      /* (theta_off[C]) shared flow scalars of all programs, or NULL                    */
  const int32_t* theta_off; /* HOST (C+1)                                                                     */
  double scale;             /* N_total / MB                                                                   */
  uint64_t seed;            /* counter mode                                                                   */
  const int32_t* step_dev;  /* counter mode: device int32 read at launch (e.g. the Adam step counter, so that a
                               captured graph draws afresh on every replay); NULL = 0                         */
  int64_t row0;             /* counter mode: global index of this call's first row                            */
} tgp_softmax;
size_t tgp_ell_softmax_workspace_bytes(int32_t N, int32_t P);
/* out[0] = ELL; mu_bar, v_bar (C,N) and theta_bar (theta_off[C]) = its gradients, written in the same launch -- all three
 * NULL: forward only.  v_bar is 0 on rows with v <= 0.  Fixed summation order, no float atomics: bit-reproducible. */
int tgp_ell_softmax_f64(const tgp_softmax* d, const double* Y, const double* mu, const double* v, const double* eps,
                        double* out, double* mu_bar, double* v_bar, double* theta_bar, void* workspace, size_t workspace_bytes,
                        void* stream);
/* eps (S,C,N) = the draws the counter mode of a call with the same (N, C, S, seed, step_dev, row0) uses. */
int tgp_mc_normals_f64(const tgp_softmax* d, double* eps, void* stream);
/* P[n][c] = 1/S sum_s softmax_c(g[s,.,n]) (MulticlassCategorical.marginal_moments); logp[n] = log P[n][y_n] when Y and logp
 * are given.  eps as above. */
int tgp_predict_softmax_f64(const tgp_softmax* d, const double* mu, const double* v, const double* eps, const double* Y,
                            double* P, double* logp, void* stream);

/* Evaluation path given q(f) moments: predictive moments m1, m2
 * (GaussianNonLinearMean.marginal_moments :152-203 / GaussianLinearMean.marginal_moments :89-118) and the
 * per-row test log-likelihood WITHOUT the -0.5*log(pi) constant (models/sparse_MF_SP.py:705-776, 786-799).
 * Y may be NULL (then logp is not written).  TGP_LIK_BERNOULLI, TGP_LIK_POISSON, TGP_LIK_NEGBIN, TGP_LIK_ORDINAL, TGP_LIK_BETA: see their #defines; Y_std is
 * ignored.
 * TGP_LIK_STUDENT, TGP_LIK_GAMMA: see their #defines (Y_std is used, the constant is included).
 * TGP_LIK_WARPED: m1 = sum_s wn_s T^-1(mu + sqrt(2 (v + noise)) xs_s), m2 = the same of (T^-1)^2, minus m1^2
 * (WarpedGaussianLinearMean.marginal_moments), logp = log N(T(y) | mu, v + noise) + log T'(y) - log Y_std, the exact warped
 * predictive density WITH its constant (float32 pi as everywhere); rowp is ignored. */
int tgp_predict_f64(const tgp_model* model, const double* mu, const double* v, const double* rowp, const double* Y,
                    double Y_std, double* m1, double* m2, double* logp, void* stream);

/* The heteroscedastic predictive (TGP_LIK_HETERO) from the moments of both latent GPs, mu, v of shape (2,N) as for
 * tgp_ell_hetero_f64, in the standardised units of tgp_predict_f64; g_s = G(mu1 + sqrt(2 v1) xs_s), a = log_var_noise[0] + mu2,
 * variances <= 0 count as 0:
 *   m1 = sum_s wn_s g_s,   m2 = sum_s wn_s g_s^2 - m1^2 + exp(a + v2 / 2)    (the empty program: mu1 and v1 + exp(a + v2 / 2)),
 *   logp = log sum_s sum_t wn_s wn_t N(y | g_s, exp(a + sqrt(2 v2) xs_t)) - log Y_std,
 * the exact log density of the raw target under the S x S product rule WITH its constant (double-precision pi), formed as a
 * max-subtracted log-sum-exp: finite for a residual of 1e8 noise standard deviations.  The S node values of a row are computed
 * once and kept in LDS.  m1, m2, logp are each optional; Y may be NULL (then logp is not written).  model->lik is ignored.
 * Limit: 1 <= S <= TGP_QUANTILE_MAX_S (TGP_E_UNSUPPORTED otherwise).  Fixed summation order: same input, same bits. */
int tgp_predict_hetero_f64(const tgp_model* model, const double* mu /* (2,N) */, const double* v /* (2,N) */, const double* rowp,
                           const double* Y, double Y_std, double* m1, double* m2, double* logp, void* stream);

/* Exact CDF and quantiles of the predictive distribution tgp_predict_f64 integrates (TGP_LIK_GAUSS and TGP_LIK_FLOW, and
 * TGP_LIK_GAMMA and TGP_LIK_BETA as described at the end; model
 * fields as for tgp_predict_f64, everything in the model's standardised units):
 *   p(y | x_n) = sum_s wn_s N(y | g_ns, sig^2),  g_ns = G(mu_n + sqrt(2 v_n) xs_s),  sig^2 = exp(log_var_noise)
 *   F_n(t) = sum_s wn_s Phi((t - g_ns) / sig),   strictly increasing, F_n' = the density above.
 * tgp_predict_cdf_f64: cdf[n] = F_n(Y[n]) (the PIT values of a calibration plot) and, when sf is given, the upper tail
 * sf[n] = sum_s wn_s Phi(-(Y[n] - g_ns) / sig) from its own sum; Phi through erfc on the side where it is small.
 * tgp_predict_quantile_f64: t[q,n] = the root of F_n(t) = probs[q];  probs[q] in (0,1) in any order, zq[q] = Phi^-1(probs[q])
 * from the host.  TGP_LIK_GAUSS or an empty program: t = mu + zq sqrt(max(v, 0) + sig^2), no iteration (the CDF: one term).
 * A row with v <= 0 counts as v = 0: t = G(mu) + zq sig.  Else the row's S node values are computed once (the sweeps of
 * tgp_predict_f64; TGP_FLAG_PER_ROW programs included) and kept in LDS for all Q roots; each root starts at
 * t0 = G(mu + zq sqrt v) + zq sig, grows a bracket by doubling steps of max(sig, |t0| 2^-20), takes Newton steps with F',
 * bisects whenever a step leaves the bracket, and stops at an exact hit or a step <= 2^-50 max(1, |t|); at most 128 evaluations
 * of F per phase.  probs[q] <= 0.5 solves sum wn Phi(z) = p, probs[q] > 0.5 the upper-tail equation sum wn Phi(-z) = 1 - p, so
 * both tails are resolved to relative accuracy.  status (device int32[1], zeroed by the caller): the call ADDS the number of
 * roots that ran out of evaluations; their t is NaN.
 * Limits: 1 <= S <= TGP_QUANTILE_MAX_S, 1 <= Q <= TGP_QUANTILE_MAX_Q; TGP_LIK_BERNOULLI, TGP_LIK_WARPED, TGP_LIK_SOFTMAX,
 * TGP_LIK_POISSON, TGP_LIK_STUDENT, TGP_LIK_NEGBIN and TGP_LIK_ORDINAL are refused -- all with TGP_E_UNSUPPORTED, tgp_last_error() names the entry.  float64, no float atomics, fixed summation order
 * over s: same input, same bits.
 * TGP_LIK_GAMMA (its #define): the same two entries on the mixture of Gammas, in tau = log t with a = exp(log_var_noise[0]):
 *   F_n(tau) = sum_s wn_s P(a, a e^(tau - g_ns)),  the upper tail sum_s wn_s Q(a, a e^(tau - g_ns)) from its own sum,
 *   F_n'(tau) = sum_s wn_s h(tau - g_ns),  h(z) = exp(a (z - expm1(z)) + [a log a - a - lgamma(a)]),
 * P and Q the regularised lower and upper incomplete gamma functions: the power series for x < a + 1 (P, Q = 1 - P), the
 * modified-Lentz continued fraction otherwise (Q, P = 1 - Q), both with the leading factor h, at most TGP_GAMMA_PQ_MAXIT terms.
 * cdf[n] = F_n(log Y[n]); Y[n] <= 0: cdf = 0, sf = sum wn.  Quantiles: t = exp(tau) in the model's units, the root rule above
 * run on tau (stop rule on tau) for every row -- v <= 0 rows and the empty program too, there is no closed form -- from
 * tau0 = G(mu + zq sqrt v) + s(a, p), s the larger of the Wilson-Hilferty value 3 log(1 - 1/(9a) + zq / (3 sqrt a)) (where its
 * argument is positive) and the small-argument value (log p + lgamma(a + 1)) / a - log a, first step
 * max(1 / sqrt a, 1 / a, |tau0| 2^-20).  Covered: TGP_GAMMA_MIN_SHAPE <= a <= TGP_GAMMA_MAX_SHAPE, v in [0, 4], p in
 * [1e-6, 1 - 1e-6].
 * TGP_LIK_BETA (its #define): the same two entries on the mixture of Betas, in x = logit t with phi = exp(log_var_noise[0]),
 * a_ns = phi sigmoid(g_ns), b_ns = phi sigmoid(-g_ns):
 *   F_n(x) = sum_s wn_s I_t(a_ns, b_ns),  the upper tail sum_s wn_s I_{1-t}(b_ns, a_ns) from its own sum,
 *   F_n'(x) = sum_s wn_s h_ns(x),  h_ns = exp(a_ns log t + b_ns log(1 - t) - log B(a_ns, b_ns)),  log t = -softplus(-x),
 *   log(1 - t) = -softplus(x),
 * I the regularised incomplete beta function by the modified-Lentz continued fraction with h as the front factor, on the side
 * where it converges fast: t < (a + 1) / (a + b + 2): I_t(a, b) = h cf(a, b, t) / a and the other tail 1 - that; else
 * I_{1-t}(b, a) = h cf(b, a, 1 - t) / b and the other tail 1 - that; at most TGP_BETA_CF_MAXIT steps.  Not a location family:
 * a_ns, b_ns and -log B of a row are computed once per row and kept in LDS beside the node values.  cdf[n] = F_n(logit Y[n]);
 * Y[n] <= 0: cdf = 0, sf = sum wn; Y[n] >= 1: cdf = sum wn, sf = 0; NaN stays NaN.  Quantiles: t = sigmoid(x), the root rule
 * above run on x (stop rule on x) for every row -- v <= 0 rows and the empty program too -- from x0 = gq + zq sqrt(1 / a + 1 / b)
 * with a, b those of gq = G(mu + zq sqrt v), first step max(2 / sqrt phi, |x0| 2^-20).  Covered: TGP_BETA_MIN_PRECISION <= phi
 * <= TGP_BETA_MAX_PRECISION, node values |g_ns| <= 12, |x| <= 15, p in [1e-6, 1 - 1e-6]: there a tail >= 1e-60 is within 2e-10
 * of its value, relatively (1.3e-10 measured; 3e-14 for |g_ns| <= 4: the tail that is 1 - the computed one loses digits when
 * the smaller shape parameter, and with it that tail, is tiny).  The root is resolved in x; the returned double t can say no
 * more about 1 - t than its spacing of 2^-53 near 1 allows, and is exactly 1 for x > 36.7. */
#define TGP_QUANTILE_MAX_S 256
#define TGP_QUANTILE_MAX_Q 32
int tgp_predict_quantile_f64(const tgp_model* model, const double* mu, const double* v, const double* rowp, const double* probs,
                             const double* zq, int32_t Q, double* t /* (Q,N) */, int32_t* status, void* stream);
int tgp_predict_cdf_f64(const tgp_model* model, const double* mu, const double* v, const double* rowp, const double* Y,
                        double* cdf /* (N) */, double* sf /* (N), optional */, void* stream);

/* Continuous ranked probability score of the same predictive at Y (TGP_LIK_GAUSS and TGP_LIK_FLOW; model fields and limits
 * as for tgp_predict_cdf_f64, standardised units), CRPS_n = int (F_n(t) - 1{t >= Y_n})^2 dt in closed form.  With
 * g_s = G(mu_n + sqrt(2 max(v_n, 0)) xs_s), sig^2 = exp(log_var_noise[0]) and
 *   a(z) = z erf(z / sqrt 2) + sqrt(2 / pi) exp(-z^2 / 2)      (= z (2 Phi(z) - 1) + 2 phi(z); even, a(z) >= |z|):
 *   T1 = sig sum_s wn_s a((Y_n - g_s) / sig)                                                             (E|Y - y|)
 *   T2 = sig / sqrt(pi) sum_s wn_s^2 + sqrt(2) sig sum_{s<t} wn_s wn_t a((g_s - g_t) / (sqrt(2) sig))    (E|Y - Y'| / 2)
 *   crps[n] = T1 - T2;   parts (optional, (2,N)): T1 in row 0, T2 in row 1, crps = T1 - T2 bit for bit.
 * TGP_LIK_GAUSS or an empty program: one term, sd = sqrt(max(v, 0) + sig^2), z = (Y - mu) / sd, T1 = sd a(z), T2 = sd / sqrt(pi),
 * CRPS = sd (a(z) - 1 / sqrt(pi)).  A row with v <= 0 counts as v = 0 (its nodes coincide; no special case).  The sums are
 * evaluated as written with the caller's wn, nothing is renormalised; every term is positive and a(z) = |z| once the
 * exponential underflows, so targets 1e8 sig away give finite values.  The S node values are computed once per row and kept in
 * LDS; T2 takes each of the S (S - 1) / 2 unordered pairs once, numbered by cyclic offset (pair k: nodes k mod S and
 * (k mod S + k div S + 1) mod S), in a fixed order that does not depend on N: no float atomics, same input, same bits, and a
 * row's value depends on that row's inputs only.  Limits: 1 <= S <= TGP_QUANTILE_MAX_S; every lik but TGP_LIK_GAUSS and
 * TGP_LIK_FLOW is refused -- TGP_E_UNSUPPORTED, tgp_last_error() starts with the entry and names lik = k or S = k.  A null
 * model, mu, v, Y, crps: -1, -2, -3, -5, -6.  Every refusal happens before any launch. */
int tgp_predict_crps_f64(const tgp_model* model, const double* mu, const double* v, const double* rowp, const double* Y,
                         double* crps /* (N) */, double* parts /* (2,N): T1 row 0, T2 row 1; optional */, void* stream);

/* Partial derivatives of tgp_predict_f64's predictive moments in the q(f) marginals (TGP_LIK_GAUSS and TGP_LIK_FLOW; model
 * fields as for tgp_predict_cdf_f64, standardised units).  With f_s = mu_n + sqrt(2 v_n) xs_s, g_s = G(f_s), g'_s = G'(f_s),
 * m1 = sum_s wn_s g_s and m2 = sum_s wn_s g_s^2 - m1^2 + exp(log_var_noise[0]):
 *   dm1[0][n] = d m1 / d mu = sum_s wn_s g'_s             dm1[1][n] = d m1 / d v = sum_s wn_s g'_s xs_s / sqrt(2 v_n)
 *   dm2[0][n] = 2 sum_s wn_s g_s g'_s - 2 m1 dm1[0][n]    dm2[1][n] = 2 sum_s wn_s g_s g'_s xs_s / sqrt(2 v_n) - 2 m1 dm1[1][n]
 * dm1, dm2: (2,N), row 0 the partial in mu, row 1 the partial in v.  TGP_LIK_GAUSS or an empty program: the closed form
 * (1, 0) and (0, 1), no sweep.  A row with v <= 0 counts as v = 0: its v-partials are exact zeros (the clamp's derivative) and
 * its mu-partials come from the one node value.  rowp (N,RP): the partials are taken at fixed per-row parameters.  The sums
 * are evaluated as written with the caller's wn; 16 lanes share a row and add their partial sums in a fixed lane order: no float
 * atomics, same input, same bits.  Limits: 1 <= S <= TGP_QUANTILE_MAX_S; every lik but TGP_LIK_GAUSS and TGP_LIK_FLOW is
 * refused -- TGP_E_UNSUPPORTED, tgp_last_error() starts with the entry and names lik = k or S = k.  A null model, mu, v, dm1,
 * dm2: -1, -2, -3, -5, -6; rowp missing with RP > 0: -4.  Every refusal happens before any launch. */
int tgp_predict_moment_grads_f64(const tgp_model* model, const double* mu, const double* v, const double* rowp,
                                 double* dm1 /* (2,N) */, double* dm2 /* (2,N) */, void* stream);

/* Acquisition functions of Bayesian optimisation on tgp_predict_f64's predictive (TGP_LIK_GAUSS and TGP_LIK_FLOW; model fields
 * as for tgp_predict_cdf_f64, standardised units) against the incumbent `best`: c = +1 (minimize == 0) or -1, sig =
 * exp(log_var_noise[0] / 2), g_s = G(mu_n + sqrt(2 v_n) xs_s), z_s = c (g_s - best) / sig, h(z) = z Phi(z) + phi(z):
 *   TGP_ACQ_EI      value[n] = sig sum_s wn_s h(z_s)                  = E[(c (y - best))_+], the expected improvement
 *   TGP_ACQ_LOG_EI  value[n] = log sig + logsumexp_s(log wn_s + log h(z_s)), finite where EI underflows (weights of 0 do not enter)
 *                   -- as long as one term is finite: where z_s^2 overflows at every node of positive weight (|z_s| > 1.3e154; mu and
 *                   v are not checked) or every weight is 0, the value is -inf and the partials are NaN
 *   TGP_ACQ_PI      value[n] = sum_s wn_s Phi(z_s)                    = P(c (y - best) > 0), the probability of improvement
 * partials (optional, (2,N)): row 0 the partial of value in mu, row 1 in v, at fixed flow parameters (rowp: fixed per-row
 * parameters), g'_s = G'(f_s): d EI / d mu = c sum wn_s Phi(z_s) g'_s, d PI / d mu = (c / sig) sum wn_s phi(z_s) g'_s, d logEI =
 * d EI / EI formed under the running maximum of the log terms with Phi / h from the stable form of h; in v the same sums with
 * g'_s xs_s / sqrt(2 v_n).  log h(z): as written for z > -1; -z^2 / 2 - log sqrt(2 pi) + log1p(z q), q = Phi / phi =
 * sqrt(pi / 2) erfcx(-z / sqrt 2), for -30 < z <= -1; the six-term asymptotic series of 1 + z q in 1 / z^2 for z <= -30.
 * grad_x (optional, (N,D)): grad_x[n,d] = partials[0][n] dmu_dx[n,d] + partials[1][n] dv_dx[n,d], the chain rule with
 * tgp_qf_input_grad_f64's Jacobians dmu_dx, dv_dx (N,D), two products and a sum per element; partials may be NULL with it.
 * TGP_LIK_GAUSS or an empty program: one Gaussian, sd = sqrt(max(v, 0) + sig^2), z = c (mu - best) / sd: EI = sd h(z) with
 * partials (c Phi(z), phi(z) / (2 sd)), PI and log EI likewise.  A row with v <= 0 counts as v = 0: its v-partial is an exact zero.
 * 16 lanes share a row, add their partial sums in a fixed lane order and join their maxima by exchange: no float atomics, same
 * input, same bits, a row's outputs depend on that row's inputs only.  Limits: 1 <= S <= TGP_QUANTILE_MAX_S; every lik but
 * TGP_LIK_GAUSS and TGP_LIK_FLOW, a kind that is none of the three and a `best` that is not finite are refused --
 * TGP_E_UNSUPPORTED, tgp_last_error() starts with the entry and names lik = k, S = k, kind = k or best.  A null model, mu, v,
 * value: -1, -2, -3, -8; rowp missing with RP > 0: -4; with grad_x, a null dmu_dx, dv_dx: -10, -11, and D < 1: -12.  Every
 * refusal happens before any launch. */
#define TGP_ACQ_EI 0
#define TGP_ACQ_LOG_EI 1
#define TGP_ACQ_PI 2
int tgp_predict_acquisition_f64(const tgp_model* model, const double* mu, const double* v, const double* rowp, int32_t kind,
                                double best, int32_t minimize, double* value /* (N) */, double* partials /* (2,N); optional */,
                                const double* dmu_dx /* (N,D) */, const double* dv_dx /* (N,D) */, int32_t D,
                                double* grad_x /* (N,D); optional */, void* stream);

/* Inducing-point initialisation: the numerical kernels behind utils.KMEANS, which replaces
 * sklearn.cluster.KMeans(init='k-means++', n_init, random_state) of dsp/utils.py:143-159.  Random draws, the stopping
 * rule and the restarts stay on the host (tgp/pytorch_amd/utils.py); D <= 16.
 *   assign : labels[n] = argmin_k |x_n - c_k|^2 (first minimum), mind2[n] = that distance (mind2 may be NULL)
 *   segsum : sums[k,:] = sum of the rows X[order[i]], offs[k] <= i < offs[k+1] (rows sorted by label; fixed order)
 *   pp     : out[t,n] = min(closest[n], |x_n - x_cand[t]|^2) for T <= 16 k-means++ trial candidates (closest NULL: +inf) */
int tgp_kmeans_assign_f64(const double* X, int32_t N, int32_t D, const double* C, int32_t K, int32_t* labels, double* mind2,
                          void* stream);
int tgp_kmeans_segsum_f64(const double* X, int32_t D, const int64_t* order, const int64_t* offs, int32_t K, double* sums,
                          void* stream);
int tgp_kmeans_pp_f64(const double* X, int32_t N, int32_t D, const int64_t* cand, int32_t T, const double* closest,
                      double* out, void* stream);

/* The per-row parameter networks of the input-dependent flows: Sinh_ArcsinhFlow's NNets_a / NNets_b,
 * models/flow.py:836-897,949-965 -- `nnets` MLPs of one architecture D -> H (x L hidden layers) -> 1, each layer
 * Linear -> activation -> Dropout(p) (pytorchlib apply_linear, flow.py:853-871; layer order unpinned).
 * Packed weights per net, torch parameter order: [W1 (H,D) | b1 (H) | W2 (H,H) | b2 (H) | ... | Wout (1,H) | bout (1)].
 * Dropout masks are a counter-based hash of (seed, step, net, layer, row, unit); `step_dev` (int32 on the device,
 * e.g. the Adam step counter of tgp_adam_dev_f64; NULL = 0) makes the mask change every step and stay valid under
 * hipGraph replay; forward and backward of one step must see the same value.  H <= 64, L <= 3.  The backward kernel also
 * keeps L activation strips of H x 66 doubles in LDS: a shape whose image exceeds one CU's 160 KiB - 1 KiB is refused by
 * tgp_mlp_backward_f64 / tgp_mlp_backward_adam_f64 with TGP_E_LDS before any launch (L = 3 with H >= 54 at D <= 8; the
 * forward, which has no strips, runs it).  The host restates the size as ops.MlpSpec.lds_bytes(). */
typedef struct tgp_mlp {
  int32_t N, D, H, L, nnets;
  int32_t act;      /* 0 relu, 1 tanh */
  int32_t training; /* != 0: dropout active (set_is_training, models/sparse_MF_SP.py:133-134) */
  int32_t reserved0;
  double drop_p;
  uint64_t seed;
} tgp_mlp;
size_t tgp_mlp_workspace_bytes(const tgp_mlp* mlp);
/* out (N, nnets): column k = output of net k (feeds `rowp` of tgp_elbo_step_f64). */
int tgp_mlp_forward_f64(const tgp_mlp* mlp, const double* X, const double* W, const int32_t* step_dev, double* out,
                        void* stream);
/* g_W (nnets * weights_per_net) = d(objective)/dW given g_out (N, nnets) (= g_rowp of tgp_elbo_step_f64). */
int tgp_mlp_backward_f64(const tgp_mlp* mlp, const double* X, const double* W, const int32_t* step_dev,
                         const double* g_out, double* g_W, void* workspace, size_t workspace_bytes, void* stream);
/* The same followed by the Adam update of the network weights (the reference's second parameter group: names containing
 * 'NNets', weight decay 1e-5, main.py:276-288; torch.optim.Adam, dsp/trainers/optimizers.py:12) in the launch that
 * reduces the weight gradients: adam->params must be W, adam->grads g_W, adam->n the number of weights; adam->step_dev is
 * the group's device step counter (bumped by this call; adam->phases is ignored).  `step_dev` (the dropout masks' step
 * word) may be the same counter: it is read before the bump.  Same arithmetic as tgp_mlp_backward_f64 +
 * tgp_adam_dev_f64(weight_decay). */
int tgp_mlp_backward_adam_f64(const tgp_mlp* mlp, const double* X, double* W, const int32_t* step_dev, const double* g_out,
                              double* g_W, void* workspace, size_t workspace_bytes, const tgp_adam_args* adam,
                              double weight_decay, void* stream);

/* Minibatch rows of a data set resident in HBM -- replaces the per-step host collation + H2D copy of the reference's
 * DataLoader (dsp/data/data.py:86-88, trainers/trainer_base.py:330): Xb[r] = X[index[cursor + offset + r]] and Yb
 * likewise for r < nrows (index NULL: the stored order; entries are row numbers < N).  `cursor_dev` = int32[2]
 * {position in the epoch, ticket}, both 0 at the start of an epoch; the launch advances the position by `advance`
 * and wraps it to 0 when it reaches `wrap`, so a captured launch serves batch after batch under hipGraph replay.
 * `offset` selects a rank's shard inside the batch. */
int tgp_gather_rows_f64(const double* X, const double* Y, int32_t N, int32_t D, const int32_t* index, int32_t* cursor_dev,
                        int32_t offset, int32_t nrows, int32_t advance, int32_t wrap, double* Xb, double* Yb, void* stream);

/* Adam on a flat parameter buffer (torch.optim.Adam semantics, dsp/trainers/optimizers.py:12; L2 weight decay
 * added to the gradient as torch does).  `maximize` != 0 ascends (gradients here are of +ELBO). */
int tgp_adam_f64(double* params, const double* grads, double* exp_avg, double* exp_avg_sq, int64_t n, double lr,
                 double beta1, double beta2, double eps, double weight_decay, int32_t step, int32_t maximize,
                 void* stream);

/* Graph-capturable Adam: the step count lives on the device (`step_dev`, int32[2] = {step, ticket}, both start at
 * 0) so that a captured launch stays valid across replays; the call uses step = step_dev[0] + 1 and the last
 * workgroup to finish increments the counter. */
int tgp_adam_dev_f64(double* params, const double* grads, double* exp_avg, double* exp_avg_sq, int64_t n, double lr,
                     double beta1, double beta2, double eps, double weight_decay, int32_t* step_dev, int32_t maximize,
                     void* stream);

/* tgp_adam_dev_f64 with two parameter groups in one buffer: elements [0, n_plain) without weight decay, elements
 * [n_plain, n) with `weight_decay_tail` -- the reference's optimiser groups (main.py:276-288: weight decay 1e-5 on
 * the parameters whose name contains 'NNets'). */
int tgp_adam_dev_groups_f64(double* params, const double* grads, double* exp_avg, double* exp_avg_sq, int64_t n,
                            double lr, double beta1, double beta2, double eps, int64_t n_plain, double weight_decay_tail,
                            int32_t* step_dev, int32_t maximize, void* stream);

/* ---- the collective of the data-parallel step (ONE sum all-reduce of the flat [gradients | ELBO, ELL, KL]
 * buffer per step over RCCL / xGMI; the reference itself is single-device, trainers/trainer_base.py:329-349) ----
 * One process per GPU, one communicator per process.  RCCL is bound at run time: tgp_comm_load(path) dlopens it
 * (NULL = "librccl.so" by the loader's rules; a process that imported torch already holds torch/lib/librccl.so), every
 * other entry point of this library works without it.  Rank 0 draws a 128-byte id (tgp_comm_unique_id), the host
 * distributes it (any channel: a file, MPI, torch.distributed's store), every rank calls tgp_comm_init on its device;
 * tgp_allreduce_f64 sums `buf` (n doubles, device memory) in place across the ranks ON `stream` -- stream-ordered like
 * the kernels, valid under stream capture, so the step [kernels -> all-reduce -> Adam] can be ONE captured graph with
 * no side stream.  The C ABI's counterpart of engine.allreduce_flat (torch.distributed, backend nccl = RCCL), which
 * stays the default of the Python engine.  Errors: TGP_E_COMM + tgp_last_error(). */
int tgp_comm_load(const char* rccl_path);
int tgp_comm_unique_id(void* id128);
int tgp_comm_init(const void* id128, int32_t nranks, int32_t rank, void** comm);
int tgp_allreduce_f64(void* comm, double* buf, int64_t n, void* stream);
int tgp_comm_destroy(void* comm);

#ifdef __cplusplus
}
#endif
#endif /* TGP_HIP_H */
