"""ctypes binding of libtgp_hip.so (C ABI declared in include/tgp_hip.h).

The product path has no CPU fallback: if the HIP library is missing or a call fails, this module
raises.  PyTorch is used only as the owner of device memory and streams.
"""
import ctypes as C
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libtgp_hip.so")

FLOW_AFFINE, FLOW_SAL, FLOW_STEPTANH = 0, 1, 2
FLOW_ARCSINH, FLOW_BOXCOX, FLOW_INV_BOXCOX = 3, 4, 5
FLOW_SINH, FLOW_NORMCDF, FLOW_TUKEY, FLOW_EXP, FLOW_SOFTPLUS = 7, 8, 9, 10, 11    # (6 is unassigned and refused)
FLAG_RESTRICT, FLAG_ADD_F0, FLAG_PER_ROW = 1, 2, 4
FLAG_NEGATE = 8             # TUKEY only, with FLAG_RESTRICT: gamma = -softplus(raw) (tukey_left)
LIK_GAUSS, LIK_FLOW = 0, 1
LIK_BERNOULLI = 3           # probit link through the flow (TGP_LIK_BERNOULLI)
LIK_WARPED = 4              # the flow warps the targets (TGP_LIK_WARPED)
LIK_SOFTMAX = 5             # softmax over C latent GPs (TGP_LIK_SOFTMAX): the stand-alone tgp_ell_softmax_f64 only
LIK_POISSON = 6             # counts, the flow as the log-rate (TGP_LIK_POISSON)
LIK_STUDENT = 7             # Student-t noise around the flow (TGP_LIK_STUDENT): log_var_noise = {log sigma^2, nu}
LIK_HETERO = 8              # heteroscedastic Gaussian, a second latent GP for the log-noise (TGP_LIK_HETERO): tgp_ell_hetero_f64 only
LIK_NEGBIN = 9              # negative-binomial counts, the flow as the log-mean (TGP_LIK_NEGBIN): log_var_noise = log r
# what a message calls the likelihoods that go through a FlowSpec on the eager path only (the step engines have none of them)
LIK_ORDINAL = 10            # ordered classes, cumulative probit around the flow (TGP_LIK_ORDINAL): log_var_noise = {log sigma^2, K, edges}
LIK_GAMMA = 11              # positive targets, Gamma noise with the flow as the log-mean (TGP_LIK_GAMMA): log_var_noise = log shape
LIK_BETA = 12               # proportions in (0, 1), Beta noise with the flow as the log-odds of the mean (TGP_LIK_BETA): log_var_noise = log precision
LIK_DISPLAY = {LIK_BERNOULLI: "Bernoulli", LIK_POISSON: "Poisson", LIK_STUDENT: "Student-t", LIK_NEGBIN: "negative-binomial",
               LIK_ORDINAL: "ordinal", LIK_GAMMA: "Gamma", LIK_BETA: "Beta"}
NEEDS_FLOWSPEC = "the %s likelihood needs a FlowSpec (an empty one for the identity flow)"
STUDENT_MAX_DF = 1e4       # the supported degrees of freedom are 2 < nu <= STUDENT_MAX_DF (include/tgp_hip.h)
GAMMA_MIN_SHAPE, GAMMA_MAX_SHAPE = 0.1, 1e3   # the supported shapes of LIK_GAMMA (include/tgp_hip.h)
BETA_MIN_PRECISION, BETA_MAX_PRECISION = 0.5, 1e3   # the supported precisions of LIK_BETA (include/tgp_hip.h)
BETA_CF_MAXIT = 174        # most steps of the incomplete beta function's continued fraction (TGP_BETA_CF_MAXIT)
GAMMA_PQ_MAXIT = 2048      # most terms of the incomplete gamma function's series / continued fraction (TGP_GAMMA_PQ_MAXIT)
ORDINAL_MAX_K = 64         # the supported number of classes is 2 <= K <= ORDINAL_MAX_K (include/tgp_hip.h)
SOFTMAX_MAX_C, SOFTMAX_MAX_S = 32, 256
QUANTILE_MAX_S, QUANTILE_MAX_Q = 256, 32   # tgp_predict_quantile_f64 / tgp_predict_cdf_f64
ACQ_EI, ACQ_LOG_EI, ACQ_PI = 0, 1, 2      # tgp_predict_acquisition_f64's kind (TGP_ACQ_*)
ACQ_KINDS = {"ei": ACQ_EI, "log_ei": ACQ_LOG_EI, "pi": ACQ_PI}
PATHWISE_MAX_R2, PATHWISE_MAX_S = 8192, 256  # tgp_pathwise_coeff_f64 / tgp_pathwise_eval_f64
XGRAD_PASS_ROWS = 16384    # rows per pass of tgp_qf_input_grad_f64 (TGP_XGRAD_PASS_ROWS)
BIG_MAX_M = 4096           # the most inducing points any entry serves (TGP_BIG_MAX_M)
E_UNSUPPORTED = -100
E_WORKSPACE = -101

_dp = C.c_void_p


KERNEL_SCALE_RBF, KERNEL_SCALE_MATERN32, KERNEL_SCALE_RQ, KERNEL_SCALE_MATERN52 = 0, 1, 3, 5      # (2 and 4: not assigned, refused)
KERNELS = {"scale_rbf": KERNEL_SCALE_RBF, "scale_matern32": KERNEL_SCALE_MATERN32, "scale_matern52": KERNEL_SCALE_MATERN52,
           "scale_rq": KERNEL_SCALE_RQ}
RQ_MIN_ALPHA, RQ_MAX_ALPHA = 1e-2, 1e4   # the supported alpha of 'scale_rq' (include/tgp_hip.h); its raw_os is {raw_outputscale, alpha}
# tgp_model.plan (include/tgp_hip.h TGP_PLAN_*): kernel-selection overrides of ONE call; 0 = the library's choice
PLAN_ROWS_AUTO, PLAN_ROWS_K16, PLAN_ROWS_K, PLAN_ROWS4_NW4, PLAN_ROWS4_NW8 = 0, 1, 2, 3, 4
PLAN_NO_CHUNK_OVERLAP = 16
PLAN_FULL_PAD = 32        # fused path: k_bwd contracts over the padding of M as well (A/B switch; same results bit for bit)


def plan_chunk_rows(n):
    """TGP_PLAN_CHUNK_ROWS(n): row chunks of at most n rows on the general-M path."""
    return (((int(n) + 127) // 128) & 0xffff) << 8


class TgpModel(C.Structure):
    _fields_ = [("N", C.c_int32), ("D", C.c_int32), ("M", C.c_int32), ("S", C.c_int32), ("nblk", C.c_int32),
                ("P", C.c_int32), ("RP", C.c_int32), ("lik", C.c_int32), ("kernel", C.c_int32), ("plan", C.c_int32),
                ("scale", C.c_double),
                ("jitter", C.c_double), ("kl_scale", C.c_double), ("jitter_ladder", C.c_double), ("Z", _dp), ("raw_ls", _dp), ("raw_os", _dp),
                ("m", _dp), ("Lam", _dp), ("log_var_noise", _dp), ("theta", _dp), ("program", _dp), ("xs", _dp),
                ("wn", _dp)]


class TgpGrads(C.Structure):
    _fields_ = [("Z", _dp), ("raw_ls", _dp), ("raw_os", _dp), ("m", _dp), ("Lam", _dp), ("log_var_noise", _dp),
                ("theta", _dp), ("rowp", _dp)]


class TgpAdamArgs(C.Structure):
    _fields_ = [("params", _dp), ("grads", _dp), ("exp_avg", _dp), ("exp_avg_sq", _dp), ("n", C.c_int64), ("lr", C.c_double),
                ("beta1", C.c_double), ("beta2", C.c_double), ("eps", C.c_double), ("step_dev", _dp), ("maximize", C.c_int32),
                ("phases", C.c_uint32)]


class TgpMlp(C.Structure):
    _fields_ = [("N", C.c_int32), ("D", C.c_int32), ("H", C.c_int32), ("L", C.c_int32), ("nnets", C.c_int32),
                ("act", C.c_int32), ("training", C.c_int32), ("reserved0", C.c_int32), ("drop_p", C.c_double),
                ("seed", C.c_uint64)]


class TgpSoftmax(C.Structure):
    _fields_ = [("N", C.c_int32), ("C", C.c_int32), ("S", C.c_int32), ("reserved0", C.c_int32), ("program", _dp),
                ("blk_off", _dp), ("theta", _dp), ("theta_off", _dp), ("scale", C.c_double), ("seed", C.c_uint64),
                ("step_dev", _dp), ("row0", C.c_int64)]


class TgpGemmEx(C.Structure):
    # (the field order is the code of a refusal: -(position, counted from 1))
    _fields_ = [("trans_a", C.c_int32), ("trans_b", C.c_int32), ("tri", C.c_int32), ("m", C.c_int32), ("n", C.c_int32),
                ("k", C.c_int32), ("alpha", C.c_double), ("A", _dp), ("lda", C.c_int32), ("B", _dp), ("ldb", C.c_int32),
                ("beta", C.c_double), ("C", _dp), ("ldc", C.c_int32), ("a_mul", _dp), ("k_scale", _dp), ("add", _dp),
                ("ldadd", C.c_int32), ("gamma", C.c_double), ("col_scale", _dp), ("row_scale", _dp), ("rowv", _dp),
                ("colv", _dp), ("ksplit", C.c_int32), ("cz", C.c_size_t), ("xcd", C.c_int32), ("scratch", _dp),
                ("scratch_doubles", C.c_size_t)]


GEMM_ROUTE_128, GEMM_ROUTE_128_PAIRED, GEMM_ROUTE_128_HEAVY, GEMM_ROUTE_128_TRIANGLE, GEMM_ROUTE_64 = 0, 1, 2, 3, 4


class TgpError(RuntimeError):
    pass


_lib = None

_SIGS = {
    "tgp_version": (C.c_int, []),
    "tgp_last_error": (C.c_char_p, []),
    "tgp_source_hash": (C.c_char_p, []),
    "tgp_workspace_bytes": (C.c_size_t, [C.c_int32] * 7),
    "tgp_workspace_bytes_kernel": (C.c_size_t, [C.c_int32] * 8),
    "tgp_workspace_bytes_plan": (C.c_size_t, [C.c_int32] * 9),
    "tgp_workspace_bytes_lik": (C.c_size_t, [C.c_int32] * 10),
    "tgp_kernel_matrix_f64": (C.c_int, [C.c_int32, _dp, C.c_int32, _dp, C.c_int32, C.c_int32, _dp, _dp, C.c_double, _dp, _dp]),
    "tgp_elbo_step_f64": (C.c_int, [C.POINTER(TgpModel), _dp, _dp, _dp, _dp, C.POINTER(TgpGrads), _dp, _dp, _dp, _dp,
                                    C.c_size_t, _dp]),
    "tgp_elbo_step_phases_f64": (C.c_int, [C.POINTER(TgpModel), _dp, _dp, _dp, _dp, C.POINTER(TgpGrads), _dp, _dp, _dp,
                                           _dp, C.c_size_t, C.c_uint32, _dp]),
    "tgp_elbo_step_adam_f64": (C.c_int, [C.POINTER(TgpModel), _dp, _dp, _dp, _dp, C.POINTER(TgpGrads), _dp, _dp, _dp, _dp,
                                         C.c_size_t, C.POINTER(TgpAdamArgs), _dp]),
    "tgp_qf_moments_f64": (C.c_int, [C.POINTER(TgpModel), _dp, _dp, _dp, _dp, _dp, C.c_size_t, _dp]),
    "tgp_qf_cov_workspace_bytes": (C.c_size_t, [C.c_int32] * 3),
    "tgp_qf_cov_f64": (C.c_int, [C.POINTER(TgpModel), _dp, _dp, _dp, _dp, _dp, C.c_size_t, _dp]),
    "tgp_qf_input_grad_workspace_bytes": (C.c_size_t, [C.c_int32] * 3),
    "tgp_qf_input_grad_f64": (C.c_int, [C.POINTER(TgpModel), _dp, _dp, _dp, _dp, _dp, C.c_size_t, _dp]),
    "tgp_qf_input_grad_var_workspace_bytes": (C.c_size_t, [C.c_int32] * 3),
    "tgp_qf_input_grad_var_f64": (C.c_int, [C.POINTER(TgpModel), _dp, _dp, _dp, _dp, C.c_size_t, _dp]),
    "tgp_predict_moment_grads_f64": (C.c_int, [C.POINTER(TgpModel), _dp, _dp, _dp, _dp, _dp, _dp]),
    "tgp_predict_acquisition_f64": (C.c_int, [C.POINTER(TgpModel), _dp, _dp, _dp, C.c_int32, C.c_double, C.c_int32, _dp, _dp, _dp,
                                              _dp, C.c_int32, _dp, _dp]),
    "tgp_qf_joint_sample_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32]),
    "tgp_qf_joint_sample_f64": (C.c_int, [_dp, _dp, C.c_int32, C.c_double, _dp, C.c_int32, _dp, _dp, _dp, _dp, C.c_size_t, _dp]),
    "tgp_mlp_backward_adam_f64": (C.c_int, [C.POINTER(TgpMlp), _dp, _dp, _dp, _dp, _dp, _dp, C.c_size_t, C.POINTER(TgpAdamArgs),
                                            C.c_double, _dp]),
    "tgp_comm_load": (C.c_int, [C.c_char_p]),
    "tgp_comm_unique_id": (C.c_int, [_dp]),
    "tgp_comm_init": (C.c_int, [_dp, C.c_int32, C.c_int32, C.POINTER(C.c_void_p)]),
    "tgp_allreduce_f64": (C.c_int, [_dp, _dp, C.c_int64, _dp]),
    "tgp_comm_destroy": (C.c_int, [_dp]),
    "tgp_qf_moments_bwd_f64": (C.c_int, [C.POINTER(TgpModel), _dp, _dp, _dp, C.POINTER(TgpGrads), _dp, _dp, C.c_size_t, _dp]),
    "tgp_kmm_f64": (C.c_int, [_dp, _dp, _dp, C.c_int32, C.c_int32, C.c_double, _dp, _dp]),
    "tgp_knm_f64": (C.c_int, [_dp, _dp, _dp, _dp, C.c_int32, C.c_int32, C.c_int32, _dp, _dp]),
    "tgp_cholesky_f64": (C.c_int, [_dp, C.c_int32, _dp, _dp, _dp, _dp, C.c_size_t, _dp]),
    "tgp_gemm_f64": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_double, _dp, C.c_int32,
                               _dp, C.c_int32, C.c_double, _dp, C.c_int32, _dp]),
    "tgp_gemm_ex_f64": (C.c_int, [C.POINTER(TgpGemmEx), _dp]),
    "tgp_gemm_pair_ex_f64": (C.c_int, [C.POINTER(TgpGemmEx), C.POINTER(TgpGemmEx), _dp]),
    "tgp_gemm_route": (C.c_int, [C.POINTER(TgpGemmEx)]),
    "tgp_cholesky_workspace_bytes": (C.c_size_t, [C.c_int32]),
    "tgp_cholesky_bwd_workspace_bytes": (C.c_size_t, [C.c_int32]),
    "tgp_cholesky_bwd_f64": (C.c_int, [_dp, _dp, _dp, C.c_int32, _dp, _dp, C.c_size_t, _dp]),
    "tgp_unwhiten_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32]),
    "tgp_unwhiten_f64": (C.c_int, [C.c_int32, _dp, _dp, _dp, C.c_int32, C.c_int32, C.c_double, _dp, _dp, _dp, _dp, _dp, _dp, _dp,
                                   _dp, C.c_size_t, _dp]),
    "tgp_unwhiten_bwd_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32]),
    "tgp_unwhiten_bwd_f64": (C.c_int, [C.c_int32, _dp, _dp, _dp, C.c_int32, C.c_int32] + [_dp] * 12 + [C.c_size_t, _dp]),
    "tgp_optimal_qu_workspace_bytes": (C.c_size_t, [C.c_int32] * 3),
    "tgp_optimal_qu_f64": (C.c_int, [C.POINTER(TgpModel), _dp, _dp, _dp, _dp, _dp, _dp, C.c_size_t, _dp]),
    "tgp_kxxk_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32]),
    "tgp_kxxk_f64": (C.c_int, [C.c_int32, _dp, C.c_int32, _dp, C.c_int32, C.c_int32, _dp, _dp, _dp, _dp, _dp, _dp, C.c_size_t,
                               _dp]),
    "tgp_kxwxk_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32]),
    "tgp_kxwxk_f64": (C.c_int, [C.c_int32, _dp, C.c_int32, _dp, C.c_int32, C.c_int32, _dp, _dp, _dp, _dp, _dp, _dp, _dp,
                                C.c_size_t, _dp]),
    "tgp_natgrad_qu_workspace_bytes": (C.c_size_t, [C.c_int32] * 3),
    "tgp_natgrad_qu_f64": (C.c_int, [C.POINTER(TgpModel), _dp, _dp, _dp, _dp, C.c_double, C.c_double, _dp, _dp, _dp, _dp,
                                     C.c_size_t, _dp]),
    "tgp_greedy_inducing_workspace_bytes": (C.c_size_t, [C.c_int32] * 3),
    "tgp_greedy_inducing_f64": (C.c_int, [_dp, C.c_int32, C.c_int32, _dp, _dp, C.c_int32, C.c_int32, C.c_double, _dp, _dp, _dp, _dp,
                                          _dp, C.c_size_t, _dp]),
    "tgp_pathwise_workspace_bytes": (C.c_size_t, [C.c_int32] * 5),
    "tgp_pathwise_coeff_f64": (C.c_int, [C.POINTER(TgpModel), _dp, C.c_int32, _dp, _dp, C.c_int32, _dp, _dp, _dp, C.c_size_t, _dp]),
    "tgp_pathwise_eval_f64": (C.c_int, [C.c_int32, _dp, C.c_int32, C.c_int32, _dp, C.c_int32, _dp, _dp, _dp, C.c_int32, _dp,
                                        C.c_int32, _dp, _dp]),
    "tgp_pathwise_grad_f64": (C.c_int, [C.c_int32, _dp, C.c_int32, C.c_int32, _dp, C.c_int32, _dp, _dp, _dp, C.c_int32, _dp,
                                        C.c_int32, _dp, _dp]),
    "tgp_mean_forward_f64": (C.c_int, [_dp, C.c_int32, C.c_int32, _dp, _dp, C.c_double, _dp, _dp, C.c_int32, C.c_int32, C.c_int32,
                                       _dp]),
    "tgp_mean_backward_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32]),
    "tgp_mean_backward_f64": (C.c_int, [_dp, C.c_int32, C.c_int32, _dp, _dp, C.c_int32, C.c_int32, _dp, _dp, _dp, _dp, C.c_size_t,
                                        _dp]),
    "tgp_ell_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32, C.c_int32]),
    "tgp_kl_whitened_f64": (C.c_int, [_dp, _dp, C.c_int32, _dp, _dp, _dp, _dp]),
    "tgp_ell_gauss_f64": (C.c_int, [_dp, _dp, _dp, C.c_int32, _dp, C.c_double, _dp, _dp, _dp, _dp, C.c_size_t, _dp]),
    "tgp_ell_flow_f64": (C.c_int, [C.POINTER(TgpModel), _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp, C.c_size_t,
                                   _dp]),
    "tgp_ell_hetero_f64": (C.c_int, [C.POINTER(TgpModel), _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp, C.c_size_t,
                                     _dp]),
    "tgp_predict_hetero_f64": (C.c_int, [C.POINTER(TgpModel), _dp, _dp, _dp, _dp, C.c_double, _dp, _dp, _dp, _dp]),
    "tgp_flow_eval_f64": (C.c_int, [C.POINTER(TgpModel), _dp, C.c_int32, C.c_int32, _dp, _dp, _dp, _dp, _dp]),
    "tgp_flow_logdet_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32]),
    "tgp_flow_logdet_f64": (C.c_int, [C.POINTER(TgpModel), _dp, C.c_int32, C.c_int32, _dp, _dp, _dp, _dp, C.c_size_t, _dp]),
    "tgp_ell_warp_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32]),
    "tgp_ell_warp_f64": (C.c_int, [C.POINTER(TgpModel), _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp, C.c_size_t, _dp]),
    "tgp_ell_softmax_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32]),
    "tgp_ell_softmax_f64": (C.c_int, [C.POINTER(TgpSoftmax), _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp, C.c_size_t, _dp]),
    "tgp_mc_normals_f64": (C.c_int, [C.POINTER(TgpSoftmax), _dp, _dp]),
    "tgp_predict_softmax_f64": (C.c_int, [C.POINTER(TgpSoftmax), _dp, _dp, _dp, _dp, _dp, _dp, _dp]),
    "tgp_flow_inverse_f64": (C.c_int, [C.POINTER(TgpModel), _dp, C.c_int32, C.c_int32, _dp, _dp, _dp, _dp]),
    "tgp_predict_f64": (C.c_int, [C.POINTER(TgpModel), _dp, _dp, _dp, _dp, C.c_double, _dp, _dp, _dp, _dp]),
    "tgp_predict_quantile_f64": (C.c_int, [C.POINTER(TgpModel), _dp, _dp, _dp, _dp, _dp, C.c_int32, _dp, _dp, _dp]),
    "tgp_predict_cdf_f64": (C.c_int, [C.POINTER(TgpModel), _dp, _dp, _dp, _dp, _dp, _dp, _dp]),
    "tgp_predict_crps_f64": (C.c_int, [C.POINTER(TgpModel), _dp, _dp, _dp, _dp, _dp, _dp, _dp]),
    "tgp_kmeans_assign_f64": (C.c_int, [_dp, C.c_int32, C.c_int32, _dp, C.c_int32, _dp, _dp, _dp]),
    "tgp_kmeans_segsum_f64": (C.c_int, [_dp, C.c_int32, _dp, _dp, C.c_int32, _dp, _dp]),
    "tgp_kmeans_pp_f64": (C.c_int, [_dp, C.c_int32, C.c_int32, _dp, C.c_int32, _dp, _dp, _dp]),
    "tgp_mlp_workspace_bytes": (C.c_size_t, [C.POINTER(TgpMlp)]),
    "tgp_mlp_forward_f64": (C.c_int, [C.POINTER(TgpMlp), _dp, _dp, _dp, _dp, _dp]),
    "tgp_mlp_backward_f64": (C.c_int, [C.POINTER(TgpMlp), _dp, _dp, _dp, _dp, _dp, _dp, C.c_size_t, _dp]),
    "tgp_gather_rows_f64": (C.c_int, [_dp, _dp, C.c_int32, C.c_int32, _dp, _dp, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _dp,
                                      _dp, _dp]),
    "tgp_adam_dev_groups_f64": (C.c_int, [_dp, _dp, _dp, _dp, C.c_int64, C.c_double, C.c_double, C.c_double, C.c_double,
                                          C.c_int64, C.c_double, _dp, C.c_int32, _dp]),
    "tgp_adam_f64": (C.c_int, [_dp, _dp, _dp, _dp, C.c_int64, C.c_double, C.c_double, C.c_double, C.c_double,
                               C.c_double, C.c_int32, C.c_int32, _dp]),
    "tgp_adam_dev_f64": (C.c_int, [_dp, _dp, _dp, _dp, C.c_int64, C.c_double, C.c_double, C.c_double, C.c_double,
                                   C.c_double, _dp, C.c_int32, _dp]),
}

EXPORTS = tuple(_SIGS.keys())


def source_hash():
    """sha256[:16] of the kernel sources in the tree, computed like the csrc Makefile does (sorted *.hip, *.hpp, then
    include/tgp_hip.h); None when the sources are not next to the library (a binary-only install)."""
    import glob
    import hashlib
    csrc = os.path.join(_HERE, "csrc")
    hdr = os.path.join(_HERE, "..", "..", "include", "tgp_hip.h")
    files = sorted(glob.glob(os.path.join(csrc, "*.hip")) + glob.glob(os.path.join(csrc, "*.hpp")),
                   key=lambda f: os.path.basename(f))
    if not files or not os.path.exists(hdr):
        return None
    h = hashlib.sha256()
    for f in files + [hdr]:
        with open(f, "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()[:16]


def load():
    """Load libtgp_hip.so once; raise (never fall back) when it is absent or was built from other sources than the
    ones in the tree (the binary is git-ignored and travels beside them: a stale one must not pass for the product)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise TgpError("libtgp_hip.so not built: run `python -c 'import __graft_entry__ as g; g.build()'` "
                           "or `make -C tgp/pytorch_amd/csrc` (%s)" % LIB_PATH)
        lib = C.CDLL(LIB_PATH)
        for name, (res, args) in _SIGS.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        want, have = source_hash(), lib.tgp_source_hash().decode()
        if want is not None and have != want and not os.environ.get("TGP_ALLOW_STALE_LIB"):
            raise TgpError("libtgp_hip.so is stale: built from sources %s, the tree has %s -- rebuild with "
                           "`make -C tgp/pytorch_amd/csrc`" % (have, want))
        _lib = lib
    return _lib


def check(rc, what):
    if rc != 0:
        msg = load().tgp_last_error().decode() if rc in (-103, E_UNSUPPORTED, E_WORKSPACE) else ""
        raise TgpError("%s failed with code %d %s" % (what, rc, msg))


def ptr(t):
    """Device pointer of a contiguous float64/int32 CUDA(HIP) tensor, or NULL."""
    if t is None:
        return None
    if not t.is_cuda:
        raise TgpError("tensor must live on the GPU (got %s)" % t.device)
    if not t.is_contiguous():
        raise TgpError("tensor must be contiguous")
    return C.c_void_p(t.data_ptr())


def stream_ptr():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)
