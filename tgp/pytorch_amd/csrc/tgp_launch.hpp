// tgp_launch.hpp -- host-side launcher declarations shared by the translation units of libtgp_hip.so
#pragma once
#include "tgp_dev.hpp"

namespace tgp {

int set_error(hipError_t e, const char* file, int line);  // records tgp_last_error(), returns TGP_E_LAUNCH
void set_error_text(const char* fmt, ...);                // records tgp_last_error()

// after a kernel launch, in a launcher that returns the ABI's int: a failed launch is recorded and returned
#define LAUNCH_CHECK()                                              \
  do {                                                              \
    hipError_t e_ = hipGetLastError();                              \
    if (e_ != hipSuccess) return set_error(e_, __FILE__, __LINE__); \
  } while (0)

// tgp_comm.hip (RCCL bound at run time)
int comm_load(const char* path);
int comm_unique_id(void* id128);
int comm_init(const void* id128, int nranks, int rank, void** comm);
int comm_allreduce(void* comm, double* buf, int64_t n, hipStream_t st);
int comm_destroy(void* comm);

// Raise a kernel's dynamic-LDS ceiling when a launch needs more than the 64 KiB default (gfx950: 160 KiB/CU).
// `cur` is the caller's per-kernel high-water mark.  Returns 0 or TGP_E_LDS.
inline int ensure_lds(const void* func, size_t bytes, size_t* cur) {
  if (bytes <= *cur) return 0;
  if (bytes > 160 * 1024 - 1024) return TGP_E_LDS;  // leave room for the static __shared__ words
  const size_t want = bytes > 63 * 1024 ? 160 * 1024 - 1024 : 63 * 1024;
  hipError_t e = hipFuncSetAttribute(func, hipFuncAttributeMaxDynamicSharedMemorySize, (int)want);
  if (e != hipSuccess) { (void)hipGetLastError(); return set_error(e, __FILE__, __LINE__); }
  *cur = want;
  return 0;
}

// tgp_mm.hip
int launch_prepare(const Plan& p, const tgp_model& md, const FlowProg& fp, double* ws, int32_t* status, hipStream_t st);
// Adam folded into the backward launches of the fused path (tgp_elbo_step_adam_f64); p == nullptr: none
struct AdamDev {
  double* p = nullptr;
  const double* g = nullptr;
  double* m = nullptr;
  double* v = nullptr;
  long n = 0, lam_off = 0, lam_n = 0;  // [lam_off, lam_off + lam_n): the q(u) factor's entries, updated beside the K_MM adjoint
  double lr = 0, b1 = 0, b2 = 0, eps = 0, ln_b1 = 0, ln_b2 = 0, sign = 1;
  int32_t* step_dev = nullptr;
};
int launch_backward_mm(const Plan& p, const tgp_model& md, const tgp_grads& g, double* out, double* ws, int32_t* status,
                       hipStream_t st, const AdamDev* adam = nullptr);
int launch_kmm(const double* Z, const double* raw_ls, const double* raw_os, int M, int D, double jitter, double* K,
               hipStream_t st);
int launch_knm(const double* X, const double* Z, const double* raw_ls, const double* raw_os, int N, int M, int D,
               double* K, hipStream_t st);
int launch_kernel_matrix(int kernel, const double* X1, int N1, const double* X2, int N2, int D, const double* raw_ls,
                         const double* raw_os, double jitter, double* K, hipStream_t st);
int launch_kl(const double* m, const double* Lam, int M, double* out, double* g_m, double* g_Lam, hipStream_t st);
int launch_cholesky(const double* A, int M, double* L, double* Linv, int32_t* status, hipStream_t st);

// tgp_rows.hip
// which row kernel a plan gets: 0 = k_rows (16 rows per wave), else the waves per workgroup of k_rows4 (4 rows per wave)
int choose_rows4(const Plan& p, bool train, int sel = 0);
// data rows per wave of k_rows for this plan (16, or 10: training with the flow likelihood at Power-like sizes)
int rows_per_wave(const Plan& p, const FlowProg& fp, bool train, int sel = 0);
// does the training launch of the row kernel fit a CU's LDS with `nslots` flow-stack slots (its leanest form: one node in flight)?
bool rows_train_lds_fits(const Plan& p, int nslots);
int launch_rows(const Plan& p, const tgp_model& md, const FlowProg& fp, const double* X, const double* Y,
                const double* rowp, double* g_rowp, double* mu, double* v, double* ws, bool train, hipStream_t st);

// tgp_big.hip (general-M path, 128 < M <= TGP_BIG_MAX_M)
size_t big_workspace_doubles(int N, int D, int M, int S, int nblk, int P, int RP, int kernel, int plan = 0);
int launch_big_step(const tgp_model& md, const FlowProg& fp, const double* X, const double* Y, const double* rowp,
                    double* out, const tgp_grads& g, double* mu, double* v, int32_t* status, double* ws, size_t ws_doubles,
                    uint32_t phases, hipStream_t st, const AdamDev* adam = nullptr);
int launch_big_moments(const tgp_model& md, const double* X, double* mu, double* v, int32_t* status, double* ws,
                       size_t ws_doubles, hipStream_t st);
size_t big_cholesky_workspace_doubles(int M);
int launch_big_cholesky(const double* A, int M, double* Lo, double* Jo, int32_t* status, double* ws, size_t ws_doubles,
                        hipStream_t st);
int launch_big_cholesky_bwd(const double* L, const double* Linv, const double* Lbar, int M, double* Abar, double* ws,
                            size_t ws_doubles, hipStream_t st);
int launch_gemm_plain(bool ta, bool tb, int tri, int m, int n, int k, double alpha, const double* A, int lda, const double* B,
                      int ldb, double beta, double* C, int ldc, hipStream_t st);
// the descriptor entries (arguments checked by the caller): launch_gemm, or gemm_mm_on's split-K + reduction when d.scratch
// is given; launch_gemm_pair_ft_ff; the route launch_gemm would take (TGP_GEMM_ROUTE_*, -1 where it refuses)
int launch_gemm_ex(const tgp_gemm_ex& d, hipStream_t st);
int launch_gemm_pair_ex(const tgp_gemm_ex& a, const tgp_gemm_ex& b, hipStream_t st);
int gemm_route_ex(const tgp_gemm_ex& d);

// One factorisation for every M <= TGP_BIG_MAX_M: the single-workgroup kernel up to TGP_FUSED_MAX_M, above it the blocked one,
// which alone needs scratch -- chol_ws_doubles(M) doubles at `cws`, a whole number of 64-double sections.
inline size_t chol_ws_doubles(int M) { return M > TGP_FUSED_MAX_M ? rup(big_cholesky_workspace_doubles(M), 64) : 0; }
inline int launch_cholesky_any(const double* A, int M, double* L, double* Linv, int32_t* status, double* cws, size_t cws_len,
                               hipStream_t st) {
  if (M > TGP_FUSED_MAX_M) return launch_big_cholesky(A, M, L, Linv, status, cws, cws_len, st);
  return launch_cholesky(A, M, L, Linv, status, st);
}
// Kmm = K_ZZ + jitter I, then its factor L and L^-1 with `status`: how every operator on the inducing points opens
inline int launch_kzz_factor(int kernel, const double* Z, const double* raw_ls, const double* raw_os, int M, int D, double jitter,
                             double* Kmm, double* L, double* Linv, int32_t* status, double* cws, size_t cws_len, hipStream_t st) {
  if (int rc = launch_kernel_matrix(kernel, Z, M, nullptr, 0, D, raw_ls, raw_os, jitter, Kmm, st)) return rc;
  return launch_cholesky_any(Kmm, M, L, Linv, status, cws, cws_len, st);
}

// The workspace of a stand-alone operator (tgp_cov.hip, tgp_unwhiten.hip, tgp_optqu.hip): sections of whole 64-double blocks,
// laid out in the order they are taken.  Its byte count carries 16 bytes of slack for open_workspace.
struct Layout {
  size_t total = 0;  // doubles
  size_t take(size_t n_doubles) {
    const size_t o = total;
    total += rup(n_doubles, 64);
    return o;
  }
  size_t bytes() const { return total * sizeof(double) + 16; }
};
// The sections of launch_kzz_factor in a Layout (K_ZZ + jitter I, L, L^-1, the factorisation's scratch) and the call on them
struct KzzSections {
  size_t Kmm, Lf, Linv, chol, chol_len;
  void take(Layout& l, int M) {
    chol_len = chol_ws_doubles(M);
    Kmm = l.take((size_t)M * M);
    Lf = l.take((size_t)M * M);
    Linv = l.take((size_t)M * M);
    chol = l.take(chol_len);
  }
  int factor(const tgp_model& md, double* ws, int32_t* status, hipStream_t st) const {
    return launch_kzz_factor(md.kernel, md.Z, md.raw_ls, md.raw_os, md.M, md.D, md.jitter, ws + Kmm, ws + Lf, ws + Linv, status,
                             ws + chol, chol_len, st);
  }
};
inline bool inducing_limits(int M, int D) { return M >= 1 && M <= TGP_BIG_MAX_M && D >= 1 && D <= 16; }
inline bool known_kernel(int kernel) {
  return kernel == TGP_KERNEL_SCALE_RBF || kernel == TGP_KERNEL_SCALE_MATERN32 || kernel == TGP_KERNEL_SCALE_MATERN52 ||
         kernel == TGP_KERNEL_SCALE_RQ;
}
// how the entries' refusal texts name them
#define TGP_KNOWN_KERNELS_TEXT "kernel TGP_KERNEL_SCALE_RBF, _MATERN32, _MATERN52 or _RQ"

// What the host asks about a likelihood, one row per TGP_LIK_* id (the table: tgp_lik.hip).  The two launchers take the same
// arguments for every row -- ell: ell_plan's LPR, NB, workgroups and LDS, `ext`: the program holds a kind past STEPTANH.
using EllLaunch = int(int LPR, int NB, int ext, int nb, size_t lds, hipStream_t st, const tgp_model& md, const FlowProg& fp,
                      const double* Y, const double* mu, const double* v, const double* rowp, double* part, double* g_mu,
                      double* g_v, double* g_rowp);
using PredictLaunch = int(const tgp_model& md, const FlowProg& fp, const double* mu, const double* v, const double* rowp,
                          const double* Y, double Y_std, double* m1, double* m2, double* logp, hipStream_t st);
struct LikRow {
  int lik;
  const char* name;          // the id's macro, as text
  bool quadrature;           // k_ell_quad integrates it by Gauss-Hermite through the flow (S, xs, wn, the program and theta are read)
  bool general_only;         // ... and has no fused row kernel: its training step takes the general-M path at every M, as MATERN32 does
  EllLaunch* ell;            // launch_ell_quad's k_ell_quad instantiations (those of EllGauss where the id has no policy of its own)
  PredictLaunch* predict;    // launch_predict's k_predict_quad instantiations; nullptr: tgp_predict_f64 has none for it
  const char* no_quantiles;  // what the quantile / CDF entries say after "no quantiles for "; nullptr: they serve it
  int ell_max_nb = 8;        // ell_plan's cap on the nodes in flight per lane (EllMaxNB, tgp_ell.hpp)
};
const LikRow* lik_row(int lik);   // nullptr: no such id
inline bool lik_is_quadrature(int lik) { const LikRow* r = lik_row(lik); return r && r->quadrature; }
inline bool lik_general_only(int lik) { const LikRow* r = lik_row(lik); return r && r->general_only; }
// *first = the first 16-byte aligned double of the caller's workspace `ws`; refused when fewer than need_doubles follow it
inline int open_workspace(const char* entry, const char* sizer, void* ws, size_t ws_bytes, size_t need_doubles, double** first) {
  const uintptr_t a = (reinterpret_cast<uintptr_t>(ws) + 15) & ~(uintptr_t)15;
  const size_t skip = a - reinterpret_cast<uintptr_t>(ws);
  const size_t have = ws_bytes > skip ? (ws_bytes - skip) / sizeof(double) : 0;
  if (have < need_doubles) {
    set_error_text("%s: workspace of %zu bytes, %s gives %zu", entry, ws_bytes, sizer, need_doubles * sizeof(double) + 16);
    return TGP_E_WORKSPACE;
  }
  *first = reinterpret_cast<double*>(a);
  return 0;
}

// tgp_kmeans.hip
int launch_kmeans_assign(const double* X, int N, int D, const double* C, int K, int32_t* labels, double* mind2, hipStream_t st);
int launch_kmeans_segsum(const double* X, int D, const int64_t* order, const int64_t* offs, int K, double* sums, hipStream_t st);
int launch_kmeans_pp(const double* X, int N, int D, const int64_t* cand, int T, const double* closest, double* out,
                     hipStream_t st);

// tgp_mlp.hip
size_t mlp_workspace_doubles(int N, int D, int H, int L, int nnets);
int launch_mlp_forward(const tgp_mlp& d, const double* X, const double* W, const int32_t* step_dev, double* out, hipStream_t st);
int launch_mlp_backward(const tgp_mlp& d, const double* X, const double* W, const int32_t* step_dev, const double* g_out,
                        double* g_W, double* ws, size_t ws_doubles, hipStream_t st, const AdamDev* adam = nullptr,
                        double weight_decay = 0.0);

// tgp_lik.hip
int launch_ell_gauss(const double* Y, const double* mu, const double* v, int N, const double* log_var_noise,
                     double scale, double* out, double* g_mu, double* g_v, double* ws, hipStream_t st);
// the quadrature likelihood through the flow, by the row of md.lik (TGP_LIK_HETERO: mu, v, g_mu, g_v are (2,N))
int launch_ell_quad(const tgp_model& md, const FlowProg& fp, const double* Y, const double* mu, const double* v, const double* rowp,
                    double* out, double* g_mu, double* g_v, double* g_theta, double* g_rowp, double* ws, hipStream_t st);
int launch_flow_eval(const tgp_model& md, const FlowProg& fp, const double* f, int S, int N, const double* rowp, double* G, double* dG,
                     double* logdG, hipStream_t st, double* sum_out = nullptr, double* ws = nullptr);
EllLaunch ell_launch_negbin;           // tgp_lik_negbin.hip: what the TGP_LIK_NEGBIN row points to
PredictLaunch predict_launch_negbin;
EllLaunch ell_launch_ordinal;          // tgp_lik_ordinal.hip: what the TGP_LIK_ORDINAL row points to
PredictLaunch predict_launch_ordinal;
EllLaunch ell_launch_gamma;            // tgp_lik_gamma.hip: what the TGP_LIK_GAMMA row points to
PredictLaunch predict_launch_gamma;
EllLaunch ell_launch_beta;             // tgp_lik_beta.hip: what the TGP_LIK_BETA row points to
PredictLaunch predict_launch_beta;
int launch_predict(const tgp_model& md, const FlowProg& fp, const double* mu, const double* v, const double* rowp, const double* Y,
                   double Y_std, double* m1, double* m2, double* logp, hipStream_t st);
int launch_adam(double* params, const double* grads, double* exp_avg, double* exp_avg_sq, int64_t n, double lr,
                double beta1, double beta2, double eps, double weight_decay, int step, int maximize, hipStream_t st);
int launch_adam_dev(double* params, const double* grads, double* exp_avg, double* exp_avg_sq, int64_t n, double lr,
                    double beta1, double beta2, double eps, double weight_decay, int32_t* step_dev, int maximize,
                    hipStream_t st, int64_t n_plain = 0, int64_t skip_off = 0, int64_t skip_n = 0);
size_t lik_workspace_doubles(int N, int P, int RP);
int launch_gather_rows(const double* X, const double* Y, int N, int D, const int32_t* index, int32_t* cursor, int offset,
                       int nrows, int advance, int wrap, double* Xb, double* Yb, hipStream_t st);


// tgp_warp.hip (warped-GP likelihood: flow on the targets, flow inverse)
#define TGP_WARP_TARGETS 0 /* t = T(Y) only (pre-pass of the training step; also zeroes the ticket word) */
#define TGP_WARP_FULL 1    /* the stand-alone likelihood: out[0..2], g_mu, g_v, g_theta, t */
#define TGP_WARP_STEP 2    /* post-pass of the training step: g_theta written, scale sum log T' added to out[0], out[1] */
size_t warp_workspace_doubles(int N, int P);
int launch_ell_warp(const tgp_model& md, const FlowProg& fp, int mode, const double* Y, const double* mu, const double* v,
                    double* out, double* g_mu, double* g_v, double* g_theta, double* t_out, double* ws, hipStream_t st);
int launch_flow_inverse(const tgp_model& md, const FlowProg& fp, const double* t, int S, int N, const double* rowp, double* x,
                        int32_t* status, hipStream_t st);
int launch_predict_warp(const tgp_model& md, const FlowProg& fp, const double* mu, const double* v, const double* Y, double Y_std,
                        double* m1, double* m2, double* logp, hipStream_t st);

// tgp_quantile.hip (exact CDF and quantiles of the Gauss-Hermite predictive; TGP_LIK_GAUSS / TGP_LIK_FLOW / TGP_LIK_GAMMA / TGP_LIK_BETA)
int launch_predict_quantile(const tgp_model& md, const FlowProg& fp, const double* mu, const double* v, const double* rowp,
                            const double* probs, const double* zq, int Q, double* t, int32_t* status, hipStream_t st);
int launch_predict_cdf(const tgp_model& md, const FlowProg& fp, const double* mu, const double* v, const double* rowp,
                       const double* Y, double* cdf, double* sf, hipStream_t st);
// ... the CRPS of the same predictive at Y: crps (N), parts (2,N) = T1, T2 (optional)
int launch_predict_crps(const tgp_model& md, const FlowProg& fp, const double* mu, const double* v, const double* rowp,
                        const double* Y, double* crps, double* parts, hipStream_t st);
// ... the partials of the predictive moments in mu and v on the same sweep: dm1, dm2 (2,N)
int launch_predict_moment_grads(const tgp_model& md, const FlowProg& fp, const double* mu, const double* v, const double* rowp,
                                double* dm1, double* dm2, hipStream_t st);
// ... EI / log EI / PI (kind: TGP_ACQ_*) against the incumbent `best`, c = +1 to maximise, -1 to minimise: value (N), partials
// (2,N) in mu and v (optional), grad_x (N,D) = the chain rule with dmu_dx, dv_dx (optional)
int launch_predict_acquisition(const tgp_model& md, const FlowProg& fp, const double* mu, const double* v, const double* rowp,
                               int kind, double best, double c, double* value, double* partials, const double* dmu_dx,
                               const double* dv_dx, int D, double* grad_x, hipStream_t st);
// ... and the heteroscedastic predictive on the same node table: mu, v (2,N), moments and the S x S log density
int launch_predict_hetero(const tgp_model& md, const FlowProg& fp, const double* mu, const double* v, const double* rowp,
                          const double* Y, double Y_std, double* m1, double* m2, double* logp, hipStream_t st);

// tgp_softmax.hip (multi-class likelihood: softmax over C latent GPs, Monte Carlo over all classes of a row)
struct SmxArgs {                 // by-value kernel argument built from a tgp_softmax descriptor
  int32_t N, C, S, P;            // P = theta_off[C]: every program's shared scalars
  int32_t blk_off[TGP_SOFTMAX_MAX_C + 1];
  double scale;
  uint64_t seed;
  const int32_t* step_dev;
  int64_t row0;
};
size_t softmax_workspace_doubles(int N, int P);
int launch_ell_softmax(const SmxArgs& a, const FlowProg& fp, const double* theta, const double* Y, const double* mu, const double* v,
                       const double* eps, double* out, double* mu_bar, double* v_bar, double* theta_bar, double* ws,
                       hipStream_t st);
int launch_mc_normals(const SmxArgs& a, double* eps, hipStream_t st);
int launch_predict_softmax(const SmxArgs& a, const FlowProg& fp, const double* theta, const double* mu, const double* v,
                           const double* eps, const double* Y, double* P, double* logp, hipStream_t st);

// tgp_cov.hip (full-covariance q(f): Sigma = K(X*, X*) + A^T W A, and joint draws mu + E chol(Sigma + jitter I)^T)
size_t qf_cov_workspace_bytes(int N, int D, int M);
int launch_qf_cov(const tgp_model& md, const double* X, double* mu, double* Sigma, int32_t* status, void* workspace,
                  size_t workspace_bytes, hipStream_t st);
size_t qf_joint_sample_workspace_bytes(int N, int S);
int launch_qf_joint_sample(const double* mu, const double* Sigma, int N, double jitter, const double* eps, int S, double* F0,
                           double* Lsig, int32_t* status, void* workspace, size_t workspace_bytes, hipStream_t st);

// ... its operand passes, for the units that build on A = L^-1 K(Z, X*) (tgp_xgrad.hip): k_cov_prep + W += L_q L_q^T on the
// padded (MP x MP) images, and k_cov_a on `rows` rows of X* (A (MP x NP), mu (rows))
int launch_cov_prep(const double* Lam, const double* Linv, int M, int MP, double* Lq, double* W, double* LinvP, hipStream_t st);
int launch_cov_a(const tgp_model& md, const double* X, int rows, const double* LinvP, int MP, double* A, int NP, double* mu,
                 hipStream_t st);

// tgp_xgrad.hip (input gradients of the q(f) marginals: dmu, dv (N,D) in passes of TGP_XGRAD_PASS_ROWS rows)
size_t qf_input_grad_workspace_bytes(int N, int D, int M);
int launch_qf_input_grad(const tgp_model& md, const double* X, double* dmu, double* dv, int32_t* status, void* workspace,
                         size_t workspace_bytes, hipStream_t st);

// ... and the variance of the derivative process: dvar (N,D), one A_d = L^-1 J_d^T, C_d = W A_d and column sum per dimension
size_t qf_input_grad_var_workspace_bytes(int N, int D, int M);
int launch_qf_input_grad_var(const tgp_model& md, const double* X, double* dvar, int32_t* status, void* workspace,
                             size_t workspace_bytes, hipStream_t st);

// tgp_unwhiten.hip (unwhitened q(u): m_w = L^-1 m, Lam_w = L^-1 tril(L_q), and the adjoint down to Z and the kernel parameters)
size_t unwhiten_workspace_bytes(int M, int D);
int launch_unwhiten(int kernel, const double* Z, const double* raw_ls, const double* raw_os, int M, int D, double jitter,
                    const double* m, const double* Lq, double* m_w, double* Lam_w, double* L, double* Linv, int32_t* status,
                    void* workspace, size_t workspace_bytes, hipStream_t st);
size_t unwhiten_bwd_workspace_bytes(int M, int D);
int launch_unwhiten_bwd(int kernel, const double* Z, const double* raw_ls, const double* raw_os, int M, int D, const double* L,
                        const double* Linv, const double* m_w, const double* Lam_w, const double* m_w_bar, const double* Lam_w_bar,
                        double* m_bar, double* Lq_bar, double* Z_bar, double* raw_ls_bar, double* raw_os_bar, void* workspace,
                        size_t workspace_bytes, hipStream_t st);

// tgp_mean.hip (linear / identity mean function: m(x) = x a + b on the rows of X, and its adjoint)
size_t mean_backward_workspace_bytes(int N, int D);
int launch_mean_forward(const double* X, int N, int D, const double* a, const double* b, double alpha, const double* in,
                        double* out, int ld, int col, int one_col, hipStream_t st);
int launch_mean_backward(const double* X, int N, int D, const double* a, const double* g, int ldg, int colg, double* g_a,
                         double* g_b, double* g_X, double* part, hipStream_t st);

// tgp_optqu.hip (closed-form optimal whitened q(u) of the Gaussian likelihood: C = K_ZX K_XZ, b = K_ZX y, then the M x M chain)
size_t kxxk_workspace_bytes(int N, int M);
int launch_kxxk(int kernel, const double* X, int N, const double* Z, int M, int D, const double* raw_ls, const double* raw_os,
                const double* Y, double* C, double* b, void* workspace, size_t workspace_bytes, hipStream_t st);
size_t optimal_qu_workspace_bytes(int N, int D, int M);
int launch_optimal_qu(const tgp_model& md, const double* X, const double* Y, double* m_out, double* Lam_out, int32_t* status,
                      void* workspace, size_t workspace_bytes, hipStream_t st);
// ... the weighted pass C = K_ZX diag(w) K_XZ, b = K_ZX r, and the natural-gradient step of q(u) on the same chain
size_t kxwxk_workspace_bytes(int N, int M);
int launch_kxwxk(int kernel, const double* X, int N, const double* Z, int M, int D, const double* raw_ls, const double* raw_os,
                 const double* w, const double* r, double* C, double* b, void* workspace, size_t workspace_bytes, hipStream_t st);
size_t natgrad_qu_workspace_bytes(int N, int D, int M);
int launch_natgrad_qu(const tgp_model& md, const double* X, const double* mu, const double* mu_bar, const double* v_bar, double rho,
                      double site_floor, double* m_out, double* Lam_out, int32_t* status, void* workspace, size_t workspace_bytes,
                      hipStream_t st);

// tgp_greedy.hip (greedy conditional-variance selection of inducing points: the pivoted Cholesky factorisation of K_XX)
size_t greedy_inducing_workspace_bytes(int N, int D, int M);
int launch_greedy_inducing(const double* X, int N, int D, const double* raw_ls, const double* raw_os, int kernel, int M,
                           double min_var, int32_t* idx, double* Z, double* trace, int32_t* count, void* workspace,
                           size_t workspace_bytes, hipStream_t st);

// tgp_pathwise.hip (pathwise posterior function draws: Fourier features of the prior + kernel columns at the inducing points)
size_t pathwise_workspace_bytes(int N, int D, int M, int R2, int S);
int launch_pathwise_coeff(const tgp_model& md, const double* omega, int R2, const double* W, const double* eps, int S, double* coef,
                          int32_t* status, void* workspace, size_t workspace_bytes, hipStream_t st);
int launch_pathwise_eval(int kernel, const double* X, int N, int D, const double* Z, int M, const double* raw_ls,
                         const double* raw_os, const double* omega, int R2, const double* coef, int S, double* F0, hipStream_t st);
// ... and their input gradients: dF0 (D,S,N)
int launch_pathwise_grad(int kernel, const double* X, int N, int D, const double* Z, int M, const double* raw_ls,
                         const double* raw_os, const double* omega, int R2, const double* coef, int S, double* dF0, hipStream_t st);

}  // namespace tgp
