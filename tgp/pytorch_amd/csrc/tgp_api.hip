// tgp_api.hip -- the extern "C" surface of libtgp_hip.so (declared in include/tgp_hip.h).
// Argument checking, plan/workspace bookkeeping and the launch sequence of one ELBO step:
//   M <= 128 : k_prep_a -> row kernel (k_rows / k_rows4) -> k_reduce -> k_bwd   (4 launches, no host sync)
//   M  > 128 : the chunked GEMM pipeline of tgp_big.hip (same entry points, chosen by M / kernel)
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "tgp_dev.hpp"
#include "tgp_launch.hpp"

namespace tgp {

static thread_local char g_err[256] = "";

int set_error(hipError_t e, const char* file, int line) {
  snprintf(g_err, sizeof(g_err), "%s:%d: %s", file, line, hipGetErrorString(e));
  return TGP_E_LAUNCH;
}

void set_error_text(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

// the flow fields of a model: a program for its blocks and the shared scalars they index; with `counts`, no negative count
// (`program` false: the entry leaves a missing program to make_prog, after its own argument checks)
static int check_flow_args(const tgp_model* m, bool counts = false, bool program = true) {
  if (counts && (m->nblk < 0 || m->P < 0 || m->RP < 0)) return -1;
  if (program && m->nblk > 0 && !m->program) return -1;
  if (m->P > 0 && !m->theta) return -1;
  return 0;
}

static int check_model(const tgp_model* m, bool need_lik) {
  if (m == nullptr) return -1;
  if (m->N < 1 || m->D < 1 || m->D > 16) return -1;
  if (m->M < 1) return -1;
  if (m->M > TGP_BIG_MAX_M) return TGP_E_UNSUPPORTED;
  if (!known_kernel(m->kernel)) return -1;
  if (!m->Z || !m->raw_ls || !m->raw_os || !m->m || !m->Lam || !m->log_var_noise) return -1;
  if (need_lik && lik_is_quadrature(m->lik))
    if (m->S < 1 || m->nblk < 0 || !m->xs || !m->wn || check_flow_args(m)) return -1;
  return 0;
}

// the arguments tgp_flow_eval_f64, tgp_flow_logdet_f64 and tgp_flow_inverse_f64 open with, under the same codes
static int check_flow_points(const tgp_model* m, bool counts, const double* f, int S, int N, const double* rowp) {
  if (!m || check_flow_args(m, counts)) return -1;
  if (!f) return -2;
  if (S < 1) return -3;
  if (N < 1) return -4;
  if (m->RP > 0 && !rowp) return -5;
  return 0;
}

// one block of a program against the `limit` parameters of the vector it indexes (`per_row_ok` false: shared parameters only)
static int check_block(int kind, int K, int poff, int flags, int limit, bool per_row_ok = true) {
  if (kind < TGP_FLOW_AFFINE || kind > TGP_FLOW_SOFTPLUS || kind == 6) return -1;   // (6 is unassigned)
  if (kind == TGP_FLOW_STEPTANH && K < 1) return -1;
  // TGP_FLAG_NEGATE: the left-skewed TUKEY block's gam = -softplus(raw), nothing else
  if ((flags & TGP_FLAG_NEGATE) && (kind != TGP_FLOW_TUKEY || !(flags & TGP_FLAG_RESTRICT))) return -1;
  // the reference never adds f to a Tukey, exp or softplus block
  if ((flags & TGP_FLAG_ADD_F0) && kind >= TGP_FLOW_TUKEY) return -1;
  if ((flags & TGP_FLAG_PER_ROW) && !per_row_ok) return TGP_E_UNSUPPORTED;
  // per-row parameters: AFFINE and SAL only (the reference has no input-dependent tanh-step, arcsinh or Box-Cox flow)
  if (kind >= TGP_FLOW_STEPTANH && (flags & TGP_FLAG_PER_ROW)) return -1;
  if (poff < 0 || poff + flow_block_params(kind, K) > limit) return -1;
  return 0;
}

// host array (nblk x 4 int32) -> by-value kernel argument; validates kinds and parameter offsets
static int make_prog(const tgp_model* m, bool flow, FlowProg& fp) {
  fp.nblk = 0;
  fp.nslots = 0;
  if (!flow || m->nblk <= 0) return 0;
  if (m->nblk > TGP_MAX_BLOCKS) return TGP_E_UNSUPPORTED;
  if (!m->program) return -1;
  fp.nblk = m->nblk;
  for (int b = 0; b < m->nblk; ++b) {
    const int32_t* blk = m->program + 4 * b;
    if (int rc = check_block(blk[0], blk[1], blk[2], blk[3], (blk[3] & TGP_FLAG_PER_ROW) ? m->RP : m->P)) return rc;
    for (int j = 0; j < 4; ++j) fp.blk[4 * b + j] = blk[j];
  }
  fp.nslots = flow_slots(fp.blk, fp.nblk);
  return 0;
}

// A warp of the targets, and anything that is inverted, must map onto the real line: NORMCDF, EXP and SOFTPLUS do not (true:
// refused, tgp_last_error() names the entry and the kind)
static bool refuse_not_onto(const FlowProg& fp, const char* entry) {
  for (int b = 0; b < fp.nblk; ++b) {
    const int kind = fp.blk[4 * b];
    if (kind == TGP_FLOW_NORMCDF || kind == TGP_FLOW_EXP || kind == TGP_FLOW_SOFTPLUS) {
      set_error_text("%s: block %d has flow kind %d (%s), which does not map onto the real line: it cannot warp targets or be "
                     "inverted", entry, b, kind,
                     kind == TGP_FLOW_NORMCDF ? "TGP_FLOW_NORMCDF" : (kind == TGP_FLOW_EXP ? "TGP_FLOW_EXP" : "TGP_FLOW_SOFTPLUS"));
      return true;
    }
  }
  return false;
}

static const FlowProg no_flow{};   // the empty program of the q(f) entries

// what a flow kernel takes by value: the program in `fp`, the model without its host program pointer in `md` (may be *m itself)
static int flow_args(const tgp_model* m, bool flow, FlowProg& fp, tgp_model& md) {
  const int rc = make_prog(m, flow, fp);
  md = *m;
  md.program = nullptr;
  return rc;
}

// `m` as the plain Gaussian model with the same q(f): no flow, no parameters of one
static tgp_model gauss_copy(const tgp_model& m, int lik = TGP_LIK_GAUSS) {
  tgp_model g = m;
  g.lik = lik; g.nblk = 0; g.P = 0; g.RP = 0; g.program = nullptr; g.theta = nullptr;
  return g;
}

// TGP_LIK_HETERO has two latent GPs: every single-output entry refuses it by name (true: refused, tgp_last_error() says where to go)
static bool refuse_hetero(const tgp_model* m, const char* entry) {
  if (m == nullptr || m->lik != TGP_LIK_HETERO) return false;
  set_error_text("%s: TGP_LIK_HETERO has two latent GPs and no single-output entry: use tgp_ell_hetero_f64 (composed with "
                 "tgp_qf_moments_f64, tgp_qf_moments_bwd_f64 and tgp_kl_whitened_f64 per latent GP) and tgp_predict_hetero_f64",
                 entry);
  return true;
}

static int check_adam(const tgp_adam_args* a) {
  return a && a->params && a->grads && a->exp_avg && a->exp_avg_sq && a->step_dev && a->n >= 1 ? 0 : -1;
}
static AdamDev adam_dev_of(const tgp_adam_args* a) {
  AdamDev ad;
  ad.p = a->params; ad.g = a->grads; ad.m = a->exp_avg; ad.v = a->exp_avg_sq; ad.n = (long)a->n;
  ad.lr = a->lr; ad.b1 = a->beta1; ad.b2 = a->beta2; ad.eps = a->eps;
  ad.ln_b1 = log(a->beta1); ad.ln_b2 = log(a->beta2); ad.sign = a->maximize ? -1.0 : 1.0;
  ad.step_dev = a->step_dev;   // (lam_off, lam_n: the step's own)
  return ad;
}

// the chunked GEMM pipeline of tgp_big.hip: every M the fused kernels do not hold, and every kernel but the RBF
static bool takes_general_path(int M, int kernel) { return M > TGP_FUSED_MAX_M || kernel != TGP_KERNEL_SCALE_RBF; }
static bool takes_general_path(const tgp_model& m) { return takes_general_path(m.M, m.kernel); }

// the Plan the fused path runs, planned again for the row kernel that choose_rows4 / rows_per_wave pick; TGP_E_WORKSPACE when
// the caller's buffer does not hold it
static int fused_plan(Plan& p, const tgp_model& m, int S, int nblk, int P, int RP, int lik, bool train, const FlowProg& fp,
                      size_t workspace_bytes) {
  const bool full_pad = (m.plan & TGP_PLAN_FULL_PAD) != 0;   // A/B switch: compute on the padding of M as well
  if (int rc = make_plan(p, m.N, m.D, m.M, S, nblk, P, RP, lik, 0, 16, full_pad)) return rc;
  p.nslots = fp.nslots;
  const int nw4 = choose_rows4(p, train, m.plan), rw = nw4 ? 16 : rows_per_wave(p, fp, train, m.plan);
  if (nw4 != 0 || rw != 16) {
    if (int rc = make_plan(p, m.N, m.D, m.M, S, nblk, P, RP, lik, nw4, rw, full_pad)) return rc;
    p.nslots = fp.nslots;
  }
  return workspace_bytes < p.total * sizeof(double) ? TGP_E_WORKSPACE : 0;
}

}  // namespace tgp

using namespace tgp;

extern "C" {

int tgp_version(void) { return TGP_VERSION; }

const char* tgp_last_error(void) { return g_err; }

#ifndef TGP_SRC_HASH
#define TGP_SRC_HASH "unstamped"
#endif
const char* tgp_source_hash(void) { return TGP_SRC_HASH; }

size_t tgp_workspace_bytes(int32_t N, int32_t D, int32_t M, int32_t S, int32_t nblk, int32_t P, int32_t RP) {
  return tgp_workspace_bytes_kernel(N, D, M, S, nblk, P, RP, TGP_KERNEL_SCALE_RBF);
}

size_t tgp_workspace_bytes_kernel(int32_t N, int32_t D, int32_t M, int32_t S, int32_t nblk, int32_t P, int32_t RP,
                                  int32_t kernel) {
  return tgp_workspace_bytes_plan(N, D, M, S, nblk, P, RP, kernel, 0);
}

size_t tgp_workspace_bytes_plan(int32_t N, int32_t D, int32_t M, int32_t S, int32_t nblk, int32_t P, int32_t RP,
                                int32_t kernel, int32_t plan) {
  if (takes_general_path(M, kernel)) return big_workspace_doubles(N, D, M, S, nblk, P, RP, kernel, plan) * sizeof(double);
  Plan p;
  if (make_plan(p, N, D, M, S, nblk, P, RP, TGP_LIK_FLOW) != 0) return 0;
  size_t d = p.total + (size_t)(plan_alloc_blocks(N) - p.nblocks) * p.slab_len;   // slabs for whichever row kernel runs
  const size_t lik = lik_workspace_doubles(N, P, RP);
  if (lik > d) d = lik;
  // A training step whose flow stack does not fit a CU's LDS beside the row kernel's tiles (M > 112 with a 5 x 6 tanh flow)
  // runs on the general-M path (elbo_step_impl): room for that path too.  The program is not known here; an upper bound
  // of its stack slots decides: a block has at most 3 slots (SAL) or 1 + K (step-tanh, whose 4 K parameters are counted in P, or in
  // RP when they are per-row), so 3 nblk + (P + RP) / 4 bounds every mix of blocks (max(nblk + P/4, 3 nblk) did not --
  // SAL + step-tanh(K = 10) has 14 slots against a "bound" of 12)
  const int slots_ub = 3 * nblk + (P + RP) / 4;
  if (nblk > 0 && !rows_train_lds_fits(p, slots_ub)) {
    const size_t big = big_workspace_doubles(N, D, M, S, nblk, P, RP, kernel, plan);
    if (big > d) d = big;
  }
  return d * sizeof(double);
}

// The workspace of a TGP_LIK_WARPED step: the Gaussian step's (gauss_bytes, gauss_doubles of it rounded to 2), then t = T(Y),
// mu, v (N each) and the partials of k_ell_warp.  All zero when the Gaussian step has no plan for the shape.
struct WarpedLayout {
  size_t gauss_bytes, gauss_doubles, total_bytes;
};
static WarpedLayout warped_layout(int N, int D, int M, int S, int P, int kernel, int plan) {
  const size_t g = tgp_workspace_bytes_plan(N, D, M, S, 0, 0, 0, kernel, plan);
  if (g == 0) return {0, 0, 0};
  const size_t gd = rup(g / sizeof(double), 2);
  return {g, gd, (gd + 3 * (size_t)N + warp_workspace_doubles(N, P)) * sizeof(double)};
}

size_t tgp_workspace_bytes_lik(int32_t N, int32_t D, int32_t M, int32_t S, int32_t nblk, int32_t P, int32_t RP,
                               int32_t kernel, int32_t plan, int32_t lik) {
  if (lik_general_only(lik)) {
    const size_t big = big_workspace_doubles(N, D, M, S, nblk, P, RP, kernel, plan);
    return big == 0 ? 0 : big * sizeof(double);
  }
  if (lik == TGP_LIK_WARPED) return N < 1 || P < 0 ? 0 : warped_layout(N, D, M, S, P, kernel, plan).total_bytes;
  return tgp_workspace_bytes_plan(N, D, M, S, nblk, P, RP, kernel, plan);
}

int tgp_elbo_step_f64(const tgp_model* model, const double* X, const double* Y, const double* rowp, double* out,
                      const tgp_grads* grads, double* mu, double* v, int32_t* status, void* workspace,
                      size_t workspace_bytes, void* stream) {
  return tgp_elbo_step_phases_f64(model, X, Y, rowp, out, grads, mu, v, status, workspace, workspace_bytes, 7u, stream);
}

static int elbo_step_impl(const tgp_model* model, const double* X, const double* Y, const double* rowp, double* out,
                          const tgp_grads* grads, double* mu, double* v, int32_t* status, void* workspace,
                          size_t workspace_bytes, uint32_t phases, const tgp_adam_args* adam, void* stream);

// TGP_LIK_WARPED: [t = T(Y)] -> the Gaussian step on t, exactly as a TGP_LIK_GAUSS call runs it -> [theta's gradient and the
// log-Jacobian term] -> (adam) ONE update launch over the flat buffer: theta's gradient does not exist before the post-pass,
// so the in-launch update of the fused path is not used.  The adjoints of mu, v, log_var_noise given t are the Gaussian ones.
static int elbo_step_warped(const tgp_model* model, const double* X, const double* Y, double* out, const tgp_grads* grads,
                            double* mu, double* v, int32_t* status, void* workspace, size_t workspace_bytes, uint32_t phases,
                            const tgp_adam_args* adam, void* stream) {
  if (int rc = check_model(model, false)) return rc;
  if (model->RP != 0) return TGP_E_UNSUPPORTED;
  if (int rc = check_flow_args(model, true)) return rc;
  if (model->nblk == 0 && model->P > 0) return -1;   // parameters of no block: their gradient would never be written
  if (!X) return -2;
  if (!Y) return -3;
  if (!out) return -5;
  if (!grads || !grads->Z || !grads->raw_ls || !grads->raw_os || !grads->m || !grads->Lam || !grads->log_var_noise) return -6;
  if (model->P > 0 && !grads->theta) return -6;
  if ((mu == nullptr) != (v == nullptr)) return -7;
  if (!status) return -9;
  if (!workspace) return -10;
  if (adam != nullptr) {
    if (check_adam(adam)) return -12;
    if (model->P > 0 && (grads->theta < adam->grads || grads->theta + model->P > adam->grads + adam->n)) return -12;
  }
  const WarpedLayout wl = warped_layout(model->N, model->D, model->M, model->S, model->P, model->kernel, model->plan);
  if (wl.total_bytes == 0) return TGP_E_UNSUPPORTED;
  if (workspace_bytes < wl.total_bytes) return TGP_E_WORKSPACE;
  const size_t N = (size_t)model->N;
  double* t = static_cast<double*>(workspace) + wl.gauss_doubles;
  double* mu_w = mu ? mu : t + N;
  double* v_w = v ? v : t + 2 * N;
  double* part = t + 3 * N;
  hipStream_t st = static_cast<hipStream_t>(stream);
  FlowProg fp;
  tgp_model mw;
  if (int rc = flow_args(model, true, fp, mw)) return rc;
  if (refuse_not_onto(fp, "tgp_elbo_step_f64 (TGP_LIK_WARPED)")) return TGP_E_UNSUPPORTED;
  // every argument of the Gaussian step has been checked above: nothing is enqueued for a call that will be refused.
  // An empty program is the Gaussian step itself on Y: t = Y, log T' = 0, no theta -- neither pass is launched.
  const bool warp = fp.nblk > 0;
  if (!warp) t = const_cast<double*>(Y);
  if (warp && (phases & TGP_PHASE_PREPARE))
    if (int rc = launch_ell_warp(mw, fp, TGP_WARP_TARGETS, Y, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, t, part, st))
      return rc;
  const tgp_model mg = gauss_copy(*model);
  tgp_grads gg = *grads;
  gg.theta = nullptr; gg.rowp = nullptr;
  if (int rc = elbo_step_impl(&mg, X, t, nullptr, out, &gg, mu_w, v_w, status, workspace, wl.gauss_bytes, phases, nullptr, stream))
    return rc;
  if (!(phases & TGP_PHASE_BACKWARD)) return 0;
  if (warp)
    if (int rc = launch_ell_warp(mw, fp, TGP_WARP_STEP, Y, mu_w, v_w, out, nullptr, nullptr, grads->theta, nullptr, part, st))
      return rc;
  if (adam != nullptr)
    return launch_adam_dev(adam->params, adam->grads, adam->exp_avg, adam->exp_avg_sq, adam->n, adam->lr, adam->beta1,
                           adam->beta2, adam->eps, 0.0, adam->step_dev, adam->maximize, st);
  return 0;
}

static int elbo_step_impl(const tgp_model* model, const double* X, const double* Y, const double* rowp, double* out,
                          const tgp_grads* grads, double* mu, double* v, int32_t* status, void* workspace,
                          size_t workspace_bytes, uint32_t phases, const tgp_adam_args* adam, void* stream) {
  if (model != nullptr && model->lik == TGP_LIK_SOFTMAX) {
    set_error_text("TGP_LIK_SOFTMAX has no single-output training step: use tgp_ell_softmax_f64 with tgp_qf_moments_f64, "
                   "tgp_qf_moments_bwd_f64 and tgp_kl_whitened_f64 per class");
    return TGP_E_UNSUPPORTED;
  }
  if (refuse_hetero(model, "tgp_elbo_step_f64")) return TGP_E_UNSUPPORTED;
  if (model != nullptr && model->lik == TGP_LIK_WARPED)
    return elbo_step_warped(model, X, Y, out, grads, mu, v, status, workspace, workspace_bytes, phases, adam, stream);
  if (int rc = check_model(model, true)) return rc;
  if (!X) return -2;
  if (!Y) return -3;
  if (model->RP > 0 && !rowp) return -4;
  if (!out) return -5;
  if (!grads || !grads->Z || !grads->raw_ls || !grads->raw_os || !grads->m || !grads->Lam || !grads->log_var_noise)
    return -6;
  const bool flowed = lik_is_quadrature(model->lik);
  if (model->P > 0 && flowed && !grads->theta) return -6;
  if (model->RP > 0 && !grads->rowp) return -6;
  if ((mu == nullptr) != (v == nullptr)) return -7;
  if (!status) return -9;
  if (!workspace) return -10;
  const int nblk = flowed ? model->nblk : 0;
  const int P = flowed ? model->P : 0;
  const int RP = flowed ? model->RP : 0;
  hipStream_t st = static_cast<hipStream_t>(stream);
  double* ws = static_cast<double*>(workspace);
  tgp_model md = *model;
  md.nblk = nblk; md.P = P; md.RP = RP;
  FlowProg fp;
  if (int rc = flow_args(&md, flowed, fp, md)) return rc;   // kernels use the by-value copy
  AdamDev ad;
  if (adam != nullptr) {
    if (check_adam(adam)) return -12;
    // every gradient of the call must be a view of adam->grads
    const double *lo = adam->grads, *hi = lo + adam->n;
    // ... START AND EXTENT: the update kernels index params / exp_avg / exp_avg_sq with the gradients' offsets, so a block
    // that ran past adam->n would be written past the caller's buffers
    const double* gp[7] = {grads->Z, grads->raw_ls, grads->raw_os, grads->m, grads->Lam, grads->log_var_noise, grads->theta};
    const size_t gn[7] = {(size_t)model->M * model->D, (size_t)model->D, 1, (size_t)model->M, (size_t)model->M * model->M, 1,
                          (size_t)P};
    for (int k = 0; k < 7; ++k)
      if (gp[k] != nullptr && gn[k] > 0 && (gp[k] < lo || gp[k] + gn[k] > hi)) return -12;
    ad = adam_dev_of(adam);
    ad.lam_off = (long)(grads->Lam - adam->grads); ad.lam_n = (long)model->M * model->M;
  }
  bool general = takes_general_path(*model) || lik_general_only(model->lik);
  if (!general && fp.nslots > 0) {
    // the fused path keeps the flow stack of a row block in LDS beside its operand tiles; a program that does not fit even
    // with one node in flight (TGP_E_LDS until round 5: M > 112 with the 5 x 6 tanh flow) takes the general-M path
    Plan pl;
    if (int rc = make_plan(pl, model->N, model->D, model->M, model->S, nblk, P, RP, model->lik)) return rc;
    general = !rows_train_lds_fits(pl, fp.nslots);
  }
  if (general) {
    const bool lam_early = adam != nullptr && (phases & TGP_PHASE_BACKWARD) && ad.lam_n > 0;
    if (int rc = launch_big_step(md, fp, X, Y, rowp, out, *grads, mu, v, status, ws, workspace_bytes / sizeof(double), phases, st,
                                 lam_early ? &ad : nullptr))
      return rc;
    if (adam != nullptr)   // general-M path: the update is a launch of its own -- except Lam's entries (the bulk: M^2 of the
                           // M^2 + M (D + 1) + ... parameters), which the kernel that forms their gradient updated beside the K_MM chain
      return launch_adam_dev(adam->params, adam->grads, adam->exp_avg, adam->exp_avg_sq, adam->n, adam->lr, adam->beta1,
                             adam->beta2, adam->eps, 0.0, adam->step_dev, adam->maximize, st, 0, lam_early ? ad.lam_off : 0,
                             lam_early ? ad.lam_n : 0);
    return 0;
  }
  Plan p;
  if (int rc = fused_plan(p, *model, model->S, nblk, P, RP, model->lik, true, fp, workspace_bytes)) return rc;
  if (phases & TGP_PHASE_PREPARE)
    if (int rc = launch_prepare(p, md, fp, ws, status, st)) return rc;
  if (phases & TGP_PHASE_ROWS)
    if (int rc = launch_rows(p, md, fp, X, Y, rowp, grads->rowp, mu, v, ws, true, st)) return rc;
  if (phases & TGP_PHASE_BACKWARD)
    if (int rc = launch_backward_mm(p, md, *grads, out, ws, status, st, adam != nullptr ? &ad : nullptr)) return rc;
  return 0;
}

int tgp_elbo_step_phases_f64(const tgp_model* model, const double* X, const double* Y, const double* rowp,
                             double* out, const tgp_grads* grads, double* mu, double* v, int32_t* status,
                             void* workspace, size_t workspace_bytes, uint32_t phases, void* stream) {
  return elbo_step_impl(model, X, Y, rowp, out, grads, mu, v, status, workspace, workspace_bytes, phases, nullptr, stream);
}

int tgp_elbo_step_adam_f64(const tgp_model* model, const double* X, const double* Y, const double* rowp, double* out,
                           const tgp_grads* grads, double* mu, double* v, int32_t* status, void* workspace,
                           size_t workspace_bytes, const tgp_adam_args* adam, void* stream) {
  if (adam == nullptr) return -12;
  const uint32_t all = TGP_PHASE_PREPARE | TGP_PHASE_ROWS | TGP_PHASE_BACKWARD;
  const uint32_t phases = adam->phases != 0 ? (adam->phases & all) : all;
  return elbo_step_impl(model, X, Y, rowp, out, grads, mu, v, status, workspace, workspace_bytes, phases,
                        (phases & TGP_PHASE_BACKWARD) ? adam : nullptr, stream);
}

int tgp_qf_moments_f64(const tgp_model* model, const double* X, double* mu, double* v, int32_t* status,
                       void* workspace, size_t workspace_bytes, void* stream) {
  if (int rc = check_model(model, false)) return rc;
  if (!X) return -2;
  if (!mu) return -3;
  if (!v) return -4;
  if (!status) return -5;
  if (!workspace) return -6;
  hipStream_t st = static_cast<hipStream_t>(stream);
  double* ws = static_cast<double*>(workspace);
  const tgp_model md = gauss_copy(*model);
  if (takes_general_path(md)) return launch_big_moments(md, X, mu, v, status, ws, workspace_bytes / sizeof(double), st);
  Plan p;
  if (int rc = fused_plan(p, md, 1, 0, 0, 0, TGP_LIK_GAUSS, false, no_flow, workspace_bytes)) return rc;
  if (int rc = launch_prepare(p, md, no_flow, ws, status, st)) return rc;
  return launch_rows(p, md, no_flow, X, nullptr, nullptr, nullptr, mu, v, ws, false, st);
}

size_t tgp_qf_cov_workspace_bytes(int32_t N, int32_t D, int32_t M) { return qf_cov_workspace_bytes(N, D, M); }

int tgp_qf_cov_f64(const tgp_model* model, const double* X, double* mu, double* Sigma, int32_t* status, void* workspace,
                   size_t workspace_bytes, void* stream) {
  if (model == nullptr) return -1;
  if (!known_kernel(model->kernel)) return -1;
  if (qf_cov_workspace_bytes(model->N, model->D, model->M) == 0) {
    set_error_text("tgp_qf_cov_f64: N = %d, D = %d, M = %d outside 1 <= N, M <= %d, 1 <= D <= 16", model->N, model->D, model->M,
                   TGP_BIG_MAX_M);
    return TGP_E_UNSUPPORTED;
  }
  if (!model->Z || !model->raw_ls || !model->raw_os || !model->m || !model->Lam) return -1;
  if (!X) return -2;
  if (!mu) return -3;
  if (!Sigma) return -4;
  if (!status) return -5;
  if (!workspace) return -6;
  return launch_qf_cov(*model, X, mu, Sigma, status, workspace, workspace_bytes, static_cast<hipStream_t>(stream));
}

size_t tgp_qf_input_grad_workspace_bytes(int32_t N, int32_t D, int32_t M) { return qf_input_grad_workspace_bytes(N, D, M); }

int tgp_qf_input_grad_f64(const tgp_model* model, const double* X, double* dmu, double* dv, int32_t* status, void* workspace,
                          size_t workspace_bytes, void* stream) {
  if (model == nullptr) return -1;
  if (!known_kernel(model->kernel)) {
    set_error_text("tgp_qf_input_grad_f64: kernel = %d is not a " TGP_KNOWN_KERNELS_TEXT, model->kernel);
    return -1;
  }
  const size_t need = qf_input_grad_workspace_bytes(model->N, model->D, model->M);
  if (need == 0) {
    set_error_text("tgp_qf_input_grad_f64: N = %d, D = %d, M = %d outside N >= 1, 1 <= M <= %d, 1 <= D <= 16", model->N, model->D,
                   model->M, TGP_BIG_MAX_M);
    return TGP_E_UNSUPPORTED;
  }
  if (!model->Z || !model->raw_ls || !model->raw_os || !model->m || !model->Lam) return -1;
  if (!X) return -2;
  if (!dmu) return -3;
  if (!dv) return -4;
  if (!status) return -5;
  if (!workspace) return -6;
  if (workspace_bytes < need) {   // (to the byte: open_workspace alone counts whole doubles behind the aligned start)
    set_error_text("tgp_qf_input_grad_f64: workspace of %zu bytes, tgp_qf_input_grad_workspace_bytes gives %zu", workspace_bytes, need);
    return TGP_E_WORKSPACE;
  }
  return launch_qf_input_grad(*model, X, dmu, dv, status, workspace, workspace_bytes, static_cast<hipStream_t>(stream));
}

size_t tgp_qf_input_grad_var_workspace_bytes(int32_t N, int32_t D, int32_t M) { return qf_input_grad_var_workspace_bytes(N, D, M); }

int tgp_qf_input_grad_var_f64(const tgp_model* model, const double* X, double* dvar, int32_t* status, void* workspace,
                              size_t workspace_bytes, void* stream) {
  if (model == nullptr) return -1;
  if (!known_kernel(model->kernel)) {
    set_error_text("tgp_qf_input_grad_var_f64: kernel = %d is not a " TGP_KNOWN_KERNELS_TEXT, model->kernel);
    return TGP_E_UNSUPPORTED;
  }
  const size_t need = qf_input_grad_var_workspace_bytes(model->N, model->D, model->M);
  if (need == 0) {
    set_error_text("tgp_qf_input_grad_var_f64: N = %d, D = %d, M = %d outside N >= 1, 1 <= M <= %d, 1 <= D <= 16", model->N,
                   model->D, model->M, TGP_BIG_MAX_M);
    return TGP_E_UNSUPPORTED;
  }
  if (!model->Z || !model->raw_ls || !model->raw_os || !model->m || !model->Lam) return -1;
  if (!X) return -2;
  if (!dvar) return -3;
  if (!status) return -4;
  if (!workspace) return -5;
  if (workspace_bytes < need) {   // (to the byte: open_workspace alone counts whole doubles behind the aligned start)
    set_error_text("tgp_qf_input_grad_var_f64: workspace of %zu bytes, tgp_qf_input_grad_var_workspace_bytes gives %zu",
                   workspace_bytes, need);
    return TGP_E_WORKSPACE;
  }
  return launch_qf_input_grad_var(*model, X, dvar, status, workspace, workspace_bytes, static_cast<hipStream_t>(stream));
}

size_t tgp_optimal_qu_workspace_bytes(int32_t N, int32_t D, int32_t M) { return optimal_qu_workspace_bytes(N, D, M); }

int tgp_optimal_qu_f64(const tgp_model* model, const double* X, const double* Y, double* m_out, double* Lam_out, int32_t* status,
                       void* workspace, size_t workspace_bytes, void* stream) {
  if (model == nullptr) return -1;
  if (refuse_hetero(model, "tgp_optimal_qu_f64")) return TGP_E_UNSUPPORTED;   // (not Gaussian in h: no closed-form optimum)
  if (!known_kernel(model->kernel)) return -1;
  if (optimal_qu_workspace_bytes(model->N, model->D, model->M) == 0) {
    set_error_text("tgp_optimal_qu_f64: N = %d, D = %d, M = %d outside N >= 1, 1 <= M <= %d, 1 <= D <= 16", model->N, model->D,
                   model->M, TGP_BIG_MAX_M);
    return TGP_E_UNSUPPORTED;
  }
  if (!model->Z || !model->raw_ls || !model->raw_os || !model->log_var_noise) return -1;
  if (!X) return -2;
  if (!Y) return -3;
  if (!m_out) return -4;
  if (!Lam_out) return -5;
  if (!status) return -6;
  if (!workspace) return -7;
  return launch_optimal_qu(*model, X, Y, m_out, Lam_out, status, workspace, workspace_bytes, static_cast<hipStream_t>(stream));
}

size_t tgp_kxxk_workspace_bytes(int32_t N, int32_t M) { return kxxk_workspace_bytes(N, M); }

int tgp_kxxk_f64(int32_t kernel, const double* X, int32_t N, const double* Z, int32_t M, int32_t D, const double* raw_ls,
                 const double* raw_os, const double* Y, double* C, double* b, void* workspace, size_t workspace_bytes,
                 void* stream) {
  if (!known_kernel(kernel)) return -1;
  if (D < 1 || D > 16 || kxxk_workspace_bytes(N, M) == 0) {
    set_error_text("tgp_kxxk_f64: N = %d, D = %d, M = %d outside N >= 1, 1 <= M <= %d, 1 <= D <= 16", N, D, M, TGP_BIG_MAX_M);
    return TGP_E_UNSUPPORTED;
  }
  if (!X) return -2;
  if (!Z || !raw_ls || !raw_os) return -4;
  if (!C) return -10;
  if (!workspace) return -12;
  return launch_kxxk(kernel, X, N, Z, M, D, raw_ls, raw_os, Y, C, b, workspace, workspace_bytes, static_cast<hipStream_t>(stream));
}

size_t tgp_kxwxk_workspace_bytes(int32_t N, int32_t M) { return kxwxk_workspace_bytes(N, M); }

int tgp_kxwxk_f64(int32_t kernel, const double* X, int32_t N, const double* Z, int32_t M, int32_t D, const double* raw_ls,
                  const double* raw_os, const double* w, const double* r, double* C, double* b, void* workspace,
                  size_t workspace_bytes, void* stream) {
  if (!known_kernel(kernel)) return -1;
  if (D < 1 || D > 16 || kxwxk_workspace_bytes(N, M) == 0) {
    set_error_text("tgp_kxwxk_f64: N = %d, D = %d, M = %d outside N >= 1, 1 <= M <= %d, 1 <= D <= 16", N, D, M, TGP_BIG_MAX_M);
    return TGP_E_UNSUPPORTED;
  }
  if (!X) return -2;
  if (!Z || !raw_ls || !raw_os) return -4;
  if (!w) return -9;
  if (!C) return -11;
  if (!workspace) return -13;
  return launch_kxwxk(kernel, X, N, Z, M, D, raw_ls, raw_os, w, r, C, b, workspace, workspace_bytes, static_cast<hipStream_t>(stream));
}

size_t tgp_natgrad_qu_workspace_bytes(int32_t N, int32_t D, int32_t M) { return natgrad_qu_workspace_bytes(N, D, M); }

int tgp_natgrad_qu_f64(const tgp_model* model, const double* X, const double* mu, const double* mu_bar, const double* v_bar,
                       double rho, double site_floor, double* m_out, double* Lam_out, int32_t* status, void* workspace,
                       size_t workspace_bytes, void* stream) {
  if (model == nullptr) return -1;
  if (!(rho > 0.0 && rho <= 1.0) || !known_kernel(model->kernel) || natgrad_qu_workspace_bytes(model->N, model->D, model->M) == 0) {
    set_error_text("tgp_natgrad_qu_f64: rho = %g, kernel = %d, N = %d, D = %d, M = %d outside 0 < rho <= 1, " TGP_KNOWN_KERNELS_TEXT
                   ", N >= 1, 1 <= M <= %d, 1 <= D <= 16", rho, model->kernel, model->N, model->D, model->M,
                   TGP_BIG_MAX_M);
    return TGP_E_UNSUPPORTED;
  }
  if (!model->Z || !model->raw_ls || !model->raw_os) return -1;
  if (rho < 1.0 && (!model->m || !model->Lam)) return -1;
  if (!X) return -2;
  if (!mu) return -3;
  if (!mu_bar) return -4;
  if (!v_bar) return -5;
  if (!m_out) return -8;
  if (!Lam_out) return -9;
  if (!status) return -10;
  if (!workspace) return -11;
  return launch_natgrad_qu(*model, X, mu, mu_bar, v_bar, rho, site_floor, m_out, Lam_out, status, workspace, workspace_bytes,
                           static_cast<hipStream_t>(stream));
}

size_t tgp_greedy_inducing_workspace_bytes(int32_t N, int32_t D, int32_t M) { return greedy_inducing_workspace_bytes(N, D, M); }

int tgp_greedy_inducing_f64(const double* X, int32_t N, int32_t D, const double* raw_ls, const double* raw_os, int32_t kernel,
                            int32_t M, double min_var, int32_t* idx, double* Z, double* trace, int32_t* count, void* workspace,
                            size_t workspace_bytes, void* stream) {
  if (!known_kernel(kernel) || greedy_inducing_workspace_bytes(N, D, M) == 0) {
    set_error_text("tgp_greedy_inducing_f64: N = %d, D = %d, M = %d, kernel = %d outside 1 <= M <= min(N, %d), 1 <= D <= 16, "
                   TGP_KNOWN_KERNELS_TEXT, N, D, M, kernel, TGP_BIG_MAX_M);
    return TGP_E_UNSUPPORTED;
  }
  if (!X) return -1;
  if (!raw_ls) return -4;
  if (!raw_os) return -5;
  if (!(min_var >= 0.0)) return -8;
  if (!idx) return -9;
  if (!Z) return -10;
  if (!trace) return -11;
  if (!count) return -12;
  if (!workspace) return -13;
  return launch_greedy_inducing(X, N, D, raw_ls, raw_os, kernel, M, min_var, idx, Z, trace, count, workspace, workspace_bytes,
                                static_cast<hipStream_t>(stream));
}

size_t tgp_pathwise_workspace_bytes(int32_t N, int32_t D, int32_t M, int32_t R2, int32_t S) {
  return pathwise_workspace_bytes(N, D, M, R2, S);
}

int tgp_pathwise_coeff_f64(const tgp_model* model, const double* omega, int32_t R2, const double* W, const double* eps, int32_t S,
                           double* coef, int32_t* status, void* workspace, size_t workspace_bytes, void* stream) {
  if (model == nullptr) return -1;
  if (!known_kernel(model->kernel) || pathwise_workspace_bytes(1, model->D, model->M, R2, S) == 0) {
    set_error_text("tgp_pathwise_coeff_f64: D = %d, M = %d, R2 = %d, S = %d, kernel = %d outside 1 <= D <= 16, 1 <= M <= %d, "
                   "1 <= R2 <= %d, 1 <= S <= %d, " TGP_KNOWN_KERNELS_TEXT, model->D, model->M, R2, S,
                   model->kernel, TGP_BIG_MAX_M, TGP_PATHWISE_MAX_R2, TGP_PATHWISE_MAX_S);
    return TGP_E_UNSUPPORTED;
  }
  if (!model->Z || !model->raw_ls || !model->raw_os || !model->m || !model->Lam) return -1;
  if (!omega) return -2;
  if (!W) return -4;
  if (!eps) return -5;
  if (!coef) return -7;
  if (!status) return -8;
  if (!workspace) return -9;
  return launch_pathwise_coeff(*model, omega, R2, W, eps, S, coef, status, workspace, workspace_bytes, static_cast<hipStream_t>(stream));
}

int tgp_pathwise_eval_f64(int32_t kernel, const double* X, int32_t N, int32_t D, const double* Z, int32_t M, const double* raw_ls,
                          const double* raw_os, const double* omega, int32_t R2, const double* coef, int32_t S, double* F0,
                          void* stream) {
  if (!known_kernel(kernel) || pathwise_workspace_bytes(N, D, M, R2, S) == 0) {
    set_error_text("tgp_pathwise_eval_f64: N = %d, D = %d, M = %d, R2 = %d, S = %d, kernel = %d outside N >= 1, 1 <= D <= 16, "
                   "1 <= M <= %d, 1 <= R2 <= %d, 1 <= S <= %d, " TGP_KNOWN_KERNELS_TEXT, N, D, M, R2, S,
                   kernel, TGP_BIG_MAX_M, TGP_PATHWISE_MAX_R2, TGP_PATHWISE_MAX_S);
    return TGP_E_UNSUPPORTED;
  }
  if (!X) return -2;
  if (!Z) return -5;
  if (!raw_ls) return -7;
  if (!raw_os) return -8;
  if (!omega) return -9;
  if (!coef) return -11;
  if (!F0) return -13;
  return launch_pathwise_eval(kernel, X, N, D, Z, M, raw_ls, raw_os, omega, R2, coef, S, F0, static_cast<hipStream_t>(stream));
}

int tgp_pathwise_grad_f64(int32_t kernel, const double* X, int32_t N, int32_t D, const double* Z, int32_t M, const double* raw_ls,
                          const double* raw_os, const double* omega, int32_t R2, const double* coef, int32_t S, double* dF0,
                          void* stream) {
  if (!known_kernel(kernel) || pathwise_workspace_bytes(N, D, M, R2, S) == 0) {
    set_error_text("tgp_pathwise_grad_f64: N = %d, D = %d, M = %d, R2 = %d, S = %d, kernel = %d outside N >= 1, 1 <= D <= 16, "
                   "1 <= M <= %d, 1 <= R2 <= %d, 1 <= S <= %d, " TGP_KNOWN_KERNELS_TEXT, N, D, M, R2, S,
                   kernel, TGP_BIG_MAX_M, TGP_PATHWISE_MAX_R2, TGP_PATHWISE_MAX_S);
    return TGP_E_UNSUPPORTED;
  }
  if (!X) return -2;
  if (!Z) return -5;
  if (!raw_ls) return -7;
  if (!raw_os) return -8;
  if (!omega) return -9;
  if (!coef) return -11;
  if (!dF0) return -13;
  return launch_pathwise_grad(kernel, X, N, D, Z, M, raw_ls, raw_os, omega, R2, coef, S, dF0, static_cast<hipStream_t>(stream));
}

size_t tgp_qf_joint_sample_workspace_bytes(int32_t N, int32_t S) { return qf_joint_sample_workspace_bytes(N, S); }

int tgp_qf_joint_sample_f64(const double* mu, const double* Sigma, int32_t N, double jitter, const double* eps, int32_t S,
                            double* F0, double* Lsig, int32_t* status, void* workspace, size_t workspace_bytes, void* stream) {
  if (qf_joint_sample_workspace_bytes(N, S) == 0) {
    set_error_text("tgp_qf_joint_sample_f64: N = %d, S = %d outside 1 <= N <= %d, 1 <= S <= 4096", N, S, TGP_BIG_MAX_M);
    return TGP_E_UNSUPPORTED;
  }
  if (!mu) return -1;
  if (!Sigma) return -2;
  if (!eps) return -5;
  if (!F0) return -7;
  if (!status) return -9;
  if (!workspace) return -10;
  return launch_qf_joint_sample(mu, Sigma, N, jitter, eps, S, F0, Lsig, status, workspace, workspace_bytes,
                                static_cast<hipStream_t>(stream));
}

int tgp_qf_moments_bwd_f64(const tgp_model* model, const double* X, const double* mu_bar, const double* v_bar,
                           const tgp_grads* grads, int32_t* status, void* workspace, size_t workspace_bytes,
                           void* stream) {
  if (int rc = check_model(model, false)) return rc;
  if (!X) return -2;
  if (!mu_bar) return -3;
  if (!v_bar) return -4;
  if (!grads || !grads->Z || !grads->raw_ls || !grads->raw_os || !grads->m || !grads->Lam || !grads->log_var_noise) return -5;
  if (!status) return -6;
  if (!workspace) return -7;
  hipStream_t st = static_cast<hipStream_t>(stream);
  double* ws = static_cast<double*>(workspace);
  tgp_model md = gauss_copy(*model, TGP_LIK_ADJOINT);
  md.S = 1; md.scale = 1.0; md.kl_scale = 0.0;
  tgp_grads g = *grads;
  g.theta = nullptr; g.rowp = nullptr;
  const FlowProg& fp = no_flow;
  const uint32_t all = TGP_PHASE_PREPARE | TGP_PHASE_ROWS | TGP_PHASE_BACKWARD;
  if (takes_general_path(md)) {
    // (the scalars of the step go to the header words the general-M plan reserves as well: its hdr is the first block)
    return launch_big_step(md, fp, X, mu_bar, v_bar, ws + H_OUT, g, nullptr, nullptr, status, ws, workspace_bytes / sizeof(double),
                           all, st);
  }
  Plan p;
  if (int rc = fused_plan(p, md, 1, 0, 0, 0, TGP_LIK_ADJOINT, true, fp, workspace_bytes)) return rc;
  if (int rc = launch_prepare(p, md, fp, ws, status, st)) return rc;
  if (int rc = launch_rows(p, md, fp, X, mu_bar, v_bar, nullptr, nullptr, nullptr, ws, true, st)) return rc;
  return launch_backward_mm(p, md, g, ws + p.hdr + H_OUT, ws, status, st);
}

int tgp_kmm_f64(const double* Z, const double* raw_ls, const double* raw_os, int32_t M, int32_t D, double jitter,
                double* K, void* stream) {
  if (!Z) return -1;
  if (!raw_ls) return -2;
  if (!raw_os) return -3;
  if (M < 1) return -4;
  if (D < 1) return -5;
  if (!K) return -7;
  return launch_kmm(Z, raw_ls, raw_os, M, D, jitter, K, static_cast<hipStream_t>(stream));
}

int tgp_kernel_matrix_f64(int32_t kernel, const double* X1, int32_t N1, const double* X2, int32_t N2, int32_t D,
                          const double* raw_ls, const double* raw_os, double jitter, double* K, void* stream) {
  if (!known_kernel(kernel)) return -1;
  if (!X1) return -2;
  if (N1 < 1) return -3;
  if (X2 && N2 < 1) return -5;
  if (D < 1) return -6;
  if (!raw_ls) return -7;
  if (!raw_os) return -8;
  if (!K) return -10;
  return launch_kernel_matrix(kernel, X1, N1, X2, N2, D, raw_ls, raw_os, jitter, K, static_cast<hipStream_t>(stream));
}

int tgp_knm_f64(const double* X, const double* Z, const double* raw_ls, const double* raw_os, int32_t N, int32_t M,
                int32_t D, double* K, void* stream) {
  if (!X) return -1;
  if (!Z) return -2;
  if (!raw_ls) return -3;
  if (!raw_os) return -4;
  if (N < 1) return -5;
  if (M < 1) return -6;
  if (D < 1) return -7;
  if (!K) return -8;
  return launch_knm(X, Z, raw_ls, raw_os, N, M, D, K, static_cast<hipStream_t>(stream));
}

size_t tgp_ell_workspace_bytes(int32_t N, int32_t P, int32_t RP) {
  if (N < 1 || P < 0 || RP < 0) return 0;
  return tgp::lik_workspace_doubles(N, P, RP) * sizeof(double);
}

size_t tgp_cholesky_workspace_bytes(int32_t M) {
  if (M <= TGP_FUSED_MAX_M) return 0;
  return big_cholesky_workspace_doubles(M) * sizeof(double);
}

int tgp_cholesky_f64(const double* A, int32_t M, double* L, double* Linv, int32_t* status, void* workspace,
                     size_t workspace_bytes, void* stream) {
  if (!A) return -1;
  if (M < 1) return -2;
  if (M > TGP_BIG_MAX_M) return TGP_E_UNSUPPORTED;
  if (!L) return -3;
  if (!status) return -5;
  if (M > TGP_FUSED_MAX_M && !workspace) return -6;  // the blocked factorisation needs tgp_cholesky_workspace_bytes(M)
  return launch_cholesky_any(A, M, L, Linv, status, static_cast<double*>(workspace), workspace_bytes / sizeof(double),
                             static_cast<hipStream_t>(stream));
}

int tgp_cholesky_bwd_f64(const double* L, const double* Linv, const double* L_bar, int32_t M, double* A_bar, void* workspace,
                         size_t workspace_bytes, void* stream) {
  if (!L) return -1;
  if (!Linv) return -2;
  if (!L_bar) return -3;
  if (M < 1) return -4;
  if (M > TGP_BIG_MAX_M) return TGP_E_UNSUPPORTED;
  if (!A_bar) return -5;
  if (!workspace) return -6;
  return launch_big_cholesky_bwd(L, Linv, L_bar, M, A_bar, static_cast<double*>(workspace), workspace_bytes / sizeof(double),
                                 static_cast<hipStream_t>(stream));
}

size_t tgp_cholesky_bwd_workspace_bytes(int32_t M) { return big_cholesky_workspace_doubles(M) * sizeof(double); }

size_t tgp_unwhiten_workspace_bytes(int32_t M, int32_t D) { return unwhiten_workspace_bytes(M, D); }

int tgp_unwhiten_f64(int32_t kernel, const double* Z, const double* raw_ls, const double* raw_os, int32_t M, int32_t D,
                     double jitter, const double* m, const double* L_q, double* m_w, double* Lam_w, double* L, double* Linv,
                     int32_t* status, void* workspace, size_t workspace_bytes, void* stream) {
  if (!known_kernel(kernel)) return -1;
  if (!inducing_limits(M, D)) {
    set_error_text("tgp_unwhiten_f64: M = %d, D = %d outside 1 <= M <= %d, 1 <= D <= 16", M, D, TGP_BIG_MAX_M);
    return TGP_E_UNSUPPORTED;
  }
  if (!Z) return -2;
  if (!raw_ls) return -3;
  if (!raw_os) return -4;
  if (!m) return -8;
  if (!L_q) return -9;
  if (!m_w) return -10;
  if (!Lam_w) return -11;
  if (!L) return -12;
  if (!Linv) return -13;
  if (!status) return -14;
  return launch_unwhiten(kernel, Z, raw_ls, raw_os, M, D, jitter, m, L_q, m_w, Lam_w, L, Linv, status, workspace, workspace_bytes,
                         static_cast<hipStream_t>(stream));
}

size_t tgp_unwhiten_bwd_workspace_bytes(int32_t M, int32_t D) { return unwhiten_bwd_workspace_bytes(M, D); }

int tgp_unwhiten_bwd_f64(int32_t kernel, const double* Z, const double* raw_ls, const double* raw_os, int32_t M, int32_t D,
                         const double* L, const double* Linv, const double* m_w, const double* Lam_w, const double* m_w_bar,
                         const double* Lam_w_bar, double* m_bar, double* L_q_bar, double* Z_bar, double* raw_ls_bar,
                         double* raw_os_bar, void* workspace, size_t workspace_bytes, void* stream) {
  if (!known_kernel(kernel)) return -1;
  if (!inducing_limits(M, D)) {
    set_error_text("tgp_unwhiten_bwd_f64: M = %d, D = %d outside 1 <= M <= %d, 1 <= D <= 16", M, D, TGP_BIG_MAX_M);
    return TGP_E_UNSUPPORTED;
  }
  if (!Z) return -2;
  if (!raw_ls) return -3;
  if (!raw_os) return -4;
  if (!L) return -7;
  if (!Linv) return -8;
  if (!m_w) return -9;
  if (!Lam_w) return -10;
  if (!m_w_bar) return -11;
  if (!Lam_w_bar) return -12;
  if (!m_bar) return -13;
  if (!L_q_bar) return -14;
  if (!Z_bar) return -15;
  if (!raw_ls_bar) return -16;
  if (!raw_os_bar) return -17;
  return launch_unwhiten_bwd(kernel, Z, raw_ls, raw_os, M, D, L, Linv, m_w, Lam_w, m_w_bar, Lam_w_bar, m_bar, L_q_bar, Z_bar,
                             raw_ls_bar, raw_os_bar, workspace, workspace_bytes, static_cast<hipStream_t>(stream));
}

int tgp_mean_forward_f64(const double* X, int32_t N, int32_t D, const double* a, const double* b, double alpha, const double* in,
                         double* out, int32_t ld, int32_t col, int32_t one_col, void* stream) {
  if (!X) return -1;
  if (N < 1) return -2;
  if (D < 1 || D > 16) {
    set_error_text("tgp_mean_forward_f64: D = %d outside 1 <= D <= 16", D);
    return TGP_E_UNSUPPORTED;
  }
  if (!a) return -4;
  if (!out) return -8;
  if (ld < 1) return -9;
  if (col < 0 || col >= ld) return -10;
  if (one_col >= ld || one_col == col) return -11;
  return launch_mean_forward(X, N, D, a, b, alpha, in, out, ld, col, one_col < 0 ? -1 : one_col, static_cast<hipStream_t>(stream));
}

size_t tgp_mean_backward_workspace_bytes(int32_t N, int32_t D) { return mean_backward_workspace_bytes(N, D); }

int tgp_mean_backward_f64(const double* X, int32_t N, int32_t D, const double* a, const double* g, int32_t ldg, int32_t colg,
                          double* g_a, double* g_b, double* g_X, void* workspace, size_t workspace_bytes, void* stream) {
  if (!X) return -1;
  if (N < 1) return -2;
  if (D < 1 || D > 16) {
    set_error_text("tgp_mean_backward_f64: D = %d outside 1 <= D <= 16", D);
    return TGP_E_UNSUPPORTED;
  }
  if (!a && g_X) return -4;
  if (!g) return -5;
  if (ldg < 1) return -6;
  if (colg < 0 || colg >= ldg) return -7;
  if (!g_a) return -8;
  if (!workspace || (reinterpret_cast<uintptr_t>(workspace) & 7)) return -11;
  if (workspace_bytes < mean_backward_workspace_bytes(N, D)) {
    set_error_text("tgp_mean_backward_f64: workspace of %zu bytes, tgp_mean_backward_workspace_bytes gives %zu", workspace_bytes,
                   mean_backward_workspace_bytes(N, D));
    return TGP_E_WORKSPACE;
  }
  return launch_mean_backward(X, N, D, a, g, ldg, colg, g_a, g_b, g_X, static_cast<double*>(workspace),
                              static_cast<hipStream_t>(stream));
}

// what the kernels' 16-byte operand loads and the row-major layout ask of A, B and the leading dimensions (the codes are
// tgp_gemm_f64's argument numbers): the launcher would refuse the first two with a bare -1 and not look at the third
static int check_gemm_operands(int32_t trans_a, int32_t trans_b, int32_t m, int32_t n, int32_t k, const double* A, int32_t lda,
                               const double* B, int32_t ldb, int32_t ldc) {
  if (reinterpret_cast<uintptr_t>(A) & 15) return -8;
  if ((lda & 1) || lda < (trans_a ? m : k)) return -9;
  if (reinterpret_cast<uintptr_t>(B) & 15) return -10;
  if ((ldb & 1) || ldb < (trans_b ? k : n)) return -11;
  if (ldc < n) return -14;
  return 0;
}

int tgp_gemm_f64(int32_t trans_a, int32_t trans_b, int32_t tri, int32_t m, int32_t n, int32_t k, double alpha,
                 const double* A, int32_t lda, const double* B, int32_t ldb, double beta, double* C, int32_t ldc,
                 void* stream) {
  if (tri < 0 || tri > 31) return -3;
  if (m < 1 || m % 128) return -4;
  if (n < 1 || n % 128) return -5;
  if (k < 1 || k % 16) return -6;
  if (!A) return -8;
  if (!B) return -10;
  if (!C) return -13;
  if (int rc = check_gemm_operands(trans_a, trans_b, m, n, k, A, lda, B, ldb, ldc)) return rc;
  return launch_gemm_plain(trans_a != 0, trans_b != 0, tri, m, n, k, alpha, A, lda, B, ldb, beta, C, ldc,
                           static_cast<hipStream_t>(stream));
}

// the descriptor's checks, in field order after tgp_gemm_f64's own (whose codes fields 1-14 share); `ptrs`: A, B, C are required
static int check_gemm_ex(const tgp_gemm_ex* d, bool ptrs) {
  if (!d) return -1;
  if (d->tri < 0 || d->tri > 31) return -3;
  if (d->m < 1 || d->m % 128) return -4;
  if (d->n < 1 || d->n % 128) return -5;
  if (d->k < 1 || d->k % 16) return -6;
  if (ptrs && !d->A) return -8;
  if (ptrs && !d->B) return -10;
  if (ptrs && !d->C) return -13;
  if (int rc = check_gemm_operands(d->trans_a, d->trans_b, d->m, d->n, d->k, d->A, d->lda, d->B, d->ldb, d->ldc)) return rc;
  if (reinterpret_cast<uintptr_t>(d->a_mul) & 15) return -15;
  if (reinterpret_cast<uintptr_t>(d->k_scale) & 15) return -16;
  if (d->add && d->beta != 0.0) return -17;
  if (d->add && d->ldadd < d->n) return -18;
  if (!d->rowv != !d->colv) return d->rowv ? -23 : -22;  // the rank-one term needs both vectors
  if (d->ksplit < 1) return -24;
  if (d->scratch && d->ksplit != 1) return -24;
  if (!d->scratch && d->ksplit > 1 && d->cz < (size_t)(d->m - 1) * (size_t)d->ldc + (size_t)d->n) return -25;
  if (d->xcd < 0 || d->xcd > 2) return -26;
  if (reinterpret_cast<uintptr_t>(d->scratch) & 7) return -27;
  return 0;
}

int tgp_gemm_ex_f64(const tgp_gemm_ex* d, void* stream) {
  if (int rc = check_gemm_ex(d, true)) return rc;
  return launch_gemm_ex(*d, static_cast<hipStream_t>(stream));
}

int tgp_gemm_pair_ex_f64(const tgp_gemm_ex* a, const tgp_gemm_ex* b, void* stream) {
  if (!a) return -1;
  if (!b) return -1 - 32;
  if (int rc = check_gemm_ex(a, true)) return rc;
  if (a->trans_a != 0) return -1;
  if (a->trans_b == 0) return -2;
  if (a->scratch) return -27;
  if (int rc = check_gemm_ex(b, true)) return rc - 32;
  if (b->trans_a != 0) return -1 - 32;
  if (b->trans_b != 0) return -2 - 32;
  if (b->scratch) return -27 - 32;
  return launch_gemm_pair_ex(*a, *b, static_cast<hipStream_t>(stream));
}

int tgp_gemm_route(const tgp_gemm_ex* d) {
  if (int rc = check_gemm_ex(d, false)) return rc;
  return gemm_route_ex(*d);
}

int tgp_kl_whitened_f64(const double* m, const double* Lam, int32_t M, double* out, double* g_m, double* g_Lam,
                        void* stream) {
  if (!m) return -1;
  if (!Lam) return -2;
  if (M < 1) return -3;
  if (!out) return -4;
  return launch_kl(m, Lam, M, out, g_m, g_Lam, static_cast<hipStream_t>(stream));
}

int tgp_ell_gauss_f64(const double* Y, const double* mu, const double* v, int32_t N, const double* log_var_noise,
                      double scale, double* out, double* g_mu, double* g_v, void* workspace, size_t workspace_bytes,
                      void* stream) {
  if (!Y) return -1;
  if (!mu) return -2;
  if (!v) return -3;
  if (N < 1) return -4;
  if (!log_var_noise) return -5;
  if (!out) return -7;
  if (!workspace) return -10;
  if (workspace_bytes < lik_workspace_doubles(N, 0, 0) * sizeof(double)) return TGP_E_WORKSPACE;
  return launch_ell_gauss(Y, mu, v, N, log_var_noise, scale, out, g_mu, g_v, static_cast<double*>(workspace),
                          static_cast<hipStream_t>(stream));
}

int tgp_ell_flow_f64(const tgp_model* model, const double* Y, const double* mu, const double* v, const double* rowp,
                     double* out, double* g_mu, double* g_v, double* g_theta, double* g_rowp, void* workspace,
                     size_t workspace_bytes, void* stream) {
  if (refuse_hetero(model, "tgp_ell_flow_f64")) return TGP_E_UNSUPPORTED;
  if (!model || model->N < 1 || model->S < 1 || !model->xs || !model->wn || !model->log_var_noise) return -1;
  if (check_flow_args(model)) return -1;
  if (!Y) return -2;
  if (!mu) return -3;
  if (!v) return -4;
  if (model->RP > 0 && !rowp) return -5;
  if (!out) return -6;
  if (!workspace) return -11;
  if (workspace_bytes < lik_workspace_doubles(model->N, model->P, model->RP) * sizeof(double)) return TGP_E_WORKSPACE;
  FlowProg fp;
  tgp_model md;
  if (int rc = flow_args(model, true, fp, md)) return rc;
  return launch_ell_quad(md, fp, Y, mu, v, rowp, out, g_mu, g_v, g_theta, g_rowp, static_cast<double*>(workspace),
                         static_cast<hipStream_t>(stream));
}

int tgp_ell_hetero_f64(const tgp_model* model, const double* Y, const double* mu, const double* v, const double* rowp,
                       double* out, double* mu_bar, double* v_bar, double* g_theta, double* g_rowp, void* workspace,
                       size_t workspace_bytes, void* stream) {
  if (!model || model->N < 1 || model->S < 1 || !model->xs || !model->wn || !model->log_var_noise) return -1;
  if (check_flow_args(model)) return -1;
  if (!Y) return -2;
  if (!mu) return -3;
  if (!v) return -4;
  if (model->RP > 0 && !rowp) return -5;
  if (!workspace) return -11;
  // the launch needs somewhere to put out[0..1]: without `out`, the two doubles past the partials (inside the sizer's slack)
  const size_t need = lik_workspace_doubles(model->N, model->P, model->RP);
  if (workspace_bytes < need * sizeof(double)) {
    set_error_text("tgp_ell_hetero_f64: workspace of %zu bytes, tgp_ell_workspace_bytes gives %zu", workspace_bytes,
                   need * sizeof(double));
    return TGP_E_WORKSPACE;
  }
  FlowProg fp;
  tgp_model md;
  if (int rc = flow_args(model, true, fp, md)) return rc;
  md.lik = TGP_LIK_HETERO;   // (whatever the caller's model says: this entry IS the likelihood)
  double* ws = static_cast<double*>(workspace);
  return launch_ell_quad(md, fp, Y, mu, v, rowp, out ? out : ws + need - 2, mu_bar, v_bar, g_theta, g_rowp, ws,
                         static_cast<hipStream_t>(stream));
}

int tgp_flow_eval_f64(const tgp_model* model, const double* f, int32_t S, int32_t N, const double* rowp, double* G,
                      double* dG, double* logdG, void* stream) {
  if (int rc = check_flow_points(model, false, f, S, N, rowp)) return rc;
  FlowProg fp;
  tgp_model md;
  if (int rc = flow_args(model, true, fp, md)) return rc;
  return launch_flow_eval(md, fp, f, S, N, rowp, G, dG, logdG, static_cast<hipStream_t>(stream));
}

size_t tgp_flow_logdet_workspace_bytes(int32_t S, int32_t N) {
  return (((size_t)S * (size_t)N + 1023) / 1024 + 16) * sizeof(double);
}

int tgp_flow_logdet_f64(const tgp_model* model, const double* f, int32_t S, int32_t N, const double* rowp, double* G,
                        double* out, void* workspace, size_t workspace_bytes, void* stream) {
  if (int rc = check_flow_points(model, false, f, S, N, rowp)) return rc;
  if (!out) return -7;
  if (!workspace) return -8;
  if (workspace_bytes < tgp_flow_logdet_workspace_bytes(S, N)) return TGP_E_WORKSPACE;
  FlowProg fp;
  tgp_model md;
  if (int rc = flow_args(model, true, fp, md)) return rc;
  return launch_flow_eval(md, fp, f, S, N, rowp, G, nullptr, nullptr, static_cast<hipStream_t>(stream), out,
                          static_cast<double*>(workspace));
}

size_t tgp_ell_warp_workspace_bytes(int32_t N, int32_t P) {
  if (N < 1 || P < 0) return 0;
  return warp_workspace_doubles(N, P) * sizeof(double);
}

int tgp_ell_warp_f64(const tgp_model* model, const double* Y, const double* mu, const double* v, double* out, double* g_mu,
                     double* g_v, double* g_theta, double* t_out, void* workspace, size_t workspace_bytes, void* stream) {
  if (!model || model->N < 1 || !model->log_var_noise || model->nblk < 0 || model->P < 0) return -1;
  if (model->RP != 0) return TGP_E_UNSUPPORTED;
  if (check_flow_args(model)) return -1;
  if (!Y) return -2;
  if (!mu) return -3;
  if (!v) return -4;
  if (!out) return -5;
  if (!workspace) return -10;
  if (workspace_bytes < tgp_ell_warp_workspace_bytes(model->N, model->P)) return TGP_E_WORKSPACE;
  FlowProg fp;
  tgp_model md;
  if (int rc = flow_args(model, true, fp, md)) return rc;
  if (refuse_not_onto(fp, "tgp_ell_warp_f64")) return TGP_E_UNSUPPORTED;
  return launch_ell_warp(md, fp, TGP_WARP_FULL, Y, mu, v, out, g_mu, g_v, g_theta, t_out, static_cast<double*>(workspace),
                         static_cast<hipStream_t>(stream));
}

// descriptor -> by-value kernel arguments: limits, then every block as make_prog checks it, poff made absolute in theta
static int make_softmax(const tgp_softmax* d, SmxArgs& a, FlowProg& fp) {
  if (!d || d->N < 1 || !d->blk_off || !d->theta_off) return -1;
  if (d->C < 3 || d->C > TGP_SOFTMAX_MAX_C || d->S < 1 || d->S > TGP_SOFTMAX_MAX_S) return TGP_E_UNSUPPORTED;
  if (d->blk_off[0] != 0 || d->theta_off[0] != 0) return -1;
  for (int c = 0; c < d->C; ++c)
    if (d->blk_off[c + 1] < d->blk_off[c] || d->theta_off[c + 1] < d->theta_off[c]) return -1;
  const int nblk = d->blk_off[d->C], P = d->theta_off[d->C];
  if (nblk > TGP_MAX_BLOCKS) return TGP_E_UNSUPPORTED;
  if (nblk > 0 && !d->program) return -1;
  if (P > 0 && !d->theta) return -1;
  a.N = d->N; a.C = d->C; a.S = d->S; a.P = P;
  a.scale = d->scale; a.seed = d->seed; a.step_dev = d->step_dev; a.row0 = d->row0;
  for (int c = 0; c <= TGP_SOFTMAX_MAX_C; ++c) a.blk_off[c] = d->blk_off[c < d->C ? c : d->C];
  fp.nblk = nblk;
  for (int c = 0; c < d->C; ++c) {
    const int Pc = d->theta_off[c + 1] - d->theta_off[c];
    for (int b = d->blk_off[c]; b < d->blk_off[c + 1]; ++b) {
      const int kind = d->program[4 * b], K = d->program[4 * b + 1], poff = d->program[4 * b + 2], flags = d->program[4 * b + 3];
      if (int rc = check_block(kind, K, poff, flags, Pc, false)) return rc;   // (RP != 0: no input-dependent flows here)
      fp.blk[4 * b] = kind; fp.blk[4 * b + 1] = K; fp.blk[4 * b + 2] = d->theta_off[c] + poff; fp.blk[4 * b + 3] = flags;
    }
  }
  fp.nslots = flow_slots(fp.blk, fp.nblk);
  return 0;
}

size_t tgp_ell_softmax_workspace_bytes(int32_t N, int32_t P) {
  if (N < 1 || P < 0) return 0;
  return softmax_workspace_doubles(N, P) * sizeof(double);
}

int tgp_ell_softmax_f64(const tgp_softmax* d, const double* Y, const double* mu, const double* v, const double* eps,
                        double* out, double* mu_bar, double* v_bar, double* theta_bar, void* workspace, size_t workspace_bytes,
                        void* stream) {
  SmxArgs a;
  FlowProg fp;
  if (int rc = make_softmax(d, a, fp)) return rc;
  if (!Y) return -2;
  if (!mu) return -3;
  if (!v) return -4;
  if (!out) return -6;
  // forward only: all three adjoints NULL; else mu_bar and v_bar, and theta_bar when there are parameters
  const bool train = mu_bar || v_bar || theta_bar;
  if (train && (!mu_bar || !v_bar)) return -7;
  if (train && a.P > 0 && !theta_bar) return -9;
  if (!workspace) return -10;
  if (workspace_bytes < tgp_ell_softmax_workspace_bytes(a.N, a.P)) return TGP_E_WORKSPACE;
  return launch_ell_softmax(a, fp, d->theta, Y, mu, v, eps, out, mu_bar, v_bar, theta_bar, static_cast<double*>(workspace),
                            static_cast<hipStream_t>(stream));
}

int tgp_mc_normals_f64(const tgp_softmax* d, double* eps, void* stream) {
  if (!d || d->N < 1) return -1;
  if (d->C < 3 || d->C > TGP_SOFTMAX_MAX_C || d->S < 1 || d->S > TGP_SOFTMAX_MAX_S) return TGP_E_UNSUPPORTED;
  if (!eps) return -2;
  SmxArgs a{};
  a.N = d->N; a.C = d->C; a.S = d->S; a.seed = d->seed; a.step_dev = d->step_dev; a.row0 = d->row0;
  return launch_mc_normals(a, eps, static_cast<hipStream_t>(stream));
}

int tgp_predict_softmax_f64(const tgp_softmax* d, const double* mu, const double* v, const double* eps, const double* Y,
                            double* P, double* logp, void* stream) {
  SmxArgs a;
  FlowProg fp;
  if (int rc = make_softmax(d, a, fp)) return rc;
  if (!mu) return -2;
  if (!v) return -3;
  if (!P) return -6;
  if (logp && !Y) return -5;
  return launch_predict_softmax(a, fp, d->theta, mu, v, eps, Y, P, logp, static_cast<hipStream_t>(stream));
}

int tgp_flow_inverse_f64(const tgp_model* model, const double* t, int32_t S, int32_t N, const double* rowp, double* x,
                         int32_t* status, void* stream) {
  if (int rc = check_flow_points(model, true, t, S, N, rowp)) return rc;
  if (!x) return -6;
  if (!status) return -7;
  FlowProg fp;
  tgp_model md;
  if (int rc = flow_args(model, true, fp, md)) return rc;
  if (refuse_not_onto(fp, "tgp_flow_inverse_f64")) return TGP_E_UNSUPPORTED;
  return launch_flow_inverse(md, fp, t, S, N, rowp, x, status, static_cast<hipStream_t>(stream));
}

int tgp_predict_f64(const tgp_model* model, const double* mu, const double* v, const double* rowp, const double* Y,
                    double Y_std, double* m1, double* m2, double* logp, void* stream) {
  if (refuse_hetero(model, "tgp_predict_f64")) return TGP_E_UNSUPPORTED;
  if (!model || model->N < 1 || !model->log_var_noise) return -1;
  if (model->lik == TGP_LIK_WARPED) {
    tgp_model mw = *model;
    mw.RP = 0;   // (rowp is ignored: the warp of the targets has shared parameters only)
    if (model->S < 1 || !model->xs || !model->wn || check_flow_args(&mw, true)) return -1;
    if (!mu) return -2;
    if (!v) return -3;
    FlowProg fpw;
    if (int rc = flow_args(&mw, true, fpw, mw)) return rc;
    if (refuse_not_onto(fpw, "tgp_predict_f64 (TGP_LIK_WARPED)")) return TGP_E_UNSUPPORTED;
    return launch_predict_warp(mw, fpw, mu, v, Y, Y_std, m1, m2, logp, static_cast<hipStream_t>(stream));
  }
  const bool flowed = lik_is_quadrature(model->lik);
  if (flowed && (model->S < 1 || !model->xs || !model->wn)) return -1;
  if (!mu) return -2;
  if (!v) return -3;
  if (flowed && model->RP > 0 && !rowp) return -4;
  FlowProg fp;
  tgp_model md;
  if (int rc = flow_args(model, flowed, fp, md)) return rc;
  return launch_predict(md, fp, mu, v, rowp, Y, Y_std, m1, m2, logp, static_cast<hipStream_t>(stream));
}

int tgp_predict_hetero_f64(const tgp_model* model, const double* mu, const double* v, const double* rowp, const double* Y,
                           double Y_std, double* m1, double* m2, double* logp, void* stream) {
  if (!model || model->N < 1 || !model->log_var_noise) return -1;
  if (model->S < 1 || model->S > TGP_QUANTILE_MAX_S) {
    set_error_text("tgp_predict_hetero_f64: S = %d outside 1..%d", model->S, TGP_QUANTILE_MAX_S);
    return TGP_E_UNSUPPORTED;
  }
  if (!model->xs || !model->wn || check_flow_args(model, true)) return -1;
  if (!mu) return -2;
  if (!v) return -3;
  if (model->RP > 0 && !rowp) return -4;
  FlowProg fp;
  tgp_model md;
  if (int rc = flow_args(model, true, fp, md)) return rc;
  return launch_predict_hetero(md, fp, mu, v, rowp, Y, Y_std, m1, m2, logp, static_cast<hipStream_t>(stream));
}

// the checks the two quantile entries share: likelihood, limits, the pointers the kernels read
static int check_quantile_model(const tgp_model* model, const double* mu, const double* v, const double* rowp, const char* entry,
                                bool* flowed) {
  if (refuse_hetero(model, entry)) return TGP_E_UNSUPPORTED;
  if (!model || model->N < 1 || !model->log_var_noise) return -1;
  const LikRow* row = lik_row(model->lik);
  if (!row) return -1;
  if (row->no_quantiles) {
    set_error_text("%s: no quantiles for %s", entry, row->no_quantiles);
    return TGP_E_UNSUPPORTED;
  }
  if (model->lik != TGP_LIK_GAUSS && model->lik != TGP_LIK_FLOW && model->lik != TGP_LIK_GAMMA && model->lik != TGP_LIK_BETA)
    return -1;
  *flowed = model->lik != TGP_LIK_GAUSS;   // TGP_LIK_GAMMA, TGP_LIK_BETA: whatever the program's length
  if (*flowed) {
    if (model->S < 1 || model->S > TGP_QUANTILE_MAX_S) {
      set_error_text("%s: S = %d outside 1..%d", entry, model->S, TGP_QUANTILE_MAX_S);
      return TGP_E_UNSUPPORTED;
    }
    if (!model->xs || !model->wn || check_flow_args(model, true, false)) return -1;
  }
  if (!mu) return -2;
  if (!v) return -3;
  if (*flowed && model->RP > 0 && !rowp) return -4;
  return 0;
}

int tgp_predict_quantile_f64(const tgp_model* model, const double* mu, const double* v, const double* rowp, const double* probs,
                             const double* zq, int32_t Q, double* t, int32_t* status, void* stream) {
  bool flowed = false;
  if (int rc = check_quantile_model(model, mu, v, rowp, "tgp_predict_quantile_f64", &flowed)) return rc;
  if (Q < 1 || Q > TGP_QUANTILE_MAX_Q) {
    set_error_text("tgp_predict_quantile_f64: Q = %d outside 1..%d", Q, TGP_QUANTILE_MAX_Q);
    return TGP_E_UNSUPPORTED;
  }
  if (!probs) return -5;
  if (!zq) return -6;
  if (!t) return -8;
  if (!status) return -9;
  FlowProg fp;
  tgp_model md;
  if (int rc = flow_args(model, flowed, fp, md)) return rc;
  return launch_predict_quantile(md, fp, mu, v, rowp, probs, zq, Q, t, status, static_cast<hipStream_t>(stream));
}

int tgp_predict_cdf_f64(const tgp_model* model, const double* mu, const double* v, const double* rowp, const double* Y,
                        double* cdf, double* sf, void* stream) {
  bool flowed = false;
  if (int rc = check_quantile_model(model, mu, v, rowp, "tgp_predict_cdf_f64", &flowed)) return rc;
  if (!Y) return -5;
  if (!cdf) return -6;
  FlowProg fp;
  tgp_model md;
  if (int rc = flow_args(model, flowed, fp, md)) return rc;
  return launch_predict_cdf(md, fp, mu, v, rowp, Y, cdf, sf, static_cast<hipStream_t>(stream));
}

int tgp_predict_crps_f64(const tgp_model* model, const double* mu, const double* v, const double* rowp, const double* Y,
                         double* crps, double* parts, void* stream) {
  // (every other likelihood by its number: the closed pair term is the Gaussian mixture's)
  if (model && model->lik != TGP_LIK_GAUSS && model->lik != TGP_LIK_FLOW) {
    set_error_text("tgp_predict_crps_f64: no closed-form CRPS for lik = %d (TGP_LIK_GAUSS and TGP_LIK_FLOW only: the pair term "
                   "is that of an equal-variance Gaussian mixture)", model->lik);
    return TGP_E_UNSUPPORTED;
  }
  bool flowed = false;
  if (int rc = check_quantile_model(model, mu, v, rowp, "tgp_predict_crps_f64", &flowed)) return rc;
  if (!Y) return -5;
  if (!crps) return -6;
  FlowProg fp;
  tgp_model md;
  if (int rc = flow_args(model, flowed, fp, md)) return rc;
  return launch_predict_crps(md, fp, mu, v, rowp, Y, crps, parts, static_cast<hipStream_t>(stream));
}

int tgp_predict_moment_grads_f64(const tgp_model* model, const double* mu, const double* v, const double* rowp, double* dm1,
                                 double* dm2, void* stream) {
  if (model && model->lik != TGP_LIK_GAUSS && model->lik != TGP_LIK_FLOW) {
    set_error_text("tgp_predict_moment_grads_f64: no moment partials for lik = %d (TGP_LIK_GAUSS and TGP_LIK_FLOW only: the "
                   "moments of the other likelihoods are not those of a Gaussian around the flow)", model->lik);
    return TGP_E_UNSUPPORTED;
  }
  bool flowed = false;
  if (int rc = check_quantile_model(model, mu, v, rowp, "tgp_predict_moment_grads_f64", &flowed)) return rc;
  if (!dm1) return -5;
  if (!dm2) return -6;
  FlowProg fp;
  tgp_model md;
  if (int rc = flow_args(model, flowed, fp, md)) return rc;
  return launch_predict_moment_grads(md, fp, mu, v, rowp, dm1, dm2, static_cast<hipStream_t>(stream));
}

int tgp_predict_acquisition_f64(const tgp_model* model, const double* mu, const double* v, const double* rowp, int32_t kind,
                                double best, int32_t minimize, double* value, double* partials, const double* dmu_dx,
                                const double* dv_dx, int32_t D, double* grad_x, void* stream) {
  if (model && model->lik != TGP_LIK_GAUSS && model->lik != TGP_LIK_FLOW) {
    set_error_text("tgp_predict_acquisition_f64: no acquisition function for lik = %d (TGP_LIK_GAUSS and TGP_LIK_FLOW only: the "
                   "improvement terms are those of a Gaussian around the flow)", model->lik);
    return TGP_E_UNSUPPORTED;
  }
  bool flowed = false;
  if (int rc = check_quantile_model(model, mu, v, rowp, "tgp_predict_acquisition_f64", &flowed)) return rc;
  if (kind != TGP_ACQ_EI && kind != TGP_ACQ_LOG_EI && kind != TGP_ACQ_PI) {
    set_error_text("tgp_predict_acquisition_f64: kind = %d is none of TGP_ACQ_EI, TGP_ACQ_LOG_EI, TGP_ACQ_PI", kind);
    return TGP_E_UNSUPPORTED;
  }
  if (!std::isfinite(best)) {
    set_error_text("tgp_predict_acquisition_f64: best = %g is not finite", best);
    return TGP_E_UNSUPPORTED;
  }
  if (!value) return -8;
  if (grad_x) {
    if (!dmu_dx) return -10;
    if (!dv_dx) return -11;
    if (D < 1) return -12;
  }
  FlowProg fp;
  tgp_model md;
  if (int rc = flow_args(model, flowed, fp, md)) return rc;
  return launch_predict_acquisition(md, fp, mu, v, rowp, kind, best, minimize ? -1.0 : 1.0, value, partials, dmu_dx, dv_dx, D,
                                    grad_x, static_cast<hipStream_t>(stream));
}

int tgp_kmeans_assign_f64(const double* X, int32_t N, int32_t D, const double* C, int32_t K, int32_t* labels, double* mind2,
                          void* stream) {
  if (!X) return -1;
  if (N < 1) return -2;
  if (D < 1 || D > 16) return -3;
  if (!C) return -4;
  if (K < 1) return -5;
  if (!labels) return -6;
  return launch_kmeans_assign(X, N, D, C, K, labels, mind2, static_cast<hipStream_t>(stream));
}

int tgp_kmeans_segsum_f64(const double* X, int32_t D, const int64_t* order, const int64_t* offs, int32_t K, double* sums,
                          void* stream) {
  if (!X) return -1;
  if (D < 1 || D > 16) return -2;
  if (!order) return -3;
  if (!offs) return -4;
  if (K < 1) return -5;
  if (!sums) return -6;
  return launch_kmeans_segsum(X, D, order, offs, K, sums, static_cast<hipStream_t>(stream));
}

int tgp_kmeans_pp_f64(const double* X, int32_t N, int32_t D, const int64_t* cand, int32_t T, const double* closest,
                      double* out, void* stream) {
  if (!X) return -1;
  if (N < 1) return -2;
  if (D < 1 || D > 16) return -3;
  if (!cand) return -4;
  if (T < 1 || T > 16) return -5;
  if (!out) return -7;
  return launch_kmeans_pp(X, N, D, cand, T, closest, out, static_cast<hipStream_t>(stream));
}

int tgp_adam_f64(double* params, const double* grads, double* exp_avg, double* exp_avg_sq, int64_t n, double lr,
                 double beta1, double beta2, double eps, double weight_decay, int32_t step, int32_t maximize,
                 void* stream) {
  if (!params) return -1;
  if (!grads) return -2;
  if (!exp_avg) return -3;
  if (!exp_avg_sq) return -4;
  if (n < 1) return -5;
  if (step < 1) return -11;
  return launch_adam(params, grads, exp_avg, exp_avg_sq, n, lr, beta1, beta2, eps, weight_decay, step, maximize,
                     static_cast<hipStream_t>(stream));
}

int tgp_adam_dev_f64(double* params, const double* grads, double* exp_avg, double* exp_avg_sq, int64_t n, double lr,
                     double beta1, double beta2, double eps, double weight_decay, int32_t* step_dev, int32_t maximize,
                     void* stream) {
  if (!params) return -1;
  if (!grads) return -2;
  if (!exp_avg) return -3;
  if (!exp_avg_sq) return -4;
  if (n < 1) return -5;
  if (!step_dev) return -11;
  return launch_adam_dev(params, grads, exp_avg, exp_avg_sq, n, lr, beta1, beta2, eps, weight_decay, step_dev, maximize,
                         static_cast<hipStream_t>(stream));
}

int tgp_gather_rows_f64(const double* X, const double* Y, int32_t N, int32_t D, const int32_t* index, int32_t* cursor_dev,
                        int32_t offset, int32_t nrows, int32_t advance, int32_t wrap, double* Xb, double* Yb, void* stream) {
  if (!X) return -1;
  if (!Y) return -2;
  if (N < 1 || D < 1) return -3;
  if (!cursor_dev) return -6;
  if (offset < 0 || nrows < 1 || nrows > N) return -8;
  if (advance < 0 || wrap < 1) return -9;
  if (!Xb) return -11;
  if (!Yb) return -12;
  return launch_gather_rows(X, Y, N, D, index, cursor_dev, offset, nrows, advance, wrap, Xb, Yb,
                            static_cast<hipStream_t>(stream));
}

int tgp_adam_dev_groups_f64(double* params, const double* grads, double* exp_avg, double* exp_avg_sq, int64_t n,
                            double lr, double beta1, double beta2, double eps, int64_t n_plain, double weight_decay_tail,
                            int32_t* step_dev, int32_t maximize, void* stream) {
  if (!params) return -1;
  if (!grads) return -2;
  if (!exp_avg) return -3;
  if (!exp_avg_sq) return -4;
  if (n < 1) return -5;
  if (n_plain < 0 || n_plain > n) return -10;
  if (!step_dev) return -12;
  return launch_adam_dev(params, grads, exp_avg, exp_avg_sq, n, lr, beta1, beta2, eps, weight_decay_tail, step_dev, maximize,
                         static_cast<hipStream_t>(stream), n_plain);
}

size_t tgp_mlp_workspace_bytes(const tgp_mlp* mlp) {
  if (!mlp) return 0;
  return mlp_workspace_doubles(mlp->N, mlp->D, mlp->H, mlp->L, mlp->nnets) * sizeof(double);
}

int tgp_mlp_forward_f64(const tgp_mlp* mlp, const double* X, const double* W, const int32_t* step_dev, double* out,
                        void* stream) {
  if (!mlp) return -1;
  if (!X) return -2;
  if (!W) return -3;
  if (!out) return -5;
  return launch_mlp_forward(*mlp, X, W, step_dev, out, static_cast<hipStream_t>(stream));
}

int tgp_mlp_backward_f64(const tgp_mlp* mlp, const double* X, const double* W, const int32_t* step_dev,
                         const double* g_out, double* g_W, void* workspace, size_t workspace_bytes, void* stream) {
  if (!mlp) return -1;
  if (!X) return -2;
  if (!W) return -3;
  if (!g_out) return -5;
  if (!g_W) return -6;
  if (!workspace) return -7;
  return launch_mlp_backward(*mlp, X, W, step_dev, g_out, g_W, static_cast<double*>(workspace),
                             workspace_bytes / sizeof(double), static_cast<hipStream_t>(stream));
}

int tgp_mlp_backward_adam_f64(const tgp_mlp* mlp, const double* X, double* W, const int32_t* step_dev, const double* g_out,
                              double* g_W, void* workspace, size_t workspace_bytes, const tgp_adam_args* adam,
                              double weight_decay, void* stream) {
  if (!mlp) return -1;
  if (!X) return -2;
  if (!W) return -3;
  if (!g_out) return -5;
  if (!g_W) return -6;
  if (!workspace) return -7;
  if (check_adam(adam) || adam->params != W || adam->grads != g_W) return -9;
  // the optimiser state must cover every weight the kernel updates (nnets x weights per net)
  {
    size_t per = (size_t)mlp->H * mlp->D + mlp->H;
    for (int l = 1; l < mlp->L; ++l) per += (size_t)mlp->H * mlp->H + mlp->H;
    per += (size_t)mlp->H + 1;
    if ((size_t)adam->n != per * (size_t)mlp->nnets) return -9;
  }
  const AdamDev ad = adam_dev_of(adam);
  return launch_mlp_backward(*mlp, X, W, step_dev, g_out, g_W, static_cast<double*>(workspace),
                             workspace_bytes / sizeof(double), static_cast<hipStream_t>(stream), &ad, weight_decay);
}

int tgp_comm_load(const char* rccl_path) { return comm_load(rccl_path); }

int tgp_comm_unique_id(void* id128) {
  if (!id128) return -1;
  return comm_unique_id(id128);
}

int tgp_comm_init(const void* id128, int32_t nranks, int32_t rank, void** comm) {
  if (!id128) return -1;
  if (nranks < 1) return -2;
  if (rank < 0 || rank >= nranks) return -3;
  if (!comm) return -4;
  return comm_init(id128, nranks, rank, comm);
}

int tgp_allreduce_f64(void* comm, double* buf, int64_t n, void* stream) {
  if (!comm) return -1;
  if (!buf) return -2;
  if (n < 1) return -3;
  return comm_allreduce(comm, buf, n, static_cast<hipStream_t>(stream));
}

int tgp_comm_destroy(void* comm) {
  if (!comm) return -1;
  return comm_destroy(comm);
}

}  // extern "C"
