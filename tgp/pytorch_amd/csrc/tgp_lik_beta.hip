// tgp_lik_beta.hip -- the Beta likelihood with a logit link (TGP_LIK_BETA): its policies and the instantiations of k_ell_quad and
// k_predict_quad (tgp_ell.hpp) for them, in a unit of their own as tgp_lik_gamma.hip and tgp_lik_negbin.hip are: two lgamma and
// two digamma per node.  The exact CDF and quantiles of its predictive are in tgp_quantile.hip (QBeta).
#include "tgp_ell.hpp"

namespace tgp {

// Proportions, the flow as the log-odds of the mean (TGP_LIK_BETA): y ~ Beta(a, b), a = mu phi, b = (1 - mu) phi, mu = sigmoid(g),
// Var = mu (1 - mu) / (1 + phi).  log_var_noise[0] = lambda = log phi, trained through partial slot 1.  With ly = log y,
// l1 = log1p(-y) and y* = ly - l1:
//   log p(y | g) = [lgamma(phi) + phi l1 - ly - l1] - lgamma(a) - lgamma(b) + a y*
//   d log p / dg = mu (1 - mu) phi [y* - psi(a) + psi(b)]
//   d log p / dlambda = phi [psi(phi) + l1] + phi [mu y* - mu psi(a) - (1 - mu) psi(b)].
// g is not clamped.  1 - mu is sigmoid(-g), from the same exp(-|g|) and the same division as mu, so that a and b both keep their
// digits at large |g|.  y* is the same for every node of a row (the compiler takes the logs out of the node loop).  The
// brackets (row_term, row_deta) depend on y and phi only: once per row, by the row's first lane.  lgamma(phi) and psi(phi) are
// launch constants.  Supported range 0.5 <= phi <= 1e3 (include/tgp_hip.h); phi is not looked at.
struct BetaConst { double lam, phi, lgphi, psiphi; };   // lgphi = lgamma(phi), psiphi = psi(phi)
struct BetaMean { double mu, nu; };                     // sigmoid(g) and sigmoid(-g)
__device__ __forceinline__ BetaMean beta_mean(double g) {
  const double e = exp(-fabs(g)), d = 1.0 / (1.0 + e), ed = e * d;
  return {g > 0.0 ? d : ed, g > 0.0 ? ed : d};
}
struct BetaNode { double lp, de, dg; };   // the node's parts of log p, of d/dlambda and of d/dg
struct EllBeta {
  static constexpr bool kNoise = true;    // partial slot 1 carries the adjoint of lambda
  static constexpr bool kClampV = true;   // as EllBern
  static constexpr bool kRowTerm = true;
  static constexpr bool kRowNoise = true;
  static constexpr bool kBlockTerm = false;
  static constexpr bool kRowConst = false;
  static constexpr int kMaxNB = 4;        // with 8 nodes in flight the kernel spills (EllMaxNB)
  static __device__ __forceinline__ BetaConst consts(const double* lvn) {
    const double lam = lvn[0], phi = exp(lam);
    return {lam, phi, lgamma(phi), digamma_d(phi)};
  }
  using Node = BetaNode;
  static __device__ __forceinline__ Node at(double g, double y, const BetaConst& k) {
    const BetaMean m = beta_mean(g);
    const double a = m.mu * k.phi, b = m.nu * k.phi, ys = log(y) - log1p(-y);
    const double pa = digamma_d(a), pb = digamma_d(b);
    return {a * ys - lgamma(a) - lgamma(b), k.phi * (m.mu * ys - m.mu * pa - m.nu * pb), m.mu * m.nu * k.phi * (ys - pa + pb)};
  }
  static __device__ __forceinline__ double log_p(const Node& t, const BetaConst&) { return t.lp; }
  static __device__ __forceinline__ double dlog_p_deta(const Node& t, const BetaConst&) { return t.de; }
  static __device__ __forceinline__ double adjoint(const Node& t, double scale, double w, const BetaConst&) {
    return scale * w * t.dg;
  }
  static __device__ __forceinline__ double row_term(double y, const BetaConst& k) {
    const double ly = log(y), l1 = log1p(-y);
    return k.lgphi + k.phi * l1 - ly - l1;
  }
  static __device__ __forceinline__ double row_deta(double y, const BetaConst& k) { return k.phi * (k.psiphi + log1p(-y)); }
};

// Prediction, mu_s = sigmoid(g_s) the mean at node s:
//   m1 = E[y] = sum_s w_s mu_s,  m2 = Var[y] = sum_s w_s mu_s (1 - mu_s) / (1 + phi) + sum_s w_s mu_s^2 - m1^2   (law of total
//   variance with Var[y | g] = mu (1 - mu) / (1 + phi)); Var[mu] = sum_s w_s mu_s^2 - m1^2 is taken from nu_s = 1 - mu_s instead,
//   sum_s w_s nu_s^2 - (sum_s w_s nu_s)^2, where that mean is the smaller one: the same number, without the cancellation of two
//   sums next to 1 when the mean is (a row at g = 9 would keep 1e-9 of its variance of 1e-7),
//   logp = logsumexp_s(log w_s + a_s y* - lgamma(a_s) - lgamma(b_s)) + lgamma(phi) + phi l1 - ly - l1,
// the empty program takes all three from the sweep as well.  Y_std is ignored: proportions are never standardised.  Nodes of
// weight 0 do not enter.
struct PredBeta : PredSweepOnly {
  static constexpr bool kClampV = true;
  using K = BetaConst;
  // sum w mu, sum w mu^2, sum w nu, sum w nu^2, sum w mu nu (nu = 1 - mu), the log-sum-exp
  struct Acc { double m1 = 0.0, e2 = 0.0, n1 = 0.0, f2 = 0.0, mn = 0.0; LogSumExp l; };
  static __device__ __forceinline__ K consts(const tgp_model& md, const FlowProg&, double) { return EllBeta::consts(md.log_var_noise); }
  static __device__ __forceinline__ void node(Acc& a, double w, double g, const PredRow& R, const K& k) {
    if (!(w > 0.0)) return;
    const BetaMean m = beta_mean(g);
    a.m1 += w * m.mu;
    a.e2 += w * m.mu * m.mu;
    a.n1 += w * m.nu;
    a.f2 += w * m.nu * m.nu;
    a.mn += w * m.mu * m.nu;
    if (R.want_lp) {
      const double sa = m.mu * k.phi, sb = m.nu * k.phi;
      lse_push(a.l, log(w) + (sa * (log(R.y) - log1p(-R.y)) - lgamma(sa) - lgamma(sb)));
    }
  }
  static __device__ __forceinline__ PredOut finish(const Acc& a, const PredRow& R, const K& k) {
    PredOut o;
    o.m1 = a.m1;
    o.m2 = a.mn / (1.0 + k.phi) + (a.m1 <= a.n1 ? a.e2 - a.m1 * a.m1 : a.f2 - a.n1 * a.n1);
    o.lp = R.want_lp ? lse_value(a.l) + EllBeta::row_term(R.y, k) : 0.0;
    return o;
  }
};

int ell_launch_beta(int LPR, int NB, int ext, int nb, size_t lds, hipStream_t st, const tgp_model& md, const FlowProg& fp,
                    const double* Y, const double* mu, const double* v, const double* rowp, double* part, double* g_mu, double* g_v,
                    double* g_rowp) {
  return ell_launch_row<EllBeta>(LPR, NB, ext, nb, lds, st, md, fp, Y, mu, v, rowp, part, g_mu, g_v, g_rowp);
}

int predict_launch_beta(const tgp_model& md, const FlowProg& fp, const double* mu, const double* v, const double* rowp,
                        const double* Y, double Y_std, double* m1, double* m2, double* logp, hipStream_t st) {
  return predict_launch<PredBeta>(md, fp, mu, v, rowp, Y, Y_std, m1, m2, logp, st);
}

}  // namespace tgp
