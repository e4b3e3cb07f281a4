// tgp_lik_gamma.hip -- the Gamma likelihood with a log link (TGP_LIK_GAMMA): its policies and the instantiations of k_ell_quad
// and k_predict_quad (tgp_ell.hpp) for them, in a unit of their own as tgp_lik_negbin.hip is.  The exact CDF and quantiles of its
// predictive are in tgp_quantile.hip (QGamma).
#include "tgp_ell.hpp"

namespace tgp {

// Positive targets, the flow as the log-mean (TGP_LIK_GAMMA): y ~ Gamma(shape a, mean exp(g)), rate a e^-g, Var = exp(2 g) / a.
// log_var_noise[0] = lambda = log a, trained through partial slot 1.  With l = log y and z = l - g:
//   log p(y | g) = [a log a - lgamma(a) - l] + a (z - e^z)
//   d log p / dg = a (e^z - 1)
//   d log p / dlambda = a (log a + 1 - psi(a)) + a (z - e^z).
// g is not clamped: a node whose e^z overflows gives -inf, as the float64 formula does.  Per node one exp, shared by the value
// and the adjoint; l is the same for every node of a row (the compiler takes the log out of the node loop).  The bracket
// (row_term) depends on y and a, the first d/dlambda term (row_deta) on a only: once per row, by the row's first lane.
// a log a - lgamma(a) and a (log a + 1 - psi(a)) are launch constants.  Supported range 0.1 <= a <= 1e3 (include/tgp_hip.h);
// a is not looked at.
struct GammaConst { double lam, a, c0, d0; };   // c0 = a log a - lgamma(a), d0 = a (log a + 1 - psi(a))
struct GammaNode { double zme, em1; };          // z - e^z and e^z - 1: the value and the adjoint share the exponential
struct EllGamma {
  static constexpr bool kNoise = true;    // partial slot 1 carries the adjoint of lambda
  static constexpr bool kClampV = true;   // as EllBern
  static constexpr bool kRowTerm = true;
  static constexpr bool kRowNoise = true;
  static constexpr bool kBlockTerm = false;
  static constexpr bool kRowConst = false;
  static __device__ __forceinline__ GammaConst consts(const double* lvn) {
    const double lam = lvn[0], a = exp(lam);
    return {lam, a, a * lam - lgamma(a), a * (lam + 1.0 - digamma_d(a))};
  }
  using Node = GammaNode;
  static __device__ __forceinline__ Node at(double g, double y, const GammaConst&) {
    const double z = log(y) - g, e = exp(z);
    return {z - e, e - 1.0};
  }
  static __device__ __forceinline__ double log_p(const Node& t, const GammaConst& k) { return k.a * t.zme; }
  static __device__ __forceinline__ double dlog_p_deta(const Node& t, const GammaConst& k) { return k.a * t.zme; }
  static __device__ __forceinline__ double adjoint(const Node& t, double scale, double w, const GammaConst& k) {
    return scale * w * (k.a * t.em1);
  }
  static __device__ __forceinline__ double row_term(double y, const GammaConst& k) { return k.c0 - log(y); }
  static __device__ __forceinline__ double row_deta(double, const GammaConst& k) { return k.d0; }
};

// Prediction, g_s the log-mean at node s:
//   m1 = E[y] = sum_s w_s exp(g_s),  m2 = Var[y] = (1 + 1/a) sum_s w_s exp(2 g_s) - m1^2   (law of total variance with
//   Var[y | g] = exp(2 g) / a: no `m1 +` term, which is what sets it apart from PredCount; the empty program: the log-normal
//   closed forms m1 = exp(mu + v / 2), m2 = (expm1(v) + exp(v) / a) m1^2, v <= 0 as 0),
//   logp = logsumexp_s(log w_s + a (z_s - e^z_s)) + a log a - lgamma(a) - l - log Y_std,
// the log density of the raw target (the family is closed under scaling); the empty program takes it from the sweep as well.
// Nodes of weight 0 do not enter.
struct PredGamma : PredSweepOnly {
  static constexpr bool kClampV = true;
  struct K { double a, c0, lYstd; bool lognormal; };
  using Acc = PredSums;
  static __device__ __forceinline__ K consts(const tgp_model& md, const FlowProg& fp, double Y_std) {
    const GammaConst g = EllGamma::consts(md.log_var_noise);
    return {g.a, g.c0, log(Y_std), fp.nblk == 0};
  }
  static __device__ __forceinline__ void node(Acc& a, double w, double g, const PredRow& R, const K& k) {
    if (!(w > 0.0)) return;
    const double e = exp(g);
    a.m1 += w * e;
    a.e2 += w * e * e;
    if (R.want_lp) {
      const double z = log(R.y) - g;
      lse_push(a.l, log(w) + k.a * (z - exp(z)));
    }
  }
  static __device__ __forceinline__ PredOut finish(const Acc& a, const PredRow& R, const K& k) {
    const double vn = R.v > 0.0 ? R.v : 0.0, c = 1.0 / k.a;
    PredOut o;
    o.m1 = k.lognormal ? exp(R.m + 0.5 * vn) : a.m1;
    o.m2 = k.lognormal ? (expm1(vn) + c * exp(vn)) * o.m1 * o.m1 : (1.0 + c) * a.e2 - a.m1 * a.m1;
    o.lp = R.want_lp ? lse_value(a.l) + k.c0 - log(R.y) - k.lYstd : 0.0;
    return o;
  }
};

int ell_launch_gamma(int LPR, int NB, int ext, int nb, size_t lds, hipStream_t st, const tgp_model& md, const FlowProg& fp,
                     const double* Y, const double* mu, const double* v, const double* rowp, double* part, double* g_mu, double* g_v,
                     double* g_rowp) {
  return ell_launch_row<EllGamma>(LPR, NB, ext, nb, lds, st, md, fp, Y, mu, v, rowp, part, g_mu, g_v, g_rowp);
}

int predict_launch_gamma(const tgp_model& md, const FlowProg& fp, const double* mu, const double* v, const double* rowp,
                         const double* Y, double Y_std, double* m1, double* m2, double* logp, hipStream_t st) {
  return predict_launch<PredGamma>(md, fp, mu, v, rowp, Y, Y_std, m1, m2, logp, st);
}

}  // namespace tgp
