// tgp_lik_negbin.hip -- the negative-binomial likelihood (TGP_LIK_NEGBIN): its policy and the instantiations of k_ell_quad and
// k_predict_quad (tgp_ell.hpp) for it, in a unit of their own: three lgamma and two digamma per kernel make these 22 kernels as
// slow to compile as two thirds of tgp_lik.hip's 115.
#include "tgp_ell.hpp"

namespace tgp {

// Negative-binomial counts, the flow as the log-mean (TGP_LIK_NEGBIN): y ~ NB(mean = exp(g), dispersion r), Var = mean + mean^2 / r,
// r -> inf the Poisson.  log_var_noise[0] = lambda = log r, trained through partial slot 1.  With u = g - lambda and
// sp(u) = log(1 + e^u) (u > 0 ? u + log1p(e^-u) : log1p(e^u)):
//   log p(y | g) = [lgamma(y + r) - lgamma(r) - lgamma(y + 1)] + y u - (y + r) sp(u)
//   d log p / dg = y - (y + r) sigmoid(u)
//   d log p / dlambda = r [psi(y + r) - psi(r)] - r sp(u) - d log p / dg.
// g is not clamped.  Per node one exp(-|u|), one log1p and one division, shared by sp and the sigmoid; the bracket (row_term) and
// the psi term (row_deta) depend on y and r only: once per row, by the row's first lane.  lgamma(r) and psi(r) are launch
// constants.  Supported range 1e-3 <= r <= 1e3: past it the terms of d/dlambda cancel (include/tgp_hip.h); r is not looked at.
struct NegBinConst { double lam, r, lgr, psir; };   // lgr = lgamma(r), psir = psi(r)
struct NegBinNode { double g, u, y, sp, sg; };      // sp = sp(u), sg = sigmoid(u)
struct EllNegBin {
  static constexpr bool kNoise = true;    // partial slot 1 carries the adjoint of lambda
  static constexpr bool kClampV = true;   // as EllBern
  static constexpr bool kRowTerm = true;
  static constexpr bool kRowNoise = true;
  static constexpr bool kBlockTerm = false;
  static constexpr bool kRowConst = false;
  static constexpr bool kOverDisp = true;   // PredCount: Var[y | mean] = mean + mean^2 excess(K)
  static __device__ __forceinline__ NegBinConst consts(const double* lvn) {
    const double lam = lvn[0], r = exp(lam);
    return {lam, r, lgamma(r), digamma_d(r)};
  }
  static __device__ __forceinline__ NegBinNode at(double g, double y, const NegBinConst& k) {
    const double u = g - k.lam, e = exp(-fabs(u)), d = 1.0 / (1.0 + e);
    return {g, u, y, (u > 0.0 ? u : 0.0) + log1p(e), u > 0.0 ? d : e * d};
  }
  static __device__ __forceinline__ double dg(const NegBinNode& t, const NegBinConst& k) { return t.y - (t.y + k.r) * t.sg; }
  static __device__ __forceinline__ double log_p(const NegBinNode& t, const NegBinConst& k) { return t.y * t.u - (t.y + k.r) * t.sp; }
  static __device__ __forceinline__ double dlog_p_deta(const NegBinNode& t, const NegBinConst& k) { return -k.r * t.sp - dg(t, k); }
  static __device__ __forceinline__ double adjoint(const NegBinNode& t, double scale, double w, const NegBinConst& k) {
    return scale * w * dg(t, k);
  }
  static __device__ __forceinline__ double row_term(double y, const NegBinConst& k) {
    return lgamma(y + k.r) - k.lgr - lgamma(y + 1.0);
  }
  static __device__ __forceinline__ double row_deta(double y, const NegBinConst& k) { return k.r * (digamma_d(y + k.r) - k.psir); }
  static __device__ __forceinline__ double rate(const NegBinNode& t) { return exp(t.g); }   // PredCount: the mean
  static __device__ __forceinline__ double excess(const NegBinConst& k) { return 1.0 / k.r; }
  static __device__ __forceinline__ double plus_log_p(double a, const NegBinNode& t, const NegBinConst& k) { return a + log_p(t, k); }
};

int ell_launch_negbin(int LPR, int NB, int ext, int nb, size_t lds, hipStream_t st, const tgp_model& md, const FlowProg& fp,
                      const double* Y, const double* mu, const double* v, const double* rowp, double* part, double* g_mu, double* g_v,
                      double* g_rowp) {
  return ell_launch_row<EllNegBin>(LPR, NB, ext, nb, lds, st, md, fp, Y, mu, v, rowp, part, g_mu, g_v, g_rowp);
}

int predict_launch_negbin(const tgp_model& md, const FlowProg& fp, const double* mu, const double* v, const double* rowp,
                          const double* Y, double Y_std, double* m1, double* m2, double* logp, hipStream_t st) {
  return predict_launch<PredCount<EllNegBin>>(md, fp, mu, v, rowp, Y, Y_std, m1, m2, logp, st);
}

}  // namespace tgp
