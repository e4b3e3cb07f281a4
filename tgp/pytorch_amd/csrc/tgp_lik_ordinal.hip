// tgp_lik_ordinal.hip -- the ordinal (cumulative-probit) likelihood (TGP_LIK_ORDINAL): its policies and the instantiations of
// k_ell_quad and k_predict_quad (tgp_ell.hpp) for them, in a unit of their own as tgp_lik_negbin.hip is: two erfcx, two erfc and
// three exponentials per node make these 22 kernels compile as slowly as the negative-binomial ones.
#include "tgp_ell.hpp"

namespace tgp {

// Ordered categories y in {0, .., K-1} with fixed bin edges b_1 < .. < b_{K-1} (b_0 = -inf, b_K = +inf) and latent noise of scale
// sigma (TGP_LIK_ORDINAL): log_var_noise = {eta = log sigma^2, K, b_1, .., b_{K-1}}.  With u = (b_{y+1} - g) / sigma, l = (b_y - g) / sigma:
//   log p(y | g) = log(Phi(u) - Phi(l)),   d log p / dg = (phi(l) - phi(u)) / (sigma p),   d log p / d eta = (l phi(l) - u phi(u)) / (2 p).
// The difference is formed on the side where both tails are small (bern_node's rule).  Bin on one side of g, near edge a = min(|l|, |u|),
// far edge c = max(|l|, |u|), E = exp(-(c^2 - a^2) / 2), D = erfcx(a / sqrt 2) - erfcx(c / sqrt 2) E:
//   p = Phi(-a) - Phi(-c) = exp(-a^2 / 2) D / 2        log p = -a^2 / 2 + log(D / 2)
//   phi(a) - phi(c) = phi(a) (1 - E)                    |d log p / dg| = sqrt(2 / pi) (1 - E) / (sigma D), towards the bin
//   a phi(a) - c phi(c) = phi(a) (a - c E)              d log p / d eta = sqrt(2 / pi) (a - c E) / (2 D)
// -- exp(-a^2 / 2) cancels out of both ratios, so they stay finite however far g is from the bin (a = 1e8: log p ~ -5e15, the
// ratios ~ a and a^2 / 2).  1 - E is -expm1(.): a narrow bin (c - a small) loses nothing there.  Bin around g (l <= 0 <= u):
//   p = 1 - erfc(-l / sqrt 2) / 2 - erfc(u / sqrt 2) / 2    log p = log1p(-(..)),   the ratios from phi(l), phi(u) and p directly.
// An infinite edge enters as E = 0, c E = 0 (one side) or erfc = 0, phi = 0, edge phi = 0 (around): no inf * 0 is formed.
// The class is y clamped into [0, K-1], a y that is not >= 0 (NaN too) is class 0: b is read at indices 0 .. K-2 only.
struct OrdConst { double eta, isig; int K; const double* b; };   // isig = 1 / sigma; b[j - 1] = b_j, j = 1 .. K-1
struct OrdNode { double lp, dg, de; };                           // log p, d log p / dg, d log p / d eta
__device__ __forceinline__ OrdConst ord_consts(const double* lvn) {
  const int K = (int)lvn[1];
  return {lvn[0], exp(-0.5 * lvn[0]), K < 2 ? 2 : (K > 64 ? 64 : K), lvn + 2};
}
__device__ __forceinline__ int ord_class(double y, int K) { return y >= 0.0 ? (y < (double)(K - 1) ? (int)y : K - 1) : 0; }
// the node term of class k at g, edges scaled by isig (the predictive's closed form passes 1 / sqrt(sigma^2 + v))
__device__ inline OrdNode ord_node(double g, int k, double isig, const OrdConst& K) {
  const bool lo_inf = k == 0, hi_inf = k == K.K - 1;
  const double l = lo_inf ? 0.0 : (K.b[k - 1] - g) * isig;    // (placeholders where the edge is infinite: never used as values)
  const double u = hi_inf ? 0.0 : (K.b[k] - g) * isig;
  const bool above = !lo_inf && l > 0.0, below = !hi_inf && u < 0.0;
  OrdNode r;
  if (above || below) {
    const double a = above ? l : -u;                            // near edge, > 0
    const bool far_inf = above ? hi_inf : lo_inf;
    const double c = far_inf ? a : (above ? u : -l);            // far edge, >= a
    const double exa = erfcx(a * 0.70710678118654752440);
    double E = 0.0, cE = 0.0, omE = 1.0;
    if (!far_inf) {
      const double h = -0.5 * (c - a) * (c + a);
      E = exp(h);
      omE = -expm1(h);
      cE = c * E;
    }
    const double D = exa - (far_inf ? 0.0 : erfcx(c * 0.70710678118654752440) * E);
    const double q = 0.79788456080286535588 / D;                // sqrt(2 / pi) / D
    r.lp = -0.5 * a * a + log(0.5 * D);
    r.dg = (above ? q : -q) * omE * isig;
    r.de = 0.5 * q * (a - cE);
  } else {
    const double al = -l, au = u;                               // both >= 0
    const double tl = lo_inf ? 0.0 : 0.5 * erfc(al * 0.70710678118654752440);
    const double tu = hi_inf ? 0.0 : 0.5 * erfc(au * 0.70710678118654752440);
    const double pl = lo_inf ? 0.0 : 0.39894228040143267794 * exp(-0.5 * al * al);   // phi(l)
    const double pu = hi_inf ? 0.0 : 0.39894228040143267794 * exp(-0.5 * au * au);   // phi(u)
    const double t = tl + tu, ip = 1.0 / (1.0 - t);
    r.lp = log1p(-t);
    r.dg = (pl - pu) * ip * isig;
    r.de = 0.5 * (l * pl - u * pu) * ip;
  }
  return r;
}

struct EllOrdinal {
  static constexpr bool kNoise = true;    // partial slot 1 carries the adjoint of eta (K and the edges are not trained)
  static constexpr bool kClampV = true;   // as EllBern
  static constexpr bool kRowTerm = false;
  static constexpr bool kRowNoise = false;
  static constexpr bool kBlockTerm = false;
  static constexpr bool kRowConst = false;
  static __device__ __forceinline__ OrdConst consts(const double* lvn) { return ord_consts(lvn); }
  static __device__ __forceinline__ OrdNode at(double g, double y, const OrdConst& k) { return ord_node(g, ord_class(y, k.K), k.isig, k); }
  static __device__ __forceinline__ double log_p(const OrdNode& t, const OrdConst&) { return t.lp; }
  static __device__ __forceinline__ double dlog_p_deta(const OrdNode& t, const OrdConst&) { return t.de; }
  static __device__ __forceinline__ double adjoint(const OrdNode& t, double scale, double w, const OrdConst&) { return scale * w * t.dg; }
};

// Prediction: with sf_j(g) = 1 - Phi((b_j - g) / sigma) = P(y >= j | g), j = 1 .. K-1,
//   m1 = E[y] = sum_s w_s sum_j sf_j(g_s),   E[y^2] = sum_s w_s sum_j (2j - 1) sf_j(g_s)   (y^2 = sum_{j <= y} (2j - 1)),   m2 = E[y^2] - m1^2,
//   logp = log sum_s w_s p(y | g_s) = logsumexp_s(log w_s + log p(y | g_s)), the log predictive pmf of class y.
// The empty program is closed: q(f) N(mu, v) and the probit noise convolve, every edge at (b_j - mu) / sqrt(sigma^2 + max(v, 0)).
// Nodes of weight 0 do not enter.  Y_std is not used: classes have no units.
struct PredOrdinal {
  static constexpr bool kClampV = true;
  using Acc = PredSums;
  static __device__ __forceinline__ void moments(double g, double isig, double w, const OrdConst& k, double& m1, double& e2) {
    double s1 = 0.0, s2 = 0.0;
    for (int j = 1; j < k.K; ++j) {
      const double sf = 0.5 * erfc((k.b[j - 1] - g) * isig * 0.70710678118654752440);
      s1 += sf;
      s2 += (double)(2 * j - 1) * sf;
    }
    m1 += w * s1;
    e2 += w * s2;
  }
  static __device__ __forceinline__ bool closed(const tgp_model&, const FlowProg& fp) { return fp.nblk == 0; }
  static __device__ __forceinline__ PredOut closed_row(const PredRow& R, const double* lvn, double) {
    const OrdConst k = ord_consts(lvn);
    const double isig = 1.0 / sqrt(exp(k.eta) + (R.v > 0.0 ? R.v : 0.0));
    double m1 = 0.0, e2 = 0.0;
    moments(R.m, isig, 1.0, k, m1, e2);
    return {m1, e2 - m1 * m1, R.want_lp ? ord_node(R.m, ord_class(R.y, k.K), isig, k).lp : 0.0};
  }
  static __device__ __forceinline__ OrdConst consts(const tgp_model& md, const FlowProg&, double) { return ord_consts(md.log_var_noise); }
  static __device__ __forceinline__ void node(Acc& a, double w, double g, const PredRow& R, const OrdConst& k) {
    if (!(w > 0.0)) return;
    moments(g, k.isig, w, k, a.m1, a.e2);
    if (R.want_lp) lse_push(a.l, log(w) + ord_node(g, ord_class(R.y, k.K), k.isig, k).lp);
  }
  static __device__ __forceinline__ PredOut finish(const Acc& a, const PredRow& R, const OrdConst&) {
    return {a.m1, a.e2 - a.m1 * a.m1, R.want_lp ? lse_value(a.l) : 0.0};
  }
};

int ell_launch_ordinal(int LPR, int NB, int ext, int nb, size_t lds, hipStream_t st, const tgp_model& md, const FlowProg& fp,
                       const double* Y, const double* mu, const double* v, const double* rowp, double* part, double* g_mu, double* g_v,
                       double* g_rowp) {
  return ell_launch_row<EllOrdinal>(LPR, NB, ext, nb, lds, st, md, fp, Y, mu, v, rowp, part, g_mu, g_v, g_rowp);
}

int predict_launch_ordinal(const tgp_model& md, const FlowProg& fp, const double* mu, const double* v, const double* rowp,
                           const double* Y, double Y_std, double* m1, double* m2, double* logp, hipStream_t st) {
  return predict_launch<PredOrdinal>(md, fp, mu, v, rowp, Y, Y_std, m1, m2, logp, st);
}

}  // namespace tgp
