// tgp_quantile.hip -- exact predictive CDF and quantiles of the Gauss-Hermite predictive of tgp_predict_f64:
//   p(y | x_n) = sum_s wn_s N(y | g_ns, sig^2),  g_ns = G(mu_n + sqrt(2 v_n) xs_s),  sig^2 = exp(log_var_noise)
//   F_n(t) = sum_s wn_s Phi((t - g_ns) / sig),   F_n'(t) = sum_s wn_s phi((t - g_ns) / sig) / sig   (the density above)
//   k_pred_cdf<C, X>    cdf = F_n(Y_n) and the upper tail 1 - F_n from its own sum
//   k_pred_quantile<C, X> t = the root of F_n(t) = p for Q probabilities per row, a bracketed Newton iteration on the S node values
//   k_quantile_gauss    TGP_LIK_GAUSS / the empty program: one Gaussian, closed forms for both
//   k_predict_hetero<X> the heteroscedastic predictive (tgp_predict_hetero_f64): moments and log density on the same node table
//   k_pred_crps<X, W>   the CRPS int (F_n(t) - 1{t >= Y_n})^2 dt in closed form: one pass over the nodes, one over their pairs
//   k_crps_gauss        ... of one Gaussian (TGP_LIK_GAUSS / the empty program)
//   k_pred_acq<KIND, X> expected improvement, its logarithm and the probability of improvement against an incumbent, with their
//                       partials in mu and v and (optionally) the chain rule with the Jacobians of q(f); k_acq_gauss: one Gaussian
// QLPR = 16 lanes share a data row (4 rows per wave, one wave per workgroup): the lanes sweep the row's S nodes -- and the Q
// starting points G(mu + zq sqrt v) -- through the flow once (flow_forward_n, 4 elements in flight per lane) into LDS, and
// every evaluation of F afterwards reads those S numbers only: lane l adds the nodes l, l + 16, ... in that order, the 16
// partial sums are added by a DPP butterfly (every lane of the row ends with the same bits).  No float atomics, fixed
// summation order: same input, same bits.  The loops are uniform over the wave (a row that is done keeps evaluating at its
// root until the wave's last row is done), so the cross-lane adds always run with every lane on.
// X: the extended flow kind set, as in k_predict_quad<Pred, X>.
// C: the mixture component of k_pred_cdf and k_pred_quantile, a policy.  QGauss is the Gaussian around the flow above.  QGamma
// (TGP_LIK_GAMMA) is a Gamma of shape a = exp(log_var_noise) and mean exp(g_ns): a location family in tau = log t,
//   F_n(tau) = sum_s wn_s P(a, a e^(tau - g_ns)),   F_n'(tau) = sum_s wn_s h(tau - g_ns)      (gamma_pq below),
// so the same root rule runs on tau and the kernel returns t = exp(tau).  QBeta (TGP_LIK_BETA) is a Beta(phi sigmoid(g_ns),
// phi sigmoid(-g_ns)), phi = exp(log_var_noise): the root rule runs on x = logit t over a regularised incomplete beta function
// (beta_cf below) and the kernel returns t = sigmoid(x).
#include "tgp_dev.hpp"
#include "tgp_launch.hpp"

namespace tgp {

#define QLPR 16                       /* lanes per data row */
#define QROWS (64 / QLPR)             /* rows per workgroup (one wave) */
#define Q_MAXIT 128                   /* evaluations of F per phase */
#define Q_SQRT1_2 0.70710678118654752440
#define Q_INV_SQRT_2PI 0.39894228040143267794

// row stride (doubles) of the node table: >= n and = 16 mod 32, so that the 16-double windows the two rows of a 32-lane half
// read together fall on different banks
static int q_row_stride(int n) { return (n + 15) / 32 * 32 + 16; }

// sum over the 16 lanes of a row, every lane gets the total (ror_sum: x[l] + x[l ^ R] once x is 2R-periodic)
__device__ __forceinline__ double row16_sum(double x) { return ror_sum<1>(ror_sum<2>(ror_sum<4>(ror_sum<8>(x)))); }

// lower = sum_s wn_s Phi(z_s), upper = sum_s wn_s Phi(-z_s), dens = sum_s wn_s phi(z_s) / sig at t, z_s = (t - g_s) / sig.
// Phi through erfc on the side where it is small (bern_node's rule): Phi(-|z|) = erfc(|z| / sqrt 2) / 2, Phi(|z|) = 1 - that.
struct QSum { double lower, upper, dens; };
template <bool DENS>
__device__ __forceinline__ QSum q_eval(const double* __restrict__ g, const double* __restrict__ wn, int S, int l16, double t,
                                       double sig) {
  double lo = 0.0, up = 0.0, dn = 0.0;
  for (int s0 = 0; s0 < S; s0 += QLPR) {
    const int s = s0 + l16, sc = s < S ? s : S - 1;
    const double w = s < S ? wn[sc] : 0.0;
    const double z = (t - g[sc]) / sig, a = fabs(z);
    const double small = 0.5 * erfc(a * Q_SQRT1_2), big = 1.0 - small;
    lo += w * (z < 0.0 ? small : big);
    up += w * (z < 0.0 ? big : small);
    if (DENS) dn += w * exp(-0.5 * z * z);
  }
  QSum r;
  r.lower = row16_sum(lo);
  r.upper = row16_sum(up);
  r.dens = DENS ? row16_sum(dn) * Q_INV_SQRT_2PI / sig : 0.0;
  return r;
}

// What a mixture component supplies to k_pred_cdf and k_pred_quantile: consts(log_var_noise) = its per-thread constants K;
// eval<DENS>(g, wn, S, l16, x, K) = the three sums at x; arg(y) = the x at which the CDF of the target y is read and value(x) the
// quantile a root x stands for; start(gq, zq, p, K) = the first x of the root of probability p, gq = G(mu + zq sqrt v), and
// first_step(x, K) the first bracket step; kZeroVarClosed: the start is the root of a row without variance.  kCols: the columns
// of S doubles its node table takes (the launchers size the row for them); prep(gs, S, Q, l16, K), after the sweep, once per
// row: what the component keeps per node beside or in place of the node value (QBeta; nothing for the other two).
struct QGauss {
  static constexpr bool kZeroVarClosed = true;   // one node value: the start is the closed form G(mu) + zq sig
  static constexpr int kCols = 1;
  struct K { double sig; };
  static __device__ __forceinline__ void prep(double*, int, int, int, K&) {}
  static __device__ __forceinline__ K consts(const double* lvn) { return {sqrt(exp(lvn[0]))}; }
  template <bool DENS>
  static __device__ __forceinline__ QSum eval(const double* __restrict__ g, const double* __restrict__ wn, int S, int l16, double x,
                                              const K& k) {
    return q_eval<DENS>(g, wn, S, l16, x, k.sig);
  }
  static __device__ __forceinline__ double arg(double y) { return y; }
  static __device__ __forceinline__ double value(double x) { return x; }
  static __device__ __forceinline__ double start(double gq, double zq, double, const K& k) { return gq + zq * k.sig; }
  static __device__ __forceinline__ double first_step(double x, const K& k) { return fmax(k.sig, fabs(x) * 9.5367431640625e-07); }
};

// The regularised incomplete gamma functions P(a, x) and Q(a, x) = 1 - P at x = a e^z, with the density of the component in z,
//   h(z) = x^a e^-x / Gamma(a) = exp(a (z - expm1(z)) + c),   c = a log a - a - lgamma(a)   (once per thread, QGamma::K::c):
// the expm1 form has none of the cancellation of a log x - x - lgamma(a) at large a.  x < a + 1: the power series
// P = h sum_n x^n / (a (a + 1) .. (a + n)), Q = 1 - P; otherwise the continued fraction of Q by the modified Lentz rule,
// P = 1 - Q: each side is computed where it is the small one or both are of order one.  x = 0 (z = -inf): (0, 1); x = +inf:
// (1, 0).  At most TGP_GAMMA_PQ_MAXIT terms (a in [0.1, 1e3], z in [-8, 3]: 268 at most, tests/test_gamma_host.py); a NaN runs
// the series to that cap and comes out as NaN.  Lanes run different trip counts and meet again behind the loop.
struct GammaPQ { double P, Q, h; };
__device__ __forceinline__ GammaPQ gamma_pq(double a, double c, double z) {
  const double x = a * exp(z);
  if (x == 0.0) return {0.0, 1.0, 0.0};
  if (x == INFINITY) return {1.0, 0.0, 0.0};
  const double h = exp(a * (z - expm1(z)) + c);
  if (x < a + 1.0) {
    double ap = a, sum = 1.0 / a, del = sum;
    for (int n = 0; n < TGP_GAMMA_PQ_MAXIT; ++n) {
      ap += 1.0;
      del *= x / ap;
      sum += del;
      if (fabs(del) < fabs(sum) * 1.1102230246251565e-16) break;
    }
    const double P = sum * h;
    return {P, 1.0 - P, h};
  }
  constexpr double FPMIN = 1e-300;
  double b = x + 1.0 - a, cc = 1.0 / FPMIN, d = 1.0 / b, f = d;
  for (int i = 1; i <= TGP_GAMMA_PQ_MAXIT; ++i) {
    const double an = -(double)i * ((double)i - a);
    b += 2.0;
    d = an * d + b;
    if (fabs(d) < FPMIN) d = FPMIN;
    cc = b + an / cc;
    if (fabs(cc) < FPMIN) cc = FPMIN;
    d = 1.0 / d;
    const double del = d * cc;
    f *= del;
    if (fabs(del - 1.0) < 1.1102230246251565e-16) break;
  }
  const double Qv = f * h;
  return {1.0 - Qv, Qv, h};
}

struct QGamma {
  static constexpr bool kZeroVarClosed = false;   // no closed form: a row without variance iterates like any other
  static constexpr int kCols = 1;
  struct K { double a, c, lga1, lam; };           // c as in gamma_pq, lga1 = lgamma(a + 1), lam = log a
  static __device__ __forceinline__ void prep(double*, int, int, int, K&) {}
  static __device__ __forceinline__ K consts(const double* lvn) {
    const double lam = lvn[0], a = exp(lam);
    return {a, a * lam - a - lgamma(a), lgamma(a + 1.0), lam};
  }
  // lower = sum_s wn_s P(a, a e^z_s), upper = sum_s wn_s Q(a, a e^z_s), dens = sum_s wn_s h(z_s) at x = tau, z_s = tau - g_s
  template <bool DENS>
  static __device__ __forceinline__ QSum eval(const double* __restrict__ g, const double* __restrict__ wn, int S, int l16, double x,
                                              const K& k) {
    double lo = 0.0, up = 0.0, dn = 0.0;
    for (int s0 = 0; s0 < S; s0 += QLPR) {
      const int s = s0 + l16, sc = s < S ? s : S - 1;
      const double w = s < S ? wn[sc] : 0.0;
      const GammaPQ r = gamma_pq(k.a, k.c, x - g[sc]);
      lo += w * r.P;
      up += w * r.Q;
      if (DENS) dn += w * r.h;
    }
    QSum r;
    r.lower = row16_sum(lo);
    r.upper = row16_sum(up);
    r.dens = DENS ? row16_sum(dn) : 0.0;
    return r;
  }
  // tau = log y; a target <= 0 has nothing below it (tau = -inf: every term is (0, 1)); a NaN stays one
  static __device__ __forceinline__ double arg(double y) { return y > 0.0 ? log(y) : (y <= 0.0 ? -INFINITY : y); }
  static __device__ __forceinline__ double value(double x) { return exp(x); }
  // the log-quantile of one Gamma(a, rate a) around the flow's value: the larger of the Wilson-Hilferty value (where its argument
  // is positive) and the small-argument value from P(a, x) ~ x^a / Gamma(a + 1)
  static __device__ __forceinline__ double start(double gq, double zq, double p, const K& k) {
    const double wh = 1.0 - 1.0 / (9.0 * k.a) + zq / (3.0 * sqrt(k.a));
    const double sm = (log(p) + k.lga1) / k.a - k.lam;
    return gq + (wh > 0.0 ? fmax(3.0 * log(wh), sm) : sm);
  }
  static __device__ __forceinline__ double first_step(double x, const K& k) {
    return fmax(fmax(1.0 / sqrt(k.a), 1.0 / k.a), fabs(x) * 9.5367431640625e-07);
  }
};

// The continued fraction of the regularised incomplete beta function, I_t(a, b) = t^a (1 - t)^b / (a B(a, b)) beta_cf(a, b, t), by
// the modified Lentz rule, two coefficients per step; it converges fast for t < (a + 1) / (a + b + 2).  At most TGP_BETA_CF_MAXIT
// steps (phi in [0.5, 1e3], |g| <= 12, |logit t| <= 15: 87 at most, tests/test_beta_host.py); a NaN runs to that cap and comes
// out as NaN.  Lanes run different trip counts and meet again behind the loop.
__device__ __forceinline__ double beta_cf(double a, double b, double t) {
  constexpr double FPMIN = 1e-300;
  const double qab = a + b, qap = a + 1.0, qam = a - 1.0;
  double c = 1.0, d = 1.0 - qab * t / qap;
  if (fabs(d) < FPMIN) d = FPMIN;
  d = 1.0 / d;
  double h = d;
  for (int m = 1; m <= TGP_BETA_CF_MAXIT; ++m) {
    const double dm = (double)m, m2 = 2.0 * dm;
    double aa = dm * (b - dm) * t / ((qam + m2) * (a + m2));
    d = 1.0 + aa * d;
    if (fabs(d) < FPMIN) d = FPMIN;
    c = 1.0 + aa / c;
    if (fabs(c) < FPMIN) c = FPMIN;
    d = 1.0 / d;
    h *= d * c;
    aa = -(a + dm) * (qab + dm) * t / ((a + m2) * (qap + m2));
    d = 1.0 + aa * d;
    if (fabs(d) < FPMIN) d = FPMIN;
    c = 1.0 + aa / c;
    if (fabs(c) < FPMIN) c = FPMIN;
    d = 1.0 / d;
    const double del = d * c;
    h *= del;
    if (fabs(del - 1.0) < 2.2204460492503131e-16) break;
  }
  return h;
}

// QBeta (TGP_LIK_BETA): the component at node s is a Beta(a_s, b_s), a_s = phi sigmoid(g_ns), b_s = phi sigmoid(-g_ns),
// phi = exp(log_var_noise).  Not a location family -- both shape parameters change from node to node -- so prep() turns the node
// table of a row, once per row, into three columns: a_s in place of g_s, then behind the Q starting points b_s and
// nlb_s = -log B(a_s, b_s) = lgamma(phi) - lgamma(a_s) - lgamma(b_s) (K::off = S + Q is where b starts).  The root rule runs on
// x = logit t and the kernel returns t = sigmoid(x); with lt = log t = -softplus(-x) and lu = log(1 - t) = -softplus(x), formed once
// per evaluation from one exp(-|x|),
//   h_s = exp(a_s lt + b_s lu + nlb_s)                the density of the component in x (the Jacobian t (1 - t) removes the two -1s)
//   t < (a_s + 1) / (phi + 2):  lower = h_s beta_cf(a_s, b_s, t) / a_s,      upper = 1 - lower
//   else:                       upper = h_s beta_cf(b_s, a_s, 1 - t) / b_s,  lower = 1 - upper,
// each tail computed where it is the small one or both are of order one.  x = -inf: (0, 1); x = +inf: (1, 0).
struct QBeta {
  static constexpr bool kZeroVarClosed = false;   // no closed form: a row without variance iterates like any other
  static constexpr int kCols = 3;                 // columns of the node table
  struct K { double phi, lgphi; int off; };
  static __device__ __forceinline__ K consts(const double* lvn) {
    const double phi = exp(lvn[0]);
    return {phi, lgamma(phi), 0};
  }
  // lane l16 rewrites the node values it wrote in q_sweep (s = l16 mod 16): no barrier in between
  static __device__ __forceinline__ void prep(double* __restrict__ gs, int S, int Q, int l16, K& k) {
    k.off = S + Q;
    for (int s = l16; s < S; s += QLPR) {
      const double g = gs[s], e = exp(-fabs(g)), d = 1.0 / (1.0 + e), ed = e * d;
      const double a = (g > 0.0 ? d : ed) * k.phi, b = (g > 0.0 ? ed : d) * k.phi;
      gs[s] = a;
      gs[k.off + s] = b;
      gs[k.off + S + s] = k.lgphi - lgamma(a) - lgamma(b);
    }
  }
  template <bool DENS>
  static __device__ __forceinline__ QSum eval(const double* __restrict__ g, const double* __restrict__ wn, int S, int l16, double x,
                                              const K& k) {
    const double e = exp(-fabs(x)), d = 1.0 / (1.0 + e), ed = e * d, l1e = log1p(e);
    const double t = x > 0.0 ? d : ed, u = x > 0.0 ? ed : d;                      // t and 1 - t
    const double lt = x > 0.0 ? -l1e : x - l1e, lu = x > 0.0 ? -x - l1e : -l1e;   // their logs
    double lo = 0.0, up = 0.0, dn = 0.0;
    for (int s0 = 0; s0 < S; s0 += QLPR) {
      const int s = s0 + l16, sc = s < S ? s : S - 1;
      const double w = s < S ? wn[sc] : 0.0;
      const double a = g[sc], b = g[k.off + sc], h = exp(a * lt + b * lu + g[k.off + S + sc]);
      const bool low = t < (a + 1.0) / (a + b + 2.0);
      const double small = low ? h * beta_cf(a, b, t) / a : h * beta_cf(b, a, u) / b, big = 1.0 - small;
      lo += w * (low ? small : big);
      up += w * (low ? big : small);
      if (DENS) dn += w * h;
    }
    QSum r;
    r.lower = row16_sum(lo);
    r.upper = row16_sum(up);
    r.dens = DENS ? row16_sum(dn) : 0.0;
    return r;
  }
  // x = logit y; a target <= 0 has nothing below it, a target >= 1 nothing above; a NaN stays one
  static __device__ __forceinline__ double arg(double y) {
    return y <= 0.0 ? -INFINITY : (y >= 1.0 ? INFINITY : log(y) - log1p(-y));
  }
  static __device__ __forceinline__ double value(double x) { return 1.0 / (1.0 + exp(-x)); }
  // the logit of one Beta(a, b) around the flow's value gq is roughly normal with variance 1 / a + 1 / b
  static __device__ __forceinline__ double start(double gq, double zq, double, const K& k) {
    const double e = exp(-fabs(gq));
    return gq + zq * sqrt((1.0 + e) * (1.0 + e) / (e * k.phi));   // 1 / a + 1 / b = 1 / (phi mu (1 - mu)), mu (1 - mu) = e d^2
  }
  // 1 / a + 1 / b >= 4 / phi
  static __device__ __forceinline__ double first_step(double x, const K& k) {
    return fmax(2.0 / sqrt(k.phi), fabs(x) * 9.5367431640625e-07);
  }
};

// The row's elements e = 0 .. S + Q - 1 through the flow into gs[e]: the quadrature nodes mu + sqrt(2 v) xs_e (the argument
// k_predict forms), then the Q starting points mu + zq_q sqrt(v).  Lane l16 takes e = l16 + 16 j, four at a time.
template <bool X>
__device__ __forceinline__ void q_sweep(const FlowDev& F, const tgp_model& md, const double* __restrict__ rp, double m_, double vn,
                                        const double* __restrict__ zq, int Q, int l16, double* __restrict__ gs) {
  constexpr int NB = 4;
  const int ne = md.S + Q;
  const double sq2 = sqrt(2.0 * vn), sq1 = sqrt(vn);
  for (int e0 = 0; e0 < ne; e0 += NB * QLPR) {
    double f[NB], der[NB];
    const double* rpn[NB];
    TGP_EACH(u, NB) {
      const int e = e0 + u * QLPR + l16, ec = e < ne ? e : ne - 1;
      f[u] = ec < md.S ? m_ + sq2 * md.xs[ec] : m_ + zq[ec - md.S] * sq1;
      rpn[u] = rp;
    }
    flow_forward_n<NB, false, X>(F, f, rpn, der);
    TGP_EACH(u, NB) {
      const int e = e0 + u * QLPR + l16;
      if (e < ne) gs[e] = f[u];
    }
  }
}

// dynamic LDS: tp, tg ((P + 2) / 2 * 2 each), wn (S rounded up to even), then QROWS node tables of q_row_stride(kCols S + Q)
template <class C, bool X>
__global__ __launch_bounds__(64) void k_pred_quantile(tgp_model md, FlowProg fp, const double* __restrict__ mu,
                                                      const double* __restrict__ v, const double* __restrict__ rowp,
                                                      const double* __restrict__ probs, const double* __restrict__ zq, int Q,
                                                      int stride, double* __restrict__ t_out, int32_t* __restrict__ status) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  double* tp = reinterpret_cast<double*>(smem_raw);
  double* tg = tp + (md.P + 2) / 2 * 2;
  double* wl = tg + (md.P + 2) / 2 * 2;
  const int lane = threadIdx.x, l16 = lane & (QLPR - 1), r = lane / QLPR, S = md.S;
  double* gs = wl + (S + 1) / 2 * 2 + (size_t)r * stride;
  for (int s = lane; s < S; s += 64) wl[s] = md.wn[s];
  flow_params_lds<X>(md.theta, fp, tp, tg);   // (ends with a barrier: wl is staged too)
  FlowDev F{fp.blk, fp.nblk, tp, tg};
  const int n = blockIdx.x * QROWS + r;
  const bool valid = n < md.N;
  const int nc = valid ? n : md.N - 1;
  const double* rp = rowp ? rowp + (size_t)nc * md.RP : nullptr;
  const double m_ = mu[nc], vr = v[nc], vn = vr > 0.0 ? vr : 0.0;
  typename C::K K = C::consts(md.log_var_noise);
  q_sweep<X>(F, md, rp, m_, vn, zq, Q, l16, gs);
  C::prep(gs, S, Q, l16, K);
  __syncthreads();
  for (int q = 0; q < Q; ++q) {
    const double p = probs[q];
    const bool upper = p > 0.5;
    const double tgt = upper ? 1.0 - p : p;
    // fx = F(x) - p, taken from the tail that is small: increasing in x on both sides, derivative = the density
    double x = C::start(gs[S + q], zq[q], p, K);
    QSum e = C::template eval<true>(gs, wl, S, l16, x, K);
    double fx = upper ? tgt - e.upper : e.lower - tgt, dn = e.dens;
    // QGauss: a row without variance has one node value: the start is its closed form G(mu) + zq sig
    bool done = (C::kZeroVarClosed && !(vr > 0.0)) || fx == 0.0, fail = false;
    // ---- bracket: doubling steps from the start
    double step = C::first_step(x, K);
    const bool grow_up = fx < 0.0;
    double lo = grow_up ? x : x - step, hi = grow_up ? x + step : x;
    bool ok = done;
    for (int it = 0; it < Q_MAXIT; ++it) {
      if (__ballot(!ok) == 0ull) break;
      const double probe = ok ? x : (grow_up ? hi : lo);
      const QSum eb = C::template eval<false>(gs, wl, S, l16, probe, K);
      const double fb = upper ? tgt - eb.upper : eb.lower - tgt;
      if (!ok) {
        if (grow_up ? fb >= 0.0 : fb <= 0.0) {
          ok = true;
        } else {
          step *= 2.0;
          if (grow_up) { lo = hi; hi = lo + step; } else { hi = lo; lo = hi - step; }
        }
      }
    }
    if (!ok) { fail = true; done = true; }
    // ---- Newton steps with the density, bisection whenever a step leaves the open bracket
    for (int it = 0; it < Q_MAXIT; ++it) {
      if (!done) {
        if (fx == 0.0) {
          done = true;
        } else {
          if (fx < 0.0) lo = x; else hi = x;
          double xn = x - fx / dn;
          if (!(xn > lo && xn < hi)) xn = 0.5 * (lo + hi);
          const double dx = fabs(xn - x);
          x = xn;
          if (dx <= 8.8817841970012523e-16 * fmax(1.0, fabs(x))) done = true;
        }
      }
      if (__ballot(!done) == 0ull) break;
      e = C::template eval<true>(gs, wl, S, l16, x, K);
      if (!done) { fx = upper ? tgt - e.upper : e.lower - tgt; dn = e.dens; }
    }
    if (!done) fail = true;
    if (valid && l16 == 0) {
      t_out[(size_t)q * md.N + n] = fail ? NAN : C::value(x);
      if (fail) atomicAdd(status, 1);
    }
  }
}

template <class C, bool X>
__global__ __launch_bounds__(64) void k_pred_cdf(tgp_model md, FlowProg fp, const double* __restrict__ mu,
                                                 const double* __restrict__ v, const double* __restrict__ rowp,
                                                 const double* __restrict__ Y, int stride, double* __restrict__ cdf,
                                                 double* __restrict__ sf) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  double* tp = reinterpret_cast<double*>(smem_raw);
  double* tg = tp + (md.P + 2) / 2 * 2;
  double* wl = tg + (md.P + 2) / 2 * 2;
  const int lane = threadIdx.x, l16 = lane & (QLPR - 1), r = lane / QLPR, S = md.S;
  double* gs = wl + (S + 1) / 2 * 2 + (size_t)r * stride;
  for (int s = lane; s < S; s += 64) wl[s] = md.wn[s];
  flow_params_lds<X>(md.theta, fp, tp, tg);
  FlowDev F{fp.blk, fp.nblk, tp, tg};
  const int n = blockIdx.x * QROWS + r;
  const bool valid = n < md.N;
  const int nc = valid ? n : md.N - 1;
  const double* rp = rowp ? rowp + (size_t)nc * md.RP : nullptr;
  const double vr = v[nc], vn = vr > 0.0 ? vr : 0.0;
  typename C::K K = C::consts(md.log_var_noise);
  q_sweep<X>(F, md, rp, mu[nc], vn, nullptr, 0, l16, gs);
  C::prep(gs, S, 0, l16, K);
  __syncthreads();
  const QSum e = C::template eval<false>(gs, wl, S, l16, C::arg(Y[nc]), K);
  if (valid && l16 == 0) {
    cdf[n] = e.lower;
    if (sf) sf[n] = e.upper;
  }
}

// The partials of the predictive moments m1 = sum_s wn_s g_s, m2 = sum_s wn_s g_s^2 - m1^2 + sig^2 in mu and v
// (tgp_predict_moment_grads_f64): with g'_s = G'(f_s) at f_s = mu + sqrt(2 v) xs_s, d f_s / d mu = 1 and d f_s / d v = xs_s / sqrt(2 v),
//   dm1 = (sum wn g',  sum wn g' xs / sqrt(2 v)),   dm2 = 2 (sum wn g g', sum wn g g' xs / sqrt(2 v)) - 2 m1 dm1.
// The row's 16 lanes sweep its S nodes with the derivative (flow_forward_n<4, true, X>), lane l the nodes l, l + 16, ... in that
// order, and keep five partial sums in registers -- no node table; row16_sum adds the 16 lanes in the fixed lane order.  A row
// with v <= 0 counts as v = 0: every node is mu, the v-partials are exact zeros.
// dynamic LDS: tp, tg ((P + 2) / 2 * 2 each), then wn and xs (S rounded up to even each)
template <bool X>
__global__ __launch_bounds__(64) void k_pred_mgrad(tgp_model md, FlowProg fp, const double* __restrict__ mu,
                                                   const double* __restrict__ v, const double* __restrict__ rowp,
                                                   double* __restrict__ dm1, double* __restrict__ dm2) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  double* tp = reinterpret_cast<double*>(smem_raw);
  double* tg = tp + (md.P + 2) / 2 * 2;
  double* wl = tg + (md.P + 2) / 2 * 2;
  const int lane = threadIdx.x, l16 = lane & (QLPR - 1), r = lane / QLPR, S = md.S;
  double* xl = wl + (S + 1) / 2 * 2;
  for (int s = lane; s < S; s += 64) { wl[s] = md.wn[s]; xl[s] = md.xs[s]; }
  flow_params_lds<X>(md.theta, fp, tp, tg);   // (ends with a barrier: wl and xl are staged too)
  FlowDev F{fp.blk, fp.nblk, tp, tg};
  const int n = blockIdx.x * QROWS + r;
  const bool valid = n < md.N;
  const int nc = valid ? n : md.N - 1;
  const double* rp = rowp ? rowp + (size_t)nc * md.RP : nullptr;
  const double m_ = mu[nc], vr = v[nc], vn = vr > 0.0 ? vr : 0.0, sq2 = sqrt(2.0 * vn);
  constexpr int NB = 4;
  double sg = 0.0, sd = 0.0, sdx = 0.0, sgd = 0.0, sgdx = 0.0;
  for (int e0 = 0; e0 < S; e0 += NB * QLPR) {
    double f[NB], der[NB];
    const double* rpn[NB];
    TGP_EACH(u, NB) {
      const int e = e0 + u * QLPR + l16, ec = e < S ? e : S - 1;
      f[u] = m_ + sq2 * xl[ec];
      rpn[u] = rp;
    }
    flow_forward_n<NB, true, X>(F, f, rpn, der);
    TGP_EACH(u, NB) {
      const int e = e0 + u * QLPR + l16, ec = e < S ? e : S - 1;
      const double w = e < S ? wl[ec] : 0.0, wd = w * der[u], wgd = wd * f[u];
      sg += w * f[u];
      sd += wd;
      sdx += wd * xl[ec];
      sgd += wgd;
      sgdx += wgd * xl[ec];
    }
  }
  const double m1 = row16_sum(sg), a = row16_sum(sd), gd = row16_sum(sgd);
  const double tdx = row16_sum(sdx), tgdx = row16_sum(sgdx);   // (the cross-lane adds run with every lane on)
  const double inv = vr > 0.0 ? 1.0 / sq2 : 0.0;
  const double b = vr > 0.0 ? tdx * inv : 0.0, gdx = vr > 0.0 ? tgdx * inv : 0.0;
  if (valid && l16 == 0) {
    dm1[n] = a;
    dm1[(size_t)md.N + n] = b;
    dm2[n] = 2.0 * gd - 2.0 * m1 * a;
    dm2[(size_t)md.N + n] = vr > 0.0 ? 2.0 * gdx - 2.0 * m1 * b : 0.0;
  }
}

// TGP_LIK_GAUSS / the empty program: m1 = mu, m2 = max(v, 0) + sig^2: (1, 0) and (0, 1 where v > 0)
__global__ __launch_bounds__(256) void k_mgrad_gauss(int N, const double* __restrict__ v, double* __restrict__ dm1,
                                                     double* __restrict__ dm2) {
  const int n = blockIdx.x * 256 + threadIdx.x;
  if (n >= N) return;
  dm1[n] = 1.0;
  dm1[(size_t)N + n] = 0.0;
  dm2[n] = 0.0;
  dm2[(size_t)N + n] = v[n] > 0.0 ? 1.0 : 0.0;
}

// Acquisition functions of the same predictive against an incumbent b (tgp_predict_acquisition_f64), c = +1 to maximise and
// -1 to minimise, z_s = c (g_s - b) / sig, h(z) = z Phi(z) + phi(z) (h' = Phi):
//   EI = sig sum_s wn_s h(z_s) = E[(c (y - b))_+],   PI = sum_s wn_s Phi(z_s),   logEI = log sig + logsumexp_s(log wn_s + log h(z_s)).
// acq_h: h, log h and the ratios Phi / h, phi / h without the cancellation of z Phi + phi at negative z.  With
// q(z) = Phi / phi = sqrt(pi / 2) erfcx(-z / sqrt 2), h = phi t, t = 1 + z q:
//   z > -1          h = z Phi + phi as written (Phi through erfc)
//   -30 < z <= -1   t = 1 + z q, log t = log1p(z q)
//   z <= -30        t = u (1 - 3 u (1 - 5 u (1 - 7 u (1 - 9 u (1 - 11 u))))), u = 1 / z^2: the asymptotic series of 1 + z q, whose
//                   direct form has lost eps z^2 of its value to the cancellation by then; the first term left out is 135135 u^7
// log h = -z^2 / 2 - log sqrt(2 pi) + log t,  Phi / h = q / t,  phi / h = 1 / t on the lower two branches.
#define Q_SQRT_PI_2 1.25331413731550025121
#define Q_LOG_SQRT_2PI 0.91893853320467274178
struct AcqH { double h, logh, Phi_h, phi_h; };
__device__ __forceinline__ AcqH acq_h(double z) {
  AcqH r;
  if (z > -1.0) {
    const double Phi = 0.5 * erfc(-z * Q_SQRT1_2), phi = Q_INV_SQRT_2PI * exp(-0.5 * z * z);
    r.h = z * Phi + phi;
    r.logh = log(r.h);
    r.Phi_h = Phi / r.h;
    r.phi_h = phi / r.h;
    return r;
  }
  const double q = Q_SQRT_PI_2 * erfcx(-z * Q_SQRT1_2);
  double t, logt;
  if (z > -30.0) {
    t = 1.0 + z * q;
    logt = log1p(z * q);
  } else {
    const double u = 1.0 / (z * z);
    t = u * (1.0 - 3.0 * u * (1.0 - 5.0 * u * (1.0 - 7.0 * u * (1.0 - 9.0 * u * (1.0 - 11.0 * u)))));
    logt = log(t);
  }
  r.logh = -0.5 * z * z - Q_LOG_SQRT_2PI + logt;
  r.h = Q_INV_SQRT_2PI * exp(-0.5 * z * z) * t;
  r.Phi_h = q / t;
  r.phi_h = 1.0 / t;
  return r;
}
// Phi(z), as q_eval forms it (PI at b is k_pred_cdf's upper or lower tail at Y = b, term for term)
__device__ __forceinline__ double acq_Phi(double z) {
  const double small = 0.5 * erfc(fabs(z) * Q_SQRT1_2);
  return z < 0.0 ? small : 1.0 - small;
}

// grad_x[n, :] = a_mu dmu_dx[n, :] + a_v dv_dx[n, :], the row's 16 lanes over d = l16, l16 + 16, ...: the chain rule of the two
// partials with the Jacobians of q(f) (tgp_qf_input_grad_f64), two products and one sum per element as written
__device__ __forceinline__ void acq_chain(double a_mu, double a_v, const double* __restrict__ dmu_dx,
                                          const double* __restrict__ dv_dx, int D, size_t n, int l16, double* __restrict__ grad_x) {
  for (int d = l16; d < D; d += QLPR) grad_x[n * D + d] = a_mu * dmu_dx[n * D + d] + a_v * dv_dx[n * D + d];
}

// The partials in mu and v at fixed flow parameters, with g'_s = G'(f_s) as in k_pred_mgrad:
//   d EI / d mu = c sum wn_s Phi(z_s) g'_s,            d PI / d mu = (c / sig) sum wn_s phi(z_s) g'_s,
//   d logEI / d mu = (c / sig) sum_s p_s (Phi / h)(z_s) g'_s,   p_s = wn_s h(z_s) / sum_t wn_t h(z_t)  (the softmax weights),
// and in v the same sums with g'_s xs_s / sqrt(2 v).  The row's 16 lanes sweep its S nodes once with the derivative, lane l the
// nodes l, l + 16, ... in that order, three partial sums in registers -- no node table.  logEI: each lane keeps its sums relative
// to its running maximum of log wn_s + log h(z_s) (weights of 0 do not enter), the 16 lanes' sums are joined under the row's
// maximum: value and partials stay finite where EI itself underflows to 0 (a row whose every term is -inf -- z^2 overflows at
// every node, or every weight is 0 -- gives -inf and NaN partials).  row16_sum adds the 16 lanes in the fixed lane
// order; no float atomics: same input, same bits, and a row's outputs depend on that row's inputs only.  A row with v <= 0
// counts as v = 0: every node is mu, the v-partial is an exact zero.  grad_x (optional): acq_chain with the row's two partials.
// dynamic LDS: tp, tg ((P + 2) / 2 * 2 each), then wn and xs (S rounded up to even each), then log wn (the same) for logEI
template <int KIND, bool X>
__global__ __launch_bounds__(64) void k_pred_acq(tgp_model md, FlowProg fp, const double* __restrict__ mu,
                                                 const double* __restrict__ v, const double* __restrict__ rowp, double best,
                                                 double c, double* __restrict__ value, double* __restrict__ partials,
                                                 const double* __restrict__ dmu_dx, const double* __restrict__ dv_dx, int D,
                                                 double* __restrict__ grad_x) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  double* tp = reinterpret_cast<double*>(smem_raw);
  double* tg = tp + (md.P + 2) / 2 * 2;
  double* wl = tg + (md.P + 2) / 2 * 2;
  const int lane = threadIdx.x, l16 = lane & (QLPR - 1), r = lane / QLPR, S = md.S, S2 = (S + 1) / 2 * 2;
  double* xl = wl + S2;
  double* lw = xl + S2;
  for (int s = lane; s < S; s += 64) {
    const double w = md.wn[s];
    wl[s] = w;
    xl[s] = md.xs[s];
    if (KIND == TGP_ACQ_LOG_EI) lw[s] = w > 0.0 ? log(w) : -INFINITY;
  }
  flow_params_lds<X>(md.theta, fp, tp, tg);   // (ends with a barrier: the tables are staged too)
  FlowDev F{fp.blk, fp.nblk, tp, tg};
  const int n = blockIdx.x * QROWS + r;
  const bool valid = n < md.N;
  const int nc = valid ? n : md.N - 1;
  const double* rp = rowp ? rowp + (size_t)nc * md.RP : nullptr;
  const double m_ = mu[nc], vr = v[nc], vn = vr > 0.0 ? vr : 0.0, sq2 = sqrt(2.0 * vn);
  const double sig = exp(0.5 * md.log_var_noise[0]), cs = c / sig;
  constexpr int NB = 4;
  double sv = 0.0, sm = 0.0, sx = 0.0, mx = -INFINITY;   // value, mu- and v-sums (logEI: relative to the running maximum mx)
  for (int e0 = 0; e0 < S; e0 += NB * QLPR) {
    double f[NB], der[NB];
    const double* rpn[NB];
    TGP_EACH(u, NB) {
      const int e = e0 + u * QLPR + l16, ec = e < S ? e : S - 1;
      f[u] = m_ + sq2 * xl[ec];
      rpn[u] = rp;
    }
    flow_forward_n<NB, true, X>(F, f, rpn, der);
    TGP_EACH(u, NB) {
      const int e = e0 + u * QLPR + l16, ec = e < S ? e : S - 1;
      const double w = e < S ? wl[ec] : 0.0, z = c * ((f[u] - best) / sig);   // (-(b - g) / sig: k_pred_cdf's argument, negated exactly)
      if (KIND == TGP_ACQ_LOG_EI) {
        if (w > 0.0) {
          const AcqH a = acq_h(z);
          const double term = lw[ec] + a.logh, gd = a.Phi_h * der[u];
          if (term > mx) {
            const double k = exp(mx - term);   // (the first term: exp(-inf) = 0)
            sv = sv * k + 1.0;
            sm = sm * k + gd;
            sx = sx * k + gd * xl[ec];
            mx = term;
          } else if (term > -INFINITY) {
            const double k = exp(term - mx);
            sv += k;
            sm += k * gd;
            sx += k * gd * xl[ec];
          }
        }
      } else {
        const double wd = w * (KIND == TGP_ACQ_EI ? acq_Phi(z) : Q_INV_SQRT_2PI * exp(-0.5 * z * z)) * der[u];
        sv += w * (KIND == TGP_ACQ_EI ? acq_h(z).h : acq_Phi(z));
        sm += wd;
        sx += wd * xl[ec];
      }
    }
  }
  double val, a_mu, a_v;
  const double inv = vr > 0.0 ? 1.0 / sq2 : 0.0;
  if (KIND == TGP_ACQ_LOG_EI) {
    double gmx = mx;
#pragma unroll
    for (int o = 1; o < QLPR; o <<= 1) gmx = fmax(gmx, __shfl_xor(gmx, o));
    const double k = mx > -INFINITY ? exp(mx - gmx) : 0.0;
    const double tot = row16_sum(sv * k), tm = row16_sum(sm * k), tx = row16_sum(sx * k);   // (every lane on)
    val = log(sig) + gmx + log(tot);
    a_mu = cs * (tm / tot);
    a_v = vr > 0.0 ? cs * (tx / tot) * inv : 0.0;
  } else {
    const double tot = row16_sum(sv), tm = row16_sum(sm), tx = row16_sum(sx);
    val = KIND == TGP_ACQ_EI ? sig * tot : tot;
    a_mu = (KIND == TGP_ACQ_EI ? c : cs) * tm;
    a_v = vr > 0.0 ? (KIND == TGP_ACQ_EI ? c : cs) * tx * inv : 0.0;
  }
  if (valid && l16 == 0) {
    value[n] = val;
    if (partials) {
      partials[n] = a_mu;
      partials[(size_t)md.N + n] = a_v;
    }
  }
  if (valid && grad_x) acq_chain(a_mu, a_v, dmu_dx, dv_dx, D, (size_t)n, l16, grad_x);
}

// TGP_LIK_GAUSS / the empty program: one Gaussian, sd = sqrt(max(v, 0) + sig^2), z = c (mu - b) / sd:
//   EI = sd h(z), (c Phi(z), phi(z) / (2 sd));   PI = Phi(z), (c phi(z) / sd, -z phi(z) / (2 sd^2));
//   logEI = log sd + log h(z), (c (Phi / h)(z) / sd, (phi / h)(z) / (2 sd^2));   a row with v <= 0: the v-partial is an exact zero.
// 16 lanes per row (each evaluates the closed form), so that acq_chain's stores are those of k_pred_acq.
__global__ __launch_bounds__(256) void k_acq_gauss(int N, const double* __restrict__ mu, const double* __restrict__ v,
                                                   const double* __restrict__ lvn, int kind, double best, double c,
                                                   double* __restrict__ value, double* __restrict__ partials,
                                                   const double* __restrict__ dmu_dx, const double* __restrict__ dv_dx, int D,
                                                   double* __restrict__ grad_x) {
  const int n = blockIdx.x * (256 / QLPR) + threadIdx.x / QLPR, l16 = threadIdx.x & (QLPR - 1);
  if (n >= N) return;
  const double vr = v[n], sd = sqrt(fmax(vr, 0.0) + exp(lvn[0])), z = c * (mu[n] - best) / sd;
  const double phi = Q_INV_SQRT_2PI * exp(-0.5 * z * z);
  double val, a_mu, a_v;
  if (kind == TGP_ACQ_PI) {
    val = acq_Phi(z);
    a_mu = c * phi / sd;
    a_v = -z * phi / (2.0 * sd * sd);
  } else {
    const AcqH a = acq_h(z);
    if (kind == TGP_ACQ_EI) {
      val = sd * a.h;
      a_mu = c * acq_Phi(z);
      a_v = phi / (2.0 * sd);
    } else {
      val = log(sd) + a.logh;
      a_mu = c * a.Phi_h / sd;
      a_v = a.phi_h / (2.0 * sd * sd);
    }
  }
  if (!(vr > 0.0)) a_v = 0.0;
  if (l16 == 0) {
    value[n] = val;
    if (partials) {
      partials[n] = a_mu;
      partials[(size_t)N + n] = a_v;
    }
  }
  if (grad_x) acq_chain(a_mu, a_v, dmu_dx, dv_dx, D, (size_t)n, l16, grad_x);
}

// TGP_LIK_GAUSS / the empty program: y ~ N(mu, max(v, 0) + sig^2).  Y == nullptr: quantiles t (Q,N); else cdf / sf (N).
__global__ __launch_bounds__(256) void k_quantile_gauss(int N, const double* __restrict__ mu, const double* __restrict__ v,
                                                        const double* __restrict__ lvn, const double* __restrict__ zq, int Q,
                                                        double* __restrict__ t_out, const double* __restrict__ Y,
                                                        double* __restrict__ cdf, double* __restrict__ sf) {
  const int n = blockIdx.x * 256 + threadIdx.x;
  if (n >= N) return;
  const double sd = sqrt(fmax(v[n], 0.0) + exp(lvn[0])), m_ = mu[n];
  if (Y == nullptr) {
    for (int q = 0; q < Q; ++q) t_out[(size_t)q * N + n] = m_ + zq[q] * sd;
    return;
  }
  const double z = (Y[n] - m_) / sd;
  const double small = 0.5 * erfc(fabs(z) * Q_SQRT1_2), big = 1.0 - small;
  cdf[n] = z < 0.0 ? small : big;
  if (sf) sf[n] = z < 0.0 ? big : small;
}

// Heteroscedastic Gaussian predictive (TGP_LIK_HETERO), mu, v of shape (2,N): row 0 the moments of f (through the flow), row 1
// those of the log-noise GP h; a = log_var_noise + mu2, variances <= 0 count as 0.  Per row, in standardised units:
//   m1 = sum_s wn_s g_s,   m2 = sum_s wn_s g_s^2 - m1^2 + exp(a + v2 / 2)     (the empty program: mu1 and v1 + exp(a + v2 / 2)),
//   logp = log sum_s sum_t wn_s wn_t N(y | g_s, exp(a + sqrt(2 v2) xs_t)) - log Y_std,
// the exact log density of the raw target under the S x S product rule, with its constant (double-precision pi, as Student-t).
// The row's 16 lanes sweep the S node values into LDS once (q_sweep); lane l then takes the noise nodes t = l, l + 16, ... and
// runs over all s for each, keeping its sum relative to its running maximum (as lse_push of tgp_ell.hpp); the 16 lanes' (maximum, sum)
// pairs are joined under the row's maximum, so logp is finite where every term underflows (|y - g| = 1e8 sigma: terms near
// -5e15).  Weights of 0 do not enter.  Fixed order, no atomics: same input, same bits.
// dynamic LDS: tp, tg, then wn, log wn, xs (S rounded up to even each), then QROWS node tables of q_row_stride(S)
template <bool X>
__global__ __launch_bounds__(64) void k_predict_hetero(tgp_model md, FlowProg fp, const double* __restrict__ mu,
                                                       const double* __restrict__ v, const double* __restrict__ rowp,
                                                       const double* __restrict__ Y, double Y_std, int stride,
                                                       double* __restrict__ m1o, double* __restrict__ m2o,
                                                       double* __restrict__ logp) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  double* tp = reinterpret_cast<double*>(smem_raw);
  double* tg = tp + (md.P + 2) / 2 * 2;
  double* wl = tg + (md.P + 2) / 2 * 2;
  const int lane = threadIdx.x, l16 = lane & (QLPR - 1), r = lane / QLPR, S = md.S, S2 = (S + 1) / 2 * 2;
  double* lw = wl + S2;
  double* xl = lw + S2;
  double* gs = xl + S2 + (size_t)r * stride;
  for (int s = lane; s < S; s += 64) {
    const double w = md.wn[s];
    wl[s] = w;
    lw[s] = w > 0.0 ? log(w) : -INFINITY;
    xl[s] = md.xs[s];
  }
  flow_params_lds<X>(md.theta, fp, tp, tg);   // (ends with a barrier: the three tables are staged too)
  FlowDev F{fp.blk, fp.nblk, tp, tg};
  const int n = blockIdx.x * QROWS + r;
  const bool valid = n < md.N;
  const int nc = valid ? n : md.N - 1;
  const double* rp = rowp ? rowp + (size_t)nc * md.RP : nullptr;
  const double m_ = mu[nc], v1 = v[nc] > 0.0 ? v[nc] : 0.0;
  const double v2r = v[(size_t)md.N + nc], v2 = v2r > 0.0 ? v2r : 0.0;
  const double a = md.log_var_noise[0] + mu[(size_t)md.N + nc];
  q_sweep<X>(F, md, rp, m_, v1, nullptr, 0, l16, gs);
  __syncthreads();
  if (m1o || m2o) {
    double s1 = 0.0, s2 = 0.0;
    for (int s0 = 0; s0 < S; s0 += QLPR) {
      const int s = s0 + l16, sc = s < S ? s : S - 1;
      const double w = s < S ? wl[sc] : 0.0, g = gs[sc];
      s1 += w * g;
      s2 += w * g * g;
    }
    s1 = row16_sum(s1);
    s2 = row16_sum(s2);
    const double noise = exp(a + 0.5 * v2);
    if (valid && l16 == 0) {
      if (m1o) m1o[n] = fp.nblk == 0 ? m_ : s1;
      if (m2o) m2o[n] = fp.nblk == 0 ? v1 + noise : s2 - s1 * s1 + noise;
    }
  }
  if (logp && Y) {
    const double y = Y[nc], sq2 = sqrt(2.0 * v2);
    double mx = -INFINITY, se = 0.0;
    for (int t0 = 0; t0 < S; t0 += QLPR) {
      const int t = t0 + l16;
      if (t < S && wl[t] > 0.0) {
        const double la = a + sq2 * xl[t], hiv = 0.5 * exp(-la);     // log variance at noise node t, 1 / (2 variance)
        const double base = lw[t] - 0.5 * (1.8378770664093454836 + la);
        for (int s = 0; s < S; ++s) {
          const double rr = y - gs[s], term = base + lw[s] - hiv * rr * rr;
          if (term > mx) { se = se * exp(mx - term) + 1.0; mx = term; }
          else if (term > -INFINITY) se += exp(term - mx);
        }
      }
    }
    double gmx = mx;
#pragma unroll
    for (int o = 1; o < QLPR; o <<= 1) gmx = fmax(gmx, __shfl_xor(gmx, o));
    const double tot = row16_sum(mx > -INFINITY ? se * exp(mx - gmx) : 0.0);
    if (valid && l16 == 0) logp[n] = gmx + log(tot) - log(Y_std);
  }
}

// Continuous ranked probability score of the predictive at Y (tgp_predict_crps_f64), CRPS_n = T1 - T2 in standardised units:
//   a(z) = z erf(z / sqrt 2) + sqrt(2 / pi) exp(-z^2 / 2)                            (even, >= |z|; = |z| once the exponential is 0)
//   T1 = sig sum_s wn_s a((y - g_s) / sig)                                           = E|Y - y|
//   T2 = sig / sqrt(pi) sum_s wn_s^2 + sqrt(2) sig sum_{s<t} wn_s wn_t a((g_s - g_t) / (sqrt(2) sig))   = E|Y - Y'| / 2
// evaluated as written with the caller's wn (nothing is renormalised); every term is positive.  A row with v <= 0 counts as
// v = 0: its nodes coincide and the sums give sig (a((y - G(mu)) / sig) - (sum wn)^2 / sqrt(pi)) with no special case.
// ORDER.  The row's 16 lanes sweep the S node values into LDS once (q_sweep).  T1 and sum wn^2: lane l adds the nodes
// l, l + 16, ... in that order (as q_eval), row16_sum joins the 16 partials.  The S (S - 1) / 2 unordered pairs are numbered by
// cyclic offset: pair k = 0 .. S (S - 1) / 2 - 1 is (s, t) = (k mod S, (k mod S + k div S + 1) mod S) -- offsets 1 .. (S - 1) / 2
// over every s, and for even S the first S / 2 pairs of offset S / 2; each pair once.  With CRPS_WAVES waves per workgroup
// (all on the same QROWS rows), lane l of wave w adds the pairs k = 16 w + l + 16 CRPS_WAVES j, j = 0, 1, ... in that order,
// row16_sum joins a wave's 16 partials, and the waves' sums are added in the order w = 0, 1, ... from LDS.  CRPS_WAVES is a
// constant of the build -- never a function of N -- so a row's bits depend on that row's inputs only.  No float atomics.
// The loops are uniform over the workgroup (a lane past the last pair adds a weight of 0).
// dynamic LDS: tp, tg, wn as k_pred_cdf, QROWS node tables of q_row_stride(S), then CRPS_WAVES x QROWS wave sums
#ifndef TGP_CRPS_WAVES
#define TGP_CRPS_WAVES 4
#endif
#define CRPS_WAVES TGP_CRPS_WAVES
#define Q_SQRT_2_OVER_PI 0.79788456080286535588
#define Q_INV_SQRT_PI 0.56418958354775628695
#define Q_SQRT2 1.41421356237309504880

__device__ __forceinline__ double crps_a(double z) { return z * erf(z * Q_SQRT1_2) + Q_SQRT_2_OVER_PI * exp(-0.5 * z * z); }

template <bool X, int W>
__global__ __launch_bounds__(64 * W) void k_pred_crps(tgp_model md, FlowProg fp, const double* __restrict__ mu,
                                                      const double* __restrict__ v, const double* __restrict__ rowp,
                                                      const double* __restrict__ Y, int stride, double* __restrict__ crps,
                                                      double* __restrict__ parts) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  double* tp = reinterpret_cast<double*>(smem_raw);
  double* tg = tp + (md.P + 2) / 2 * 2;
  double* wl = tg + (md.P + 2) / 2 * 2;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, l16 = lane & (QLPR - 1), r = lane / QLPR, S = md.S;
  double* gs = wl + (S + 1) / 2 * 2 + (size_t)r * stride;
  double* red = wl + (S + 1) / 2 * 2 + (size_t)QROWS * stride;
  for (int s = tid; s < S; s += 64 * W) wl[s] = md.wn[s];
  flow_params_lds<X>(md.theta, fp, tp, tg);   // (ends with a barrier: wl is staged too)
  FlowDev F{fp.blk, fp.nblk, tp, tg};
  const int n = blockIdx.x * QROWS + r;
  const bool valid = n < md.N;
  const int nc = valid ? n : md.N - 1;
  const double* rp = rowp ? rowp + (size_t)nc * md.RP : nullptr;
  const double vr = v[nc], vn = vr > 0.0 ? vr : 0.0;
  const double sig = sqrt(exp(md.log_var_noise[0]));
  if (wv == 0) q_sweep<X>(F, md, rp, mu[nc], vn, nullptr, 0, l16, gs);
  __syncthreads();
  // ---- the pairs, dealt over the W waves
  const int npair = S * (S - 1) / 2;
  const double sig2 = Q_SQRT2 * sig;
  double pr = 0.0;
  {
    int k = wv * QLPR + l16, d = k / S, s = k - d * S;       // pair k: offset d + 1 from node s
    for (int k0 = 0; k0 < npair; k0 += QLPR * W) {
      const bool in = k < npair;
      int t = s + d + 1;
      if (t >= S) t -= S;
      const int sc = in ? s : 0, tc = in ? t : 0;
      const double w = in ? wl[sc] * wl[tc] : 0.0;
      pr += w * crps_a((gs[sc] - gs[tc]) / sig2);
      k += QLPR * W;
      s += QLPR * W;
      while (s >= S) { s -= S; ++d; }
    }
  }
  pr = row16_sum(pr);
  if constexpr (W > 1) {
    if (l16 == 0) red[wv * QROWS + r] = pr;
    __syncthreads();
    if (wv != 0) return;
    pr = red[r];
    for (int w = 1; w < W; ++w) pr += red[w * QROWS + r];
  }
  // ---- T1 and the diagonal of T2: one pass over the nodes
  const double y = Y[nc];
  double t1 = 0.0, w2 = 0.0;
  for (int s0 = 0; s0 < S; s0 += QLPR) {
    const int s = s0 + l16, sc = s < S ? s : S - 1;
    const double w = s < S ? wl[sc] : 0.0;
    t1 += w * crps_a((y - gs[sc]) / sig);
    w2 += w * w;
  }
  t1 = row16_sum(t1);
  w2 = row16_sum(w2);
  if (valid && l16 == 0) {
    const double T1 = sig * t1, T2 = sig * Q_INV_SQRT_PI * w2 + sig2 * pr;
    crps[n] = T1 - T2;
    if (parts) {
      parts[n] = T1;
      parts[(size_t)md.N + n] = T2;
    }
  }
}

// TGP_LIK_GAUSS / the empty program: one Gaussian of sd^2 = max(v, 0) + sig^2, z = (y - mu) / sd:
// T1 = sd a(z), T2 = sd / sqrt(pi), CRPS = T1 - T2 = sd (a(z) - 1 / sqrt(pi)).
__global__ __launch_bounds__(256) void k_crps_gauss(int N, const double* __restrict__ mu, const double* __restrict__ v,
                                                    const double* __restrict__ lvn, const double* __restrict__ Y,
                                                    double* __restrict__ crps, double* __restrict__ parts) {
  const int n = blockIdx.x * 256 + threadIdx.x;
  if (n >= N) return;
  const double sd = sqrt(fmax(v[n], 0.0) + exp(lvn[0]));
  const double T1 = sd * crps_a((Y[n] - mu[n]) / sd), T2 = sd * Q_INV_SQRT_PI;
  crps[n] = T1 - T2;
  if (parts) {
    parts[n] = T1;
    parts[(size_t)N + n] = T2;
  }
}

// ---------------------------------------------------------------------------------------------------
// host launchers
// ---------------------------------------------------------------------------------------------------
int launch_predict_hetero(const tgp_model& md, const FlowProg& fp, const double* mu, const double* v, const double* rowp,
                          const double* Y, double Y_std, double* m1, double* m2, double* logp, hipStream_t st) {
  const int stride = q_row_stride(md.S);
  const size_t lds = (2 * (size_t)((md.P + 2) / 2 * 2) + 3 * (size_t)((md.S + 1) / 2 * 2) + (size_t)QROWS * stride) * sizeof(double);
  const bool ext = flow_prog_extended(fp.blk, fp.nblk);
  static size_t cur[2] = {48 * 1024, 48 * 1024};
  auto* const kern = ext ? k_predict_hetero<true> : k_predict_hetero<false>;
  if (int rc = ensure_lds(reinterpret_cast<const void*>(kern), lds, &cur[ext])) return rc;
  hipLaunchKernelGGL(kern, dim3((md.N + QROWS - 1) / QROWS), dim3(64), lds, st, md, fp, mu, v, rowp, Y, Y_std, stride, m1, m2, logp);
  LAUNCH_CHECK();
  return 0;
}

static size_t q_lds_bytes(const tgp_model& md, int Q, int* stride, int cols = 1) {
  *stride = q_row_stride(cols * md.S + Q);
  return (2 * (size_t)((md.P + 2) / 2 * 2) + (size_t)((md.S + 1) / 2 * 2) + (size_t)QROWS * *stride) * sizeof(double);
}

int launch_predict_quantile(const tgp_model& md, const FlowProg& fp, const double* mu, const double* v, const double* rowp,
                            const double* probs, const double* zq, int Q, double* t, int32_t* status, hipStream_t st) {
  // TGP_LIK_GAMMA, TGP_LIK_BETA: no Gaussian shortcut, the empty program runs the kernel on g_s = mu + sqrt(2 v) xs_s
  const int comp = md.lik == TGP_LIK_GAMMA ? 1 : md.lik == TGP_LIK_BETA ? 2 : 0;
  if (!comp && (md.lik == TGP_LIK_GAUSS || fp.nblk == 0)) {
    hipLaunchKernelGGL(k_quantile_gauss, dim3((md.N + 255) / 256), dim3(256), 0, st, md.N, mu, v, md.log_var_noise, zq, Q, t,
                       (const double*)nullptr, (double*)nullptr, (double*)nullptr);
    LAUNCH_CHECK();
    return 0;
  }
  int stride = 0;
  const size_t lds = q_lds_bytes(md, Q, &stride, comp == 2 ? QBeta::kCols : 1);
  const bool ext = flow_prog_extended(fp.blk, fp.nblk);
  static size_t cur[6] = {48 * 1024, 48 * 1024, 48 * 1024, 48 * 1024, 48 * 1024, 48 * 1024};
  auto* const kern = comp == 2   ? (ext ? k_pred_quantile<QBeta, true> : k_pred_quantile<QBeta, false>)
                     : comp == 1 ? (ext ? k_pred_quantile<QGamma, true> : k_pred_quantile<QGamma, false>)
                                 : (ext ? k_pred_quantile<QGauss, true> : k_pred_quantile<QGauss, false>);
  if (int rc = ensure_lds(reinterpret_cast<const void*>(kern), lds, &cur[2 * comp + ext])) return rc;
  hipLaunchKernelGGL(kern, dim3((md.N + QROWS - 1) / QROWS), dim3(64), lds, st, md, fp, mu, v, rowp, probs, zq, Q, stride, t,
                     status);
  LAUNCH_CHECK();
  return 0;
}

int launch_predict_cdf(const tgp_model& md, const FlowProg& fp, const double* mu, const double* v, const double* rowp,
                       const double* Y, double* cdf, double* sf, hipStream_t st) {
  const int comp = md.lik == TGP_LIK_GAMMA ? 1 : md.lik == TGP_LIK_BETA ? 2 : 0;
  if (!comp && (md.lik == TGP_LIK_GAUSS || fp.nblk == 0)) {
    hipLaunchKernelGGL(k_quantile_gauss, dim3((md.N + 255) / 256), dim3(256), 0, st, md.N, mu, v, md.log_var_noise,
                       (const double*)nullptr, 0, (double*)nullptr, Y, cdf, sf);
    LAUNCH_CHECK();
    return 0;
  }
  int stride = 0;
  const size_t lds = q_lds_bytes(md, 0, &stride, comp == 2 ? QBeta::kCols : 1);
  const bool ext = flow_prog_extended(fp.blk, fp.nblk);
  static size_t cur[6] = {48 * 1024, 48 * 1024, 48 * 1024, 48 * 1024, 48 * 1024, 48 * 1024};
  auto* const kern = comp == 2   ? (ext ? k_pred_cdf<QBeta, true> : k_pred_cdf<QBeta, false>)
                     : comp == 1 ? (ext ? k_pred_cdf<QGamma, true> : k_pred_cdf<QGamma, false>)
                                 : (ext ? k_pred_cdf<QGauss, true> : k_pred_cdf<QGauss, false>);
  if (int rc = ensure_lds(reinterpret_cast<const void*>(kern), lds, &cur[2 * comp + ext])) return rc;
  hipLaunchKernelGGL(kern, dim3((md.N + QROWS - 1) / QROWS), dim3(64), lds, st, md, fp, mu, v, rowp, Y, stride, cdf, sf);
  LAUNCH_CHECK();
  return 0;
}

int launch_predict_moment_grads(const tgp_model& md, const FlowProg& fp, const double* mu, const double* v, const double* rowp,
                                double* dm1, double* dm2, hipStream_t st) {
  if (md.lik == TGP_LIK_GAUSS || fp.nblk == 0) {
    hipLaunchKernelGGL(k_mgrad_gauss, dim3((md.N + 255) / 256), dim3(256), 0, st, md.N, v, dm1, dm2);
    LAUNCH_CHECK();
    return 0;
  }
  const size_t lds = (2 * (size_t)((md.P + 2) / 2 * 2) + 2 * (size_t)((md.S + 1) / 2 * 2)) * sizeof(double);
  const bool ext = flow_prog_extended(fp.blk, fp.nblk);
  static size_t cur[2] = {48 * 1024, 48 * 1024};
  auto* const kern = ext ? k_pred_mgrad<true> : k_pred_mgrad<false>;
  if (int rc = ensure_lds(reinterpret_cast<const void*>(kern), lds, &cur[ext])) return rc;
  hipLaunchKernelGGL(kern, dim3((md.N + QROWS - 1) / QROWS), dim3(64), lds, st, md, fp, mu, v, rowp, dm1, dm2);
  LAUNCH_CHECK();
  return 0;
}

int launch_predict_acquisition(const tgp_model& md, const FlowProg& fp, const double* mu, const double* v, const double* rowp,
                               int kind, double best, double c, double* value, double* partials, const double* dmu_dx,
                               const double* dv_dx, int D, double* grad_x, hipStream_t st) {
  if (md.lik == TGP_LIK_GAUSS || fp.nblk == 0) {
    constexpr int rows = 256 / QLPR;
    hipLaunchKernelGGL(k_acq_gauss, dim3((md.N + rows - 1) / rows), dim3(256), 0, st, md.N, mu, v, md.log_var_noise, kind, best, c,
                       value, partials, dmu_dx, dv_dx, D, grad_x);
    LAUNCH_CHECK();
    return 0;
  }
  const size_t lds = (2 * (size_t)((md.P + 2) / 2 * 2) + (kind == TGP_ACQ_LOG_EI ? 3 : 2) * (size_t)((md.S + 1) / 2 * 2)) * sizeof(double);
  const bool ext = flow_prog_extended(fp.blk, fp.nblk);
  static size_t cur[6] = {48 * 1024, 48 * 1024, 48 * 1024, 48 * 1024, 48 * 1024, 48 * 1024};
  auto* const kern = kind == TGP_ACQ_EI       ? (ext ? k_pred_acq<TGP_ACQ_EI, true> : k_pred_acq<TGP_ACQ_EI, false>)
                     : kind == TGP_ACQ_LOG_EI ? (ext ? k_pred_acq<TGP_ACQ_LOG_EI, true> : k_pred_acq<TGP_ACQ_LOG_EI, false>)
                                              : (ext ? k_pred_acq<TGP_ACQ_PI, true> : k_pred_acq<TGP_ACQ_PI, false>);
  if (int rc = ensure_lds(reinterpret_cast<const void*>(kern), lds, &cur[2 * kind + ext])) return rc;
  hipLaunchKernelGGL(kern, dim3((md.N + QROWS - 1) / QROWS), dim3(64), lds, st, md, fp, mu, v, rowp, best, c, value, partials,
                     dmu_dx, dv_dx, D, grad_x);
  LAUNCH_CHECK();
  return 0;
}

int launch_predict_crps(const tgp_model& md, const FlowProg& fp, const double* mu, const double* v, const double* rowp,
                        const double* Y, double* crps, double* parts, hipStream_t st) {
  if (md.lik == TGP_LIK_GAUSS || fp.nblk == 0) {
    hipLaunchKernelGGL(k_crps_gauss, dim3((md.N + 255) / 256), dim3(256), 0, st, md.N, mu, v, md.log_var_noise, Y, crps, parts);
    LAUNCH_CHECK();
    return 0;
  }
  int stride = 0;
  const size_t lds = q_lds_bytes(md, 0, &stride) + (size_t)CRPS_WAVES * QROWS * sizeof(double);
  const bool ext = flow_prog_extended(fp.blk, fp.nblk);
  static size_t cur[2] = {48 * 1024, 48 * 1024};
  auto* const kern = ext ? k_pred_crps<true, CRPS_WAVES> : k_pred_crps<false, CRPS_WAVES>;
  if (int rc = ensure_lds(reinterpret_cast<const void*>(kern), lds, &cur[ext])) return rc;
  hipLaunchKernelGGL(kern, dim3((md.N + QROWS - 1) / QROWS), dim3(64 * CRPS_WAVES), lds, st, md, fp, mu, v, rowp, Y, stride, crps,
                     parts);
  LAUNCH_CHECK();
  return 0;
}

}  // namespace tgp
