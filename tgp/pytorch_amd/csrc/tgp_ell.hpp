// tgp_ell.hpp -- the quadrature likelihood through the flow as templates over a likelihood policy: the training policies and
// k_ell_quad, the predictive policies and k_predict_quad, each with its launch helper.  tgp_lik.hip instantiates them for the
// Gaussian, Bernoulli, Poisson, Student-t and heteroscedastic policies and holds the table of likelihoods (lik_row),
// tgp_lik_negbin.hip instantiates them for the negative-binomial policy and tgp_lik_ordinal.hip for the ordinal policies
// (EllOrdinal, PredOrdinal), tgp_lik_gamma.hip for the Gamma policies (EllGamma, PredGamma) and tgp_lik_beta.hip for the Beta
// policies (EllBeta, PredBeta), each in a unit of its own for the compile time.
#pragma once
#include <type_traits>
#include "tgp_dev.hpp"
#include "tgp_launch.hpp"

namespace tgp {

// ---------------------------------------------------------------------------------------------------
// Quadrature likelihoods through the flow with gradients, E_q(f0)[log p(y | G(f0))] by Gauss-Hermite:
//   Gaussian  (likelihoods/GaussianNonLinearMean.py:64-150)
//   Bernoulli (likelihoods/Bernoulli.py), probit link: log p(y | g) = y log Phi(g) + (1 - y) log Phi(-g)
//   Poisson   (no counterpart in the reference), log link: log p(y | g) = y g - exp(g) - lgamma(y + 1)
//   Student-t (no counterpart in the reference), location G(f0), scale sigma, nu degrees of freedom (TGP_LIK_STUDENT)
//   negative binomial (no counterpart in the reference), log link, dispersion r: mean exp(g), variance mean + mean^2 / r (TGP_LIK_NEGBIN)
//   heteroscedastic Gaussian (no counterpart in the reference), log noise variance c + h, h a second latent GP (TGP_LIK_HETERO)
//   ordinal (no counterpart in the reference), cumulative probit over K ordered classes with fixed bin edges b_1 < .. < b_{K-1}:
//     log p(y | g) = log(Phi((b_{y+1} - g) / sigma) - Phi((b_y - g) / sigma)); the flow learns the spacing of the levels
//     (TGP_LIK_ORDINAL, tgp_lik_ordinal.hip)
//   Gamma (no counterpart in the reference), log link, shape a: mean exp(g), variance exp(2 g) / a (TGP_LIK_GAMMA, tgp_lik_gamma.hip)
//   Beta (no counterpart in the reference), logit link, precision phi: mean mu = sigmoid(g), variance mu (1 - mu) / (1 + phi)
//     (TGP_LIK_BETA, tgp_lik_beta.hip)
// ---------------------------------------------------------------------------------------------------

// The node term shared by k_ell_quad<EllBern> and PredBern.  With a = |g|, t = a / sqrt 2:
//   Phi(-a) = erfc(t) / 2 = erfcx(t) exp(-a^2 / 2) / 2      log Phi(-a) = log(erfcx(t) / 2) - a^2 / 2
//   Phi(a)  = 1 - erfc(t) / 2                                log Phi(a)  = log1p(-erfc(t) / 2)
//   lambda(z) = phi(z) / Phi(z):  lambda(-a) = sqrt(2 / pi) / erfcx(t),  lambda(a) = phi(a) / Phi(a)
// Every quantity stays finite and accurate however large |g| is (the reference forms Phi first: its BCELoss clamps the log
// at -100 once |g| passes ~8).  lp = y log Phi(g) + (1 - y) log Phi(-g), dg = d lp / dg = y lambda(g) - (1 - y) lambda(-g);
// pp / pm (optional) = Phi(g) / Phi(-g).
struct BernNode { double lp, dg, pp, pm; };
__device__ inline BernNode bern_node(double g, double y) {
  const double a = fabs(g), t = a * 0.70710678118654752440;
  const double ec = erfc(t), ex = erfcx(t);
  const double phia = 0.39894228040143267794 * exp(-0.5 * a * a);   // phi(a)
  const double lp_hi = log1p(-0.5 * ec);                              // log Phi(a)
  const double lp_lo = log(0.5 * ex) - 0.5 * a * a;                   // log Phi(-a)
  const double lam_hi = phia / (1.0 - 0.5 * ec);                      // lambda(a)
  const double lam_lo = 0.79788456080286535588 / ex;                  // lambda(-a)
  const bool pos = g >= 0.0;
  BernNode r;
  r.lp = y * (pos ? lp_hi : lp_lo) + (1.0 - y) * (pos ? lp_lo : lp_hi);
  r.dg = y * (pos ? lam_hi : lam_lo) - (1.0 - y) * (pos ? lam_lo : lam_hi);
  r.pp = pos ? 1.0 - 0.5 * ec : 0.5 * ec;
  r.pm = pos ? 0.5 * ec : 1.0 - 0.5 * ec;
  return r;
}

// What a likelihood supplies to k_ell_quad.  Once per launch: consts(log_var_noise) = its launch constants K (a struct of its
// own: the noise pair, nothing, or StudentConst).  Per quadrature node with g = G(f0): at(g, y, K) = whatever the three
// terms share, then
//   log_p = log p(y | g),  dlog_p_deta = its derivative in eta = log_var_noise[0] (kNoise only),
//   adjoint = scale w d log p / dg for the node's normalised weight w, which starts the reverse sweep.
// log_var_noise is read only where kNoise is set.
// kRowTerm: log p has a part that depends on y alone, row_term(y), which the kernel adds once per row instead of once per node.
// kRowNoise (with kRowTerm and kNoise): that part depends on the launch constants too -- row_term(y, K) -- and so does its
// derivative in eta, row_deta(y, K), which a row adds once to the noise adjoint (partial slot 1) beside its nodes' dlog_p_deta.
// The count policies (EllPois, EllNegBin) also serve the predictive policy PredCount: rate(t) = exp(g) of a node, and kOverDisp
// says whether the conditional variance exceeds the mean, by mean^2 excess(K); plus_log_p(a, t, K) = a + log_p(t, K), a the log
// weight of the node.
// kBlockTerm: log p has a part that is the same for every row and node, block_term(K), which the kernel adds once per
// workgroup, times its number of rows (the weights of a row sum to 1).
// kRowConst: the constants differ from row to row.  mu, v, g_mu, g_v are then (2,N): row 1 holds the moments of a second latent
// GP, from which row_consts(K, mu2, v2) makes the row's own K; per node row_acc(t, w) is summed over the row's nodes into A, and
// row_mu_bar(A, K), row_v_bar(A, K) are d log p / d mu2, d log p / d v2 of the row, written (times scale) to row 1 of g_mu, g_v.
struct EllNoise { double eta, einv; };    // eta = log noise variance, einv = exp(-eta)
struct EllNone {};
struct EllGauss {
  static constexpr bool kNoise = true;    // partial slot 1 carries the noise adjoint
  static constexpr bool kClampV = false;
  static constexpr bool kRowTerm = false;
  static constexpr bool kRowNoise = false;
  static constexpr bool kBlockTerm = false;
  static constexpr bool kRowConst = false;
  static __device__ __forceinline__ EllNoise consts(const double* lvn) { return {lvn[0], exp(-lvn[0])}; }
  static __device__ __forceinline__ double at(double g, double y, const EllNoise&) { return y - g; }   // the residual
  static __device__ __forceinline__ double log_p(double r, const EllNoise& k) {
    return -0.5 * TGP_LOG_2PI_REF - 0.5 * k.eta - 0.5 * k.einv * r * r;
  }
  static __device__ __forceinline__ double dlog_p_deta(double r, const EllNoise& k) { return -0.5 + 0.5 * k.einv * r * r; }
  static __device__ __forceinline__ double adjoint(double r, double scale, double w, const EllNoise& k) {
    return scale * k.einv * w * r;
  }
};
struct EllBern {
  static constexpr bool kNoise = false;   // no noise parameter: partial slot 1 is 0
  // q(f) variances below 0 count as 0 (Bernoulli.py: gauss_cov[gauss_cov < 0] = 0), where the adjoint of v is 0
  static constexpr bool kClampV = true;
  static constexpr bool kRowTerm = false;
  static constexpr bool kRowNoise = false;
  static constexpr bool kBlockTerm = false;
  static constexpr bool kRowConst = false;
  static __device__ __forceinline__ EllNone consts(const double*) { return {}; }
  static __device__ __forceinline__ BernNode at(double g, double y, const EllNone&) { return bern_node(g, y); }
  static __device__ __forceinline__ double log_p(const BernNode& b, const EllNone&) { return b.lp; }
  static __device__ __forceinline__ double adjoint(const BernNode& b, double scale, double w, const EllNone&) {
    return scale * w * b.dg;
  }
};
// Poisson counts, the flow as the log-rate: log p(y | g) = y g - exp(g) - lgamma(y + 1), d log p / dg = y - exp(g).  g is not
// clamped: a node whose exp overflows gives -inf, as the float64 formula does.  The exponential is taken once per node and
// shared by the value and the adjoint; lgamma once per row (row_term).
struct PoisNode { double g, e, y; };
struct EllPois {
  static constexpr bool kNoise = false;   // no noise parameter: partial slot 1 is 0
  static constexpr bool kClampV = true;   // as EllBern
  static constexpr bool kRowTerm = true;
  static constexpr bool kRowNoise = false;
  static constexpr bool kBlockTerm = false;
  static constexpr bool kRowConst = false;
  static constexpr bool kOverDisp = false;   // PredCount: Var[y | rate] = rate
  static __device__ __forceinline__ EllNone consts(const double*) { return {}; }
  static __device__ __forceinline__ PoisNode at(double g, double y, const EllNone&) { return {g, exp(g), y}; }
  static __device__ __forceinline__ double log_p(const PoisNode& t, const EllNone&) { return t.y * t.g - t.e; }
  static __device__ __forceinline__ double adjoint(const PoisNode& t, double scale, double w, const EllNone&) {
    return scale * w * (t.y - t.e);
  }
  static __device__ __forceinline__ double row_term(double y) { return -lgamma(y + 1.0); }
  static __device__ __forceinline__ double rate(const PoisNode& t) { return t.e; }   // PredCount: exp(g)
  // a + log_p, in the order the predictive has always summed it
  static __device__ __forceinline__ double plus_log_p(double a, const PoisNode& t, const EllNone&) { return a + t.y * t.g - t.e; }
};
// Student-t noise of scale sigma around the flow, nu degrees of freedom (TGP_LIK_STUDENT): log_var_noise = {eta = log sigma^2,
// nu}.  With r = y - g and q = nu sigma^2 + r^2:
//   log p(y | g) = c(nu, eta) - (nu + 1) / 2 log1p(r^2 / (nu sigma^2)),  c = lgamma((nu + 1) / 2) - lgamma(nu / 2) - log(nu pi) / 2 - eta / 2
//   d log p / dg = (nu + 1) r / q,   d log p / d eta = -1/2 + (nu + 1) r^2 / (2 q).
// g is not clamped.  One division per node, h = (nu + 1) / q, shared by both derivatives; 1 / (nu sigma^2) once per launch; c,
// with its two lgamma, once per workgroup (block_term), by one lane.  |r| = 10^8 sigma: r^2 / (nu sigma^2) ~ 10^16, nothing
// overflows.
struct StudentConst { double eta, nu, nu1, nus2, inus2; };   // nu1 = nu + 1, nus2 = nu sigma^2, inus2 = 1 / nus2
struct StudentNode { double r, r2, h; };                     // h = (nu + 1) / (nu sigma^2 + r^2)
__device__ inline double student_log_const(double nu, double eta) {
  return lgamma(0.5 * (nu + 1.0)) - lgamma(0.5 * nu) - 0.5 * log(nu * 3.14159265358979323846) - 0.5 * eta;
}
struct EllStudent {
  static constexpr bool kNoise = true;    // partial slot 1 carries the adjoint of eta (nu is not trained)
  static constexpr bool kClampV = true;   // as EllBern
  static constexpr bool kRowTerm = false;
  static constexpr bool kRowNoise = false;
  static constexpr bool kBlockTerm = true;
  static constexpr bool kRowConst = false;
  static __device__ __forceinline__ StudentConst consts(const double* lvn) {
    const double eta = lvn[0], nu = lvn[1], nus2 = nu * exp(eta);
    return {eta, nu, nu + 1.0, nus2, 1.0 / nus2};
  }
  static __device__ __forceinline__ StudentNode at(double g, double y, const StudentConst& k) {
    const double r = y - g, r2 = r * r;
    return {r, r2, k.nu1 / (k.nus2 + r2)};
  }
  static __device__ __forceinline__ double log_p(const StudentNode& t, const StudentConst& k) {
    return -0.5 * k.nu1 * log1p(t.r2 * k.inus2);
  }
  static __device__ __forceinline__ double dlog_p_deta(const StudentNode& t, const StudentConst&) { return -0.5 + 0.5 * t.h * t.r2; }
  static __device__ __forceinline__ double adjoint(const StudentNode& t, double scale, double w, const StudentConst&) {
    return scale * w * t.h * t.r;
  }
  static __device__ __forceinline__ double block_term(const StudentConst& k) { return student_log_const(k.nu, k.eta); }
};
// Heteroscedastic Gaussian noise around the flow (TGP_LIK_HETERO): y ~ N(G(f), exp(c + h)), c = log_var_noise[0], h a second latent
// GP with q(h_n) = N(mu2_n, v2_n) independent of q(f_n).  h integrates out in closed form: with a = c + mu2 and
// p = E_q[exp(-(c + h))] = exp(-a + v2 / 2),
//   E_q(h)[log N(y | g, e^(c+h))] = -log(2 pi) / 2 - a / 2 - p r^2 / 2,      r = y - g,
// which is EllGauss's node term at the row's own pair (eta, einv) = (a, p): the node functions are EllGauss's.  With
// A = sum_s w_s r_s^2:  d/dmu2 = -1/2 + p A / 2,  d/dv2 = -p A / 4,  d/dc = sum_n d/dmu2_n (partial slot 1, as the noise adjoint).
// v2 <= 0 counts as 0 and its adjoint is 0 (as for v1); p is not clamped: the float64 formula.
struct HeteroRow : EllNoise { bool v2pos; };
struct EllHetero {
  static constexpr bool kNoise = true;    // partial slot 1 carries the adjoint of c
  static constexpr bool kClampV = true;   // as EllBern
  static constexpr bool kRowTerm = false;
  static constexpr bool kRowNoise = false;
  static constexpr bool kBlockTerm = false;
  static constexpr bool kRowConst = true;
  static __device__ __forceinline__ double consts(const double* lvn) { return lvn[0]; }
  static __device__ __forceinline__ HeteroRow row_consts(double c, double mu2, double v2) {
    const bool pos = v2 > 0.0;
    const double a = c + mu2;
    HeteroRow k;
    k.eta = a; k.einv = exp(-a + (pos ? 0.5 * v2 : 0.0)); k.v2pos = pos;
    return k;
  }
  static __device__ __forceinline__ double at(double g, double y, const HeteroRow&) { return y - g; }
  static __device__ __forceinline__ double log_p(double r, const HeteroRow& k) { return EllGauss::log_p(r, k); }
  static __device__ __forceinline__ double dlog_p_deta(double r, const HeteroRow& k) { return EllGauss::dlog_p_deta(r, k); }
  static __device__ __forceinline__ double adjoint(double r, double scale, double w, const HeteroRow& k) {
    return EllGauss::adjoint(r, scale, w, k);
  }
  static __device__ __forceinline__ double row_acc(double r, double w) { return w * r * r; }
  static __device__ __forceinline__ double row_mu_bar(double A, const HeteroRow& k) { return -0.5 + 0.5 * k.einv * A; }
  static __device__ __forceinline__ double row_v_bar(double A, const HeteroRow& k) { return k.v2pos ? -0.25 * k.einv * A : 0.0; }
};
// the constants of data row nc: the launch constants, or what the policy makes of them and the row's second pair of moments
template <class Lik, class K0>
__device__ __forceinline__ auto ell_row_consts(const K0& k0, const double* __restrict__ mu, const double* __restrict__ v, int N, int nc) {
  if constexpr (Lik::kRowConst) return Lik::row_consts(k0, mu[(size_t)N + nc], v[(size_t)N + nc]);
  else return k0;
}

// LPR lanes share a data row (64 / LPR rows per wave: row = lane % RW, node group = lane / RW), NB nodes in flight per
// lane.  The launcher picks LPR from N so that a chunk of ~16k rows still yields ~1000 workgroups.
// NBX = NB | TGP_FLOWX or TGP_FLOWX2: the flow sweeps know the extended kind set (X; see k_rows)
template <class Lik, int LPR, int NBX>
__global__ __launch_bounds__(256) void k_ell_quad(tgp_model md, FlowProg fp, const double* __restrict__ Y,
                                                   const double* __restrict__ mu, const double* __restrict__ v,
                                                   const double* __restrict__ rowp, double* __restrict__ part,
                                                   double* __restrict__ g_mu, double* __restrict__ g_v,
                                                   double* __restrict__ g_rowp) {
  constexpr int NB = NBX & (TGP_FLOWX - 1);
  constexpr int X = TGP_XK_OF(NBX);
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  double* sm = reinterpret_cast<double*>(smem_raw);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, P = md.P, RP = md.RP;
  const int nb = fp.nblk > 0 ? fp.nblk : 1;
  constexpr int RW = 64 / LPR;                              // rows per wave
  double* stack = sm;                                       // nblk * NB * 256: block inputs (checkpoint mode)
  double* accw = stack + (size_t)nb * NB * 256;             // 4 waves x P: per-wave shared-parameter accumulators
  double* accr = accw + (size_t)4 * (P > 0 ? P : 1);        // RP * 256 (per-row parameters, lane-private)
  double* red = accr + (size_t)RP * 256;                    // 16
  double* tp = red + 16;                                    // P+2
  double* tg = tp + (P + 2) / 2 * 2;                        // P+2
  double* ti = tg + (P + 2) / 2 * 2;                        // P+2: reciprocals (flow_rcp_param)
  for (int i = tid; i < 4 * (P > 0 ? P : 1) + RP * 256; i += 256) accw[i] = 0.0;
  flow_params_lds<X>(md.theta, fp, tp, tg, ti);
  // lane group q takes the quadrature nodes s = q + LPR (NB j + u).  Every lane runs the same trip count (wave-wide
  // sums inside the reverse sweep); nodes past S and padding rows carry weight 0.
  const int qn = lane / RW;
  const int n = blockIdx.x * (4 * RW) + wave * RW + (lane % RW);
  auto group_sum = [&](double x) {   // over the LPR lanes of a row: lanes differing in the bits above log2(RW)
#pragma unroll
    for (int o = RW; o < 64; o <<= 1) x += __shfl_xor(x, o);
    return x;
  };
  const bool valid = n < md.N;
  const int nc = valid ? n : md.N - 1;
  const auto K = ell_row_consts<Lik>(Lik::consts(md.log_var_noise), mu, v, md.N, nc);
  FlowDev F{fp.blk, fp.nblk, tp, tg, ti};
  double ellp = 0.0, etap = 0.0, cm = 0.0, cv = 0.0;
  [[maybe_unused]] double racc = 0.0;   // kRowConst: this lane's part of the row's A
  const double m_ = mu[nc], vn = Lik::kClampV ? (v[nc] > 0.0 ? v[nc] : 0.0) : v[nc];
  const double sq = sqrt(2.0 * vn), y = Y[nc];
  const double* rp = rowp ? rowp + (size_t)nc * RP : nullptr;
  double* aw = accw + (size_t)wave * (P > 0 ? P : 1);
  for (int s0 = 0; s0 < md.S; s0 += LPR * NB) {
    double f[NB], c[NB], xsn[NB], wsn[NB];
#pragma unroll
    for (int u = 0; u < NB; ++u) {
      const int s = s0 + LPR * u + qn, sc = s < md.S ? s : md.S - 1;
      xsn[u] = md.xs[sc];
      wsn[u] = (valid && s < md.S) ? md.wn[sc] : 0.0;
      f[u] = m_ + sq * xsn[u];
    }
    flow_forward_ckpt<NB, X>(F, f, rp, stack + tid, 256);
#pragma unroll
    for (int u = 0; u < NB; ++u) {
      const auto t = Lik::at(f[u], y, K);
      ellp += wsn[u] * Lik::log_p(t, K);
      if constexpr (Lik::kNoise) etap += wsn[u] * Lik::dlog_p_deta(t, K);
      if constexpr (Lik::kRowConst) racc += Lik::row_acc(t, wsn[u]);
      c[u] = Lik::adjoint(t, md.scale, wsn[u], K);
    }
    flow_backward_ckpt<NB, X>(F, c, rp, stack + tid, 256, aw, lane, accr + tid, 256);
#pragma unroll
    for (int u = 0; u < NB; ++u) { cm += c[u]; cv += c[u] * xsn[u]; }
  }
  if constexpr (Lik::kRowTerm) {   // the weights sum to 1: the part of log p that is constant over the nodes, once per row
    if constexpr (Lik::kRowNoise) {   // ... of y and the launch constants, with its share of the noise adjoint
      if (valid && qn == 0) { ellp += Lik::row_term(y, K); etap += Lik::row_deta(y, K); }
    } else {
      if (valid && qn == 0) ellp += Lik::row_term(y);
    }
  }
  cm = group_sum(cm);
  cv = group_sum(cv);
  for (int j = 0; j < RP; ++j) {
    const double a = group_sum(accr[(size_t)j * 256 + tid]);
    if (valid && qn == 0 && g_rowp) g_rowp[(size_t)n * RP + j] = a;
  }
  if (valid && qn == 0) {
    if (g_mu) g_mu[n] = cm;
    if (g_v) g_v[n] = (!Lik::kClampV || vn > 0.0) ? cv / sq : 0.0;
  }
  if constexpr (Lik::kRowConst) {   // the adjoints of the row's second pair of moments: row 1 of the (2,N) outputs
    const double A = group_sum(racc);
    if (valid && qn == 0) {
      if (g_mu) g_mu[(size_t)md.N + n] = md.scale * Lik::row_mu_bar(A, K);
      if (g_v) g_v[(size_t)md.N + n] = md.scale * Lik::row_v_bar(A, K);
    }
  }
  ellp = wave_sum(ellp);
  if constexpr (Lik::kNoise) etap = wave_sum(etap);
  if (lane == 0) {
    red[wave] = ellp;
    if constexpr (Lik::kNoise) red[4 + wave] = etap;
  }
  __syncthreads();
  double* pb = part + (size_t)blockIdx.x * (2 + P);
  if (tid == 0) {
    if constexpr (Lik::kBlockTerm) {   // the part of log p that no row or node changes, times this workgroup's rows
      const int r0 = blockIdx.x * (4 * RW), nr = md.N - r0 < 4 * RW ? md.N - r0 : 4 * RW;
      red[0] += (double)nr * Lik::block_term(K);
    }
    pb[0] = md.scale * (red[0] + red[1] + red[2] + red[3]);
    pb[1] = Lik::kNoise ? md.scale * (red[4] + red[5] + red[6] + red[7]) : 0.0;
  }
  for (int j = tid; j < P; j += 256) pb[2 + j] = (accw[j] + accw[P + j]) + (accw[2 * P + j] + accw[3 * P + j]);
}

// ---------------------------------------------------------------------------------------------------
// Prediction given the q(f) moments of a row: m1, m2 and the test log-likelihood logp, by the same Gauss-Hermite sweep through
// the flow, g_s = G(mu + sqrt(2 v) x_s), as a template over a predictive policy (k_predict_quad).  A policy supplies
//   kClampV                     v <= 0 counts as 0 in the sweep
//   consts(md, fp, Y_std)       its launch constants K, from md.log_var_noise
//   Acc                         what it sums over the nodes (a small struct that starts at its neutral element)
//   node(a, w, g, R, K)         adds the node of normalised weight w to a; the nodes arrive in the order s = 0 .. S - 1, the
//                               padding of the last group of four after them at weight 0
//   finish(a, R, K)             (m1, m2, logp) from the sums
//   closed(md, fp)              the launch needs no sweep: closed_row(R, log_var_noise, Y_std) gives the three at once
// R is the row: mu and v as stored, its target y (0 when no logp is asked for) and want_lp.
// ---------------------------------------------------------------------------------------------------
struct PredRow { double m, v, y; bool want_lp; };
struct PredOut { double m1, m2, lp; };

// log sum_i exp(t_i), kept relative to its running maximum (rescaled when a larger term arrives): finite where every single term
// underflows -- a count of 10^4 at a rate of e^2 has terms near -10^5.  A term of -inf adds nothing; all of them: -inf.
struct LogSumExp { double mx = -INFINITY, se = 0.0; };
__device__ __forceinline__ void lse_push(LogSumExp& l, double t) {
  if (t > l.mx) { l.se = l.se * exp(l.mx - t) + 1.0; l.mx = t; }
  else if (t > -INFINITY) l.se += exp(t - l.mx);
}
__device__ __forceinline__ double lse_value(const LogSumExp& l) { return l.mx + log(l.se); }
struct PredSums { double m1 = 0.0, e2 = 0.0; LogSumExp l; };   // sum w x, sum w x^2 and the log-sum-exp of log w + log p(y | g)
struct PredSweepOnly {   // a policy without a closed form
  static __device__ __forceinline__ bool closed(const tgp_model&, const FlowProg&) { return false; }
  static __device__ __forceinline__ PredOut closed_row(const PredRow&, const double*, double) { return {}; }
};

// Gaussian noise around the flow (TGP_LIK_FLOW) and the plain Gaussian (TGP_LIK_GAUSS), in the standardised units of the targets;
// logp is the per-row kernel of the test log-likelihood (without the -0.5 log(pi) constant: log w_s = log(wn_s) + 0.5 log(pi), the
// caller adds the reference's constants)
//   flow : GaussianNonLinearMean.marginal_moments (:176-203) ; sparse_MF_SP.test_log_likelihood (:705-776)
//   gauss: GaussianLinearMean.marginal_moments (:89-118)     ; sparse_MF_SP.py:786-799
// v is not clamped.  Nodes of weight 0 do not enter.  A TGP_LIK_FLOW call with an empty program runs the sweep.
struct PredGauss {
  static constexpr bool kClampV = false;
  struct K { double noise, Y_std, lvar, ivar; };   // of var = Y_std^2 noise: its log and reciprocal
  using Acc = PredSums;
  static __device__ __forceinline__ bool closed(const tgp_model& md, const FlowProg&) { return md.lik == TGP_LIK_GAUSS; }
  static __device__ __forceinline__ PredOut closed_row(const PredRow& R, const double* lvn, double Y_std) {
    const double m1 = R.m, m2 = exp(lvn[0]) + R.v;
    if (!R.want_lp) return {m1, m2, 0.0};
    const double sd = Y_std * sqrt(m2), var = sd * sd, r = Y_std * R.y - Y_std * m1;
    return {m1, m2, -0.5 * (TGP_LOG_2PI_REF + log(var) + r * r / var)};
  }
  static __device__ __forceinline__ K consts(const tgp_model& md, const FlowProg&, double Y_std) {
    const double noise = exp(md.log_var_noise[0]), sdy = Y_std * sqrt(noise), var = sdy * sdy;
    return {noise, Y_std, log(var), 1.0 / var};
  }
  static __device__ __forceinline__ void node(Acc& a, double w, double g, const PredRow& R, const K& k) {
    if (!(w > 0.0)) return;
    a.m1 += w * g;
    a.e2 += w * g * g;
    if (R.want_lp) {
      const double r = k.Y_std * R.y - k.Y_std * g;
      lse_push(a.l, log(w) - 0.5 * (TGP_LOG_2PI_REF + k.lvar + r * r * k.ivar));
    }
  }
  static __device__ __forceinline__ PredOut finish(const Acc& a, const PredRow& R, const K& k) {
    return {a.m1, k.noise + a.e2 - a.m1 * a.m1, R.want_lp ? lse_value(a.l) : 0.0};
  }
};

// Bernoulli, probit link: P = Phi(mu / sqrt(1 + v)) for the empty program (R&W eq. 3.80, Bernoulli.py marginal_moments; v as
// stored), else sum_s w_s Phi(g_s), clamped to [0, 1].  P(y = 1) and P(y = 0) are each summed on their own (no 1 - P cancellation).
// m1 = P, m2 = P (1 - P), logp = y log P + (1 - y) log(1 - P) (no constant).
struct PredBern {
  static constexpr bool kClampV = true;
  struct Acc { double P1 = 0.0, P0 = 0.0; };
  static __device__ __forceinline__ bool closed(const tgp_model&, const FlowProg& fp) { return fp.nblk == 0; }
  // the node term gives log P and log(1 - P) without forming P (finite however far out mu / sqrt(1 + v) is)
  static __device__ __forceinline__ PredOut closed_row(const PredRow& R, const double*, double) {
    const BernNode b = bern_node(R.m / sqrt(1.0 + R.v), R.y);
    return {b.pp, b.pp * b.pm, b.lp};
  }
  static __device__ __forceinline__ EllNone consts(const tgp_model&, const FlowProg&, double) { return {}; }
  static __device__ __forceinline__ void node(Acc& a, double w, double g, const PredRow&, const EllNone&) {
    const BernNode b = bern_node(g, 0.0);
    a.P1 += w * b.pp;
    a.P0 += w * b.pm;
  }
  static __device__ __forceinline__ PredOut finish(const Acc& a, const PredRow& R, const EllNone&) {
    const double P1 = fmin(fmax(a.P1, 0.0), 1.0), P0 = fmin(fmax(a.P0, 0.0), 1.0);
    if (!R.want_lp) return {P1, P1 * P0, 0.0};
    return {P1, P1 * P0, (R.y != 0.0 ? R.y * log(P1) : 0.0) + (R.y != 1.0 ? (1.0 - R.y) * log(P0) : 0.0)};
  }
};

// Student-t noise (EllStudent's constants), in the standardised units of PredGauss:
//   m1 = sum_s w_s g_s,  m2 = sum_s w_s g_s^2 - m1^2 + sigma^2 nu / (nu - 2)   (+inf for nu <= 2: no variance),
//   logp = log sum_s w_s t_nu(y | g_s, sigma) - log Y_std = logsumexp_s(log w_s - (nu + 1) / 2 log1p(r_s^2 / (nu sigma^2)))
//          + c(nu, eta) - log Y_std,
// the exact log predictive density of the raw target with every constant.  No closed form (the Gaussian-Student convolution has
// none): the empty program runs the sweep, and the two moments are exact at S >= 2.  Nodes of weight 0 do not enter.
struct PredStudent : PredSweepOnly {
  static constexpr bool kClampV = true;
  struct K : StudentConst { double Y_std; };
  using Acc = PredSums;
  static __device__ __forceinline__ K consts(const tgp_model& md, const FlowProg&, double Y_std) {
    return {EllStudent::consts(md.log_var_noise), Y_std};
  }
  static __device__ __forceinline__ void node(Acc& a, double w, double g, const PredRow& R, const K& k) {
    if (!(w > 0.0)) return;
    a.m1 += w * g;
    a.e2 += w * g * g;
    if (R.want_lp) {
      const double r = R.y - g;
      lse_push(a.l, log(w) - 0.5 * k.nu1 * log1p(r * r * k.inus2));
    }
  }
  static __device__ __forceinline__ PredOut finish(const Acc& a, const PredRow& R, const K& k) {
    return {a.m1, k.nu > 2.0 ? a.e2 - a.m1 * a.m1 + k.nus2 / (k.nu - 2.0) : INFINITY,
            R.want_lp ? lse_value(a.l) + student_log_const(k.nu, k.eta) - log(k.Y_std) : 0.0};
  }
};

// The count likelihoods (Lik = EllPois, EllNegBin), g_s the log-rate at node s.  Poisson:
//   m1 = E[y] = sum_s w_s exp(g_s),  m2 = Var[y] = m1 + sum_s w_s exp(2 g_s) - m1^2   (law of total variance; the empty
//   program: the log-normal closed forms m1 = exp(mu + v / 2), m2 = m1 + (exp(v) - 1) m1^2, v <= 0 as 0),
//   logp = log sum_s w_s Poisson(y | exp(g_s)) = logsumexp_s(log w_s + y g_s - exp(g_s)) - lgamma(y + 1),
// the log predictive pmf with its constant; the empty program takes it from the sweep as well.  Nodes of weight 0 do not enter.
// Negative binomial (kOverDisp): the same with the policy's node term and row term,
//   m2 = m1 + (1 + 1/r) sum_s w_s exp(2 g_s) - m1^2   (the empty program: E[mean^2] = exp(2 mu + 2 v) = exp(v) m1^2),
//   logp = logsumexp_s(log w_s + y u_s - (y + r) sp(u_s)) + lgamma(y + r) - lgamma(r) - lgamma(y + 1).
template <class Lik>
struct PredCount : PredSweepOnly {
  static constexpr bool kClampV = true;
  struct K { decltype(Lik::consts(nullptr)) lik; bool lognormal; };   // lognormal: the empty program, the moments in closed form
  using Acc = PredSums;
  static __device__ __forceinline__ K consts(const tgp_model& md, const FlowProg& fp, double) {
    return {Lik::consts(md.log_var_noise), fp.nblk == 0};
  }
  static __device__ __forceinline__ void node(Acc& a, double w, double g, const PredRow& R, const K& k) {
    if (!(w > 0.0)) return;
    const auto nd = Lik::at(g, R.y, k.lik);
    const double e = Lik::rate(nd);
    a.m1 += w * e;
    a.e2 += w * e * e;
    if (R.want_lp) lse_push(a.l, Lik::plus_log_p(log(w), nd, k.lik));
  }
  static __device__ __forceinline__ PredOut finish(const Acc& a, const PredRow& R, const K& k) {
    const double vn = R.v > 0.0 ? R.v : 0.0;
    PredOut o;
    if constexpr (Lik::kOverDisp) {
      const double c = Lik::excess(k.lik);
      o.m1 = k.lognormal ? exp(R.m + 0.5 * vn) : a.m1;
      o.m2 = k.lognormal ? o.m1 + (expm1(vn) + c * exp(vn)) * o.m1 * o.m1 : a.m1 + (1.0 + c) * a.e2 - a.m1 * a.m1;
    } else {
      o.m1 = k.lognormal ? exp(R.m + 0.5 * vn) : a.m1;
      o.m2 = k.lognormal ? o.m1 + expm1(vn) * o.m1 * o.m1 : a.m1 + a.e2 - a.m1 * a.m1;
    }
    if (!R.want_lp) o.lp = 0.0;
    else if constexpr (Lik::kRowNoise) o.lp = lse_value(a.l) + Lik::row_term(R.y, k.lik);
    else o.lp = lse_value(a.l) + Lik::row_term(R.y);
    return o;
  }
};

// 256 rows per workgroup, one row per lane, NB = 4 nodes per flow_forward_n call; dynamic LDS: 2 (P + 2) doubles.  The last
// group of four is filled up with node S - 1 again at weight 0.  Y may be null (no logp), m1o and m2o too.
// The log-sum-exp skips a term of -inf in every policy.  k_predict, which this kernel replaced for PredGauss, had no such guard
// and let in every node s < S: a row whose every term is -inf now gets logp = -inf where it got NaN, and so does a row whose
// first node has weight 0 -- which no Gauss-Hermite rule of S <= 256 nodes has: none of their weights underflows, so "weight
// above 0" and "s < S" name the same nodes there.  On finite terms the two forms are the same arithmetic.
// X: the extended kind set.
template <class Pred, bool X>
__global__ __launch_bounds__(256) void k_predict_quad(tgp_model md, FlowProg fp, const double* __restrict__ mu,
                                                      const double* __restrict__ v, const double* __restrict__ rowp,
                                                      const double* __restrict__ Y, double Y_std, double* __restrict__ m1o,
                                                      double* __restrict__ m2o, double* __restrict__ logp) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  double* tp = reinterpret_cast<double*>(smem_raw);
  double* tg = tp + (md.P + 2) / 2 * 2;
  const bool closed = Pred::closed(md, fp);
  if (!closed) flow_params_lds<X>(md.theta, fp, tp, tg);
  const int n = blockIdx.x * 256 + threadIdx.x;
  if (n >= md.N) return;
  const bool want_lp = logp && Y;
  const double y = want_lp ? Y[n] : 0.0;
  PredOut o;
  // (each arm reads its row itself, the sweep after its set-up, as the kernels before this one did: read once ahead of the
  //  branch, the same loads cost PredBern 6 VGPRs, 129 for 123, and with them its fourth wave per SIMD)
  if (closed) {
    o = Pred::closed_row(PredRow{mu[n], v[n], y, want_lp}, md.log_var_noise, Y_std);
  } else {
    const auto K = Pred::consts(md, fp, Y_std);
    FlowDev F{fp.blk, fp.nblk, tp, tg};
    const double* rp = rowp ? rowp + (size_t)n * md.RP : nullptr;
    const PredRow R{mu[n], v[n], y, want_lp};
    const double vn = Pred::kClampV ? (R.v > 0.0 ? R.v : 0.0) : R.v;
    const double sq = sqrt(2.0 * vn);
    typename Pred::Acc a;
    constexpr int NB = 4;   // quadrature nodes in flight (stage-by-stage evaluation, flow_forward_n)
    for (int s0 = 0; s0 < md.S; s0 += NB) {
      double g[NB], der[NB], wsn[NB];
      const double* rpn[NB];
      TGP_EACH(u, NB) {
        const int s = s0 + u < md.S ? s0 + u : md.S - 1;
        g[u] = R.m + sq * md.xs[s];
        wsn[u] = s0 + u < md.S ? md.wn[s] : 0.0;
        rpn[u] = rp;
      }
      flow_forward_n<NB, false, X>(F, g, rpn, der);
      TGP_EACH(u, NB) Pred::node(a, wsn[u], g[u], R, K);
    }
    o = Pred::finish(a, R, K);
  }
  if (m1o) m1o[n] = o.m1;
  if (m2o) m2o[n] = o.m2;
  if (want_lp) logp[n] = o.lp;
}

// one launch of k_predict_quad<Pred, false> or, for a program with a kind past STEPTANH, k_predict_quad<Pred, true>
template <class Pred>
static int predict_launch(const tgp_model& md, const FlowProg& fp, const double* mu, const double* v, const double* rowp,
                          const double* Y, double Y_std, double* m1, double* m2, double* logp, hipStream_t st) {
  auto* const kern = flow_prog_extended(fp.blk, fp.nblk) ? k_predict_quad<Pred, true> : k_predict_quad<Pred, false>;
  hipLaunchKernelGGL(kern, dim3((md.N + 255) / 256), dim3(256), 2 * (size_t)(md.P + 2) * sizeof(double), st, md, fp, mu, v, rowp,
                     Y, Y_std, m1, m2, logp);
  LAUNCH_CHECK();
  return 0;
}

// one launch of k_ell_quad<Lik, LPR, NB> or, for a program with a kind past STEPTANH, k_ell_quad<Lik, LPR, NB | ext>, ext =
// flow_prog_xbit: TGP_FLOWX, or TGP_FLOWX2 with a kind past INV_BOXCOX; each of the three kernel functions has its own
// dynamic-LDS high-water mark (ensure_lds)
template <class Lik, int LPR, int NB, class... Args>
static int ell_launch_one(int ext, int nb, size_t lds, hipStream_t st, Args... args) {
  static size_t cur[3] = {48 * 1024, 48 * 1024, 48 * 1024};
  auto* const kern = ext == TGP_FLOWX2 ? k_ell_quad<Lik, LPR, NB | TGP_FLOWX2>
                                       : (ext ? k_ell_quad<Lik, LPR, NB | TGP_FLOWX> : k_ell_quad<Lik, LPR, NB>);
  if (int rc = ensure_lds(reinterpret_cast<const void*>(kern), lds, &cur[ext == TGP_FLOWX2 ? 2 : (ext ? 1 : 0)])) return rc;
  hipLaunchKernelGGL(kern, dim3(nb), dim3(256), lds, st, args...);
  LAUNCH_CHECK();
  return 0;
}
// the most nodes in flight k_ell_quad is built with for a policy: Lik::kMaxNB where the policy names one (EllBeta: 4, the kernel
// spills at 8), else 8.  The policy's LikRow carries the same number to ell_plan (ell_max_nb).
template <class Lik, class = void>
struct EllMaxNB { static constexpr int value = 8; };
template <class Lik>
struct EllMaxNB<Lik, std::void_t<decltype(Lik::kMaxNB)>> { static constexpr int value = Lik::kMaxNB; };
// the instantiation for ell_plan's (LPR, NB)
template <class Lik, class... Args>
static int ell_launch(int LPR, int NB, Args... args) {
  if (LPR == 4) {
    if constexpr (EllMaxNB<Lik>::value >= 8) {
      if (NB == 8) return ell_launch_one<Lik, 4, 8>(args...);
    }
    if (NB == 4) return ell_launch_one<Lik, 4, 4>(args...);
    if (NB == 2) return ell_launch_one<Lik, 4, 2>(args...);
    return ell_launch_one<Lik, 4, 1>(args...);
  }
  if (LPR == 16) {
    if (NB == 4) return ell_launch_one<Lik, 16, 4>(args...);
    if (NB == 2) return ell_launch_one<Lik, 16, 2>(args...);
    return ell_launch_one<Lik, 16, 1>(args...);
  }
  if (NB == 4) return ell_launch_one<Lik, 32, 4>(args...);
  if (NB == 2) return ell_launch_one<Lik, 32, 2>(args...);
  return ell_launch_one<Lik, 32, 1>(args...);
}
// ... under the signature of a LikRow
template <class Lik>
static int ell_launch_row(int LPR, int NB, int ext, int nb, size_t lds, hipStream_t st, const tgp_model& md, const FlowProg& fp,
                          const double* Y, const double* mu, const double* v, const double* rowp, double* part, double* g_mu,
                          double* g_v, double* g_rowp) {
  return ell_launch<Lik>(LPR, NB, ext, nb, lds, st, md, fp, Y, mu, v, rowp, part, g_mu, g_v, g_rowp);
}

}  // namespace tgp
