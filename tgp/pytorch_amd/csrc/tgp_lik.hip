// tgp_lik.hip -- stand-alone likelihood, flow, prediction and optimiser kernels.
//
// These serve the evaluation path, the operator-level API (K10/K11 of SURVEY 2.2) and
// the trainer; the training step itself uses the fused row kernel (tgp_rows.hpp), which shares the
// flow code in tgp_dev.hpp.  All of them are HBM/VALU-bound streaming kernels: one thread per row,
// coalesced row-major reads, lane-private LDS accumulators, two-pass deterministic reductions.
#include "tgp_dev.hpp"
#include "tgp_launch.hpp"

namespace tgp {

// k_ell_quad: lanes per data row.  4 by default (64 rows per workgroup); 16 for small problems (16 rows per workgroup): a
// rank's 1 250 rows of an 8-GPU minibatch were 20 workgroups, each lane walking 8 quadrature nodes through 30 tanh steps
// and back -- 91 us of one dependent chain, whatever N; with 16 lanes per row a lane has 2 nodes and 79 workgroups run.
// Round 6: 32 lanes per row (8 rows per workgroup, one node per lane at S = 32) below 2 560 rows -- the 1 250-row share again: 79
// workgroups leave three quarters of the SIMDs without a wave, and a lane's chain is as long as its nodes.
#define ELL_LPR16_MAXN 12288
#define ELL_LPR32_MAXN 2560
static int ell_lpr(int N) { return N <= ELL_LPR32_MAXN ? 32 : (N <= ELL_LPR16_MAXN ? 16 : 4); }

// Sized for ANY call with at most N rows: a caller that sizes once for its largest chunk (the general-M path) may
// launch a ragged last chunk that falls into the 16-lanes-per-row mode and then has MORE workgroups than the largest one.
size_t lik_workspace_doubles(int N, int P, int RP) {
  const size_t nb16 = (size_t)((N < ELL_LPR16_MAXN ? N : ELL_LPR16_MAXN) + 15) / 16, nb64 = (size_t)(N + 63) / 64;
  const size_t nb32 = (size_t)((N < ELL_LPR32_MAXN ? N : ELL_LPR32_MAXN) + 7) / 8;
  const size_t nbm = nb16 > nb64 ? nb16 : nb64;
  const size_t nb = (nbm > nb32 ? nbm : nb32) + 1;  // k_ell_quad: one partial per workgroup
  return nb * (size_t)(2 + P) + 2 * (size_t)P + 64;
}

// ---------------------------------------------------------------------------------------------------
// SVGP closed form: likelihoods/GaussianLinearMean.py:60-87 + dsp/utils.py:164-195
// ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_ell_gauss(const double* __restrict__ Y, const double* __restrict__ mu,
                                                    const double* __restrict__ v, int N,
                                                    const double* __restrict__ lvn, double scale,
                                                    double* __restrict__ part, double* __restrict__ g_mu,
                                                    double* __restrict__ g_v) {
  __shared__ double red[8];
  const int n = blockIdx.x * 256 + threadIdx.x;
  const double eta = lvn[0], einv = exp(-eta);
  double e = 0.0, et = 0.0;
  if (n < N) {
    const double r = Y[n] - mu[n];
    e = -0.5 * TGP_LOG_2PI_REF - 0.5 * eta - 0.5 * einv * (r * r + v[n]);
    et = -0.5 + 0.5 * einv * (r * r + v[n]);
    if (g_mu) g_mu[n] = scale * einv * r;
    if (g_v) g_v[n] = -0.5 * scale * einv;
  }
  e = wave_sum(e); et = wave_sum(et);
  if ((threadIdx.x & 63) == 0) { red[threadIdx.x >> 6] = e; red[4 + (threadIdx.x >> 6)] = et; }
  __syncthreads();
  if (threadIdx.x == 0) {
    part[2 * blockIdx.x] = scale * (red[0] + red[1] + red[2] + red[3]);
    part[2 * blockIdx.x + 1] = scale * (red[4] + red[5] + red[6] + red[7]);
  }
}

// sum `nb` partial vectors of length `len` (stride len) into out[0..split) / out2; block = 32 columns x 8 row groups
__global__ __launch_bounds__(256) void k_sum_parts(const double* __restrict__ part, int nb, int len,
                                                    double* __restrict__ out, double* __restrict__ out2, int split) {
  __shared__ double red[8][33];
  const int c = threadIdx.x & 31, g = threadIdx.x >> 5, j = blockIdx.x * 32 + c;
  double s0 = 0.0, s1 = 0.0;
  if (j < len) {
    int b = g;
    // (eight partials requested before the first add, added in the order of the two-at-a-time loop that follows: with two
    //  loads in flight per thread the 625 workgroup partials of a 10 000-row likelihood were 39 dependent round trips, 15 us)
    for (; b + 56 < nb; b += 64) {
      double t[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) t[u] = part[(size_t)(b + 8 * u) * len + j];
#pragma unroll
      for (int u = 0; u < 8; u += 2) { s0 += t[u]; s1 += t[u + 1]; }
    }
    for (; b + 8 < nb; b += 16) {
      s0 += part[(size_t)b * len + j];
      s1 += part[(size_t)(b + 8) * len + j];
    }
    if (b < nb) s0 += part[(size_t)b * len + j];
  }
  red[g][c] = s0 + s1;
  __syncthreads();
  if (g == 0 && j < len) {
    const double s = ((red[0][c] + red[1][c]) + (red[2][c] + red[3][c])) + ((red[4][c] + red[5][c]) + (red[6][c] + red[7][c]));
    if (j < split) out[j] = s;
    else if (out2) out2[j - split] = s;
  }
}

// ---------------------------------------------------------------------------------------------------
// Quadrature likelihoods through the flow with gradients, E_q(f0)[log p(y | G(f0))] by Gauss-Hermite:
//   Gaussian  (likelihoods/GaussianNonLinearMean.py:64-150)
//   Bernoulli (likelihoods/Bernoulli.py), probit link: log p(y | g) = y log Phi(g) + (1 - y) log Phi(-g)
//   Poisson   (no counterpart in the reference), log link: log p(y | g) = y g - exp(g) - lgamma(y + 1)
//   Student-t (no counterpart in the reference), location G(f0), scale sigma, nu degrees of freedom (TGP_LIK_STUDENT)
//   heteroscedastic Gaussian (no counterpart in the reference), log noise variance c + h, h a second latent GP (TGP_LIK_HETERO)
// ---------------------------------------------------------------------------------------------------

// The node term shared by k_ell_quad<EllBern> and k_predict_bern.  With a = |g|, t = a / sqrt 2:
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
  static constexpr bool kBlockTerm = false;
  static constexpr bool kRowConst = false;
  static __device__ __forceinline__ EllNone consts(const double*) { return {}; }
  static __device__ __forceinline__ PoisNode at(double g, double y, const EllNone&) { return {g, exp(g), y}; }
  static __device__ __forceinline__ double log_p(const PoisNode& t, const EllNone&) { return t.y * t.g - t.e; }
  static __device__ __forceinline__ double adjoint(const PoisNode& t, double scale, double w, const EllNone&) {
    return scale * w * (t.y - t.e);
  }
  static __device__ __forceinline__ double row_term(double y) { return -lgamma(y + 1.0); }
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
// NBX = NB | TGP_FLOWX: the flow sweeps know the extended kind set (X; see k_rows)
template <class Lik, int LPR, int NBX>
__global__ __launch_bounds__(256) void k_ell_quad(tgp_model md, FlowProg fp, const double* __restrict__ Y,
                                                   const double* __restrict__ mu, const double* __restrict__ v,
                                                   const double* __restrict__ rowp, double* __restrict__ part,
                                                   double* __restrict__ g_mu, double* __restrict__ g_v,
                                                   double* __restrict__ g_rowp) {
  constexpr int NB = NBX & (TGP_FLOWX - 1);
  constexpr bool X = NBX & TGP_FLOWX;
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
    if (valid && qn == 0) ellp += Lik::row_term(y);
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
// flow evaluation: G, dG/df, log dG/df over an (S,N) array (row n = idx % N)
// X: the extended kind set (ARCSINH, BOXCOX, INV_BOXCOX; the host picks it for programs that hold one)
// ---------------------------------------------------------------------------------------------------
template <bool X>
__global__ __launch_bounds__(256) void k_flow_eval(tgp_model md, FlowProg fp, const double* __restrict__ f, size_t total, int N,
                                                    const double* __restrict__ rowp, double* __restrict__ G,
                                                    double* __restrict__ dG, double* __restrict__ logdG,
                                                    double* __restrict__ part) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  double* tp = reinterpret_cast<double*>(smem_raw);
  double* tg = tp + (md.P + 2) / 2 * 2;
  double* ti = tg + (md.P + 2) / 2 * 2;
  __shared__ double redl[4];
  flow_params_lds<X>(md.theta, fp, tp, tg, ti);
  FlowDev F{fp.blk, fp.nblk, tp, tg, ti};
  // four elements per thread, a grid stride apart (coalesced), evaluated stage by stage (flow_forward_n)
  constexpr int NB = 4;
  const size_t i0 = (size_t)blockIdx.x * 256 + threadIdx.x, stride = (size_t)gridDim.x * 256;
  double fv[NB], der[NB];
  const double* rp[NB];
  TGP_EACH(u, NB) {
    const size_t i = i0 + u * stride;
    const size_t ic = i < total ? i : 0;
    fv[u] = f[ic];
    rp[u] = rowp ? rowp + (ic % N) * md.RP : nullptr;
  }
  if (dG || logdG || part) flow_forward_n<NB, true, X>(F, fv, rp, der);
  else flow_forward_n<NB, false, X>(F, fv, rp, der);
  if (part) {
    // fused log-Jacobian accumulation: sum of log dG/df over this workgroup's elements, fixed order (lane partials ->
    // butterfly over the wave -> the four waves in LDS); the launcher's second kernel adds the workgroups' partials
    double sl = 0.0;
    TGP_EACH(u, NB) sl += (i0 + u * stride < total) ? log(der[u]) : 0.0;
    sl = wave_sum(sl);
    if ((threadIdx.x & 63) == 0) redl[threadIdx.x >> 6] = sl;
    __syncthreads();
    if (threadIdx.x == 0) part[blockIdx.x] = (redl[0] + redl[1]) + (redl[2] + redl[3]);
  }
  if (logdG) {
    double lg[NB];
    TGP_EACH(u, NB) lg[u] = der[u];
    TGP_EACH(u, NB) {
      const size_t i = i0 + u * stride;
      if (i < total) logdG[i] = log(lg[u]);
    }
  }
  TGP_EACH(u, NB) {
    const size_t i = i0 + u * stride;
    if (i < total) {
      if (G) G[i] = fv[u];
      if (dG) dG[i] = der[u];
    }
  }
}

// ---------------------------------------------------------------------------------------------------
// prediction given q(f) moments: m1, m2 and per-row test log-likelihood (without the -0.5 log(pi) constant)
//   flow : GaussianNonLinearMean.marginal_moments (:176-203) ; sparse_MF_SP.test_log_likelihood (:705-776)
//   gauss: GaussianLinearMean.marginal_moments (:89-118)     ; sparse_MF_SP.py:786-799
// X: the extended kind set
// ---------------------------------------------------------------------------------------------------
template <bool X>
__global__ __launch_bounds__(256) void k_predict(tgp_model md, FlowProg fp, const double* __restrict__ mu,
                                                  const double* __restrict__ v, const double* __restrict__ rowp,
                                                  const double* __restrict__ Y, double Y_std, double* __restrict__ m1o,
                                                  double* __restrict__ m2o, double* __restrict__ logp) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  double* tp = reinterpret_cast<double*>(smem_raw);
  double* tg = tp + (md.P + 2) / 2 * 2;
  if (md.lik == TGP_LIK_FLOW) flow_params_lds<X>(md.theta, fp, tp, tg);
  const int n = blockIdx.x * 256 + threadIdx.x;
  if (n >= md.N) return;
  const double noise = exp(md.log_var_noise[0]);
  if (md.lik == TGP_LIK_GAUSS) {
    const double m1 = mu[n], m2 = noise + v[n];
    if (m1o) m1o[n] = m1;
    if (m2o) m2o[n] = m2;
    if (logp && Y) {
      const double sd = Y_std * sqrt(m2), var = sd * sd, r = Y_std * Y[n] - Y_std * m1;
      logp[n] = -0.5 * (TGP_LOG_2PI_REF + log(var) + r * r / var);
    }
    return;
  }
  FlowDev F{fp.blk, fp.nblk, tp, tg};
  const double* rp = rowp ? rowp + (size_t)n * md.RP : nullptr;
  const double m_ = mu[n], sq = sqrt(2.0 * v[n]);
  const double sdy = Y_std * sqrt(noise), var = sdy * sdy;
  const double yy = Y ? Y_std * Y[n] : 0.0;
  double m1 = 0.0, e2 = 0.0, mx = -INFINITY, se = 0.0;
  const double lvar = log(var), ivar = 1.0 / var;
  constexpr int NB = 4;  // quadrature nodes in flight (stage-by-stage evaluation, flow_forward_n)
  for (int s0 = 0; s0 < md.S; s0 += NB) {
    double g[NB], der[NB], wsn[NB];
    const double* rpn[NB];
    TGP_EACH(u, NB) {
      const int s = s0 + u < md.S ? s0 + u : md.S - 1;
      g[u] = m_ + sq * md.xs[s];
      wsn[u] = s0 + u < md.S ? md.wn[s] : 0.0;
      rpn[u] = rp;
    }
    flow_forward_n<NB, false, X>(F, g, rpn, der);
    TGP_EACH(u, NB) {
      if (s0 + u < md.S) {
        m1 += wsn[u] * g[u];
        e2 += wsn[u] * g[u] * g[u];
        if (logp && Y) {
          // log w_s = log(wn_s) + 0.5 log(pi); the caller adds the reference's constants
          const double r = yy - Y_std * g[u];
          const double t = log(wsn[u]) - 0.5 * (TGP_LOG_2PI_REF + lvar + r * r * ivar);
          if (t > mx) { se = se * exp(mx - t) + 1.0; mx = t; }
          else se += exp(t - mx);
        }
      }
    }
  }
  if (m1o) m1o[n] = m1;
  if (m2o) m2o[n] = noise + e2 - m1 * m1;
  if (logp && Y) logp[n] = mx + log(se);
}

// Predictive probability per row: P = Phi(mu / sqrt(1 + v)) for the empty program (R&W eq. 3.80, Bernoulli.py
// marginal_moments), else sum_s w_s Phi(G(mu + sqrt(2 v) x_s)) with the row's own v, clamped to [0, 1].
// m1 = P, m2 = P (1 - P), logp = y log P + (1 - y) log(1 - P) (no constant).  X: the extended kind set.
template <bool X>
__global__ __launch_bounds__(256) void k_predict_bern(tgp_model md, FlowProg fp, const double* __restrict__ mu,
                                                       const double* __restrict__ v, const double* __restrict__ rowp,
                                                       const double* __restrict__ Y, double* __restrict__ m1o,
                                                       double* __restrict__ m2o, double* __restrict__ logp) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  double* tp = reinterpret_cast<double*>(smem_raw);
  double* tg = tp + (md.P + 2) / 2 * 2;
  flow_params_lds<X>(md.theta, fp, tp, tg);
  const int n = blockIdx.x * 256 + threadIdx.x;
  if (n >= md.N) return;
  const double y = (logp && Y) ? Y[n] : 0.0;
  double P1 = 0.0, P0 = 0.0;   // P(y = 1), P(y = 0), each summed on its own (no 1 - P cancellation)
  double lp = 0.0;
  bool lp_done = false;
  if (fp.nblk == 0) {
    // closed form: the node term gives log P and log(1 - P) without forming P (finite however far out mu / sqrt(1 + v) is)
    const BernNode b = bern_node(mu[n] / sqrt(1.0 + v[n]), y);
    P1 = b.pp;
    P0 = b.pm;
    lp = b.lp;
    lp_done = true;
  } else {
    FlowDev F{fp.blk, fp.nblk, tp, tg};
    const double* rp = rowp ? rowp + (size_t)n * md.RP : nullptr;
    const double vn = v[n] > 0.0 ? v[n] : 0.0;
    const double m_ = mu[n], sq = sqrt(2.0 * vn);
    constexpr int NB = 4;
    for (int s0 = 0; s0 < md.S; s0 += NB) {
      double g[NB], der[NB], wsn[NB];
      const double* rpn[NB];
      TGP_EACH(u, NB) {
        const int s = s0 + u < md.S ? s0 + u : md.S - 1;
        g[u] = m_ + sq * md.xs[s];
        wsn[u] = s0 + u < md.S ? md.wn[s] : 0.0;
        rpn[u] = rp;
      }
      flow_forward_n<NB, false, X>(F, g, rpn, der);
      TGP_EACH(u, NB) {
        const BernNode b = bern_node(g[u], 0.0);
        P1 += wsn[u] * b.pp;
        P0 += wsn[u] * b.pm;
      }
    }
    P1 = fmin(fmax(P1, 0.0), 1.0);
    P0 = fmin(fmax(P0, 0.0), 1.0);
  }
  if (m1o) m1o[n] = P1;
  if (m2o) m2o[n] = P1 * P0;
  if (logp && Y) logp[n] = lp_done ? lp : (y != 0.0 ? y * log(P1) : 0.0) + (y != 1.0 ? (1.0 - y) * log(P0) : 0.0);
}

// Poisson predictive per row, g_s = G(mu + sqrt(2 v) x_s) the log-rate at node s (v <= 0 counts as 0):
//   m1 = E[y] = sum_s w_s exp(g_s),  m2 = Var[y] = m1 + sum_s w_s exp(2 g_s) - m1^2   (law of total variance; the empty
//   program: the log-normal closed forms m1 = exp(mu + v / 2), m2 = m1 + (exp(v) - 1) m1^2),
//   logp = log sum_s w_s Poisson(y | exp(g_s)) = logsumexp_s(log w_s + y g_s - exp(g_s)) - lgamma(y + 1),
// the log predictive pmf with its constant.  The sum is kept relative to its running maximum (rescaled when a larger term
// arrives), so logp is finite where every single term underflows -- y = 10^4 at a rate of e^2: terms near -10^5.  Nodes past S
// and nodes of weight 0 do not enter.  X: the extended kind set.
template <bool X>
__global__ __launch_bounds__(256) void k_predict_pois(tgp_model md, FlowProg fp, const double* __restrict__ mu,
                                                       const double* __restrict__ v, const double* __restrict__ rowp,
                                                       const double* __restrict__ Y, double* __restrict__ m1o,
                                                       double* __restrict__ m2o, double* __restrict__ logp) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  double* tp = reinterpret_cast<double*>(smem_raw);
  double* tg = tp + (md.P + 2) / 2 * 2;
  flow_params_lds<X>(md.theta, fp, tp, tg);
  const int n = blockIdx.x * 256 + threadIdx.x;
  if (n >= md.N) return;
  const bool want_lp = logp && Y;
  const double y = want_lp ? Y[n] : 0.0;
  FlowDev F{fp.blk, fp.nblk, tp, tg};
  const double* rp = rowp ? rowp + (size_t)n * md.RP : nullptr;
  const double vn = v[n] > 0.0 ? v[n] : 0.0;
  const double m_ = mu[n], sq = sqrt(2.0 * vn);
  double m1 = 0.0, e2 = 0.0, mx = -INFINITY, se = 0.0;
  constexpr int NB = 4;
  for (int s0 = 0; s0 < md.S; s0 += NB) {
    double g[NB], der[NB], wsn[NB];
    const double* rpn[NB];
    TGP_EACH(u, NB) {
      const int s = s0 + u < md.S ? s0 + u : md.S - 1;
      g[u] = m_ + sq * md.xs[s];
      wsn[u] = s0 + u < md.S ? md.wn[s] : 0.0;
      rpn[u] = rp;
    }
    flow_forward_n<NB, false, X>(F, g, rpn, der);
    TGP_EACH(u, NB) {
      if (wsn[u] > 0.0) {
        const double e = exp(g[u]);
        m1 += wsn[u] * e;
        e2 += wsn[u] * e * e;
        if (want_lp) {
          const double t = log(wsn[u]) + y * g[u] - e;
          if (t > mx) { se = se * exp(mx - t) + 1.0; mx = t; }
          else if (t > -INFINITY) se += exp(t - mx);
        }
      }
    }
  }
  double m2 = m1 + e2 - m1 * m1;
  if (fp.nblk == 0) {
    m1 = exp(m_ + 0.5 * vn);
    m2 = m1 + expm1(vn) * m1 * m1;
  }
  if (m1o) m1o[n] = m1;
  if (m2o) m2o[n] = m2;
  if (want_lp) logp[n] = mx + log(se) - lgamma(y + 1.0);
}

// Student-t predictive per row, in the standardised units of k_predict, g_s = G(mu + sqrt(2 v) x_s) (v <= 0 counts as 0):
//   m1 = sum_s w_s g_s,  m2 = sum_s w_s g_s^2 - m1^2 + sigma^2 nu / (nu - 2)   (+inf for nu <= 2: no variance),
//   logp = log sum_s w_s t_nu(y | g_s, sigma) - log Y_std = logsumexp_s(log w_s - (nu + 1) / 2 log1p(r_s^2 / (nu sigma^2)))
//          + c(nu, eta) - log Y_std,
// the exact log predictive density of the raw target with every constant; the sum is kept relative to its running maximum
// as in k_predict_pois.  The empty program runs the same loop (no closed form for the Gaussian-Student convolution; the
// two moments are exact at S >= 2).  Nodes past S and nodes of weight 0 do not enter.  X: the extended kind set.
template <bool X>
__global__ __launch_bounds__(256) void k_predict_student(tgp_model md, FlowProg fp, const double* __restrict__ mu,
                                                          const double* __restrict__ v, const double* __restrict__ rowp,
                                                          const double* __restrict__ Y, double Y_std, double* __restrict__ m1o,
                                                          double* __restrict__ m2o, double* __restrict__ logp) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  double* tp = reinterpret_cast<double*>(smem_raw);
  double* tg = tp + (md.P + 2) / 2 * 2;
  flow_params_lds<X>(md.theta, fp, tp, tg);
  const int n = blockIdx.x * 256 + threadIdx.x;
  if (n >= md.N) return;
  const bool want_lp = logp && Y;
  const double y = want_lp ? Y[n] : 0.0;
  const StudentConst K = EllStudent::consts(md.log_var_noise);
  FlowDev F{fp.blk, fp.nblk, tp, tg};
  const double* rp = rowp ? rowp + (size_t)n * md.RP : nullptr;
  const double vn = v[n] > 0.0 ? v[n] : 0.0;
  const double m_ = mu[n], sq = sqrt(2.0 * vn);
  double m1 = 0.0, e2 = 0.0, mx = -INFINITY, se = 0.0;
  constexpr int NB = 4;
  for (int s0 = 0; s0 < md.S; s0 += NB) {
    double g[NB], der[NB], wsn[NB];
    const double* rpn[NB];
    TGP_EACH(u, NB) {
      const int s = s0 + u < md.S ? s0 + u : md.S - 1;
      g[u] = m_ + sq * md.xs[s];
      wsn[u] = s0 + u < md.S ? md.wn[s] : 0.0;
      rpn[u] = rp;
    }
    flow_forward_n<NB, false, X>(F, g, rpn, der);
    TGP_EACH(u, NB) {
      if (wsn[u] > 0.0) {
        m1 += wsn[u] * g[u];
        e2 += wsn[u] * g[u] * g[u];
        if (want_lp) {
          const double r = y - g[u];
          const double t = log(wsn[u]) - 0.5 * K.nu1 * log1p(r * r * K.inus2);
          if (t > mx) { se = se * exp(mx - t) + 1.0; mx = t; }
          else if (t > -INFINITY) se += exp(t - mx);
        }
      }
    }
  }
  if (m1o) m1o[n] = m1;
  if (m2o) m2o[n] = K.nu > 2.0 ? e2 - m1 * m1 + K.nus2 / (K.nu - 2.0) : INFINITY;
  if (want_lp) logp[n] = mx + log(se) + student_log_const(K.nu, K.eta) - log(Y_std);
}

// ---------------------------------------------------------------------------------------------------
// Adam (torch.optim.Adam semantics; dsp/trainers/optimizers.py:12)
// ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_adam(double* __restrict__ p, const double* __restrict__ g,
                                               double* __restrict__ m, double* __restrict__ v, int64_t n, double lr,
                                               double b1, double b2, double eps, double wd, double bc1, double bc2s,
                                               double sign) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  double gi = sign * g[i];
  if (wd != 0.0) gi += wd * p[i];
  const double mi = b1 * m[i] + (1.0 - b1) * gi;
  const double vi = b2 * v[i] + (1.0 - b2) * gi * gi;
  m[i] = mi;
  v[i] = vi;
  p[i] -= (lr / bc1) * mi / (sqrt(vi) / bc2s + eps);
}

// device-side step counter variant (hipGraph replay): step = *step_dev + 1, counter bumped by k_step_inc afterwards
__global__ __launch_bounds__(256) void k_adam_dev(double* __restrict__ p, const double* __restrict__ g,
                                                   double* __restrict__ m, double* __restrict__ v, int64_t n, double lr,
                                                   double b1, double b2, double eps, double wd,
                                                   int32_t* __restrict__ step_dev, double sign, int64_t n_plain,
                                                   double ln_b1, double ln_b2, int64_t skip_off, int64_t skip_n) {
  const double step = (double)(step_dev[0] + 1);
  // beta^step = exp(step ln beta), ln beta from the host: the library pow() is ~300 dependent f64 instructions per
  // call and every thread made two of them -- 3 of this kernel's 4.3 us (relative error of the power <= 1e-14 at
  // step 1e5, far inside the 1e-8 the parity tests hold the optimiser trajectory to)
  const double bc1 = 1.0 - exp_fast(step * ln_b1), bc2s = sqrt(1.0 - exp_fast(step * ln_b2));
  // grid-stride: the launcher caps the grid (the ticket below is one atomic per workgroup on ONE word, ~12 ns each:
  // the 4 096 workgroups of a 1 M-parameter buffer spent 50 us queueing for it)
  // [skip_off, skip_off + skip_n): entries another launch of this step has updated already (general-M path: Lam, in k_big_glam)
  for (int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x; j < n - skip_n; j += (int64_t)gridDim.x * 256) {
    const int64_t i = j < skip_off ? j : j + skip_n;
    double gi = sign * g[i];
    if (wd != 0.0 && i >= n_plain) gi += wd * p[i];  // weight decay only on the tail group
    const double mi = b1 * m[i] + (1.0 - b1) * gi;
    const double vi = b2 * v[i] + (1.0 - b2) * gi * gi;
    m[i] = mi;
    v[i] = vi;
    p[i] -= (lr / bc1) * mi / (sqrt(vi) / bc2s + eps);
  }
  // Every block has read step_dev[0] before it takes a ticket; the block that draws the last ticket bumps the
  // counter for the next launch (no second kernel, valid under hipGraph replay).
  __syncthreads();
  if (threadIdx.x == 0) {
    const int t = atomicAdd(&step_dev[1], 1);
    if (t == (int)gridDim.x - 1) {
      step_dev[1] = 0;
      atomicAdd(&step_dev[0], 1);
    }
  }
}

// ---------------------------------------------------------------------------------------------------
// Minibatch rows of a data set that stays resident in HBM (the reference's DataLoader re-collates the rows on the host
// and copies them every step, dsp/data/data.py:86-88, trainers/trainer_base.py:330):
//   Xb[r] = X[index[cursor + offset + r]],  Yb[r] = Y[...]     r < nrows   (index == NULL: the stored order)
// `cursor` = int32[2] {position in the epoch, ticket} on the device: every workgroup reads the position before it
// takes a ticket, the last one advances it (wrapping to 0 at `wrap`), so a captured launch walks through the epoch
// replay after replay without the host touching it.
// ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_gather_rows(const double* __restrict__ X, const double* __restrict__ Y, int N, int D,
                                                      const int32_t* __restrict__ index, int32_t* __restrict__ cursor,
                                                      int offset, int nrows, int advance, int wrap,
                                                      double* __restrict__ Xb, double* __restrict__ Yb) {
  const int c0 = cursor[0];
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i < (long long)nrows * (D + 1)) {
    const int r = (int)(i / (D + 1)), d = (int)(i % (D + 1));
    int src = c0 + offset + r;
    src = src < N ? src : N - 1;
    if (index != nullptr) src = index[src];
    src = src < 0 ? 0 : (src < N ? src : N - 1);
    if (d < D) Xb[(size_t)r * D + d] = X[(size_t)src * D + d];
    else Yb[r] = Y[src];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const int t = atomicAdd(&cursor[1], 1);
    if (t == (int)gridDim.x - 1) {
      cursor[1] = 0;
      const int nx = c0 + advance;
      cursor[0] = nx >= wrap ? 0 : nx;
    }
  }
}

int launch_gather_rows(const double* X, const double* Y, int N, int D, const int32_t* index, int32_t* cursor, int offset,
                       int nrows, int advance, int wrap, double* Xb, double* Yb, hipStream_t st) {
  const long long n = (long long)nrows * (D + 1);
  hipLaunchKernelGGL(k_gather_rows, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, X, Y, N, D, index, cursor, offset,
                     nrows, advance, wrap, Xb, Yb);
  LAUNCH_CHECK();
  return 0;
}

// ---------------------------------------------------------------------------------------------------
// host launchers
// ---------------------------------------------------------------------------------------------------
int launch_ell_gauss(const double* Y, const double* mu, const double* v, int N, const double* lvn, double scale,
                     double* out, double* g_mu, double* g_v, double* ws, hipStream_t st) {
  const int nb = (N + 255) / 256;
  hipLaunchKernelGGL(k_ell_gauss, dim3(nb), dim3(256), 0, st, Y, mu, v, N, lvn, scale, ws, g_mu, g_v);
  LAUNCH_CHECK();
  hipLaunchKernelGGL(k_sum_parts, dim3(1), dim3(256), 0, st, ws, nb, 2, out, (double*)nullptr, 2);
  LAUNCH_CHECK();
  return 0;
}

static int flow_lds(const tgp_model& md, int nblk, int NB, size_t* bytes) {
  const size_t d = (size_t)(nblk > 0 ? nblk : 1) * NB * 256 + (size_t)(md.P > 0 ? md.P : 1) * 4 + (size_t)md.RP * 256 + 16 +
                   3 * (size_t)(md.P + 2);
  *bytes = d * sizeof(double);
  return *bytes > 160 * 1024 - 1024 ? TGP_E_LDS : 0;
}

// lanes per row, nodes in flight per lane and dynamic LDS of k_ell_quad
static int ell_plan(const tgp_model& md, const FlowProg& fp, int* lpr, int* nbn, size_t* lds) {
  const int LPR = ell_lpr(md.N);
  int NB = LPR == 4 ? (md.S > 16 ? 8 : 4) : (LPR == 16 ? (md.S > 32 ? 4 : (md.S > 16 ? 2 : 1)) : (md.S > 64 ? 4 : (md.S > 32 ? 2 : 1)));
  while (NB > 1 && (flow_lds(md, fp.nblk, NB, lds) != 0 || *lds > 120 * 1024)) NB >>= 1;
  *lpr = LPR;
  *nbn = NB;
  return flow_lds(md, fp.nblk, NB, lds);
}

// one launch of k_ell_quad<Lik, LPR, NB> or, for a program with a kind past STEPTANH (ext), k_ell_quad<Lik, LPR, NB | TGP_FLOWX>;
// each of the two kernel functions has its own dynamic-LDS high-water mark (ensure_lds)
template <class Lik, int LPR, int NB, class... Args>
static int ell_launch_one(bool ext, int nb, size_t lds, hipStream_t st, Args... args) {
  static size_t cur[2] = {48 * 1024, 48 * 1024};
  auto* const kern = ext ? k_ell_quad<Lik, LPR, NB | TGP_FLOWX> : k_ell_quad<Lik, LPR, NB>;
  if (int rc = ensure_lds(reinterpret_cast<const void*>(kern), lds, &cur[ext])) return rc;
  hipLaunchKernelGGL(kern, dim3(nb), dim3(256), lds, st, args...);
  LAUNCH_CHECK();
  return 0;
}
// the instantiation for ell_plan's (LPR, NB)
template <class Lik, class... Args>
static int ell_launch(int LPR, int NB, Args... args) {
  if (LPR == 4) {
    if (NB == 8) return ell_launch_one<Lik, 4, 8>(args...);
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

int launch_ell_quad(const tgp_model& md, const FlowProg& fp, const double* Y, const double* mu, const double* v, const double* rowp,
                    double* out, double* g_mu, double* g_v, double* g_theta, double* g_rowp, double* ws, hipStream_t st) {
  // nodes in flight per lane: all of the lane's nodes when the checkpoint stack fits (the per-step wave reductions of
  // the shared-parameter partials are then paid once), else fewer
  size_t lds = 0;
  int LPR = 0, NB = 0;
  if (int rc = ell_plan(md, fp, &LPR, &NB, &lds)) return rc;
  const int rows = 256 / LPR;
  const int nb = (md.N + rows - 1) / rows;
  const bool ext = flow_prog_extended(fp.blk, fp.nblk);
  if (int rc = md.lik == TGP_LIK_BERNOULLI
                   ? ell_launch<EllBern>(LPR, NB, ext, nb, lds, st, md, fp, Y, mu, v, rowp, ws, g_mu, g_v, g_rowp)
               : md.lik == TGP_LIK_POISSON
                   ? ell_launch<EllPois>(LPR, NB, ext, nb, lds, st, md, fp, Y, mu, v, rowp, ws, g_mu, g_v, g_rowp)
               : md.lik == TGP_LIK_STUDENT
                   ? ell_launch<EllStudent>(LPR, NB, ext, nb, lds, st, md, fp, Y, mu, v, rowp, ws, g_mu, g_v, g_rowp)
               : md.lik == TGP_LIK_HETERO   // (tgp_ell_hetero_f64 only: mu, v, g_mu, g_v are (2,N))
                   ? ell_launch<EllHetero>(LPR, NB, ext, nb, lds, st, md, fp, Y, mu, v, rowp, ws, g_mu, g_v, g_rowp)
                   : ell_launch<EllGauss>(LPR, NB, ext, nb, lds, st, md, fp, Y, mu, v, rowp, ws, g_mu, g_v, g_rowp))
    return rc;
  hipLaunchKernelGGL(k_sum_parts, dim3((2 + md.P + 31) / 32), dim3(256), 0, st, ws, nb, 2 + md.P, out, g_theta, 2);
  LAUNCH_CHECK();
  return 0;
}

int launch_flow_eval(const tgp_model& md, const FlowProg& fp, const double* f, int S, int N, const double* rowp, double* G, double* dG,
                     double* logdG, hipStream_t st, double* sum_out, double* ws) {
  const size_t total = (size_t)S * N;
  const size_t lds = 3 * (size_t)(md.P + 2) * sizeof(double);
  const unsigned nb = (unsigned)((total + 1023) / 1024);
  double* part = sum_out != nullptr ? ws : (double*)nullptr;
  if (flow_prog_extended(fp.blk, fp.nblk))
    hipLaunchKernelGGL(k_flow_eval<true>, dim3(nb), dim3(256), lds, st, md, fp, f, total, N, rowp, G, dG, logdG, part);
  else
    hipLaunchKernelGGL(k_flow_eval<false>, dim3(nb), dim3(256), lds, st, md, fp, f, total, N, rowp, G, dG, logdG, part);
  LAUNCH_CHECK();
  if (sum_out != nullptr) {
    hipLaunchKernelGGL(k_sum_parts, dim3(1), dim3(256), 0, st, ws, (int)nb, 1, sum_out, (double*)nullptr, 1);
    LAUNCH_CHECK();
  }
  return 0;
}

int launch_predict(const tgp_model& md, const FlowProg& fp, const double* mu, const double* v, const double* rowp, const double* Y,
                   double Y_std, double* m1, double* m2, double* logp, hipStream_t st) {
  const size_t lds = 2 * (size_t)(md.P + 2) * sizeof(double);
  if (md.lik == TGP_LIK_BERNOULLI) {
    if (flow_prog_extended(fp.blk, fp.nblk))
      hipLaunchKernelGGL(k_predict_bern<true>, dim3((md.N + 255) / 256), dim3(256), lds, st, md, fp, mu, v, rowp, Y, m1, m2, logp);
    else
      hipLaunchKernelGGL(k_predict_bern<false>, dim3((md.N + 255) / 256), dim3(256), lds, st, md, fp, mu, v, rowp, Y, m1, m2, logp);
  } else if (md.lik == TGP_LIK_POISSON) {
    if (flow_prog_extended(fp.blk, fp.nblk))
      hipLaunchKernelGGL(k_predict_pois<true>, dim3((md.N + 255) / 256), dim3(256), lds, st, md, fp, mu, v, rowp, Y, m1, m2, logp);
    else
      hipLaunchKernelGGL(k_predict_pois<false>, dim3((md.N + 255) / 256), dim3(256), lds, st, md, fp, mu, v, rowp, Y, m1, m2, logp);
  } else if (md.lik == TGP_LIK_STUDENT) {
    if (flow_prog_extended(fp.blk, fp.nblk))
      hipLaunchKernelGGL(k_predict_student<true>, dim3((md.N + 255) / 256), dim3(256), lds, st, md, fp, mu, v, rowp, Y, Y_std, m1, m2, logp);
    else
      hipLaunchKernelGGL(k_predict_student<false>, dim3((md.N + 255) / 256), dim3(256), lds, st, md, fp, mu, v, rowp, Y, Y_std, m1, m2, logp);
  } else if (flow_prog_extended(fp.blk, fp.nblk))
    hipLaunchKernelGGL(k_predict<true>, dim3((md.N + 255) / 256), dim3(256), lds, st, md, fp, mu, v, rowp, Y, Y_std, m1, m2, logp);
  else
    hipLaunchKernelGGL(k_predict<false>, dim3((md.N + 255) / 256), dim3(256), lds, st, md, fp, mu, v, rowp, Y, Y_std, m1, m2, logp);
  LAUNCH_CHECK();
  return 0;
}

int launch_adam(double* params, const double* grads, double* exp_avg, double* exp_avg_sq, int64_t n, double lr,
                double beta1, double beta2, double eps, double weight_decay, int step, int maximize, hipStream_t st) {
  const double bc1 = 1.0 - pow(beta1, (double)step);
  const double bc2s = sqrt(1.0 - pow(beta2, (double)step));
  hipLaunchKernelGGL(k_adam, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, params, grads, exp_avg, exp_avg_sq, n,
                     lr, beta1, beta2, eps, weight_decay, bc1, bc2s, maximize ? -1.0 : 1.0);
  LAUNCH_CHECK();
  return 0;
}

int launch_adam_dev(double* params, const double* grads, double* exp_avg, double* exp_avg_sq, int64_t n, double lr,
                    double beta1, double beta2, double eps, double weight_decay, int32_t* step_dev, int maximize,
                    hipStream_t st, int64_t n_plain, int64_t skip_off, int64_t skip_n) {
  const int64_t nb = (n - skip_n + 255) / 256 > 0 ? (n - skip_n + 255) / 256 : 1;
  hipLaunchKernelGGL(k_adam_dev, dim3((unsigned)(nb < 512 ? nb : 512)), dim3(256), 0, st, params, grads, exp_avg, exp_avg_sq,
                     n, lr, beta1, beta2, eps, weight_decay, step_dev, maximize ? -1.0 : 1.0, n_plain, log(beta1), log(beta2), skip_off, skip_n);
  LAUNCH_CHECK();
  return 0;
}

}  // namespace tgp
