// tgp_pathwise.hip -- pathwise posterior function draws (tgp_pathwise_coeff_f64, tgp_pathwise_eval_f64, tgp_pathwise_grad_f64): Wilson et al. 2020,
// "Efficiently sampling functions from Gaussian process posteriors", for the whitened sparse GP.
//
// With l = softplus(raw_ls), s2 = softplus(raw_os), K = K_ZZ + jitter I = L L^T, Lam = tril(Lam), frequencies omega (R2, D) of the
// unit-length-scale kernel, amp = sqrt(s2 / R2) and a_j(x) = sum_d omega[j,d] x_d / l_d (in the order of d):
//   phi_j(x) = amp cos a_j(x),   phi_{R2+j}(x) = amp sin a_j(x)                       j < R2
//   nu_s     = L^-T (m + Lam eps_s - L^-1 Phi_Z W_s^T)
//   f0_s(x)  = sum_{j < 2 R2} phi_j(x) W[s,j] + sum_{i < M} k(x, z_i) nu_s[i]
// A draw is the column s of coef (2 R2 + M, S): rows [0, 2 R2) hold amp W[s,j], rows [2 R2, 2 R2 + M) hold nu_s[i].
//
// k_pw_eval is the row kernel.  A workgroup owns 64 data rows (16 of them up to PW_SMALL_N rows) and all S samples.  It walks
// the contraction rows in steps of 16: first R2 / 8 steps of 8 frequencies (one sincos gives the cos row j and the sin row
// R2 + j), then M / 16 steps of 16 inducing points (cov_value).  The [16][rows] operand tile is generated in LDS from the rows'
// scaled coordinates and never reaches HBM; the matching [16][S] coefficient tile is staged beside it; wave w multiplies them on
// the matrix cores for the data rows 16 w .. 16 w + 15 against every tile of 16 samples (with 16 rows: for all rows against
// every fourth sample tile).  A step's rows of omega (or scaled rows of Z) are fetched one step ahead into a two-deep LDS
// buffer and its coefficient tile is loaded before the generation, so no global latency sits in front of the sincos chain.
// A value of F0 depends on its data row and on coef only: the contraction order is fixed and no lane's result depends on
// another data row, so X evaluated at once or in pieces gives the same bits.
// k_pw_grad (tgp_pathwise_grad_f64) is the same walk for d f0_s(x) / d x_d: the derivative of each feature in its place, one set
// of accumulators per input dimension, the dimensions split over grid.y (see the kernel).
//
// Launch sequence of tgp_pathwise_coeff_f64 (one stream, no host sync; operands padded to multiples of 128 in the workspace):
//   K, its factor and L^-1   launch_kzz_factor; status[0]
//   k_pw_prep                L^-1, L^-T and tril(Lam) in zero-padded (MP x MP) images, eps^T (MP x SP), Pt := 0,
//                            coef rows [0, 2 R2) = amp W^T
//   k_pw_eval                Pt (SP x MP) = (Phi_Z W^T)^T: the row kernel on X = Z with the feature rows only
//   G = Lam eps^T, T = L^-1 P   launch_gemm_plain (twice)
//   k_pw_comb                V = m + G - T (zero padded)
//   Nu = L^-T V              launch_gemm_plain
//   k_pw_out                 coef rows [2 R2, 2 R2 + M) = Nu
// Every sum has a fixed order and nothing is accumulated with atomics: two calls on the same input are bit-identical.
#include "tgp_dev.hpp"
#include "tgp_launch.hpp"
#include "tgp_tile.hpp"

namespace tgp {

#define PW_SMALL_N 16384 /* up to here a workgroup owns 16 data rows, above it 64: 256 workgroups of 64 rows fill the chip once */

// LDS stride (f64) of the [16 k][16 NT] coefficient tile: 16 mod 32, the same bank argument as TL_LDN
template <int NT>
struct PwLdc {
  static constexpr int v = NT == 1 ? 16 : 16 * NT + 16;
};

// One step's product: D[s][n] += sum_k Ct[k][s] Ft[k][n] for the wave's row tile (offset rt in Ft) and its NTW sample tiles
// t0, t0 + tstep, ...  (Inline like the staging and the distances: from shared functions k_pw_eval measured 0.5 % slower.)
template <int NTW, int LDN, int LDC>
__device__ __forceinline__ void pw_mma(const double* Ft, const double* Ct, int rt, int t0, int tstep, int lr, int lq, d4* acc) {
#pragma unroll
  for (int kk = 0; kk < 4; ++kk) {
    const double b = Ft[(kk * 4 + lq) * LDN + rt + lr];
#pragma unroll
    for (int u = 0; u < NTW; ++u) acc[u] = TGP_MFMA(Ct[(kk * 4 + lq) * LDC + 16 * (t0 + tstep * u) + lr], b, acc[u]);
  }
}

// F0[s ldf + n] = sum_k feat_k(x_n) coef[k S + s] over the rows k of coef: [0, 2 R2) Fourier features, [2 R2, 2 R2 + M) kernel
// columns (M == 0: none).  NT = tiles of 16 samples (16 NT >= S), DP = padded input dimension, RW = data rows of a workgroup:
//   RW = 64   wave w holds data rows 16 w .. 16 w + 15 against all NT sample tiles
//   RW = 16   (few rows: four times the workgroups, a quarter of the chain each) the four waves share the 16 data rows and
//             wave w holds the sample tiles w, w + 4, ...
// Every element of F0 goes through the same sequence of matrix-core products in both: the same bits.  Rows past N are computed
// on the clamped row N - 1, samples past S and contraction rows past the end meet zero coefficients; none is stored.
template <int NT, int DP, int RW>
__global__ __launch_bounds__(256) void k_pw_eval(int kernel, const double* __restrict__ X, int N, int D, const double* __restrict__ Z,
                                                  int M, const double* __restrict__ raw_ls, const double* __restrict__ raw_os,
                                                  const double* __restrict__ omega, int R2, const double* __restrict__ coef, int S,
                                                  double* __restrict__ F0, size_t ldf) {
  static_assert(RW == 64 || RW == 16, "row tile");
  constexpr int LDC = PwLdc<NT>::v;
  constexpr int LDN = RW == 64 ? TL_LDN : 16;                   // (16: the same bank argument, a tile of one MFMA operand)
  constexpr int NTW = RW == 64 ? NT : (NT >= 4 ? NT / 4 : 1);   // sample tiles of a wave
  __shared__ double Ft[TL_KC * LDN];
  __shared__ double Ct[TL_KC * LDC];
  __shared__ double xsT[DP * RW];    // [d][data row]: scaled rows of X
  __shared__ double omS[2][8 * 16];  // [step parity][frequency of the step][d]: the step's rows of omega
  __shared__ double zS[2][16 * 16];  // [step parity][inducing point of the step][d]: the step's scaled rows of Z
  __shared__ double ils[TL_ILS];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, lr = lane & 15, lq = lane >> 4;
  const size_t n0 = (size_t)blockIdx.x * RW;
  const int pk = tid >> 4, pd = tid & 15;  // staging role: row pk of a step's omega / Z rows, dimension pd
  // the wave's part of the product (wave-uniform): with RW = 16 and one sample tile only wave 0 multiplies
  const int rt = RW == 64 ? 16 * w : 0, t0 = RW == 64 ? 0 : w, tstep = RW == 64 ? 1 : 4;
  const bool mma = RW == 64 || NT >= 4 || w == 0;
  tile_scales(kernel, D, raw_ls, raw_os, ils);
  __syncthreads();
  for (int i = tid; i < DP * RW; i += 256) {
    const int d = i / RW, c = i % RW;
    const size_t n = n0 + c < (size_t)N ? n0 + c : (size_t)N - 1;  // clamped: rows past N are computed and never stored
    xsT[i] = d < D ? X[n * D + d] * ils[d] : 0.0;
  }
  // the first step's rows of omega and of Z; every later step's are fetched one step ahead, under the step before it
  if (tid < 128) omS[0][tid] = pd < D ? omega[(size_t)(pk < R2 ? pk : R2 - 1) * D + pd] : 0.0;
  if (M > 0) zS[0][tid] = pd < D ? Z[(size_t)(pk < M ? pk : M - 1) * D + pd] * ils[pd] : 0.0;
  __syncthreads();
  const Cov cov = tile_cov(kernel, ils);
  d4 acc[NTW];
#pragma unroll
  for (int u = 0; u < NTW; ++u) acc[u] = d4{0.0, 0.0, 0.0, 0.0};
  // coefficient tile roles: element u of a thread is element tid + 256 u of the step's [16][16 NT] tile, row major
  constexpr int CW = 16 * NT, CPT = TL_KC * CW / 256;  // CPT = NT elements per thread
  double cv[CPT];

  // ---- Fourier rows: step = frequencies j0 .. j0 + 7; tile rows 0..7 are their cos rows, 8..15 their sin rows
  {
    // generation role: frequency gk of the step; RW = 64: data rows gc and gc + 32, RW = 16: data row gc, waves 0 and 1 only
    constexpr int FU = RW == 64 ? 2 : 1;
    const int gk = RW == 64 ? tid >> 5 : tid >> 4, gc = RW == 64 ? tid & 31 : tid & 15;
    const bool gen = RW == 64 || tid < 128;
    for (int j0 = 0, par = 0; j0 < R2; j0 += 8, par ^= 1) {
      double pre = 0.0;  // the next step's element of omega (frequencies past R2 clamped: their coefficient rows are zeros)
      if (tid < 128 && pd < D) pre = omega[(size_t)(j0 + 8 + pk < R2 ? j0 + 8 + pk : R2 - 1) * D + pd];
#pragma unroll
      for (int u = 0; u < CPT; ++u) {
        const int idx = tid + 256 * u, r = idx / CW, c = idx - r * CW;
        const int j = j0 + (r & 7);
        const size_t row = (size_t)(r < 8 ? 0 : R2) + j;
        cv[u] = (j < R2 && c < S) ? coef[row * S + c] : 0.0;
      }
      if (gen) {
        double om[DP];
#pragma unroll
        for (int d = 0; d < DP; ++d) om[d] = omS[par][gk * 16 + d];
#pragma unroll
        for (int u = 0; u < FU; ++u) {
          const int c = gc + 32 * u;
          double a = 0.0;
#pragma unroll
          for (int d = 0; d < DP; ++d) a += om[d] * xsT[d * RW + c];  // (dimensions past D add exact zeros)
          double sn, cs;
          sincos(a, &sn, &cs);
          Ft[gk * LDN + c] = cs;
          Ft[(gk + 8) * LDN + c] = sn;
        }
      }
      if (tid < 128) omS[par ^ 1][tid] = pre;  // (read by the next step, behind this step's two barriers)
#pragma unroll
      for (int u = 0; u < CPT; ++u) {
        const int idx = tid + 256 * u, r = idx / CW, c = idx - r * CW;
        Ct[r * LDC + c] = cv[u];
      }
      __syncthreads();
      if (mma) pw_mma<NTW, LDN, LDC>(Ft, Ct, rt, t0, tstep, lr, lq, acc);
      __syncthreads();
    }
  }

  // ---- kernel columns: step = inducing points i0 .. i0 + 15
  {
    const int gk = tid >> 4, gc = tid & 15;  // generation role: inducing point gk of the step, data rows gc + 16 u
    for (int i0 = 0, par = 0; i0 < M; i0 += TL_KC, par ^= 1) {
      double pre = 0.0;  // the next step's element of Z (inducing points past M clamped: their coefficient rows are zeros)
      if (pd < D) pre = Z[(size_t)(i0 + TL_KC + pk < M ? i0 + TL_KC + pk : M - 1) * D + pd] * ils[pd];
#pragma unroll
      for (int u = 0; u < CPT; ++u) {
        const int idx = tid + 256 * u, r = idx / CW, c = idx - r * CW;
        cv[u] = (i0 + r < M && c < S) ? coef[((size_t)2 * R2 + i0 + r) * S + c] : 0.0;
      }
      {
        double z[DP];
#pragma unroll
        for (int d = 0; d < DP; ++d) z[d] = zS[par][gk * 16 + d];
#pragma unroll
        for (int u = 0; u < RW / 16; ++u) {
          const int c = gc + 16 * u;
          double d2 = 0.0;
#pragma unroll
          for (int d = 0; d < DP; ++d) {  // (dimensions past D hold zeros on both sides: they add exact zeros)
            const double q = xsT[d * RW + c] - z[d];
            d2 += q * q;
          }
          Ft[gk * LDN + c] = cov_value(cov, d2);
        }
      }
      zS[par ^ 1][tid] = pre;  // (read by the next step, behind this step's two barriers)
#pragma unroll
      for (int u = 0; u < CPT; ++u) {
        const int idx = tid + 256 * u, r = idx / CW, c = idx - r * CW;
        Ct[r * LDC + c] = cv[u];
      }
      __syncthreads();
      if (mma) pw_mma<NTW, LDN, LDC>(Ft, Ct, rt, t0, tstep, lr, lq, acc);
      __syncthreads();
    }
  }

  const size_t n = n0 + rt + lr;
  if (mma && n < (size_t)N) {
#pragma unroll
    for (int u = 0; u < NTW; ++u)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int s = 16 * (t0 + tstep * u) + lq + 4 * r;
        if (s < S) F0[(size_t)s * ldf + n] = acc[u][r];
      }
  }
}

// Dimensions of a workgroup of k_pw_grad: one set of NTW accumulator tiles per dimension, 16 tiles (128 registers) at the most
template <int NT, int DP, int RW>
struct PwDg {
  static constexpr int ntw = RW == 64 ? NT : (NT >= 4 ? NT / 4 : 1);
  static constexpr int v = 16 / ntw < DP ? 16 / ntw : DP;
};

// dF0[(d S + s) ldf + n] = d f0_s(x_n) / d x_nd = sum_k dfeat_k(x_n) / dx_nd coef[k S + s]: k_pw_eval's walk over the rows of
// coef with the derivative of each feature in its place.  With w_jd = omega[j,d] / l_d and q_d = (x_d - z_id) / l_d:
//   d cos a_j / dx_d = -sin a_j w_jd     d sin a_j / dx_d = cos a_j w_jd     d k(x, z_i) / dx_d = -k_g(d2) q_d / l_d
// A workgroup owns RW data rows, all S samples and the DG dimensions d0 .. d0 + DG - 1 of blockIdx.y (D x NT accumulator tiles
// do not fit in registers: the dimensions are split over the grid).  Per step the base quantities -- sincos of the step's 8
// frequencies, k_g of its 16 inducing points -- are generated once into registers; for each dimension of the group they are
// scaled into one of two operand tiles (the other one is still being multiplied) and multiplied against the step's coefficient
// tile, which is staged once.  One barrier per dimension and one at the end of the step.  (x - z) is formed directly from the
// scaled rows.  Tilings, prefetch and roles are k_pw_eval's; every element goes through the same products in the same order
// under both tilings and whatever the group: an element depends on its row of X, its d and coef only.
template <int NT, int DP, int RW>
__global__ __launch_bounds__(256) void k_pw_grad(int kernel, const double* __restrict__ X, int N, int D, const double* __restrict__ Z,
                                                  int M, const double* __restrict__ raw_ls, const double* __restrict__ raw_os,
                                                  const double* __restrict__ omega, int R2, const double* __restrict__ coef, int S,
                                                  double* __restrict__ dF0, size_t ldf) {
  static_assert(RW == 64 || RW == 16, "row tile");
  constexpr int LDC = PwLdc<NT>::v;
  constexpr int LDN = RW == 64 ? TL_LDN : 16;
  constexpr int NTW = PwDg<NT, DP, RW>::ntw;
  constexpr int DG = PwDg<NT, DP, RW>::v;
  __shared__ double Ft[2][TL_KC * LDN];  // [dimension parity]: the operand tile of one dimension
  __shared__ double Ct[TL_KC * LDC];
  __shared__ double xsT[DP * RW];
  __shared__ double omS[2][8 * 16];
  __shared__ double zS[2][16 * 16];
  __shared__ double ils[TL_ILS];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, lr = lane & 15, lq = lane >> 4;
  const size_t n0 = (size_t)blockIdx.x * RW;
  const int d0 = blockIdx.y * DG, dn = D - d0 < DG ? D - d0 : DG;  // the group's dimensions d0 .. d0 + dn - 1
  const int pk = tid >> 4, pd = tid & 15;
  const int rt = RW == 64 ? 16 * w : 0, t0 = RW == 64 ? 0 : w, tstep = RW == 64 ? 1 : 4;
  const bool mma = RW == 64 || NT >= 4 || w == 0;
  tile_scales(kernel, D, raw_ls, raw_os, ils);
  __syncthreads();
  for (int i = tid; i < DP * RW; i += 256) {
    const int d = i / RW, c = i % RW;
    const size_t n = n0 + c < (size_t)N ? n0 + c : (size_t)N - 1;  // clamped: rows past N are computed and never stored
    xsT[i] = d < D ? X[n * D + d] * ils[d] : 0.0;
  }
  if (tid < 128) omS[0][tid] = pd < D ? omega[(size_t)(pk < R2 ? pk : R2 - 1) * D + pd] : 0.0;
  zS[0][tid] = pd < D ? Z[(size_t)(pk < M ? pk : M - 1) * D + pd] * ils[pd] : 0.0;
  __syncthreads();
  const Cov cov = tile_cov(kernel, ils);
  d4 acc[DG][NTW];
#pragma unroll
  for (int dd = 0; dd < DG; ++dd)
#pragma unroll
    for (int u = 0; u < NTW; ++u) acc[dd][u] = d4{0.0, 0.0, 0.0, 0.0};
  constexpr int CW = 16 * NT, CPT = TL_KC * CW / 256;
  double cv[CPT];

  // ---- Fourier rows: tile rows 0..7 meet the cos coefficients (-sin a w_jd), rows 8..15 the sin coefficients (cos a w_jd)
  {
    constexpr int FU = RW == 64 ? 2 : 1;
    const int gk = RW == 64 ? tid >> 5 : tid >> 4, gc = RW == 64 ? tid & 31 : tid & 15;
    const bool gen = RW == 64 || tid < 128;
    for (int j0 = 0, par = 0; j0 < R2; j0 += 8, par ^= 1) {
      double pre = 0.0;
      if (tid < 128 && pd < D) pre = omega[(size_t)(j0 + 8 + pk < R2 ? j0 + 8 + pk : R2 - 1) * D + pd];
#pragma unroll
      for (int u = 0; u < CPT; ++u) {
        const int idx = tid + 256 * u, r = idx / CW, c = idx - r * CW;
        const int j = j0 + (r & 7);
        const size_t row = (size_t)(r < 8 ? 0 : R2) + j;
        cv[u] = (j < R2 && c < S) ? coef[row * S + c] : 0.0;
      }
      double sn[FU] = {}, cs[FU] = {};
      if (gen) {
        double om[DP];
#pragma unroll
        for (int d = 0; d < DP; ++d) om[d] = omS[par][gk * 16 + d];
#pragma unroll
        for (int u = 0; u < FU; ++u) {
          const int c = gc + 32 * u;
          double a = 0.0;
#pragma unroll
          for (int d = 0; d < DP; ++d) a += om[d] * xsT[d * RW + c];  // (dimensions past D add exact zeros)
          sincos(a, &sn[u], &cs[u]);
        }
      }
#pragma unroll
      for (int dd = 0; dd < DG; ++dd) {
        if (dd < dn) {  // (uniform over the workgroup)
          double* F = Ft[dd & 1];
          if (gen) {
            const double wd = omS[par][gk * 16 + d0 + dd] * ils[d0 + dd];
#pragma unroll
            for (int u = 0; u < FU; ++u) {
              const int c = gc + 32 * u;
              F[gk * LDN + c] = -(sn[u] * wd);
              F[(gk + 8) * LDN + c] = cs[u] * wd;
            }
          }
          if (dd == 0) {
            if (tid < 128) omS[par ^ 1][tid] = pre;  // (read by the next step, behind this step's barriers)
#pragma unroll
            for (int u = 0; u < CPT; ++u) {
              const int idx = tid + 256 * u, r = idx / CW, c = idx - r * CW;
              Ct[r * LDC + c] = cv[u];
            }
          }
          __syncthreads();
          if (mma) pw_mma<NTW, LDN, LDC>(F, Ct, rt, t0, tstep, lr, lq, acc[dd]);
        }
      }
      __syncthreads();
    }
  }

  // ---- kernel columns: tile row gk = -k_g(d2) q_d / l_d of the step's inducing point gk
  {
    const int gk = tid >> 4, gc = tid & 15;
    for (int i0 = 0, par = 0; i0 < M; i0 += TL_KC, par ^= 1) {
      double pre = 0.0;
      if (pd < D) pre = Z[(size_t)(i0 + TL_KC + pk < M ? i0 + TL_KC + pk : M - 1) * D + pd] * ils[pd];
#pragma unroll
      for (int u = 0; u < CPT; ++u) {
        const int idx = tid + 256 * u, r = idx / CW, c = idx - r * CW;
        cv[u] = (i0 + r < M && c < S) ? coef[((size_t)2 * R2 + i0 + r) * S + c] : 0.0;
      }
      double kg[RW / 16];
      {
        double z[DP];
#pragma unroll
        for (int d = 0; d < DP; ++d) z[d] = zS[par][gk * 16 + d];
#pragma unroll
        for (int u = 0; u < RW / 16; ++u) {
          const int c = gc + 16 * u;
          double d2 = 0.0;
#pragma unroll
          for (int d = 0; d < DP; ++d) {  // (dimensions past D hold zeros on both sides: they add exact zeros)
            const double q = xsT[d * RW + c] - z[d];
            d2 += q * q;
          }
          kg[u] = cov_gweight(cov, d2);
        }
      }
#pragma unroll
      for (int dd = 0; dd < DG; ++dd) {
        if (dd < dn) {  // (uniform over the workgroup)
          double* F = Ft[dd & 1];
          const double zd = zS[par][gk * 16 + d0 + dd], il = ils[d0 + dd];
#pragma unroll
          for (int u = 0; u < RW / 16; ++u) {
            const int c = gc + 16 * u;
            const double q = xsT[(d0 + dd) * RW + c] - zd;
            F[gk * LDN + c] = -((kg[u] * q) * il);
          }
          if (dd == 0) {
            zS[par ^ 1][tid] = pre;  // (read by the next step, behind this step's barriers)
#pragma unroll
            for (int u = 0; u < CPT; ++u) {
              const int idx = tid + 256 * u, r = idx / CW, c = idx - r * CW;
              Ct[r * LDC + c] = cv[u];
            }
          }
          __syncthreads();
          if (mma) pw_mma<NTW, LDN, LDC>(F, Ct, rt, t0, tstep, lr, lq, acc[dd]);
        }
      }
      __syncthreads();
    }
  }

  const size_t n = n0 + rt + lr;
  if (mma && n < (size_t)N) {
#pragma unroll
    for (int dd = 0; dd < DG; ++dd)
      if (dd < dn) {
        double* const P = dF0 + (size_t)(d0 + dd) * S * ldf;
#pragma unroll
        for (int u = 0; u < NTW; ++u)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int s = 16 * (t0 + tstep * u) + lq + 4 * r;
            if (s < S) P[(size_t)s * ldf + n] = acc[dd][u][r];
          }
      }
  }
}

// The padded operands of the M x M chain and the feature rows of coef.  Thread e serves element e of every image it is inside.
__global__ __launch_bounds__(256) void k_pw_prep(const double* __restrict__ Lam, const double* __restrict__ Linv,
                                                  const double* __restrict__ eps, const double* __restrict__ W,
                                                  const double* __restrict__ raw_os, int M, int MP, int S, int SP, int R2,
                                                  double* __restrict__ LinvP, double* __restrict__ LinvTP, double* __restrict__ LamP,
                                                  double* __restrict__ Pt, double* __restrict__ EpsT, double* __restrict__ coef) {
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e < (size_t)MP * MP) {
    const int row = (int)(e / MP), col = (int)(e % MP);
    const bool in = row < M && col <= row;
    LinvP[e] = in ? Linv[(size_t)row * M + col] : 0.0;
    LamP[e] = in ? Lam[(size_t)row * M + col] : 0.0;
    LinvTP[e] = (col < M && row <= col) ? Linv[(size_t)col * M + row] : 0.0;
  }
  if (e < (size_t)MP * SP) {
    const int i = (int)(e / SP), s = (int)(e % SP);
    EpsT[e] = (i < M && s < S) ? eps[(size_t)s * M + i] : 0.0;
    Pt[e] = 0.0;
  }
  if (e < (size_t)2 * R2 * S) {
    const size_t j = e / S, s = e % S;
    const double amp = sqrt(softplus_d(raw_os[0]) / (double)R2);
    coef[e] = amp * W[s * ((size_t)2 * R2) + j];
  }
}

// V = m + G - T on the first M rows and S columns, zeros elsewhere
__global__ __launch_bounds__(256) void k_pw_comb(const double* __restrict__ mvec, const double* __restrict__ G,
                                                  const double* __restrict__ T, int M, int S, int SP, double* __restrict__ V) {
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  const int i = (int)(e / SP), s = (int)(e % SP);
  V[e] = (i < M && s < S) ? (mvec[i] + G[e]) - T[e] : 0.0;
}

// coef rows [2 R2, 2 R2 + M) = Nu
__global__ __launch_bounds__(256) void k_pw_out(const double* __restrict__ Nu, int M, int S, int SP, int R2, double* __restrict__ coef) {
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (size_t)M * S) return;
  const size_t i = e / S, s = e % S;
  coef[((size_t)2 * R2 + i) * S + s] = Nu[i * SP + s];
}

// ---- host side ----------------------------------------------------------------------------------------------------
namespace {
struct PwPlan : Layout {
  int MP, SP;
  KzzSections kzz;
  size_t LinvP, LinvTP, LamP, Pt, EpsT, G, T, V, Nu;
};
bool pw_limits(int N, int D, int M, int R2, int S) {
  return N >= 1 && inducing_limits(M, D) && R2 >= 1 && R2 <= TGP_PATHWISE_MAX_R2 && S >= 1 && S <= TGP_PATHWISE_MAX_S;
}
bool pw_plan(PwPlan& p, int N, int D, int M, int R2, int S) {
  if (!pw_limits(N, D, M, R2, S)) return false;
  p.MP = (int)rup((size_t)M, 128);
  p.SP = (int)rup((size_t)S, 128);
  const size_t pp = (size_t)p.MP * p.MP, ps = (size_t)p.MP * p.SP;
  p.kzz.take(p, M);
  p.LinvP = p.take(pp);
  p.LinvTP = p.take(pp);
  p.LamP = p.take(pp);
  p.Pt = p.take(ps);
  p.EpsT = p.take(ps);
  p.G = p.take(ps);
  p.T = p.take(ps);
  p.V = p.take(ps);
  p.Nu = p.take(ps);
  return true;
}

template <int NT, int RW>
int run_eval_rw(int kernel, const double* X, int N, int D, const double* Z, int M, const double* raw_ls, const double* raw_os,
                const double* omega, int R2, const double* coef, int S, double* F0, size_t ldf, hipStream_t st) {
  const dim3 grid((unsigned)(((size_t)N + RW - 1) / RW)), block(256);
  dispatch_dp(D, [&](auto dp) {
    hipLaunchKernelGGL((k_pw_eval<NT, decltype(dp)::value, RW>), grid, block, 0, st, kernel, X, N, D, Z, M, raw_ls, raw_os, omega, R2,
                       coef, S, F0, ldf);
  });
  LAUNCH_CHECK();
  return 0;
}
// up to PW_SMALL_N rows the 16-row workgroups (a constant: the choice must not depend on the device; the bits do not depend on it)
template <int NT>
int run_eval_nt(int kernel, const double* X, int N, int D, const double* Z, int M, const double* raw_ls, const double* raw_os,
                const double* omega, int R2, const double* coef, int S, double* F0, size_t ldf, hipStream_t st) {
  if (N <= PW_SMALL_N) return run_eval_rw<NT, 16>(kernel, X, N, D, Z, M, raw_ls, raw_os, omega, R2, coef, S, F0, ldf, st);
  return run_eval_rw<NT, 64>(kernel, X, N, D, Z, M, raw_ls, raw_os, omega, R2, coef, S, F0, ldf, st);
}
// the row kernel with the fewest sample tiles that hold S
int run_eval(int kernel, const double* X, int N, int D, const double* Z, int M, const double* raw_ls, const double* raw_os,
             const double* omega, int R2, const double* coef, int S, double* F0, size_t ldf, hipStream_t st) {
  if (S <= 16) return run_eval_nt<1>(kernel, X, N, D, Z, M, raw_ls, raw_os, omega, R2, coef, S, F0, ldf, st);
  if (S <= 64) return run_eval_nt<4>(kernel, X, N, D, Z, M, raw_ls, raw_os, omega, R2, coef, S, F0, ldf, st);
  if (S <= 128) return run_eval_nt<8>(kernel, X, N, D, Z, M, raw_ls, raw_os, omega, R2, coef, S, F0, ldf, st);
  return run_eval_nt<16>(kernel, X, N, D, Z, M, raw_ls, raw_os, omega, R2, coef, S, F0, ldf, st);
}

// k_pw_grad under the same choices: the fewest sample tiles that hold S, the 16-row workgroups up to PW_SMALL_N rows; the
// dimensions in groups of PwDg over grid.y
template <int NT, int RW>
int run_grad_rw(int kernel, const double* X, int N, int D, const double* Z, int M, const double* raw_ls, const double* raw_os,
                const double* omega, int R2, const double* coef, int S, double* dF0, size_t ldf, hipStream_t st) {
  dispatch_dp(D, [&](auto dp) {
    constexpr int DP = decltype(dp)::value, DG = PwDg<NT, DP, RW>::v;
    const dim3 grid((unsigned)(((size_t)N + RW - 1) / RW), (unsigned)((D + DG - 1) / DG)), block(256);
    hipLaunchKernelGGL((k_pw_grad<NT, DP, RW>), grid, block, 0, st, kernel, X, N, D, Z, M, raw_ls, raw_os, omega, R2, coef, S, dF0,
                       ldf);
  });
  LAUNCH_CHECK();
  return 0;
}
template <int NT>
int run_grad_nt(int kernel, const double* X, int N, int D, const double* Z, int M, const double* raw_ls, const double* raw_os,
                const double* omega, int R2, const double* coef, int S, double* dF0, size_t ldf, hipStream_t st) {
  if (N <= PW_SMALL_N) return run_grad_rw<NT, 16>(kernel, X, N, D, Z, M, raw_ls, raw_os, omega, R2, coef, S, dF0, ldf, st);
  return run_grad_rw<NT, 64>(kernel, X, N, D, Z, M, raw_ls, raw_os, omega, R2, coef, S, dF0, ldf, st);
}
}  // namespace

size_t pathwise_workspace_bytes(int N, int D, int M, int R2, int S) {
  PwPlan p;
  return pw_plan(p, N, D, M, R2, S) ? p.bytes() : 0;
}

int launch_pathwise_eval(int kernel, const double* X, int N, int D, const double* Z, int M, const double* raw_ls,
                         const double* raw_os, const double* omega, int R2, const double* coef, int S, double* F0, hipStream_t st) {
  if (!pw_limits(N, D, M, R2, S)) return TGP_E_UNSUPPORTED;  // (tgp_pathwise_eval_f64 has named the limits)
  return run_eval(kernel, X, N, D, Z, M, raw_ls, raw_os, omega, R2, coef, S, F0, (size_t)N, st);
}

int launch_pathwise_grad(int kernel, const double* X, int N, int D, const double* Z, int M, const double* raw_ls,
                         const double* raw_os, const double* omega, int R2, const double* coef, int S, double* dF0, hipStream_t st) {
  if (!pw_limits(N, D, M, R2, S)) return TGP_E_UNSUPPORTED;  // (tgp_pathwise_grad_f64 has named the limits)
  const size_t ldf = (size_t)N;
  if (S <= 16) return run_grad_nt<1>(kernel, X, N, D, Z, M, raw_ls, raw_os, omega, R2, coef, S, dF0, ldf, st);
  if (S <= 64) return run_grad_nt<4>(kernel, X, N, D, Z, M, raw_ls, raw_os, omega, R2, coef, S, dF0, ldf, st);
  if (S <= 128) return run_grad_nt<8>(kernel, X, N, D, Z, M, raw_ls, raw_os, omega, R2, coef, S, dF0, ldf, st);
  return run_grad_nt<16>(kernel, X, N, D, Z, M, raw_ls, raw_os, omega, R2, coef, S, dF0, ldf, st);
}

int launch_pathwise_coeff(const tgp_model& md, const double* omega, int R2, const double* W, const double* eps, int S, double* coef,
                          int32_t* status, void* workspace, size_t workspace_bytes, hipStream_t st) {
  PwPlan p;
  if (!pw_plan(p, 1, md.D, md.M, R2, S)) return TGP_E_UNSUPPORTED;  // (tgp_pathwise_coeff_f64 has named the limits)
  double* ws;
  if (int rc = open_workspace("tgp_pathwise_coeff_f64", "tgp_pathwise_workspace_bytes", workspace, workspace_bytes, p.total, &ws))
    return rc;
  const int D = md.D, M = md.M, MP = p.MP, SP = p.SP;
  const size_t pp = (size_t)MP * MP, ps = (size_t)MP * SP, fs = (size_t)2 * R2 * S;
  const size_t most = pp > ps ? (pp > fs ? pp : fs) : (ps > fs ? ps : fs);
  if (int rc = p.kzz.factor(md, ws, status, st)) return rc;
  hipLaunchKernelGGL(k_pw_prep, dim3((unsigned)((most + 255) / 256)), dim3(256), 0, st, md.Lam, ws + p.kzz.Linv, eps, W, md.raw_os, M, MP,
                     S, SP, R2, ws + p.LinvP, ws + p.LinvTP, ws + p.LamP, ws + p.Pt, ws + p.EpsT, coef);
  LAUNCH_CHECK();
  if (int rc = run_eval(md.kernel, md.Z, M, D, md.Z, 0, md.raw_ls, md.raw_os, omega, R2, coef, S, ws + p.Pt, (size_t)MP, st)) return rc;
  if (int rc = launch_gemm_plain(false, false, 0, MP, SP, MP, 1.0, ws + p.LamP, MP, ws + p.EpsT, SP, 0.0, ws + p.G, SP, st)) return rc;
  if (int rc = launch_gemm_plain(false, true, 0, MP, SP, MP, 1.0, ws + p.LinvP, MP, ws + p.Pt, MP, 0.0, ws + p.T, SP, st)) return rc;
  hipLaunchKernelGGL(k_pw_comb, dim3((unsigned)(ps / 256)), dim3(256), 0, st, md.m, ws + p.G, ws + p.T, M, S, SP, ws + p.V);
  LAUNCH_CHECK();
  if (int rc = launch_gemm_plain(false, false, 0, MP, SP, MP, 1.0, ws + p.LinvTP, MP, ws + p.V, SP, 0.0, ws + p.Nu, SP, st)) return rc;
  hipLaunchKernelGGL(k_pw_out, dim3((unsigned)(((size_t)M * S + 255) / 256)), dim3(256), 0, st, ws + p.Nu, M, S, SP, R2, coef);
  LAUNCH_CHECK();
  return 0;
}

}  // namespace tgp
