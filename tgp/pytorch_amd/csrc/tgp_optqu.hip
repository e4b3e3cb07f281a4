// tgp_optqu.hip -- closed-form optimal q(u) of the Gaussian likelihood (tgp_optimal_qu_f64, tgp_kxxk_f64) and, on the same chain with
// per-row pseudo-observations, the natural-gradient step of q(u) for any likelihood (tgp_natgrad_qu_f64, tgp_kxwxk_f64: below).
//
// Whitened q(u) = N(m, Lam Lam^T), zero prior mean, sigma^2 = exp(log_var_noise), c = N_total / MB (model->scale).  With
// K = K_ZZ + jitter I = L L^T the maximiser of the Gaussian ELBO over (m, Lam) -- the q(u) behind Titsias' collapsed bound -- is
//   C = K_ZX K_XZ (M x M),   b = K_ZX y (M)
//   B = I + (c / sigma^2) L^-1 C L^-T,   S* = B^-1 = Lam* Lam*^T,   m* = (c / sigma^2) S* L^-1 b
// and a LOWER factor of B^-1 comes from one factorisation of the index-reversed matrix: J B J = L' L'^T gives
// B^-1 = (J L'^-T J)(J L'^-T J)^T with J L'^-T J lower triangular and a positive diagonal.
//
// Launch sequence of tgp_optimal_qu_f64 (one stream, no host sync):
//   K, its factor and L^-1     the existing launchers (launch_kernel_matrix, launch_cholesky / launch_big_cholesky); status[0]
//   k_kxxk                     per (64 x 64 tile of the lower block triangle, row group): the partial tile of C on the matrix
//                              cores, both operand tiles of K_ZX generated in LDS from the scaled rows (never in HBM); the
//                              partial of b rides on tile column 0
//   k_kxxk_fin                 the groups summed in order, C mirrored to the upper triangle, b finished
//   k_optqu_pad                L^-1 and C into zero-padded (MP x MP) images, MP a multiple of 128
//   T = L^-1 C,  Phi = T L^-T  launch_gemm_plain (twice)
//   k_optqu_b                  J B J from the lower triangle of Phi (exactly symmetric), sigma^2 read on the device
//   L', L'^-1                  the existing launchers again, on status words of the workspace
//   k_optqu_lam                Lam* = J L'^-T J (zeros above the diagonal) and its transpose
//   k_optqu_mv (three times)   v1 = L^-1 b,  v2 = Lam*^T v1,  m* = (c / sigma^2) Lam* v2
// The row groups' size is a function of N and M alone, every sum has a fixed order and nothing is accumulated with atomics:
// two runs on the same input are bit-identical, on any device.
#include "tgp_dev.hpp"
#include "tgp_launch.hpp"
#include "tgp_tile.hpp"

namespace tgp {

#define OQ_MIN_G 128 /* smallest row group                                                                                    */
#define OQ_WGS 1024  /* workgroups k_kxxk aims at when it splits the rows (a constant: the split must not depend on the device) */

// Partial tile (ti, tj) of C = K_ZX K_XZ over the rows [g G, min(N, (g + 1) G)) and, on tile column 0, the partial of b = K_ZX y.
// Per step of 16 rows thread (gk, gc) evaluates K(z_i, x_n) for row n = gk of the step against the inducing points gc + 16 u of
// both tile sides into the [16 n][64 i] LDS operand tiles (a diagonal tile has one); rows past the group's end give exact
// zeros.  Wave w holds rows 16 w .. 16 w + 15 of the tile against all 64 columns in four accumulators (k_cov_sigma's
// layout).  Inducing points past M are clamped to M - 1: their rows and columns are computed and never read by k_kxxk_fin.
//
// The weighted instantiation (RW = RowWeights) forms C = K_ZX diag(w) K_XZ and b = K_ZX r: the A operand of every MFMA is scaled
// by its row's weight as it is read from LDS, the B operand is not, so a diagonal tile still needs one operand tile and w may
// have any sign.  The 16 weights of a step sit in the first words of `red`, which is otherwise idle until the loop has ended.
// The unweighted instantiation (RW = NoWeights, an empty trailing argument) is the code it was.
struct NoWeights {};
struct RowWeights {
  // sites == 0: w_n = a[n], r_n = b[n] (b may be null: no b).  sites == 1, the sites of a natural-gradient step from the
  // adjoints of c ELL: lambda_n = max(-2 v_bar_n, floor) (a NaN floor: no clamp), r_n = mu_bar_n + lambda_n mu_n, with
  // a = v_bar, b = mu_bar.
  const double *a, *b, *mu;
  double floor;
  int sites;
};

template <int DP, class RW>
__global__ __launch_bounds__(256) void k_kxxk(int kernel, const double* __restrict__ X, int N, const double* __restrict__ Z, int M,
                                               int D, const double* __restrict__ raw_ls, const double* __restrict__ raw_os,
                                               const double* __restrict__ Y, int G, int ntile, int nti, double* __restrict__ part,
                                               double* __restrict__ bpart, RW rw) {
  constexpr bool W = !std::is_empty<RW>::value;
  __shared__ double Ki[TL_KC * TL_LDN], Kj[TL_KC * TL_LDN];
  __shared__ double ziT[DP * TL_T], zjT[DP * TL_T];  // [d][inducing point]: scaled rows of Z
  __shared__ double red[16 * TL_T];
  __shared__ double ils[TL_ILS];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, lr = lane & 15, lq = lane >> 4;
  const int t = blockIdx.x, g = blockIdx.y;
  int ti, tj;
  tile_lower(t, ti, tj);
  const int i0 = ti * TL_T, j0 = tj * TL_T;
  bool has_r = Y != nullptr;
  if constexpr (W) has_r = rw.b != nullptr;
  const bool diag = ti == tj, want_b = tj == 0 && has_r && bpart != nullptr;
  tile_scales(kernel, D, raw_ls, raw_os, ils);
  __syncthreads();
  for (int i = tid; i < DP * TL_T; i += 256) {
    const int d = i >> 6, c = i & 63;
    const int mi = i0 + c < M ? i0 + c : M - 1, mj = j0 + c < M ? j0 + c : M - 1;
    ziT[i] = d < D ? Z[(size_t)mi * D + d] * ils[d] : 0.0;
    zjT[i] = d < D ? Z[(size_t)mj * D + d] * ils[d] : 0.0;
  }
  __syncthreads();
  const Cov cov = tile_cov(kernel, ils);
  const int gk = tid >> 4, gc = tid & 15;  // generation role: row gk of the step, inducing points gc + 16 u
  const int n_begin = g * G, n_end = n_begin + G < N ? n_begin + G : N;
  const double* Bt = diag ? Ki : Kj;
  d4 acc[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) acc[c] = d4{0.0, 0.0, 0.0, 0.0};
  double bp[4] = {0.0, 0.0, 0.0, 0.0};
  for (int n0 = n_begin; n0 < n_end; n0 += TL_KC) {
    {
      const int n = n0 + gk;
      const bool valid = n < n_end;
      const int nc = valid ? n : N - 1;  // clamped: the row is read and its covariances are replaced by zeros
      double x[DP];
#pragma unroll
      for (int d = 0; d < DP; ++d) x[d] = d < D ? X[(size_t)nc * D + d] * ils[d] : 0.0;
      double yv = 0.0;
      if constexpr (W) {
        double lam = 0.0;  // (rows past the group's end weigh nothing)
        if (valid) {
          if (rw.sites) {
            lam = -2.0 * rw.a[nc];
            if (lam < rw.floor) lam = rw.floor;
            if (want_b) yv = rw.b[nc] + lam * rw.mu[nc];
          } else {
            lam = rw.a[nc];
            if (want_b) yv = rw.b[nc];
          }
        }
        if (gc == 0) red[gk] = lam;
      } else {
        yv = (want_b && valid) ? Y[nc] : 0.0;
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int c = gc + 16 * u;
        double d2 = 0.0;
#pragma unroll
        for (int d = 0; d < DP; ++d) {  // (dimensions past D hold zeros on both sides: they add exact zeros)
          const double q = ziT[d * TL_T + c] - x[d];
          d2 += q * q;
        }
        const double kv = valid ? cov_value(cov, d2) : 0.0;
        Ki[gk * TL_LDN + c] = kv;
        bp[u] += kv * yv;
      }
      if (!diag) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int c = gc + 16 * u;
          double d2 = 0.0;
#pragma unroll
          for (int d = 0; d < DP; ++d) {
            const double q = zjT[d * TL_T + c] - x[d];
            d2 += q * q;
          }
          Kj[gk * TL_LDN + c] = valid ? cov_value(cov, d2) : 0.0;
        }
      }
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      double a = Ki[(kk * 4 + lq) * TL_LDN + 16 * w + lr];
      if constexpr (W) a *= red[kk * 4 + lq];
#pragma unroll
      for (int c = 0; c < 4; ++c) acc[c] = TGP_MFMA(a, Bt[(kk * 4 + lq) * TL_LDN + 16 * c + lr], acc[c]);
    }
    __syncthreads();
  }
  double* pt = part + ((size_t)g * ntile + t) * (TL_T * TL_T);
#pragma unroll
  for (int c = 0; c < 4; ++c)
#pragma unroll
    for (int r = 0; r < 4; ++r) pt[(16 * w + lq + 4 * r) * TL_T + 16 * c + lr] = acc[c][r];
  if (want_b) {  // (uniform over the workgroup)
#pragma unroll
    for (int u = 0; u < 4; ++u) red[gk * TL_T + gc + 16 * u] = bp[u];
    __syncthreads();
    if (tid < TL_T) {
      double s = 0.0;
      for (int k = 0; k < 16; ++k) s += red[k * TL_T + tid];
      bpart[((size_t)g * nti + ti) * TL_T + tid] = s;
    }
  }
}

// C tile (ti, tj) = the groups' partial tiles summed in the order g = 0, 1, ..., written as (i, j) and mirrored as (j, i); a
// diagonal tile writes element (r, c) from the value summed for (max(r, c), min(r, c)): C[i][j] == C[j][i] bit for bit.  Tile
// column 0 finishes b the same way.  Rows and columns past M are masked.
__global__ __launch_bounds__(256) void k_kxxk_fin(const double* __restrict__ part, const double* __restrict__ bpart, int ngroup,
                                                   int ntile, int nti, int M, double* __restrict__ C, int ldc, double* __restrict__ b) {
  __shared__ double buf[TL_T * TL_LDT];
  const int tid = threadIdx.x, t = blockIdx.x;
  int ti, tj;
  tile_lower(t, ti, tj);
  const int i0 = ti * TL_T, j0 = tj * TL_T;
  for (int e = tid; e < TL_T * TL_T; e += 256) {
    double s = 0.0;
    for (int g = 0; g < ngroup; ++g) s += part[((size_t)g * ntile + t) * (TL_T * TL_T) + e];
    buf[(e >> 6) * TL_LDT + (e & 63)] = s;
  }
  if (tj == 0 && b != nullptr && bpart != nullptr && tid < TL_T) {
    double s = 0.0;
    for (int g = 0; g < ngroup; ++g) s += bpart[((size_t)g * nti + ti) * TL_T + tid];
    if (i0 + tid < M) b[i0 + tid] = s;
  }
  __syncthreads();
  if (ti != tj) {
    for (int e = tid; e < TL_T * TL_T; e += 256) {
      const int r = e >> 6, c = e & 63;
      if (i0 + r < M && j0 + c < M) C[(size_t)(i0 + r) * ldc + j0 + c] = buf[r * TL_LDT + c];
    }
    for (int e = tid; e < TL_T * TL_T; e += 256) {
      const int c = e >> 6, r = e & 63;
      if (i0 + r < M && j0 + c < M) C[(size_t)(j0 + c) * ldc + i0 + r] = buf[r * TL_LDT + c];
    }
  } else {
    for (int e = tid; e < TL_T * TL_T; e += 256) {
      const int r = e >> 6, c = e & 63;
      const int hi = r > c ? r : c, lo = r > c ? c : r;
      if (i0 + r < M && i0 + c < M) C[(size_t)(i0 + r) * ldc + i0 + c] = buf[hi * TL_LDT + lo];
    }
  }
}

// L^-1 (its lower triangle) and C in their zero-padded (MP x MP) images; the second factorisation's status words zeroed
__global__ __launch_bounds__(256) void k_optqu_pad(const double* __restrict__ Linv, const double* __restrict__ C, int M, int MP,
                                                    double* __restrict__ LinvP, double* __restrict__ CP, int32_t* __restrict__ st2) {
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  const int row = (int)(e / MP), col = (int)(e % MP);
  const size_t s = (size_t)row * M + col;
  LinvP[e] = (row < M && col <= row) ? Linv[s] : 0.0;
  CP[e] = (row < M && col < M) ? C[s] : 0.0;
  if (e < 8) st2[e] = 0;
}

// c / sigma^2 of the model, on the device
__device__ __forceinline__ double oq_prec(const double* __restrict__ lvn, double scale) { return scale * exp(-lvn[0]); }

// Bm = J B J, B = I + (c / sigma^2) Phi, from the lower triangle of Phi: exactly symmetric
__global__ __launch_bounds__(256) void k_optqu_b(const double* __restrict__ Phi, int MP, int M, const double* __restrict__ lvn,
                                                  double scale, double* __restrict__ Bm) {
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (size_t)M * M) return;
  const int i = (int)(e / M), j = (int)(e % M);
  const int ri = M - 1 - i, rj = M - 1 - j;
  const int hi = ri > rj ? ri : rj, lo = ri > rj ? rj : ri;
  Bm[e] = oq_prec(lvn, scale) * Phi[(size_t)hi * MP + lo] + (i == j ? 1.0 : 0.0);
}

// Lam* = J L'^-T J: Lam*[i][j] = L'^-1[M-1-j][M-1-i] for j <= i, zeros above; LamT its transpose.  A failure of the second
// factorisation is reported in status[0] when K's succeeded.
__global__ __launch_bounds__(256) void k_optqu_lam(const double* __restrict__ Lpinv, int M, double* __restrict__ Lam,
                                                    double* __restrict__ LamT, const int32_t* __restrict__ st2,
                                                    int32_t* __restrict__ status) {
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e == 0) {
    if (st2[0] != 0 && status[0] == 0) status[0] = st2[0];
    if (st2[1] != 0) status[1] = st2[1];
  }
  if (e >= (size_t)M * M) return;
  const int i = (int)(e / M), j = (int)(e % M);
  const double v = j <= i ? Lpinv[(size_t)(M - 1 - j) * M + (M - 1 - i)] : 0.0;
  Lam[e] = v;
  LamT[(size_t)j * M + i] = v;
}

// y = alpha A x, A (M x M, row stride ld), alpha = c / sigma^2 with lvn, else 1.  One wave per row: lane l sums the columns
// l, l + 64, ... in order, then the wave butterfly.
__global__ __launch_bounds__(256) void k_optqu_mv(const double* __restrict__ A, int ld, int M, const double* __restrict__ x,
                                                   const double* __restrict__ lvn, double scale, double* __restrict__ y) {
  const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= M) return;  // (whole waves)
  double s = 0.0;
  for (int k = lane; k < M; k += 64) s += A[(size_t)row * ld + k] * x[k];
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) s += __shfl_xor(s, o, 64);
  if (lane == 0) y[row] = (lvn != nullptr ? oq_prec(lvn, scale) : 1.0) * s;
}

// ---- the natural-gradient step (tgp_natgrad_qu_f64): what the chain above lacks ------------------------------------
// The lower triangle of A (M x M), or its transpose with `tr`, in a zero-padded (MP x MP) image
__global__ __launch_bounds__(256) void k_nq_tril(const double* __restrict__ A, int M, int MP, int tr, double* __restrict__ AP) {
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  const int row = (int)(e / MP), col = (int)(e % MP);
  const int r = tr ? col : row, c = tr ? row : col;
  AP[e] = (r < M && c <= r) ? A[(size_t)r * M + c] : 0.0;
}

// A (M x M) from the lower triangle of the padded image AP: exactly symmetric
__global__ __launch_bounds__(256) void k_nq_sym(const double* __restrict__ AP, int MP, int M, double* __restrict__ A) {
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (size_t)M * M) return;
  const int i = (int)(e / M), j = (int)(e % M);
  const int hi = i > j ? i : j, lo = i > j ? j : i;
  A[e] = AP[(size_t)hi * MP + lo];
}

// Bm = J P' J, P' = (1 - rho) P + rho (I + Phi), from the lower triangles of Phi and P: exactly symmetric.  rho = 1: P is not read.
__global__ __launch_bounds__(256) void k_nq_b(const double* __restrict__ Phi, const double* __restrict__ P, int MP, int M, double rho,
                                               double* __restrict__ Bm) {
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (size_t)M * M) return;
  const int i = (int)(e / M), j = (int)(e % M);
  const int ri = M - 1 - i, rj = M - 1 - j;
  const int hi = ri > rj ? ri : rj, lo = ri > rj ? rj : ri;
  double v = Phi[(size_t)hi * MP + lo] + (i == j ? 1.0 : 0.0);
  if (rho < 1.0) v = (1.0 - rho) * P[(size_t)hi * MP + lo] + rho * v;
  Bm[e] = v;
}

// h' = (1 - rho) P m + rho h, in place of h
__global__ __launch_bounds__(256) void k_nq_h(const double* __restrict__ pm, int M, double rho, double* __restrict__ h) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < M) h[i] = (1.0 - rho) * pm[i] + rho * h[i];
}

// status[1] <- the q(u)-side factorisations when K's succeeded and found no NaN (status[1] == 1 stays K's NaN flag): -(pivot) of
// S = Lam Lam^T, else 1 + the pivot of P'; a factorisation that met NaNs and no pivot counts as pivot M + 1.  ok[0] = 1 when every
// factorisation of the call succeeded.
__global__ void k_nq_flag(const int32_t* __restrict__ stS, const int32_t* __restrict__ st2, int with_S, int M,
                          int32_t* __restrict__ status, int32_t* __restrict__ ok) {
  if (threadIdx.x != 0) return;
  int q = 0;
  if (with_S && (stS[0] != 0 || stS[1] != 0)) q = -(stS[0] != 0 ? stS[0] : M + 1);
  else if (st2[0] != 0 || st2[1] != 0) q = 1 + (st2[0] != 0 ? st2[0] : M + 1);
  const bool k_ok = status[0] == 0 && status[1] == 0;
  if (k_ok && q != 0) status[1] = q;
  ok[0] = (k_ok && q == 0) ? 1 : 0;
}

// (m_out, Lam_out) <- the step's result, only when ok[0]
__global__ __launch_bounds__(256) void k_nq_commit(const int32_t* __restrict__ ok, const double* __restrict__ mn,
                                                    const double* __restrict__ Lamn, int M, double* __restrict__ m_out,
                                                    double* __restrict__ Lam_out) {
  if (ok[0] == 0) return;
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e < (size_t)M * M) Lam_out[e] = Lamn[e];
  if (e < (size_t)M) m_out[e] = mn[e];
}

// ---- host side ----------------------------------------------------------------------------------------------------
namespace {
struct KxPlan : Layout {  // the row split of k_kxxk: a function of N and M alone
  int nti, ntile, G, ngroup;
  size_t part, bpart;
};
bool kx_plan(KxPlan& p, int N, int M) {
  if (N < 1 || M < 1 || M > TGP_BIG_MAX_M) return false;
  p.nti = (M + TL_T - 1) / TL_T;
  p.ntile = p.nti * (p.nti + 1) / 2;
  const int want = OQ_WGS / p.ntile > 1 ? OQ_WGS / p.ntile : 1;
  const size_t g = rup(((size_t)N + want - 1) / want, TL_KC);
  p.G = g > OQ_MIN_G ? (int)g : OQ_MIN_G;
  p.ngroup = (N + p.G - 1) / p.G;  // <= want <= OQ_WGS
  p.part = p.take((size_t)p.ngroup * p.ntile * TL_T * TL_T);
  p.bpart = p.take((size_t)p.ngroup * p.nti * TL_T);
  return true;
}
struct OqPlan : Layout {
  int MP;
  // kzz.Kmm is J B J later, kzz.Lf is L', CP is Lam*^T and T is L'^-1 once their first contents have been consumed
  KzzSections kzz;
  size_t LinvP, CP, T, Phi, C, b, v1, v2, st2, kx;
  KxPlan k;
};
bool oq_plan(OqPlan& p, int N, int D, int M) {
  if (!inducing_limits(M, D) || !kx_plan(p.k, N, M)) return false;
  p.MP = (int)rup((size_t)M, 128);
  const size_t mm = (size_t)M * M, pp = (size_t)p.MP * p.MP;
  p.kzz.take(p, M);
  p.LinvP = p.take(pp);
  p.CP = p.take(pp);
  p.T = p.take(pp);
  p.Phi = p.take(pp);
  p.C = p.take(mm);
  p.b = p.take(M);
  p.v1 = p.take(M);
  p.v2 = p.take(M);
  p.st2 = p.take(64);
  p.kx = p.take(p.k.total);
  return true;
}
template <class RW>
int run_kxxk(const KxPlan& k, int kernel, const double* X, int N, const double* Z, int M, int D, const double* raw_ls,
             const double* raw_os, const double* Y, double* C, double* b, double* ws, hipStream_t st, RW rw, bool has_r) {
  const dim3 grid((unsigned)k.ntile, (unsigned)k.ngroup), block(256);
  double* bpart = (has_r && b != nullptr) ? ws + k.bpart : nullptr;
  dispatch_dp(D, [&](auto dp) {
    hipLaunchKernelGGL((k_kxxk<decltype(dp)::value, RW>), grid, block, 0, st, kernel, X, N, Z, M, D, raw_ls, raw_os, Y, k.G, k.ntile,
                       k.nti, ws + k.part, bpart, rw);
  });
  LAUNCH_CHECK();
  hipLaunchKernelGGL(k_kxxk_fin, dim3((unsigned)k.ntile), block, 0, st, ws + k.part, bpart, k.ngroup, k.ntile, k.nti, M, C, M, b);
  LAUNCH_CHECK();
  return 0;
}
int run_kxxk(const KxPlan& k, int kernel, const double* X, int N, const double* Z, int M, int D, const double* raw_ls,
             const double* raw_os, const double* Y, double* C, double* b, double* ws, hipStream_t st) {
  return run_kxxk(k, kernel, X, N, Z, M, D, raw_ls, raw_os, Y, C, b, ws, st, NoWeights{}, Y != nullptr);
}
int run_kxwxk(const KxPlan& k, int kernel, const double* X, int N, const double* Z, int M, int D, const double* raw_ls,
              const double* raw_os, const RowWeights& rw, double* C, double* b, double* ws, hipStream_t st) {
  return run_kxxk(k, kernel, X, N, Z, M, D, raw_ls, raw_os, nullptr, C, b, ws, st, rw, rw.b != nullptr);
}
// The workspace of tgp_natgrad_qu_f64: tgp_optimal_qu_f64's sections and, for rho < 1, S = Lam Lam^T, its factor and inverse.
// CP and T take turns as in OqPlan: C_lambda padded / tril(Lam) padded / L_S^-T padded / Lam'^T, and L^-1 C / S / P / L'^-1.
struct NqPlan : OqPlan {
  size_t Sm, Ls, Lsi, pm, mn, Lamn;
};
bool nq_plan(NqPlan& p, int N, int D, int M) {
  if (!oq_plan(p, N, D, M)) return false;
  const size_t mm = (size_t)M * M;
  p.Sm = p.take(mm);
  p.Ls = p.take(mm);
  p.Lsi = p.take(mm);
  p.pm = p.take(M);
  p.mn = p.take(M);
  p.Lamn = p.take(mm);
  return true;
}
}  // namespace

size_t kxxk_workspace_bytes(int N, int M) {
  KxPlan k;
  return kx_plan(k, N, M) ? k.bytes() : 0;
}

size_t optimal_qu_workspace_bytes(int N, int D, int M) {
  OqPlan p;
  return oq_plan(p, N, D, M) ? p.bytes() : 0;
}

int launch_kxxk(int kernel, const double* X, int N, const double* Z, int M, int D, const double* raw_ls, const double* raw_os,
                const double* Y, double* C, double* b, void* workspace, size_t workspace_bytes, hipStream_t st) {
  KxPlan k;
  if (!inducing_limits(M, D) || !kx_plan(k, N, M)) return TGP_E_UNSUPPORTED;  // (tgp_kxxk_f64 has named the limits)
  double* ws;
  if (int rc = open_workspace("tgp_kxxk_f64", "tgp_kxxk_workspace_bytes", workspace, workspace_bytes, k.total, &ws)) return rc;
  return run_kxxk(k, kernel, X, N, Z, M, D, raw_ls, raw_os, Y, C, b, ws, st);
}

int launch_optimal_qu(const tgp_model& md, const double* X, const double* Y, double* m_out, double* Lam_out, int32_t* status,
                      void* workspace, size_t workspace_bytes, hipStream_t st) {
  OqPlan p;
  if (!oq_plan(p, md.N, md.D, md.M)) return TGP_E_UNSUPPORTED;  // (tgp_optimal_qu_f64 has named the limits)
  double* ws;
  if (int rc = open_workspace("tgp_optimal_qu_f64", "tgp_optimal_qu_workspace_bytes", workspace, workspace_bytes, p.total, &ws))
    return rc;
  const int N = md.N, D = md.D, M = md.M, MP = p.MP;
  const unsigned gmm = (unsigned)(((size_t)M * M + 255) / 256), gpp = (unsigned)((size_t)MP * MP / 256), gmv = (unsigned)((M + 3) / 4);
  int32_t* st2 = reinterpret_cast<int32_t*>(ws + p.st2);
  double *Bm = ws + p.kzz.Kmm, *Lp = ws + p.kzz.Lf, *Lpinv = ws + p.T, *LamT = ws + p.CP;  // second lives of consumed sections
  if (int rc = p.kzz.factor(md, ws, status, st)) return rc;
  if (int rc = run_kxxk(p.k, md.kernel, X, N, md.Z, M, D, md.raw_ls, md.raw_os, Y, ws + p.C, ws + p.b, ws + p.kx, st)) return rc;
  hipLaunchKernelGGL(k_optqu_pad, dim3(gpp), dim3(256), 0, st, ws + p.kzz.Linv, ws + p.C, M, MP, ws + p.LinvP, ws + p.CP, st2);
  LAUNCH_CHECK();
  if (int rc = launch_gemm_plain(false, false, 0, MP, MP, MP, 1.0, ws + p.LinvP, MP, ws + p.CP, MP, 0.0, ws + p.T, MP, st)) return rc;
  if (int rc = launch_gemm_plain(false, true, 0, MP, MP, MP, 1.0, ws + p.T, MP, ws + p.LinvP, MP, 0.0, ws + p.Phi, MP, st)) return rc;
  hipLaunchKernelGGL(k_optqu_b, dim3(gmm), dim3(256), 0, st, ws + p.Phi, MP, M, md.log_var_noise, md.scale, Bm);
  LAUNCH_CHECK();
  if (int rc = launch_cholesky_any(Bm, M, Lp, Lpinv, st2, ws + p.kzz.chol, p.kzz.chol_len, st)) return rc;
  hipLaunchKernelGGL(k_optqu_lam, dim3(gmm), dim3(256), 0, st, Lpinv, M, Lam_out, LamT, st2, status);
  LAUNCH_CHECK();
  hipLaunchKernelGGL(k_optqu_mv, dim3(gmv), dim3(256), 0, st, ws + p.LinvP, MP, M, ws + p.b, nullptr, 1.0, ws + p.v1);
  LAUNCH_CHECK();
  hipLaunchKernelGGL(k_optqu_mv, dim3(gmv), dim3(256), 0, st, LamT, M, M, ws + p.v1, nullptr, 1.0, ws + p.v2);
  LAUNCH_CHECK();
  hipLaunchKernelGGL(k_optqu_mv, dim3(gmv), dim3(256), 0, st, Lam_out, M, M, ws + p.v2, md.log_var_noise, md.scale, m_out);
  LAUNCH_CHECK();
  return 0;
}

size_t kxwxk_workspace_bytes(int N, int M) { return kxxk_workspace_bytes(N, M); }

int launch_kxwxk(int kernel, const double* X, int N, const double* Z, int M, int D, const double* raw_ls, const double* raw_os,
                 const double* w, const double* r, double* C, double* b, void* workspace, size_t workspace_bytes, hipStream_t st) {
  KxPlan k;
  if (!inducing_limits(M, D) || !kx_plan(k, N, M)) return TGP_E_UNSUPPORTED;  // (tgp_kxwxk_f64 has named the limits)
  double* ws;
  if (int rc = open_workspace("tgp_kxwxk_f64", "tgp_kxwxk_workspace_bytes", workspace, workspace_bytes, k.total, &ws)) return rc;
  const RowWeights rw{w, b != nullptr ? r : nullptr, nullptr, 0.0, 0};
  return run_kxwxk(k, kernel, X, N, Z, M, D, raw_ls, raw_os, rw, C, b, ws, st);
}

size_t natgrad_qu_workspace_bytes(int N, int D, int M) {
  NqPlan p;
  return nq_plan(p, N, D, M) ? p.bytes() : 0;
}

// Launch sequence (one stream, no host sync): the workspace's status words zeroed -> K's factor (status[0]) -> the weighted k_kxxk with the sites formed per row, and
// k_kxxk_fin -> k_optqu_pad, T = L^-1 C_lambda, Phi = T L^-T -> h = L^-1 b_r -> [rho < 1: tril(Lam) padded, S = Lam Lam^T, its
// factor and inverse, L_S^-T padded, P = L_S^-T L_S^-1, P m, h' = (1 - rho) P m + rho h] -> J P' J, its factor and inverse ->
// k_optqu_lam -> Lam'^T h', m' = Lam' (Lam'^T h') -> status[1] and the copy to the outputs when nothing failed.
int launch_natgrad_qu(const tgp_model& md, const double* X, const double* mu, const double* mu_bar, const double* v_bar, double rho,
                      double site_floor, double* m_out, double* Lam_out, int32_t* status, void* workspace, size_t workspace_bytes,
                      hipStream_t st) {
  NqPlan p;
  if (!nq_plan(p, md.N, md.D, md.M)) return TGP_E_UNSUPPORTED;  // (tgp_natgrad_qu_f64 has named the limits)
  double* ws;
  if (int rc = open_workspace("tgp_natgrad_qu_f64", "tgp_natgrad_qu_workspace_bytes", workspace, workspace_bytes, p.total, &ws))
    return rc;
  const int N = md.N, D = md.D, M = md.M, MP = p.MP;
  const unsigned gmm = (unsigned)(((size_t)M * M + 255) / 256), gpp = (unsigned)((size_t)MP * MP / 256), gmv = (unsigned)((M + 3) / 4);
  const bool damped = rho < 1.0;
  // status words of the workspace: [0, 8) P''s factorisation, [8, 16) S's, [16, 24) what k_optqu_lam reports, [24] ok
  int32_t *st2 = reinterpret_cast<int32_t*>(ws + p.st2), *stS = st2 + 8, *st3 = st2 + 16, *ok = st2 + 24;
  if (hipError_t e = hipMemsetAsync(stS, 0, 24 * sizeof(int32_t), st)) return set_error(e, __FILE__, __LINE__);  // ([0, 8): k_optqu_pad)
  double *Bm = ws + p.kzz.Kmm, *Lp = ws + p.kzz.Lf, *Lpinv = ws + p.T, *LamT = ws + p.CP;  // second lives of consumed sections
  if (int rc = p.kzz.factor(md, ws, status, st)) return rc;
  const RowWeights rw{v_bar, mu_bar, mu, site_floor, 1};
  if (int rc = run_kxwxk(p.k, md.kernel, X, N, md.Z, M, D, md.raw_ls, md.raw_os, rw, ws + p.C, ws + p.b, ws + p.kx, st)) return rc;
  hipLaunchKernelGGL(k_optqu_pad, dim3(gpp), dim3(256), 0, st, ws + p.kzz.Linv, ws + p.C, M, MP, ws + p.LinvP, ws + p.CP, st2);
  LAUNCH_CHECK();
  if (int rc = launch_gemm_plain(false, false, 0, MP, MP, MP, 1.0, ws + p.LinvP, MP, ws + p.CP, MP, 0.0, ws + p.T, MP, st)) return rc;
  if (int rc = launch_gemm_plain(false, true, 0, MP, MP, MP, 1.0, ws + p.T, MP, ws + p.LinvP, MP, 0.0, ws + p.Phi, MP, st)) return rc;
  hipLaunchKernelGGL(k_optqu_mv, dim3(gmv), dim3(256), 0, st, ws + p.LinvP, MP, M, ws + p.b, nullptr, 1.0, ws + p.v1);
  LAUNCH_CHECK();
  if (damped) {
    hipLaunchKernelGGL(k_nq_tril, dim3(gpp), dim3(256), 0, st, md.Lam, M, MP, 0, ws + p.CP);
    LAUNCH_CHECK();
    if (int rc = launch_gemm_plain(false, true, 0, MP, MP, MP, 1.0, ws + p.CP, MP, ws + p.CP, MP, 0.0, ws + p.T, MP, st)) return rc;
    hipLaunchKernelGGL(k_nq_sym, dim3(gmm), dim3(256), 0, st, ws + p.T, MP, M, ws + p.Sm);
    LAUNCH_CHECK();
    if (int rc = launch_cholesky_any(ws + p.Sm, M, ws + p.Ls, ws + p.Lsi, stS, ws + p.kzz.chol, p.kzz.chol_len, st)) return rc;
    hipLaunchKernelGGL(k_nq_tril, dim3(gpp), dim3(256), 0, st, ws + p.Lsi, M, MP, 1, ws + p.CP);
    LAUNCH_CHECK();
    if (int rc = launch_gemm_plain(false, true, 0, MP, MP, MP, 1.0, ws + p.CP, MP, ws + p.CP, MP, 0.0, ws + p.T, MP, st)) return rc;
    hipLaunchKernelGGL(k_optqu_mv, dim3(gmv), dim3(256), 0, st, ws + p.T, MP, M, md.m, nullptr, 1.0, ws + p.pm);
    LAUNCH_CHECK();
    hipLaunchKernelGGL(k_nq_h, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, st, ws + p.pm, M, rho, ws + p.v1);
    LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(k_nq_b, dim3(gmm), dim3(256), 0, st, ws + p.Phi, ws + p.T, MP, M, rho, Bm);
  LAUNCH_CHECK();
  if (int rc = launch_cholesky_any(Bm, M, Lp, Lpinv, st2, ws + p.kzz.chol, p.kzz.chol_len, st)) return rc;
  hipLaunchKernelGGL(k_optqu_lam, dim3(gmm), dim3(256), 0, st, Lpinv, M, ws + p.Lamn, LamT, st2, st3);
  LAUNCH_CHECK();
  hipLaunchKernelGGL(k_optqu_mv, dim3(gmv), dim3(256), 0, st, LamT, M, M, ws + p.v1, nullptr, 1.0, ws + p.v2);
  LAUNCH_CHECK();
  hipLaunchKernelGGL(k_optqu_mv, dim3(gmv), dim3(256), 0, st, ws + p.Lamn, M, M, ws + p.v2, nullptr, 1.0, ws + p.mn);
  LAUNCH_CHECK();
  hipLaunchKernelGGL(k_nq_flag, dim3(1), dim3(64), 0, st, stS, st2, damped ? 1 : 0, M, status, ok);
  LAUNCH_CHECK();
  hipLaunchKernelGGL(k_nq_commit, dim3(gmm), dim3(256), 0, st, ok, ws + p.mn, ws + p.Lamn, M, m_out, Lam_out);
  LAUNCH_CHECK();
  return 0;
}

}  // namespace tgp
