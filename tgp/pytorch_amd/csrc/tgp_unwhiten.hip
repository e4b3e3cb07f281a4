// tgp_unwhiten.hip -- the unwhitened q(u) parameterisation (tgp_unwhiten_f64, tgp_unwhiten_bwd_f64).
//
// sparse_MF_SP with is_whiten=False (models/sparse_MF_SP.py:352-391, :433-453): (m, L_q) describe q(u) = N(m, L_q L_q^T) on
// the inducing values.  With L L^T = K_ZZ + jitter I and the zero mean function, the affine change of variables
//   m_w = L^-1 m,   Lam_w = L^-1 tril(L_q)                                   (lower x lower = lower)
// gives the whitened model with the same q(f) and the same KL, so every whitened kernel serves the unwhitened model at
// (m_w, Lam_w).  This unit holds the transform, its adjoint and the adjoint of K_ZZ with respect to Z and the kernel parameters:
//   forward   K_ZZ + jitter I, its factor and L^-1      the existing launchers
//             k_unwhiten<UW_FWD>                         Lam_w = L^-1 tril(L_q), m_w = L^-1 m
//   backward  k_unwhiten<UW_ATB>                         L_q_bar = tril(L^-T Lam_w_bar), m_bar = L^-T m_w_bar
//             k_unwhiten<UW_ABT>                         P = tril(Lam_w_bar Lam_w^T + m_w_bar m_w^T)
//             k_unwhiten<UW_ATB>                         L_bar = -tril(L^-T P)
//             the Cholesky adjoint                       K_bar (symmetric), the launcher behind tgp_cholesky_bwd_f64
//             k_kmm_bwd, k_kmm_bwd_fin                   Z_bar, raw_ls_bar, raw_os_bar from K_bar + K_bar^T
// The M x M products run in one kernel of their own on unpadded operands (triangular masks applied while the tiles are staged)
// rather than behind launch_gemm_plain: that one needs three padded images per product, and these products are triangular on
// all three sides.  Every reduction has a fixed order and nothing is accumulated with atomics: same input, same bits.
#include "tgp_dev.hpp"
#include "tgp_launch.hpp"
#include "tgp_tile.hpp"

namespace tgp {

#define UW_FWD 0 /* C = tril(A B),                 A, B lower: k in [j, i]                                      */
#define UW_ATB 1 /* C = alpha tril(A^T B),         A, B lower: k >= i                                           */
#define UW_ABT 2 /* C = tril(A B^T + u w^T),       A, B lower: k <= j                                           */

// One triangular x triangular product on the f64 matrix cores.  Workgroup (tj, ti) owns the 64 x 64 tile of C at rows 64 ti,
// columns 64 tj; a tile above the diagonal is written as zeros and nothing is computed for it.  Wave w holds rows 16 w ..
// 16 w + 15 of the tile against all 64 columns in four accumulators.  Both operands are read with their lower-triangle masks
// (an entry above the diagonal of A or B is never loaded), tails in M are zero filled, and the contraction runs over the
// steps that can hold a non-zero term only.  The strict upper triangle of C is written as exact zeros.
// With `vin`, the workgroups of tile column 0 (their contraction covers a whole row of op(A)) also form vout = op(A) vin for
// their 64 rows, one thread per row, summed in the order of k.
template <int MODE>
__global__ __launch_bounds__(256) void k_unwhiten(const double* __restrict__ A, const double* __restrict__ B, int M, double alpha,
                                                   double* __restrict__ C, const double* __restrict__ vin, double* __restrict__ vout,
                                                   const double* __restrict__ ru, const double* __restrict__ rw) {
  __shared__ double As[TL_T * TL_LDK];
  __shared__ double Bs[TL_KC * TL_LDN];
  __shared__ double vs[TL_KC];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, lr = lane & 15, lq = lane >> 4;
  const int ti = blockIdx.y, tj = blockIdx.x;
  const int i0 = ti * TL_T, j0 = tj * TL_T;
  if (tj > ti) {
    for (int e = tid; e < TL_T * TL_T; e += 256) {
      const int row = i0 + (e >> 6), col = j0 + (e & 63);
      if (row < M && col < M) C[(size_t)row * M + col] = 0.0;
    }
    return;
  }
  const bool mv = vin != nullptr && tj == 0;
  const int iend = i0 + TL_T < M ? i0 + TL_T : M, jend = j0 + TL_T < M ? j0 + TL_T : M;
  const int kb = MODE == UW_FWD ? j0 : (MODE == UW_ATB ? i0 : 0);
  const int ke = MODE == UW_FWD ? iend : (MODE == UW_ATB ? M : jend);
  d4 acc[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) acc[c] = d4{0.0, 0.0, 0.0, 0.0};
  double vacc = 0.0;
  for (int k0 = kb; k0 < ke; k0 += TL_KC) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int idx = tid + 256 * u;
      {  // op(A): element (r, k) of the step
        const int r = MODE == UW_ATB ? (idx & 63) : (idx >> 4), k = MODE == UW_ATB ? (idx >> 6) : (idx & 15);
        const int row = i0 + r, kk = k0 + k;
        double val;
        if (MODE == UW_ATB)
          val = (kk < M && row <= kk) ? A[(size_t)kk * M + row] : 0.0;
        else
          val = (row < M && kk <= row) ? A[(size_t)row * M + kk] : 0.0;
        As[r * TL_LDK + k] = val;
      }
      {  // op(B): element (k, c) of the step
        const int c = MODE == UW_ABT ? (idx >> 4) : (idx & 63), k = MODE == UW_ABT ? (idx & 15) : (idx >> 6);
        const int col = j0 + c, kk = k0 + k;
        double val;
        if (MODE == UW_ABT)
          val = (col < M && kk <= col) ? B[(size_t)col * M + kk] : 0.0;
        else
          val = (kk < M && col <= kk) ? B[(size_t)kk * M + col] : 0.0;
        Bs[k * TL_LDN + c] = val;
      }
    }
    if (mv && tid < TL_KC) vs[tid] = k0 + tid < M ? vin[k0 + tid] : 0.0;
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      const double a = As[(16 * w + lr) * TL_LDK + kk * 4 + lq];
#pragma unroll
      for (int c = 0; c < 4; ++c) acc[c] = TGP_MFMA(a, Bs[(kk * 4 + lq) * TL_LDN + 16 * c + lr], acc[c]);
    }
    if (mv && tid < TL_T) {
#pragma unroll
      for (int k = 0; k < TL_KC; ++k) vacc += As[tid * TL_LDK + k] * vs[k];
    }
    __syncthreads();
  }
#pragma unroll
  for (int c = 0; c < 4; ++c)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = i0 + 16 * w + lq + 4 * r, col = j0 + 16 * c + lr;
      if (row < M && col < M) {
        double val = alpha * acc[c][r];
        if (MODE == UW_ABT && ru != nullptr) val += ru[row] * rw[col];
        C[(size_t)row * M + col] = col <= row ? val : 0.0;
      }
    }
  if (mv && tid < TL_T && i0 + tid < M) vout[i0 + tid] = vacc;
}

// Adjoint of K_ZZ = s2 f(d2), d2_ij = |(z_i - z_j) / l|^2, for a (symmetric) K_bar: with S = K_bar + K_bar^T and the derivative
// weight k_g = -2 dK/d(d2) of tgp_dev.hpp (same max(d2, 1e-30) clamp as cov_value),
//   Z_bar[i, d]   = -sum_j S_ij k_g(d2_ij) (z_id - z_jd) / l_d^2        (j = i adds an exact zero: no gradient from the diagonal,
//                                                                        none from the jitter)
//   l_d_bar       = 1/2 sum_ij S_ij k_g(d2_ij) (z_id - z_jd)^2 / l_d^3
//   s2_bar        = 1/2 sum_ij S_ij f(d2_ij)
// One wave per row i: the lanes walk j = lane, lane + 64, ..., the wave butterfly sums them.  Z_bar's row is final; the row's
// terms of the lengthscale and outputscale sums go to part[i][0..16] and are summed over the rows by k_kmm_bwd_fin.
__global__ __launch_bounds__(256) void k_kmm_bwd(int kernel, const double* __restrict__ Z, int M, int D,
                                                  const double* __restrict__ raw_ls, const double* __restrict__ raw_os,
                                                  const double* __restrict__ Kbar, double* __restrict__ Zbar,
                                                  double* __restrict__ part) {
  __shared__ double ils[TL_ILS];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  tile_scales(kernel, D, raw_ls, raw_os, ils);
  __syncthreads();
  const int i = blockIdx.x * 4 + w;
  if (i >= M) return;
  const Cov cov = tile_cov(kernel, ils), cov1 = make_cov(kernel, 1.0, cov.alpha);
  double zi[16], gz[16], gl[16], go = 0.0;
#pragma unroll
  for (int d = 0; d < 16; ++d) {
    zi[d] = d < D ? Z[(size_t)i * D + d] * ils[d] : 0.0;
    gz[d] = 0.0;
    gl[d] = 0.0;
  }
  for (int j = lane; j < M; j += 64) {
    double u[16], d2 = 0.0;
#pragma unroll
    for (int d = 0; d < 16; ++d) {  // (dimensions past D hold zeros on both sides: they add exact zeros)
      u[d] = zi[d] - (d < D ? Z[(size_t)j * D + d] * ils[d] : 0.0);
      d2 += u[d] * u[d];
    }
    const double s = Kbar[(size_t)i * M + j] + Kbar[(size_t)j * M + i];
    go += s * cov_value(cov1, d2);
    const double sk = s * cov_gweight(cov, d2);
#pragma unroll
    for (int d = 0; d < 16; ++d) {
      const double t = sk * u[d];
      gz[d] -= t;
      gl[d] += t * u[d];
    }
  }
#pragma unroll
  for (int d = 0; d < 16; ++d) {
    const double a = wave_sum(gz[d]), b = wave_sum(gl[d]);
    if (lane == 0) {
      if (d < D) Zbar[(size_t)i * D + d] = a * ils[d];
      part[(size_t)i * 17 + d] = b;
    }
  }
  go = wave_sum(go);
  if (lane == 0) part[(size_t)i * 17 + 16] = go;
}

// Workgroup o (one wave) sums column o of part[M][17] over the rows, lanes striding the rows and the butterfly on top, and
// applies the chain through the softplus: o < D the raw lengthscale o, o = 16 the raw outputscale.
__global__ __launch_bounds__(64) void k_kmm_bwd_fin(const double* __restrict__ part, int M, int D, const double* __restrict__ raw_ls,
                                                     const double* __restrict__ raw_os, double* __restrict__ g_ls,
                                                     double* __restrict__ g_os) {
  const int o = blockIdx.x, lane = threadIdx.x;
  if (o < 16 && o >= D) return;
  double a = 0.0;
  for (int i = lane; i < M; i += 64) a += part[(size_t)i * 17 + o];
  a = wave_sum(a);
  if (lane != 0) return;
  if (o < 16)
    g_ls[o] = 0.5 * a * (1.0 / softplus_d(raw_ls[o])) * sigmoid_d(raw_ls[o]);
  else
    g_os[0] = 0.5 * a * sigmoid_d(raw_os[0]);
}

// ---- host side ----------------------------------------------------------------------------------------------------
namespace {
struct UwPlan : Layout {
  size_t Kmm, chol, chol_len;
};
bool uw_plan(UwPlan& p, int M, int D) {
  if (!inducing_limits(M, D)) return false;
  p.chol_len = chol_ws_doubles(M);
  p.Kmm = p.take((size_t)M * M);
  p.chol = p.take(p.chol_len);
  return true;
}
struct UwBwdPlan : Layout {
  size_t P, Lbar, Kbar, part, chol, chol_len;
};
bool uw_bwd_plan(UwBwdPlan& p, int M, int D) {
  if (!inducing_limits(M, D)) return false;
  p.chol_len = rup(big_cholesky_workspace_doubles(M), 64);  // (the adjoint runs the blocked path at every M)
  p.P = p.take((size_t)M * M);
  p.Lbar = p.take((size_t)M * M);
  p.Kbar = p.take((size_t)M * M);
  p.part = p.take((size_t)M * 17);
  p.chol = p.take(p.chol_len);
  return true;
}
template <int MODE>
int launch_tri(const double* A, const double* B, int M, double alpha, double* C, const double* vin, double* vout, const double* ru,
               const double* rw, hipStream_t st) {
  const unsigned nt = (unsigned)((M + TL_T - 1) / TL_T);
  hipLaunchKernelGGL(k_unwhiten<MODE>, dim3(nt, nt), dim3(256), 0, st, A, B, M, alpha, C, vin, vout, ru, rw);
  LAUNCH_CHECK();
  return 0;
}
}  // namespace

size_t unwhiten_workspace_bytes(int M, int D) {
  UwPlan p;
  return uw_plan(p, M, D) ? p.bytes() : 0;
}

size_t unwhiten_bwd_workspace_bytes(int M, int D) {
  UwBwdPlan p;
  return uw_bwd_plan(p, M, D) ? p.bytes() : 0;
}

int launch_unwhiten(int kernel, const double* Z, const double* raw_ls, const double* raw_os, int M, int D, double jitter,
                    const double* m, const double* Lq, double* m_w, double* Lam_w, double* L, double* Linv, int32_t* status,
                    void* workspace, size_t workspace_bytes, hipStream_t st) {
  UwPlan p;
  if (!uw_plan(p, M, D)) return TGP_E_UNSUPPORTED;  // (tgp_unwhiten_f64 has named the limits)
  double* ws;
  if (int rc = open_workspace("tgp_unwhiten_f64", "tgp_unwhiten_workspace_bytes", workspace, workspace_bytes, p.total, &ws))
    return rc;
  if (int rc = launch_kzz_factor(kernel, Z, raw_ls, raw_os, M, D, jitter, ws + p.Kmm, L, Linv, status, ws + p.chol, p.chol_len, st))
    return rc;
  return launch_tri<UW_FWD>(Linv, Lq, M, 1.0, Lam_w, m, m_w, nullptr, nullptr, st);
}

int launch_unwhiten_bwd(int kernel, const double* Z, const double* raw_ls, const double* raw_os, int M, int D, const double* L,
                        const double* Linv, const double* m_w, const double* Lam_w, const double* m_w_bar, const double* Lam_w_bar,
                        double* m_bar, double* Lq_bar, double* Z_bar, double* raw_ls_bar, double* raw_os_bar, void* workspace,
                        size_t workspace_bytes, hipStream_t st) {
  UwBwdPlan p;
  if (!uw_bwd_plan(p, M, D)) return TGP_E_UNSUPPORTED;  // (tgp_unwhiten_bwd_f64 has named the limits)
  double* ws;
  if (int rc = open_workspace("tgp_unwhiten_bwd_f64", "tgp_unwhiten_bwd_workspace_bytes", workspace, workspace_bytes, p.total, &ws))
    return rc;
  if (int rc = launch_tri<UW_ATB>(Linv, Lam_w_bar, M, 1.0, Lq_bar, m_w_bar, m_bar, nullptr, nullptr, st)) return rc;
  if (int rc = launch_tri<UW_ABT>(Lam_w_bar, Lam_w, M, 1.0, ws + p.P, nullptr, nullptr, m_w_bar, m_w, st)) return rc;
  if (int rc = launch_tri<UW_ATB>(Linv, ws + p.P, M, -1.0, ws + p.Lbar, nullptr, nullptr, nullptr, nullptr, st)) return rc;
  if (int rc = launch_big_cholesky_bwd(L, Linv, ws + p.Lbar, M, ws + p.Kbar, ws + p.chol, p.chol_len, st)) return rc;
  hipLaunchKernelGGL(k_kmm_bwd, dim3((unsigned)((M + 3) / 4)), dim3(256), 0, st, kernel, Z, M, D, raw_ls, raw_os, ws + p.Kbar, Z_bar,
                     ws + p.part);
  LAUNCH_CHECK();
  hipLaunchKernelGGL(k_kmm_bwd_fin, dim3(17), dim3(64), 0, st, ws + p.part, M, D, raw_ls, raw_os, raw_ls_bar, raw_os_bar);
  LAUNCH_CHECK();
  return 0;
}

}  // namespace tgp
