// tgp_cov.hip -- full-covariance q(f) and joint function draws (tgp_qf_cov_f64, tgp_qf_joint_sample_f64).
//
// sparse_MF_SP.marginal_variational_qf_parameters with diagonal=False (models/sparse_MF_SP.py:384), whitened q(u):
//   A = L^-1 K(Z, X*)   (M x N),   L_q = tril(Lam),   W = L_q L_q^T - I
//   mu = A^T m,   Sigma = K(X*, X*) + A^T W A          (the row kernel's (S - I) A form, for all pairs of rows)
// and a joint draw  F0 = mu + E chol(Sigma + jitter I)^T  for caller-supplied standard normals E (S x N).
//
// Launch sequence of tgp_qf_cov_f64 (one stream, no host sync; operands padded to multiples of 128 in the workspace):
//   K_MM + jitter I, its factor and L^-1      the existing launchers (launch_kernel_matrix, launch_cholesky / launch_big_cholesky)
//   k_cov_prep      L_q (tril, zero padded), W := -I,  L^-1 copied into its padded image
//   W += L_q L_q^T  launch_gemm_plain
//   k_cov_a         A = L^-1 K(Z, X*), the K(Z, X*) tiles generated in LDS; mu = A^T m in the same pass
//   C = W A         launch_gemm_plain
//   k_cov_sigma     Sigma tile (i, j), j <= i: sum_m A[m,i] C[m,j] on the matrix cores + K(x_i, x_j) in the epilogue, mirrored
// tgp_qf_joint_sample_f64:  k_joint_jit (Sigma + jitter I) -> the existing Cholesky -> k_joint_draw.
// Every reduction has a fixed order and nothing is accumulated with atomics: two runs on the same input are bit-identical.
#include "tgp_dev.hpp"
#include "tgp_launch.hpp"
#include "tgp_tile.hpp"

namespace tgp {

// L_q = tril(Lam) and L^-1 in their zero-padded (MP x MP) images, W = -I on the first M diagonal entries (the product
// L_q L_q^T is added by the GEMM that follows).
__global__ __launch_bounds__(256) void k_cov_prep(const double* __restrict__ Lam, const double* __restrict__ Linv, int M, int MP,
                                                   double* __restrict__ Lq, double* __restrict__ W, double* __restrict__ LinvP) {
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  const int row = (int)(e / MP), col = (int)(e % MP);
  const bool in = row < M && col <= row;
  const size_t s = (size_t)row * M + col;
  Lq[e] = in ? Lam[s] : 0.0;
  LinvP[e] = in ? Linv[s] : 0.0;
  W[e] = (row == col && row < M) ? -1.0 : 0.0;
}

// A = L^-1 K(Z, X*) and mu = A^T m.  One workgroup per block of 64 columns (rows of X*); it walks the rows of A in groups of
// 64, so that mu is summed in one fixed order.  Per step of 16 contraction indices the tile of L^-1 is staged with 16-byte
// loads and the 16 x 64 tile of K(Z, X*) is evaluated into LDS from the scaled rows (the element function of tgp_dev.hpp);
// wave w owns columns 16 w .. 16 w + 15 and the four 16-row tiles of the group.  L^-1 is lower triangular: the contraction
// stops at the group's last row.  Rows m >= M of A come out as exact zeros (their rows of the padded L^-1 are zero),
// columns n >= N are written as zeros.
__global__ __launch_bounds__(256) void k_cov_a(int kernel, const double* __restrict__ X, int N, const double* __restrict__ Z, int M,
                                                int D, const double* __restrict__ raw_ls, const double* __restrict__ raw_os,
                                                const double* __restrict__ LinvP, int MP, const double* __restrict__ mvec,
                                                double* __restrict__ A, int NP, double* __restrict__ mu) {
  __shared__ __attribute__((aligned(16))) double Ls[TL_T * TL_LDK];
  __shared__ double Kt[TL_KC * TL_LDN];
  __shared__ double xsT[16 * TL_T];  // [d][column]: scaled rows of X*
  __shared__ double red[256];
  __shared__ double ils[TL_ILS];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, lr = lane & 15, lq = lane >> 4;
  const int n0 = blockIdx.x * TL_T;
  tile_scales(kernel, D, raw_ls, raw_os, ils);
  __syncthreads();
  for (int i = tid; i < 16 * TL_T; i += 256) {
    const int d = i >> 6, c = i & 63;
    const int n = n0 + c < N ? n0 + c : N - 1;  // clamped: columns past N are computed and never stored
    xsT[i] = d < D ? X[(size_t)n * D + d] * ils[d] : 0.0;
  }
  __syncthreads();
  const Cov cov = tile_cov(kernel, ils);
  const int gk = tid >> 4, gc = tid & 15;  // generation role: contraction index gk of the step, columns gc + 16 u
  const int M16 = (M + 15) / 16 * 16;
  double mup = 0.0;
  for (int mg = 0; mg < MP; mg += TL_T) {
    d4 acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = d4{0.0, 0.0, 0.0, 0.0};
    const int kend = mg < M ? (mg + TL_T < M16 ? mg + TL_T : M16) : 0;
    for (int k0 = 0; k0 < kend; k0 += TL_KC) {
#pragma unroll
      for (int u = 0; u < 2; ++u) {  // 64 rows x 16 k of L^-1: 512 pairs
        const int idx = tid + 256 * u, r = idx >> 3, c2 = (idx & 7) * 2;
        *reinterpret_cast<double2*>(Ls + r * TL_LDK + c2) =
            *reinterpret_cast<const double2*>(LinvP + (size_t)(mg + r) * MP + k0 + c2);
      }
      {
        const int kz = k0 + gk < M ? k0 + gk : M - 1;  // clamped: its row of L^-1 is zero
        double z[16];
#pragma unroll
        for (int d = 0; d < 16; ++d) z[d] = d < D ? Z[(size_t)kz * D + d] * ils[d] : 0.0;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int c = gc + 16 * u;
          double d2 = 0.0;
#pragma unroll
          for (int d = 0; d < 16; ++d) {  // (dimensions past D hold zeros on both sides: they add exact zeros)
            const double t = xsT[d * TL_T + c] - z[d];
            d2 += t * t;
          }
          Kt[gk * TL_LDN + c] = cov_value(cov, d2);
        }
      }
      __syncthreads();
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) {
        const double b = Kt[(kk * 4 + lq) * TL_LDN + 16 * w + lr];
#pragma unroll
        for (int t = 0; t < 4; ++t) acc[t] = TGP_MFMA(Ls[(16 * t + lr) * TL_LDK + kk * 4 + lq], b, acc[t]);
      }
      __syncthreads();
    }
    const int n = n0 + 16 * w + lr;
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int m = mg + 16 * t + lq + 4 * r;
        const double val = n < N ? acc[t][r] : 0.0;
        A[(size_t)m * NP + n] = val;
        mup += val * (m < M ? mvec[m] : 0.0);
      }
  }
  red[tid] = mup;
  __syncthreads();
  if (tid < 64) {
    const int w2 = tid >> 4, c = tid & 15, n = n0 + tid;
    const double s = ((red[w2 * 64 + c] + red[w2 * 64 + 16 + c]) + red[w2 * 64 + 32 + c]) + red[w2 * 64 + 48 + c];
    if (n < N) mu[n] = s;
  }
}

// Sigma tile (ti, tj), tj <= ti:  sum_m A[m,i] C[m,j]  +  K(x_i, x_j).  The [16 m][64] tiles of A and C are staged through LDS
// with 16-byte loads (the next step's loads are in flight while this step's MFMAs run); wave w holds rows 16 w .. 16 w + 15 of
// the tile against all 64 columns in four accumulators.  The epilogue adds the covariance of the two rows, parks the tile in
// LDS and writes it twice with coalesced stores: as (i, j) and transposed as (j, i).  A diagonal tile writes element (r, c)
// from the value computed for (max(r, c), min(r, c)): Sigma[i,j] == Sigma[j,i] bit for bit.  Rows and columns past N are masked.
__global__ __launch_bounds__(256) void k_cov_sigma(int kernel, const double* __restrict__ X, int N, int D,
                                                    const double* __restrict__ raw_ls, const double* __restrict__ raw_os,
                                                    const double* __restrict__ A, const double* __restrict__ C, int M16, int NP,
                                                    double* __restrict__ Sigma) {
  __shared__ __attribute__((aligned(16))) double buf[TL_T * TL_LDT];  // operand tiles (2 x 16 x 80), then the output tile
  __shared__ double xiT[16 * TL_T], xjT[16 * TL_T];
  __shared__ double ils[TL_ILS];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, lr = lane & 15, lq = lane >> 4;
  int ti, tj;
  tile_lower(blockIdx.x, ti, tj);
  const int i0 = ti * TL_T, j0 = tj * TL_T;
  tile_scales(kernel, D, raw_ls, raw_os, ils);
  __syncthreads();
  for (int i = tid; i < 16 * TL_T; i += 256) {
    const int d = i >> 6, c = i & 63;
    const int ni = i0 + c < N ? i0 + c : N - 1, nj = j0 + c < N ? j0 + c : N - 1;
    xiT[i] = d < D ? X[(size_t)ni * D + d] * ils[d] : 0.0;
    xjT[i] = d < D ? X[(size_t)nj * D + d] * ils[d] : 0.0;
  }
  const Cov cov = tile_cov(kernel, ils);
  double* At = buf;
  double* Ct = buf + TL_KC * TL_LDN;
  d4 acc[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) acc[c] = d4{0.0, 0.0, 0.0, 0.0};
  // (element pair u of a thread: row pr + 8 u of the step, columns pc2, pc2 + 1)
  const int pr = tid >> 5, pc2 = (tid & 31) * 2;
  const double* Ag = A + (size_t)pr * NP + i0 + pc2;
  const double* Cg = C + (size_t)pr * NP + j0 + pc2;
  const size_t half = (size_t)8 * NP;
  double2 pa0 = *reinterpret_cast<const double2*>(Ag), pa1 = *reinterpret_cast<const double2*>(Ag + half);
  double2 pc0 = *reinterpret_cast<const double2*>(Cg), pc1 = *reinterpret_cast<const double2*>(Cg + half);
  for (int k0 = 0; k0 < M16; k0 += TL_KC) {
    *reinterpret_cast<double2*>(At + pr * TL_LDN + pc2) = pa0;
    *reinterpret_cast<double2*>(At + (pr + 8) * TL_LDN + pc2) = pa1;
    *reinterpret_cast<double2*>(Ct + pr * TL_LDN + pc2) = pc0;
    *reinterpret_cast<double2*>(Ct + (pr + 8) * TL_LDN + pc2) = pc1;
    __syncthreads();
    if (k0 + TL_KC < M16) {
      Ag += (size_t)TL_KC * NP;
      Cg += (size_t)TL_KC * NP;
      pa0 = *reinterpret_cast<const double2*>(Ag);
      pa1 = *reinterpret_cast<const double2*>(Ag + half);
      pc0 = *reinterpret_cast<const double2*>(Cg);
      pc1 = *reinterpret_cast<const double2*>(Cg + half);
    }
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      const double a = At[(kk * 4 + lq) * TL_LDN + 16 * w + lr];
#pragma unroll
      for (int c = 0; c < 4; ++c) acc[c] = TGP_MFMA(a, Ct[(kk * 4 + lq) * TL_LDN + 16 * c + lr], acc[c]);
    }
    __syncthreads();
  }
  // epilogue: + K(x_i, x_j), tile to LDS
#pragma unroll
  for (int c = 0; c < 4; ++c)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int il = 16 * w + lq + 4 * r, jl = 16 * c + lr;
      double d2 = 0.0;
#pragma unroll
      for (int d = 0; d < 16; ++d) {
        const double u = xiT[d * TL_T + il] - xjT[d * TL_T + jl];
        d2 += u * u;
      }
      buf[il * TL_LDT + jl] = cov_value(cov, d2) + acc[c][r];
    }
  __syncthreads();
  if (ti != tj) {
    for (int e = tid; e < TL_T * TL_T; e += 256) {
      const int r = e >> 6, c = e & 63;
      if (i0 + r < N && j0 + c < N) Sigma[(size_t)(i0 + r) * N + j0 + c] = buf[r * TL_LDT + c];
    }
    for (int e = tid; e < TL_T * TL_T; e += 256) {
      const int c = e >> 6, r = e & 63;
      if (i0 + r < N && j0 + c < N) Sigma[(size_t)(j0 + c) * N + i0 + r] = buf[r * TL_LDT + c];
    }
  } else {
    for (int e = tid; e < TL_T * TL_T; e += 256) {
      const int r = e >> 6, c = e & 63;
      const int hi = r > c ? r : c, lo = r > c ? c : r;
      if (i0 + r < N && i0 + c < N) Sigma[(size_t)(i0 + r) * N + i0 + c] = buf[hi * TL_LDT + lo];
    }
  }
}

// Sj = Sigma + jitter I (the matrix the joint draw factorises)
__global__ __launch_bounds__(256) void k_joint_jit(const double* __restrict__ Sigma, int N, double jitter, double* __restrict__ Sj) {
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (size_t)N * N) return;
  Sj[e] = Sigma[e] + ((int)(e / N) == (int)(e % N) ? jitter : 0.0);
}

// F0 = mu + E L^T, E (S, N) standard normals, L (N, N) lower, F0 (S, N).  Workgroup = 16 samples x 64 columns, wave w the columns
// 16 w .. 16 w + 15; L is lower triangular, so the contraction stops at the tile's last column.  Tails in S, N and k are zero
// filled when the operands are staged.
__global__ __launch_bounds__(256) void k_joint_draw(const double* __restrict__ mu, const double* __restrict__ L, int N,
                                                     const double* __restrict__ E, int S, double* __restrict__ F0) {
  __shared__ double Et[16 * TL_LDK];
  __shared__ double Lt[TL_T * TL_LDK];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, lr = lane & 15, lq = lane >> 4;
  const int n0 = blockIdx.x * TL_T, s0 = blockIdx.y * 16;
  const int kend = n0 + TL_T < N ? n0 + TL_T : N;
  d4 acc = d4{0.0, 0.0, 0.0, 0.0};
  for (int k0 = 0; k0 < kend; k0 += TL_KC) {
    {
      const int r = tid >> 4, c = tid & 15, s = s0 + r, k = k0 + c;
      Et[r * TL_LDK + c] = (s < S && k < N) ? E[(size_t)s * N + k] : 0.0;
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int idx = tid + 256 * u, r = idx >> 4, c = idx & 15, n = n0 + r, k = k0 + c;
      Lt[r * TL_LDK + c] = (n < N && k <= n) ? L[(size_t)n * N + k] : 0.0;
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < 4; ++kk)
      acc = TGP_MFMA(Et[lr * TL_LDK + kk * 4 + lq], Lt[(16 * w + lr) * TL_LDK + kk * 4 + lq], acc);
    __syncthreads();
  }
  const int n = n0 + 16 * w + lr;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int s = s0 + lq + 4 * r;
    if (s < S && n < N) F0[(size_t)s * N + n] = mu[n] + acc[r];
  }
}

// ---- host side ----------------------------------------------------------------------------------------------------
namespace {
struct CovPlan : Layout {
  int MP, NP;
  KzzSections kzz;
  size_t LinvP, Lq, W, A, C;
};
bool cov_plan(CovPlan& p, int N, int D, int M) {
  if (N < 1 || N > TGP_BIG_MAX_M || !inducing_limits(M, D)) return false;
  p.MP = (int)rup((size_t)M, 128);
  p.NP = (int)rup((size_t)N, 128);
  const size_t pp = (size_t)p.MP * p.MP, pn = (size_t)p.MP * p.NP;
  p.kzz.take(p, M);
  p.LinvP = p.take(pp);
  p.Lq = p.take(pp);
  p.W = p.take(pp);
  p.A = p.take(pn);
  p.C = p.take(pn);
  return true;
}
struct DrawPlan : Layout {
  size_t Sj, Lf, chol, chol_len;
};
bool draw_plan(DrawPlan& p, int N, int S) {
  if (N < 1 || N > TGP_BIG_MAX_M || S < 1 || S > 4096) return false;
  p.chol_len = chol_ws_doubles(N);
  p.Sj = p.take((size_t)N * N);
  p.Lf = p.take((size_t)N * N);
  p.chol = p.take(p.chol_len);
  return true;
}
}  // namespace

size_t qf_cov_workspace_bytes(int N, int D, int M) {
  CovPlan p;
  return cov_plan(p, N, D, M) ? p.bytes() : 0;
}

size_t qf_joint_sample_workspace_bytes(int N, int S) {
  DrawPlan p;
  return draw_plan(p, N, S) ? p.bytes() : 0;
}

int launch_cov_prep(const double* Lam, const double* Linv, int M, int MP, double* Lq, double* W, double* LinvP, hipStream_t st) {
  hipLaunchKernelGGL(k_cov_prep, dim3((unsigned)((size_t)MP * MP / 256)), dim3(256), 0, st, Lam, Linv, M, MP, Lq, W, LinvP);
  LAUNCH_CHECK();
  return launch_gemm_plain(false, true, 0, MP, MP, MP, 1.0, Lq, MP, Lq, MP, 1.0, W, MP, st);
}

int launch_cov_a(const tgp_model& md, const double* X, int rows, const double* LinvP, int MP, double* A, int NP, double* mu,
                 hipStream_t st) {
  hipLaunchKernelGGL(k_cov_a, dim3((unsigned)(NP / TL_T)), dim3(256), 0, st, md.kernel, X, rows, md.Z, md.M, md.D, md.raw_ls,
                     md.raw_os, LinvP, MP, md.m, A, NP, mu);
  LAUNCH_CHECK();
  return 0;
}

int launch_qf_cov(const tgp_model& md, const double* X, double* mu, double* Sigma, int32_t* status, void* workspace,
                  size_t workspace_bytes, hipStream_t st) {
  CovPlan p;
  if (!cov_plan(p, md.N, md.D, md.M)) return TGP_E_UNSUPPORTED;  // (tgp_qf_cov_f64 has named the limits)
  double* ws;
  if (int rc = open_workspace("tgp_qf_cov_f64", "tgp_qf_cov_workspace_bytes", workspace, workspace_bytes, p.total, &ws)) return rc;
  const int N = md.N, D = md.D, M = md.M, MP = p.MP, NP = p.NP;
  if (int rc = p.kzz.factor(md, ws, status, st)) return rc;
  if (int rc = launch_cov_prep(md.Lam, ws + p.kzz.Linv, M, MP, ws + p.Lq, ws + p.W, ws + p.LinvP, st)) return rc;
  if (int rc = launch_cov_a(md, X, N, ws + p.LinvP, MP, ws + p.A, NP, mu, st)) return rc;
  if (int rc = launch_gemm_plain(false, false, 0, MP, NP, MP, 1.0, ws + p.W, MP, ws + p.A, NP, 0.0, ws + p.C, NP, st)) return rc;
  const int nt = (N + TL_T - 1) / TL_T;
  hipLaunchKernelGGL(k_cov_sigma, dim3((unsigned)(nt * (nt + 1) / 2)), dim3(256), 0, st, md.kernel, X, N, D, md.raw_ls, md.raw_os,
                     ws + p.A, ws + p.C, (M + 15) / 16 * 16, NP, Sigma);
  LAUNCH_CHECK();
  return 0;
}

int launch_qf_joint_sample(const double* mu, const double* Sigma, int N, double jitter, const double* eps, int S, double* F0,
                           double* Lsig, int32_t* status, void* workspace, size_t workspace_bytes, hipStream_t st) {
  DrawPlan p;
  if (!draw_plan(p, N, S)) return TGP_E_UNSUPPORTED;  // (tgp_qf_joint_sample_f64 has named the limits)
  double* ws;
  if (int rc = open_workspace("tgp_qf_joint_sample_f64", "tgp_qf_joint_sample_workspace_bytes", workspace, workspace_bytes, p.total,
                              &ws))
    return rc;
  double* Lf = Lsig != nullptr ? Lsig : ws + p.Lf;
  hipLaunchKernelGGL(k_joint_jit, dim3((unsigned)(((size_t)N * N + 255) / 256)), dim3(256), 0, st, Sigma, N, jitter, ws + p.Sj);
  LAUNCH_CHECK();
  if (int rc = launch_cholesky_any(ws + p.Sj, N, Lf, nullptr, status, ws + p.chol, p.chol_len, st)) return rc;
  hipLaunchKernelGGL(k_joint_draw, dim3((unsigned)((N + TL_T - 1) / TL_T), (unsigned)((S + 15) / 16)), dim3(256), 0, st, mu, Lf, N,
                     eps, S, F0);
  LAUNCH_CHECK();
  return 0;
}

}  // namespace tgp
