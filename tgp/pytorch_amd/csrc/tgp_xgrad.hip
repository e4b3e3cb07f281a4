// tgp_xgrad.hip -- input gradients of the q(f) marginals (tgp_qf_input_grad_f64): d mu_n / d x_nd and d v_n / d x_nd, and the
// variance of the derivative process under q(f) (tgp_qf_input_grad_var_f64).
//
// With K_ZZ + jitter I = L L^T, A = L^-1 K(Z, X), W = tril(Lam) tril(Lam)^T - I, C = W A (the operands of tgp_cov.hip),
// a = L^-T m and U = L^-T C (M x N):
//   mu_n = sum_m k_nm a_m,   v_n = s2 + sum_m k_nm U_mn
//   J[n,m,d] = dk(x_n, z_m) / dx_nd = -k_g(d2_nm) (x_nd - z_md) / l_d^2        (k_g = -2 dk/d(d2): cov_gweight, tgp_dev.hpp)
//   dmu[n,d] = sum_m J[n,m,d] a_m,   dv[n,d] = 2 sum_m J[n,m,d] U_mn
// U is held fixed in the second sum: v_n = s2 + k_n^T B k_n with the symmetric B = L^-T W L^-1, whose derivative is 2 J^T B k_n.
//
// Launch sequence (one stream, no host sync; operands padded to multiples of 128 in the workspace):
//   K_ZZ + jitter I, its factor and L^-1      KzzSections::factor
//   k_cov_prep, W += L_q L_q^T                launch_cov_prep (tgp_cov.hip)
//   k_xgrad_a                                 a = L^-T m
//   per pass of TGP_XGRAD_PASS_ROWS rows:
//     k_cov_a        A = L^-1 K(Z, X_pass)    launch_cov_a (tgp_cov.hip; its mu goes to scratch)
//     C = W A, U = L^-T C                     launch_gemm_plain twice (U takes A's place)
//     k_xgrad<DP>    the two Jacobians of the pass's rows
// Every reduction has a fixed order and nothing is accumulated with atomics: two runs on the same input are bit-identical, and
// a row's result does not depend on N or on the pass it falls in (the GEMMs contract over m in an order fixed by M alone).
//
// The variance of the derivative process (tgp_qf_input_grad_var_f64), the error bar of dmu: with the symmetric B = L^-T W L^-1 the
// posterior covariance is Sigma(x, x') = k(x, x') + k(x, Z) B k(Z, x'), and its mixed derivative in x_d, x'_d at x' = x is
//   dvar[n,d] = k_g(0) / l_d^2 + sum_{m,m'} J[n,m,d] B[m,m'] J[n,m',d]
// Launch sequence: the same prologue and k_cov_prep, then per pass and per input dimension d
//   k_xgrad_va       A_d = L^-1 J_d^T (M x rows), the tiles of J_d generated on chip
//   C_d = W A_d      launch_gemm_plain
//   k_xgrad_vcol     dvar[n,d] = k_g(0) / l_d^2 + sum_m A_d[m,n] C_d[m,n], m ascending
// with the same guarantees: fixed orders, no atomics, a row's result independent of N and of its pass.
#include "tgp_dev.hpp"
#include "tgp_launch.hpp"
#include "tgp_tile.hpp"

namespace tgp {

constexpr int XG_ROWS = 16;  // rows of X per workgroup: N = 957 still gives 60 workgroups, and a 16-lane group reads 128 contiguous bytes of U
constexpr int XG_MC = 64;    // inducing points staged per step
constexpr int XG_SL = 256 / XG_ROWS;  // slices of m per workgroup (16): thread (r, sl) takes m = sl, sl + 16, ... of each step

// a = L^-T m: a[j] = sum_{i >= j} L^-1[i,j] m[i], one thread per j, i ascending
__global__ __launch_bounds__(256) void k_xgrad_a(const double* __restrict__ Linv, const double* __restrict__ mvec, int M,
                                                  double* __restrict__ a) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= M) return;
  double s = 0.0;
  for (int i = j; i < M; ++i) s += Linv[(size_t)i * M + j] * mvec[i];
  a[j] = s;
}

// dmu, dv of the rows n0 .. n0 + 15.  Thread (r, sl): row n0 + r against the inducing points m = m0 + sl + 16 j of each step of
// 64, whose scaled rows are staged in LDS (a 16-lane group reads one of them: a broadcast); it forms t_d = (x_nd - z_md) / l_d
// directly, d2 = sum t_d^2, k_g(d2), and keeps sum_m k_g a_m t_d and sum_m k_g U_mn t_d (2 DP accumulators) in registers.  The 16
// slices of a row are added in a fixed order: the four of a wave by two cross-lane adds, the four waves through LDS.  The
// factor -1 / l_d (and the 2 of dv) is applied once, at the store.  U is read row-contiguous over n: 128 bytes per 16-lane group.
template <int DP>
__global__ __launch_bounds__(256) void k_xgrad(int kernel, const double* __restrict__ X, int N, const double* __restrict__ Z, int M,
                                                int D, const double* __restrict__ raw_ls, const double* __restrict__ raw_os,
                                                const double* __restrict__ a, const double* __restrict__ U, int NP,
                                                double* __restrict__ dmu, double* __restrict__ dv) {
  constexpr int LDZ = DP + 1;  // the four rows of Z a wave reads together fall in distinct banks
  __shared__ double zs[XG_MC * LDZ];
  __shared__ double as[XG_MC];
  __shared__ double red[4 * 2 * DP * XG_ROWS];
  __shared__ double ils[TL_ILS];
  const int tid = threadIdx.x, r = tid & (XG_ROWS - 1), sl = tid / XG_ROWS, lane = tid & 63, w = tid >> 6;
  const int n0 = blockIdx.x * XG_ROWS;
  const int nc = n0 + r < N ? n0 + r : N - 1;  // clamped: rows past N are computed and never stored
  tile_scales(kernel, D, raw_ls, raw_os, ils);
  __syncthreads();
  const Cov cov = tile_cov(kernel, ils);
  double x[DP], gm[DP], gv[DP];
#pragma unroll
  for (int d = 0; d < DP; ++d) {
    x[d] = d < D ? X[(size_t)nc * D + d] * ils[d] : 0.0;
    gm[d] = 0.0;
    gv[d] = 0.0;
  }
  for (int m0 = 0; m0 < M; m0 += XG_MC) {
    for (int i = tid; i < XG_MC * DP; i += 256) {
      const int c = i / DP, d = i % DP, m = m0 + c;
      zs[c * LDZ + d] = (m < M && d < D) ? Z[(size_t)m * D + d] * ils[d] : 0.0;
    }
    if (tid < XG_MC) as[tid] = m0 + tid < M ? a[m0 + tid] : 0.0;
    __syncthreads();
#pragma unroll
    for (int j = 0; j < XG_MC / XG_SL; ++j) {
      const int c = sl + XG_SL * j, m = m0 + c;
      if (m < M) {
        double t[DP], d2 = 0.0;
#pragma unroll
        for (int d = 0; d < DP; ++d) {  // (dimensions past D hold zeros on both sides: they add exact zeros)
          t[d] = x[d] - zs[c * LDZ + d];
          d2 += t[d] * t[d];
        }
        const double kg = cov_gweight(cov, d2);
        const double wa = kg * as[c], wu = kg * U[(size_t)m * NP + n0 + r];
#pragma unroll
        for (int d = 0; d < DP; ++d) {
          gm[d] += wa * t[d];
          gv[d] += wu * t[d];
        }
      }
    }
    __syncthreads();
  }
  // the wave's four slices (lanes r, r + 16, r + 32, r + 48), then the four waves
#pragma unroll
  for (int d = 0; d < DP; ++d) {
    gm[d] += __shfl_xor(gm[d], 16);
    gm[d] += __shfl_xor(gm[d], 32);
    gv[d] += __shfl_xor(gv[d], 16);
    gv[d] += __shfl_xor(gv[d], 32);
  }
  if (lane < XG_ROWS) {
#pragma unroll
    for (int d = 0; d < DP; ++d) {
      red[(w * 2 * DP + d) * XG_ROWS + r] = gm[d];
      red[(w * 2 * DP + DP + d) * XG_ROWS + r] = gv[d];
    }
  }
  __syncthreads();
  for (int i = tid; i < 2 * DP * XG_ROWS; i += 256) {
    const int rr = i / (2 * DP), k = i % (2 * DP), d = k % DP, n = n0 + rr;  // (consecutive threads: consecutive d of a row)
    if (n >= N || d >= D) continue;
    const int o = k * XG_ROWS + rr, st = 2 * DP * XG_ROWS;
    const double s = ((red[o] + red[st + o]) + red[2 * st + o]) + red[3 * st + o];
    if (k < DP) dmu[(size_t)n * D + d] = -ils[d] * s;
    else dv[(size_t)n * D + d] = -2.0 * ils[d] * s;
  }
}

// A_d = L^-1 J_d^T for one input dimension d (M x rows), J_d[n,m] = dk(x_n, z_m) / dx_nd = -k_g(d2_nm) (x_nd - z_md) / l_d^2:
// k_cov_a's walk (tgp_cov.hip: 64 columns per workgroup, groups of 64 rows of A, steps of 16 contraction indices, the tile of
// L^-1 staged with 16-byte loads, the contraction cut at the group's last row) with the 16 x 64 tile of J_d^T generated in LDS
// in the place of K(Z, X*); J never reaches HBM.  (x - z) is formed directly from the scaled rows: a row of X that is a row of Z
// bit for bit gives an exact zero there.  Rows m >= M of A_d come out as exact zeros, columns n >= rows are written as zeros.
__global__ __launch_bounds__(256) void k_xgrad_va(int kernel, const double* __restrict__ X, int N, const double* __restrict__ Z,
                                                   int M, int D, int dsel, const double* __restrict__ raw_ls,
                                                   const double* __restrict__ raw_os, const double* __restrict__ LinvP, int MP,
                                                   double* __restrict__ A, int NP) {
  __shared__ __attribute__((aligned(16))) double Ls[TL_T * TL_LDK];
  __shared__ double Jt[TL_KC * TL_LDN];
  __shared__ double xsT[16 * TL_T];  // [d][column]: scaled rows of X
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
  const double il = ils[dsel];
  const int gk = tid >> 4, gc = tid & 15;  // generation role: contraction index gk of the step, columns gc + 16 u
  const int M16 = (M + 15) / 16 * 16;
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
        const double zd = Z[(size_t)kz * D + dsel] * il;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int c = gc + 16 * u;
          double d2 = 0.0;
#pragma unroll
          for (int d = 0; d < 16; ++d) {  // (dimensions past D hold zeros on both sides: they add exact zeros)
            const double t = xsT[d * TL_T + c] - z[d];
            d2 += t * t;
          }
          Jt[gk * TL_LDN + c] = -((cov_gweight(cov, d2) * (xsT[dsel * TL_T + c] - zd)) * il);
        }
      }
      __syncthreads();
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) {
        const double b = Jt[(kk * 4 + lq) * TL_LDN + 16 * w + lr];
#pragma unroll
        for (int t = 0; t < 4; ++t) acc[t] = TGP_MFMA(Ls[(16 * t + lr) * TL_LDK + kk * 4 + lq], b, acc[t]);
      }
      __syncthreads();
    }
    const int n = n0 + 16 * w + lr;
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) A[(size_t)(mg + 16 * t + lq + 4 * r) * NP + n] = n < N ? acc[t][r] : 0.0;
  }
}

// dvar[n,d] = k_g(0) / l_d^2 + sum_m A_d[m,n] C_d[m,n], C_d = W A_d: one thread per row n, m ascending (consecutive threads read
// consecutive n: coalesced).  The value is stored as computed, never clamped.
__global__ __launch_bounds__(64) void k_xgrad_vcol(int kernel, const double* __restrict__ raw_ls, const double* __restrict__ raw_os,
                                                    const double* __restrict__ A, const double* __restrict__ C, int M, int NP,
                                                    int rows, int D, int dsel, double* __restrict__ dvar) {
  const int n = blockIdx.x * 64 + threadIdx.x;
  if (n >= rows) return;
  const double il = 1.0 / softplus_d(raw_ls[dsel]);
  const Cov cov = make_cov(kernel, softplus_d(raw_os[0]), cov_alpha(kernel, raw_os));
  double s = 0.0;
  for (int m = 0; m < M; ++m) s += A[(size_t)m * NP + n] * C[(size_t)m * NP + n];
  dvar[(size_t)n * D + dsel] = cov_gweight(cov, 0.0) * il * il + s;
}

// ---- host side ----------------------------------------------------------------------------------------------------
namespace {
struct XgradPlan : Layout {
  int MP, NP;  // NP: the padded rows of one pass
  KzzSections kzz;
  size_t LinvP, Lq, W, a, mu, A, C;
};
bool xgrad_plan(XgradPlan& p, int N, int D, int M) {
  if (N < 1 || !inducing_limits(M, D)) return false;
  p.MP = (int)rup((size_t)M, 128);
  p.NP = (int)rup((size_t)(N < TGP_XGRAD_PASS_ROWS ? N : TGP_XGRAD_PASS_ROWS), 128);
  const size_t pp = (size_t)p.MP * p.MP, pn = (size_t)p.MP * p.NP;
  p.kzz.take(p, M);
  p.LinvP = p.take(pp);
  p.Lq = p.take(pp);
  p.W = p.take(pp);
  p.a = p.take((size_t)M);
  p.mu = p.take((size_t)p.NP);
  p.A = p.take(pn);
  p.C = p.take(pn);
  return true;
}
// the slope variance: the same sections without a, mu
struct XgradVarPlan : Layout {
  int MP, NP;  // NP: the padded rows of one pass
  KzzSections kzz;
  size_t LinvP, Lq, W, A, C;
};
bool xgrad_var_plan(XgradVarPlan& p, int N, int D, int M) {
  if (N < 1 || !inducing_limits(M, D)) return false;
  p.MP = (int)rup((size_t)M, 128);
  p.NP = (int)rup((size_t)(N < TGP_XGRAD_PASS_ROWS ? N : TGP_XGRAD_PASS_ROWS), 128);
  const size_t pp = (size_t)p.MP * p.MP, pn = (size_t)p.MP * p.NP;
  p.kzz.take(p, M);
  p.LinvP = p.take(pp);
  p.Lq = p.take(pp);
  p.W = p.take(pp);
  p.A = p.take(pn);
  p.C = p.take(pn);
  return true;
}
}  // namespace

size_t qf_input_grad_var_workspace_bytes(int N, int D, int M) {
  XgradVarPlan p;
  return xgrad_var_plan(p, N, D, M) ? p.bytes() : 0;
}

int launch_qf_input_grad_var(const tgp_model& md, const double* X, double* dvar, int32_t* status, void* workspace,
                             size_t workspace_bytes, hipStream_t st) {
  XgradVarPlan p;
  if (!xgrad_var_plan(p, md.N, md.D, md.M)) return TGP_E_UNSUPPORTED;  // (tgp_qf_input_grad_var_f64 has named the limits)
  double* ws;
  if (int rc = open_workspace("tgp_qf_input_grad_var_f64", "tgp_qf_input_grad_var_workspace_bytes", workspace, workspace_bytes,
                              p.total, &ws))
    return rc;
  const int N = md.N, D = md.D, M = md.M, MP = p.MP;
  if (int rc = p.kzz.factor(md, ws, status, st)) return rc;
  if (int rc = launch_cov_prep(md.Lam, ws + p.kzz.Linv, M, MP, ws + p.Lq, ws + p.W, ws + p.LinvP, st)) return rc;
  for (int r0 = 0; r0 < N; r0 += TGP_XGRAD_PASS_ROWS) {
    const int rows = N - r0 < TGP_XGRAD_PASS_ROWS ? N - r0 : TGP_XGRAD_PASS_ROWS;
    const int NP = (int)rup((size_t)rows, 128);
    const double* Xp = X + (size_t)r0 * D;
    for (int d = 0; d < D; ++d) {
      hipLaunchKernelGGL(k_xgrad_va, dim3((unsigned)(NP / TL_T)), dim3(256), 0, st, md.kernel, Xp, rows, md.Z, M, D, d, md.raw_ls,
                         md.raw_os, ws + p.LinvP, MP, ws + p.A, NP);
      LAUNCH_CHECK();
      if (int rc = launch_gemm_plain(false, false, 0, MP, NP, MP, 1.0, ws + p.W, MP, ws + p.A, NP, 0.0, ws + p.C, NP, st)) return rc;
      hipLaunchKernelGGL(k_xgrad_vcol, dim3((unsigned)((rows + 63) / 64)), dim3(64), 0, st, md.kernel, md.raw_ls, md.raw_os, ws + p.A,
                         ws + p.C, M, NP, rows, D, d, dvar + (size_t)r0 * D);
      LAUNCH_CHECK();
    }
  }
  return 0;
}

size_t qf_input_grad_workspace_bytes(int N, int D, int M) {
  XgradPlan p;
  return xgrad_plan(p, N, D, M) ? p.bytes() : 0;
}

int launch_qf_input_grad(const tgp_model& md, const double* X, double* dmu, double* dv, int32_t* status, void* workspace,
                         size_t workspace_bytes, hipStream_t st) {
  XgradPlan p;
  if (!xgrad_plan(p, md.N, md.D, md.M)) return TGP_E_UNSUPPORTED;  // (tgp_qf_input_grad_f64 has named the limits)
  double* ws;
  if (int rc = open_workspace("tgp_qf_input_grad_f64", "tgp_qf_input_grad_workspace_bytes", workspace, workspace_bytes, p.total, &ws))
    return rc;
  const int N = md.N, D = md.D, M = md.M, MP = p.MP;
  if (int rc = p.kzz.factor(md, ws, status, st)) return rc;
  if (int rc = launch_cov_prep(md.Lam, ws + p.kzz.Linv, M, MP, ws + p.Lq, ws + p.W, ws + p.LinvP, st)) return rc;
  hipLaunchKernelGGL(k_xgrad_a, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, st, ws + p.kzz.Linv, md.m, M, ws + p.a);
  LAUNCH_CHECK();
  double* const U = ws + p.A;  // (A is dead once C = W A is formed)
  for (int r0 = 0; r0 < N; r0 += TGP_XGRAD_PASS_ROWS) {
    const int rows = N - r0 < TGP_XGRAD_PASS_ROWS ? N - r0 : TGP_XGRAD_PASS_ROWS;
    const int NP = (int)rup((size_t)rows, 128);
    const double* Xp = X + (size_t)r0 * D;
    if (int rc = launch_cov_a(md, Xp, rows, ws + p.LinvP, MP, ws + p.A, NP, ws + p.mu, st)) return rc;
    if (int rc = launch_gemm_plain(false, false, 0, MP, NP, MP, 1.0, ws + p.W, MP, ws + p.A, NP, 0.0, ws + p.C, NP, st)) return rc;
    if (int rc = launch_gemm_plain(true, false, 0, MP, NP, MP, 1.0, ws + p.LinvP, MP, ws + p.C, NP, 0.0, U, NP, st)) return rc;
    const dim3 grid((unsigned)((rows + XG_ROWS - 1) / XG_ROWS));
    int rc = 0;
    dispatch_dp(D, [&](auto dp) {
      hipLaunchKernelGGL(k_xgrad<decltype(dp)::value>, grid, dim3(256), 0, st, md.kernel, Xp, rows, md.Z, M, D, md.raw_ls, md.raw_os,
                         ws + p.a, U, NP, dmu + (size_t)r0 * D, dv + (size_t)r0 * D);
      const hipError_t e = hipGetLastError();
      if (e != hipSuccess) rc = set_error(e, __FILE__, __LINE__);
    });
    if (rc) return rc;
  }
  return 0;
}

}  // namespace tgp
