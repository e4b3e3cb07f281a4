// tgp_xgrad.hip -- input gradients of the q(f) marginals (tgp_qf_input_grad_f64): d mu_n / d x_nd and d v_n / d x_nd.
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
}  // namespace

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
