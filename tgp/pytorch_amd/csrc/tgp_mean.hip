// tgp_mean.hip -- the linear and identity mean functions (tgp_mean_forward_f64, tgp_mean_backward_f64).
//
// The reference's model class takes a mean m(x) = x a + b ('linear', a and b trainable) or m(x) = x W ('identity', W a fixed
// projection), models/means.py, and uses it in three places: mu_qf = ... + m(X) (models/sparse_MF_SP.py:314,355,360), m - m(Z)
// in the unwhitened mean (:359) and p(u) = N(m(Z), K_ZZ) in the unwhitened KL (:446).  Dy = 1: a is a vector of D entries.
//   forward   k_mean_fwd       out[n ld + col] = alpha (sum_d x_nd a_d + b) + in[n], optionally 1.0 beside it: the (N, 2) row
//                              parameters (1, m(x_n)) of a per-row TGP_FLOW_AFFINE block, Y - m(X), or mu + m(X)
//   backward  k_mean_bwd       g_X[n, d] = g_n a_d, and per workgroup the partial sums of g_n x_nd (d < D) and of g_n
//             k_mean_bwd_fin   the partials summed in workgroup order: g_a, g_b
// One data row per lane, consecutive lanes on consecutive rows: a wave reads 64 D contiguous doubles of X.  Every sum has a
// fixed order and the grids depend on N only (never on the CU count), nothing is accumulated with atomics: same input, same
// bits, on any device.  Both kernels move N (D + 2) doubles and are launch-latency bound at the sizes of a training step.
#include "tgp_dev.hpp"
#include "tgp_launch.hpp"

namespace tgp {

#define MEAN_TPB 256  /* threads per workgroup                                            */
#define MEAN_RPL 4    /* backward: rows per lane; a workgroup owns MEAN_TPB * MEAN_RPL rows */
#define MEAN_NP 17    /* partial sums per workgroup: 16 slots of g_a, then g_b            */

__global__ __launch_bounds__(MEAN_TPB) void k_mean_fwd(const double* __restrict__ X, int N, int D, const double* __restrict__ a,
                                                        const double* __restrict__ b, double alpha, const double* __restrict__ in,
                                                        double* __restrict__ out, int ld, int col, int one_col) {
  __shared__ double ab[MEAN_NP];
  const int tid = threadIdx.x;
  if (tid < 16) ab[tid] = tid < D ? a[tid] : 0.0;
  if (tid == 64) ab[16] = b != nullptr ? b[0] : 0.0;
  __syncthreads();
  const long n = (long)blockIdx.x * MEAN_TPB + tid;
  if (n >= N) return;
  const double* x = X + (size_t)n * D;
  double s = 0.0;
  for (int d = 0; d < D; ++d) s += x[d] * ab[d];  // in the order d = 0 .. D-1
  double r = alpha * (s + ab[16]);
  if (in != nullptr) r += in[n];
  out[(size_t)n * ld + col] = r;
  if (one_col >= 0) out[(size_t)n * ld + one_col] = 1.0;
}

// Workgroup w owns rows [1024 w, 1024 w + 1024): lane t sums its rows 1024 w + t + 256 i, i = 0 .. 3, in that order into
// D + 1 registers; the wave butterfly; the four waves in order through LDS; part[w][0 .. 16].
__global__ __launch_bounds__(MEAN_TPB) void k_mean_bwd(const double* __restrict__ X, int N, int D, const double* __restrict__ a,
                                                        const double* __restrict__ g, int ldg, int colg, double* __restrict__ g_X,
                                                        double* __restrict__ part) {
  __shared__ double as[16];
  __shared__ double red[MEAN_TPB / 64][MEAN_NP];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  if (tid < 16) as[tid] = (g_X != nullptr && tid < D) ? a[tid] : 0.0;
  __syncthreads();
  double acc[16], accb = 0.0;
#pragma unroll
  for (int d = 0; d < 16; ++d) acc[d] = 0.0;
  const long base = (long)blockIdx.x * (MEAN_TPB * MEAN_RPL) + tid;
  for (int i = 0; i < MEAN_RPL; ++i) {
    const long n = base + (long)i * MEAN_TPB;
    if (n >= N) break;
    const double gn = g[(size_t)n * ldg + colg];
    const double* x = X + (size_t)n * D;
    accb += gn;
#pragma unroll
    for (int d = 0; d < 16; ++d)
      if (d < D) {
        acc[d] += gn * x[d];
        if (g_X != nullptr) g_X[(size_t)n * D + d] = gn * as[d];
      }
  }
#pragma unroll
  for (int d = 0; d < 16; ++d) {
    const double t = wave_sum(acc[d]);
    if (lane == 0) red[w][d] = t;
  }
  accb = wave_sum(accb);
  if (lane == 0) red[w][16] = accb;
  __syncthreads();
  if (tid < MEAN_NP) {
    double t = red[0][tid];
#pragma unroll
    for (int k = 1; k < MEAN_TPB / 64; ++k) t += red[k][tid];
    part[(size_t)blockIdx.x * MEAN_NP + tid] = t;
  }
}

// Thread o sums slot o of the G workgroup partials in workgroup order.
__global__ __launch_bounds__(64) void k_mean_bwd_fin(const double* __restrict__ part, int G, int D, double* __restrict__ g_a,
                                                      double* __restrict__ g_b) {
  const int o = threadIdx.x;
  if (o >= MEAN_NP || (o < 16 && o >= D) || (o == 16 && g_b == nullptr)) return;
  double t = 0.0;
  for (int w = 0; w < G; ++w) t += part[(size_t)w * MEAN_NP + o];
  if (o < 16)
    g_a[o] = t;
  else
    g_b[0] = t;
}

namespace {
inline int mean_bwd_groups(int N) { return (int)(((long)N + MEAN_TPB * MEAN_RPL - 1) / (MEAN_TPB * MEAN_RPL)); }
}  // namespace

size_t mean_backward_workspace_bytes(int N, int D) {
  if (N < 1 || D < 1 || D > 16) return 0;
  return (size_t)mean_bwd_groups(N) * MEAN_NP * sizeof(double);
}

int launch_mean_forward(const double* X, int N, int D, const double* a, const double* b, double alpha, const double* in,
                        double* out, int ld, int col, int one_col, hipStream_t st) {
  const unsigned nb = (unsigned)(((long)N + MEAN_TPB - 1) / MEAN_TPB);
  hipLaunchKernelGGL(k_mean_fwd, dim3(nb), dim3(MEAN_TPB), 0, st, X, N, D, a, b, alpha, in, out, ld, col, one_col);
  LAUNCH_CHECK();
  return 0;
}

int launch_mean_backward(const double* X, int N, int D, const double* a, const double* g, int ldg, int colg, double* g_a,
                         double* g_b, double* g_X, double* part, hipStream_t st) {
  const int G = mean_bwd_groups(N);
  hipLaunchKernelGGL(k_mean_bwd, dim3((unsigned)G), dim3(MEAN_TPB), 0, st, X, N, D, a, g, ldg, colg, g_X, part);
  LAUNCH_CHECK();
  hipLaunchKernelGGL(k_mean_bwd_fin, dim3(1), dim3(64), 0, st, part, G, D, g_a, g_b);
  LAUNCH_CHECK();
  return 0;
}

}  // namespace tgp
