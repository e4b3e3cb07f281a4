// tgp_greedy.hip -- greedy conditional-variance selection of inducing points (tgp_greedy_inducing_f64): the pivoted Cholesky
// factorisation of K_XX (Burt, Rasmussen, van der Wilk 2020), which picks the M data rows that most reduce tr(K_XX - Q_XX).
//
// Start with d_n = s2 for all rows and no picked rows.  For j = 0 .. M-1:
//   1. p_j = argmax_n d_n over rows not yet picked; ties go to the smallest index (step 0 is an exact tie: p_0 = 0)
//   2. if d_{p_j} <= min_var, stop: M_eff = j
//   3. c_n = (k(x_n, x_{p_j}) - sum_{l<j} C[l,n] C[l,p_j]) / sqrt(d_{p_j}), the sum in the order of l
//   4. C[j,n] = c_n
//   5. d_n <- max(d_n - c_n^2, 0)
//   6. row p_j is marked picked (d = -1): it never competes again and adds nothing to the trace
//   7. trace[j+1] = sum_{n not picked} d_n;  trace[0] = N s2
//
// One launch per step (k_greedy_step), then k_greedy_fin; the host enqueues all M + 1 without reading anything back.  A lane owns
// a data row; the grid is ceil(N / 256), a function of N alone.  The hand-over between steps is the launch boundary and nothing
// else: launch j leaves one (largest d, its smallest index, sum of d) record per workgroup, and EVERY workgroup of launch j + 1
// reduces those records itself in its prologue, all in the same order, so all reach the same pivot p_{j+1} and trace[j+1].  The
// records alternate between two buffers by the parity of j: a workgroup of launch j + 1 writes its record while others still read
// launch j's.  No grid barrier, no workgroup waits on another, no ticket, no float atomics: same input, same bits on any device.
// A stop is sticky: workgroup 0 of the launch that finds d_max <= min_var writes M_eff to a device word (launch 0 re-initialises
// it), every later launch reads that word first and returns.
#include <climits>

#include "tgp_dev.hpp"
#include "tgp_launch.hpp"
#include "tgp_tile.hpp"

namespace tgp {

#define GR_WG 256  /* lanes = data rows per workgroup                                                             */
#define GR_REC 4   /* doubles per workgroup record: largest d, sum of d, index of the largest (exact in a double), pad */
#define GR_HEAD 48 /* doubles of LDS in front of the pivot column: scaled pivot row [16], 1 / length-scale [16], wave records [16] */

// (v, i) <- the better of (v, i) and (v2, i2): the larger value, at equal values the smaller index
__device__ __forceinline__ void gr_take(double& v, int& i, double v2, int i2) {
  if (v2 > v || (v2 == v && i2 < i)) {
    v = v2;
    i = i2;
  }
}

// The workgroup's (largest value, its smallest index, sum): a wave butterfly, then the four waves in order through LDS.  Every
// thread returns the same triple.  Lanes with nothing to offer pass (-1, INT_MAX, 0).
__device__ __forceinline__ void gr_reduce(double& v, int& i, double& s, double* red) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const double v2 = __shfl_xor(v, o, 64);
    const int i2 = __shfl_xor(i, o, 64);
    s += __shfl_xor(s, o, 64);
    gr_take(v, i, v2, i2);
  }
  const int w = threadIdx.x >> 6;
  __syncthreads();  // (an earlier call's records have been read)
  if ((threadIdx.x & 63) == 0) {
    red[3 * w] = v;
    red[3 * w + 1] = (double)i;
    red[3 * w + 2] = s;
  }
  __syncthreads();
  v = red[0];
  i = (int)red[1];
  s = red[2];
#pragma unroll
  for (int k = 1; k < GR_WG / 64; ++k) {
    gr_take(v, i, red[3 * k], (int)red[3 * k + 1]);
    s += red[3 * k + 2];
  }
}

// the records of one launch reduced by one workgroup: thread t takes records t, t + 256, ... in order, then gr_reduce
__device__ __forceinline__ void gr_reduce_records(const double* __restrict__ rec, unsigned nwg, double& v, int& i, double& s,
                                                  double* red) {
  v = -1.0;
  i = INT_MAX;
  s = 0.0;
  for (unsigned r = threadIdx.x; r < nwg; r += GR_WG) {
    gr_take(v, i, rec[(size_t)r * GR_REC], (int)rec[(size_t)r * GR_REC + 2]);
    s += rec[(size_t)r * GR_REC + 1];
  }
  gr_reduce(v, i, s, red);
}

// Step j.  C [M][N] (row j written here, rows l < j read: the wave's reads are contiguous), d [N], part [2][nwg][GR_REC].
// Workgroup 0 also writes idx[j] and trace[j].  The pivot's column C[0..j-1][p] and its scaled row are staged in LDS once.
template <int DP>
__global__ __launch_bounds__(GR_WG) void k_greedy_step(int kernel, const double* __restrict__ X, int N, int D,
                                                        const double* __restrict__ raw_ls, const double* __restrict__ raw_os, int j,
                                                        double min_var, double* __restrict__ C, double* __restrict__ d,
                                                        double* __restrict__ part, unsigned nwg, int32_t* __restrict__ stop,
                                                        int32_t* __restrict__ idx, double* __restrict__ trace) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  double* xp = reinterpret_cast<double*>(smem_raw);  // [16] scaled pivot row
  double* ils = xp + 16;                             // [16] 1 / length-scale
  double* red = ils + 16;                            // [16] wave records of gr_reduce
  double* cp = xp + GR_HEAD;                         // [j]  pivot column
  const int tid = threadIdx.x;
  // An EARLIER launch stopped.  Workgroup 0 of this launch may write stop[0] = j below while the waves of other workgroups
  // are still loading the word, so a value of j is not acted on here: whoever reads it goes on and finds `stopping` from the
  // records, as every wave of the grid does.  What is left (-1, or l < j from a launch that has ended) cannot change during
  // this launch, so the waves of a workgroup agree and none leaves its siblings at a barrier.
  const int32_t st = stop[0];
  if (j > 0 && st >= 0 && st < j) return;
  if (tid < 16) ils[tid] = tid < D ? 1.0 / softplus_d(raw_ls[tid]) : 0.0;
  const double s2 = softplus_d(raw_os[0]);
  const Cov cov = make_cov(kernel, s2, cov_alpha(kernel, raw_os));
  double dp = s2, tr = (double)N * s2;
  int p = 0;
  if (j > 0) gr_reduce_records(part + (size_t)((j - 1) & 1) * nwg * GR_REC, nwg, dp, p, tr, red);
  const bool stopping = dp <= min_var;  // (no unpicked row left would give dp = -1: stops as well)
  if (blockIdx.x == 0 && tid == 0) {
    trace[j] = tr;
    if (stopping) stop[0] = j;
    else if (j == 0) stop[0] = -1;
    if (!stopping) idx[j] = p;
  }
  if (stopping) return;
  for (int l = tid; l < j; l += GR_WG) cp[l] = C[(size_t)l * N + p];
  if (tid < DP) xp[tid] = tid < D ? X[(size_t)p * D + tid] * ils[tid] : 0.0;
  __syncthreads();
  const size_t n = (size_t)blockIdx.x * GR_WG + tid;
  double v = -1.0, s = 0.0;
  int bi = INT_MAX;
  if (n < (size_t)N) {
    double d2 = 0.0;
#pragma unroll
    for (int q = 0; q < DP; ++q) {  // (dimensions past D hold zeros on both sides: they add exact zeros)
      const double t = xp[q] - (q < D ? X[n * D + q] * ils[q] : 0.0);
      d2 += t * t;
    }
    const double* cn = C + n;
    double acc = 0.0;
#pragma unroll 8
    for (int l = 0; l < j; ++l) acc += cn[(size_t)l * N] * cp[l];
    const double c = (cov_value(cov, d2) - acc) / sqrt(dp);
    C[(size_t)j * N + n] = c;
    const double dold = j == 0 ? s2 : d[n];
    const bool picked = dold < 0.0 || n == (size_t)p;
    const double dn = picked ? -1.0 : fmax(dold - c * c, 0.0);
    d[n] = dn;
    if (!picked) {
      v = dn;
      s = dn;
      bi = (int)n;
    }
  }
  gr_reduce(v, bi, s, red);
  if (tid == 0) {
    double* rec = part + ((size_t)(j & 1) * nwg + blockIdx.x) * GR_REC;
    rec[0] = v;
    rec[1] = s;
    rec[2] = (double)bi;
  }
}

// One workgroup: M_eff and, when no launch stopped, trace[M] from the last step's records; Z = X[idx]; the unused tails
// idx = -1, trace = NaN, Z = NaN.
__global__ __launch_bounds__(GR_WG) void k_greedy_fin(const double* __restrict__ X, int D, int M, const double* __restrict__ part,
                                                       unsigned nwg, const int32_t* __restrict__ stop, int32_t* __restrict__ idx,
                                                       double* __restrict__ Z, double* __restrict__ trace,
                                                       int32_t* __restrict__ count) {
  __shared__ double red[16];
  const int tid = threadIdx.x;
  int meff = stop[0];
  if (meff < 0) {
    double v, s;
    int i;
    gr_reduce_records(part + (size_t)((M - 1) & 1) * nwg * GR_REC, nwg, v, i, s, red);
    meff = M;
    if (tid == 0) trace[M] = s;
  }
  if (tid == 0) count[0] = meff;
  const double nan = __longlong_as_double(0x7ff8000000000000LL);
  for (int i = meff + tid; i < M; i += GR_WG) {
    idx[i] = -1;
    trace[i + 1] = nan;
  }
  for (int e = tid; e < M * D; e += GR_WG) {
    const int r = e / D;
    Z[e] = r < meff ? X[(size_t)idx[r] * D + (e - r * D)] : nan;
  }
}

// ---- host side ----------------------------------------------------------------------------------------------------
namespace {
struct GrPlan : Layout {
  unsigned nwg;
  size_t C, d, part, stop;  // C [M][N], d [N], part [2][nwg][GR_REC], the stop word (int32) in a section of its own
};
bool gr_plan(GrPlan& p, int N, int D, int M) {
  if (N < 1 || !inducing_limits(M, D) || M > N) return false;
  p.nwg = (unsigned)(((size_t)N + GR_WG - 1) / GR_WG);
  p.C = p.take((size_t)M * (size_t)N);
  p.d = p.take((size_t)N);
  p.part = p.take((size_t)2 * p.nwg * GR_REC);
  p.stop = p.take(64);
  return true;
}
}  // namespace

size_t greedy_inducing_workspace_bytes(int N, int D, int M) {
  GrPlan p;
  return gr_plan(p, N, D, M) ? p.bytes() : 0;
}

int launch_greedy_inducing(const double* X, int N, int D, const double* raw_ls, const double* raw_os, int kernel, int M,
                           double min_var, int32_t* idx, double* Z, double* trace, int32_t* count, void* workspace,
                           size_t workspace_bytes, hipStream_t st) {
  GrPlan p;
  if (!gr_plan(p, N, D, M)) return TGP_E_UNSUPPORTED;  // (tgp_greedy_inducing_f64 has named the limits)
  double* ws;
  if (int rc = open_workspace("tgp_greedy_inducing_f64", "tgp_greedy_inducing_workspace_bytes", workspace, workspace_bytes, p.total,
                              &ws))
    return rc;
  int32_t* stop = reinterpret_cast<int32_t*>(ws + p.stop);
  const dim3 grid(p.nwg), block(GR_WG);
  for (int j = 0; j < M; ++j) {
    const size_t lds = (size_t)(GR_HEAD + j) * sizeof(double);  // <= 33 144 bytes: under the default ceiling
    dispatch_dp(D, [&](auto dp) {
      hipLaunchKernelGGL(k_greedy_step<decltype(dp)::value>, grid, block, lds, st, kernel, X, N, D, raw_ls, raw_os, j, min_var,
                         ws + p.C, ws + p.d, ws + p.part, p.nwg, stop, idx, trace);
    });
    LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(k_greedy_fin, dim3(1), block, 0, st, X, D, M, ws + p.part, p.nwg, stop, idx, Z, trace, count);
  LAUNCH_CHECK();
  return 0;
}

}  // namespace tgp
