// tgp_softmax.hip -- the multi-class likelihood (likelihoods/MulticlassCategorical.py): softmax over C latent GPs, each pushed
// through its own flow G_c, integrated by Monte Carlo over all C latents of a row at once.
//   k_ell_softmax      f0 = mu + sqrt(max(v, 0)) eps, g = G_c(f0), ELL = scale/S sum_{n,s} (g[y_n] - logsumexp_c g) and its
//                      adjoints down to mu, v and every program's theta, one launch
//   k_mc_normals       the counter-based draws below written to an (S,C,N) buffer (what the counter mode uses, for tests)
//   k_predict_softmax  P[n][c] = 1/S sum_s softmax_c(g[s,.,n]) and log P[n][y_n]
// Layout: one data row per lane, 64 rows per workgroup; the waves of a workgroup take the samples s = wave, wave + nw, ...
// of those rows and loop over the C classes inside the lane (a sample needs all its classes in one place).  The flows run
// on the checkpoint sweeps of tgp_dev.hpp (flow_forward_ckpt / flow_backward_ckpt, extended kind set, one node in flight):
// the forward keeps every block's input in LDS, the softmax weights w = scale/S (1[c = y] - softmax_c) start the reverse
// sweeps, which add the shared-parameter partials into the wave's accumulator row in a fixed order.
// Reductions: mu_bar / v_bar over the waves of the workgroup in wave order; ELL and theta_bar by butterfly over the wave,
// the waves in order into the workgroup's partial, the partials in order by the LAST workgroup to take a ticket -- no float
// atomics, bit-reproducible for a given (N, C, S, programs).
//
// Counter-based standard normals (eps == NULL), one per (s, c, row), row = row0 + n -- the exact recipe, all in uint64:
//   x  = seed + 0x9E3779B97F4A7C15 * step                      (step = *step_dev as an unsigned 32-bit value, 0 if NULL)
//   x ^= (s << 56) ^ (c << 48) ^ (row & (2^48 - 1))            (s < 256, c < 32: an injective packing)
//   fin(z): z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9;  z = (z ^ z >> 27) * 0x94D049BB133111EB;  return z ^ z >> 31   (splitmix64)
//   h1 = fin(x),  h2 = fin(h1 + 0x9E3779B97F4A7C15)
//   u1 = ((h1 >> 11) + 1) * 2^-53   in (0, 1],    u2 = (h2 >> 11) * 2^-53   in [0, 1)
//   eps = sqrt(-2 log(u1)) * cos(6.283185307179586 * u2)       (the cosine branch of Box-Muller; the sine twin is not used)
// Nothing of size S x C x N exists in memory in this mode.
#include "tgp_dev.hpp"
#include "tgp_launch.hpp"

namespace tgp {

#define SMX_ROWS 64   // data rows per workgroup (one per lane)

__device__ __forceinline__ uint64_t smx_fin(uint64_t z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
// the recipe of the header comment
__device__ __forceinline__ double smx_normal(uint64_t seed, uint32_t step, int s, int c, int64_t row) {
  uint64_t x = seed + 0x9E3779B97F4A7C15ull * (uint64_t)step;
  x ^= ((uint64_t)(unsigned)s << 56) ^ ((uint64_t)(unsigned)c << 48) ^ ((uint64_t)row & 0xFFFFFFFFFFFFull);
  const uint64_t h1 = smx_fin(x), h2 = smx_fin(h1 + 0x9E3779B97F4A7C15ull);
  const double u1 = (double)((h1 >> 11) + 1) * 0x1.0p-53, u2 = (double)(h2 >> 11) * 0x1.0p-53;
  return sqrt(-2.0 * log(u1)) * cos(6.283185307179586 * u2);
}

// the program into LDS (the sweeps read their block descriptors from there), then the shared parameters (flow_params_lds, whose
// barrier also covers the program copy)
__device__ inline void smx_setup_lds(const FlowProg& fp, const double* __restrict__ theta, int32_t* prog, double* tp, double* tg) {
  for (int i = threadIdx.x; i < 4 * fp.nblk; i += blockDim.x) prog[i] = fp.blk[i];
  flow_params_lds<true>(theta, fp, tp, tg);
}

__device__ __forceinline__ FlowDev smx_flow(const SmxArgs& a, const int32_t* prog, const double* tp, const double* tg, int c) {
  const int b0 = a.blk_off[c];
  return FlowDev{prog + 4 * b0, a.blk_off[c + 1] - b0, tp, tg};
}

// LDS of k_ell_softmax in bytes: [program][tp, tg][nw accumulator rows][wave sums][g, eps, A, B: C x nt each][stack: nblk x nt]
static size_t smx_ell_lds(int nt, int C, int nblk, int P) {
  const size_t Pp = P > 0 ? P : 1, nw = nt / 64;
  return 16 * (size_t)(nblk > 0 ? nblk : 1) + ((2 + nw) * Pp + 8 + (size_t)(4 * C + (nblk > 0 ? nblk : 1)) * nt) * sizeof(double);
}

__global__ __launch_bounds__(256) void k_ell_softmax(SmxArgs a, FlowProg fp, const double* __restrict__ theta,
                                                      const double* __restrict__ Y, const double* __restrict__ mu,
                                                      const double* __restrict__ v, const double* __restrict__ eps,
                                                      double* __restrict__ out, double* __restrict__ mu_bar,
                                                      double* __restrict__ v_bar, double* __restrict__ theta_bar,
                                                      double* __restrict__ part, int32_t* __restrict__ ticket) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  const int tid = threadIdx.x, nt = blockDim.x, lane = tid & 63, wave = tid >> 6, nw = nt >> 6;
  const int N = a.N, C = a.C, S = a.S, P = a.P, Pp = P > 0 ? P : 1, nbk = fp.nblk > 0 ? fp.nblk : 1;
  const bool train = mu_bar != nullptr;
  int32_t* prog = reinterpret_cast<int32_t*>(smem_raw);
  double* tp = reinterpret_cast<double*>(smem_raw + 16 * (size_t)nbk);   // P
  double* tg = tp + Pp;                                                   // P
  double* accw = tg + Pp;                                                 // nw x P: per-wave parameter adjoints
  double* red = accw + (size_t)nw * Pp;                                   // 8: the waves' ELL sums
  double* gL = red + 8;                                                   // C x nt: g of the sample in hand
  double* eL = gL + (size_t)C * nt;                                       // C x nt: its eps
  double* aL = eL + (size_t)C * nt;                                       // C x nt: sum_s dELL/df0
  double* bL = aL + (size_t)C * nt;                                       // C x nt: sum_s dELL/df0 eps
  double* stack = bL + (size_t)C * nt;                                    // nblk x nt: block inputs
  __shared__ int s_last;
  smx_setup_lds(fp, theta, prog, tp, tg);
  for (int i = tid; i < nw * Pp; i += nt) accw[i] = 0.0;
  for (int c = 0; c < C; ++c) { aL[c * nt + tid] = 0.0; bL[c * nt + tid] = 0.0; }
  __syncthreads();
  const int n = blockIdx.x * SMX_ROWS + lane;
  const bool valid = n < N;
  const int nc = valid ? n : N - 1;
  const int y = (int)Y[nc];
  const uint32_t step = a.step_dev ? (uint32_t)a.step_dev[0] : 0u;
  const double wsc = a.scale / (double)S;
  double* aw = accw + (size_t)wave * Pp;
  double ell = 0.0;
  for (int s = wave; s < S; s += nw) {
    // ---- forward: every class of this sample
    double gmax = -INFINITY;
    for (int c = 0; c < C; ++c) {
      const double e = eps ? eps[((size_t)s * C + c) * N + nc] : smx_normal(a.seed, step, s, c, a.row0 + nc);
      double f[1] = {mu[(size_t)c * N + nc] + sqrt(fmax(v[(size_t)c * N + nc], 0.0)) * e};
      const FlowDev F = smx_flow(a, prog, tp, tg, c);
      flow_forward_ckpt<1, true>(F, f, nullptr, stack + (size_t)a.blk_off[c] * nt + tid, nt);
      gL[c * nt + tid] = f[0];
      eL[c * nt + tid] = e;
      gmax = fmax(gmax, f[0]);
    }
    double se = 0.0, gy = 0.0;
    for (int c = 0; c < C; ++c) {
      const double g = gL[c * nt + tid];
      se += exp(g - gmax);
      if (c == y) gy = g;
    }
    const double lse = gmax + log(se);
    if (valid) ell += gy - lse;
    if (!train) continue;
    // ---- reverse: w = scale/S (1[c = y] - softmax_c) down every class's flow
    for (int c = 0; c < C; ++c) {
      const double p = exp(gL[c * nt + tid] - lse);
      double cc[1] = {valid ? wsc * ((c == y ? 1.0 : 0.0) - p) : 0.0};
      const FlowDev F = smx_flow(a, prog, tp, tg, c);
      flow_backward_ckpt<1, true>(F, cc, nullptr, stack + (size_t)a.blk_off[c] * nt + tid, nt, aw, lane, nullptr, 0);
      aL[c * nt + tid] += cc[0];
      bL[c * nt + tid] += cc[0] * eL[c * nt + tid];
    }
  }
  // ---- workgroup: rows' adjoints over the waves in order, then the partial {ELL, theta_bar}
  ell = wave_sum(ell);
  if (lane == 0) red[wave] = ell;
  __syncthreads();
  if (train) {
    for (int i = tid; i < C * SMX_ROWS; i += nt) {
      const int c = i >> 6, l = i & 63, r = blockIdx.x * SMX_ROWS + l;
      if (r >= N) continue;
      double A = aL[c * nt + l], B = bL[c * nt + l];
      for (int w = 1; w < nw; ++w) { A += aL[c * nt + 64 * w + l]; B += bL[c * nt + 64 * w + l]; }
      const double vv = v[(size_t)c * N + r];
      mu_bar[(size_t)c * N + r] = A;
      v_bar[(size_t)c * N + r] = vv > 0.0 ? B / (2.0 * sqrt(vv)) : 0.0;
    }
  }
  const int len = 1 + P;
  double* pb = part + (size_t)blockIdx.x * len;
  if (tid == 0) {
    double sacc = red[0];
    for (int w = 1; w < nw; ++w) sacc += red[w];
    st_agent(pb, wsc * sacc);
  }
  for (int j = tid; j < P; j += nt) {
    double sacc = accw[j];
    for (int w = 1; w < nw; ++w) sacc += accw[(size_t)w * Pp + j];
    st_agent(pb + 1 + j, sacc);
  }
  // ---- the last workgroup to arrive adds the partials in a fixed order
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");   // every wave's partial stores have landed
  if (tid == 0) {
    const int tk = __hip_atomic_fetch_add(ticket, 1, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
    s_last = tk == (int)gridDim.x - 1;
  }
  __syncthreads();
  if (!s_last) return;
  const int nb = (int)gridDim.x;
  for (int j = tid; j < len; j += nt) {
    if (j > 0 && !train) break;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
    int b = 0;
    for (; b + 3 < nb; b += 4) {
      const double t0 = ld_agent(part + (size_t)b * len + j), t1 = ld_agent(part + (size_t)(b + 1) * len + j);
      const double t2 = ld_agent(part + (size_t)(b + 2) * len + j), t3 = ld_agent(part + (size_t)(b + 3) * len + j);
      s0 += t0; s1 += t1; s2 += t2; s3 += t3;
    }
    for (; b < nb; ++b) s0 += ld_agent(part + (size_t)b * len + j);
    const double sacc = (s0 + s1) + (s2 + s3);
    if (j == 0) out[0] = sacc;
    else theta_bar[j - 1] = sacc;
  }
  if (tid == 0) __hip_atomic_store(ticket, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(256) void k_mc_normals(SmxArgs a, double* __restrict__ eps) {
  const size_t total = (size_t)a.S * a.C * a.N, i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int n = (int)(i % (size_t)a.N), c = (int)((i / (size_t)a.N) % (size_t)a.C), s = (int)(i / ((size_t)a.N * a.C));
  const uint32_t step = a.step_dev ? (uint32_t)a.step_dev[0] : 0u;
  eps[i] = smx_normal(a.seed, step, s, c, a.row0 + n);
}

// one row per lane, every sample in turn; LDS: [program][tp, tg][g, P: C x 64 each]
__global__ __launch_bounds__(SMX_ROWS) void k_predict_softmax(SmxArgs a, FlowProg fp, const double* __restrict__ theta,
                                                               const double* __restrict__ mu, const double* __restrict__ v,
                                                               const double* __restrict__ eps, const double* __restrict__ Y,
                                                               double* __restrict__ Pout, double* __restrict__ logp) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  const int tid = threadIdx.x, nt = SMX_ROWS, N = a.N, C = a.C, S = a.S, Pp = a.P > 0 ? a.P : 1, nbk = fp.nblk > 0 ? fp.nblk : 1;
  int32_t* prog = reinterpret_cast<int32_t*>(smem_raw);
  double* tp = reinterpret_cast<double*>(smem_raw + 16 * (size_t)nbk);
  double* tg = tp + Pp;
  double* gL = tg + Pp;
  double* pL = gL + (size_t)C * nt;
  smx_setup_lds(fp, theta, prog, tp, tg);
  const int n = blockIdx.x * SMX_ROWS + tid;
  if (n >= N) return;
  const uint32_t step = a.step_dev ? (uint32_t)a.step_dev[0] : 0u;
  for (int c = 0; c < C; ++c) pL[c * nt + tid] = 0.0;
  for (int s = 0; s < S; ++s) {
    double gmax = -INFINITY;
    for (int c = 0; c < C; ++c) {
      const double e = eps ? eps[((size_t)s * C + c) * N + n] : smx_normal(a.seed, step, s, c, a.row0 + n);
      double f[1] = {mu[(size_t)c * N + n] + sqrt(fmax(v[(size_t)c * N + n], 0.0)) * e}, der[1];
      const double* const rp[1] = {nullptr};
      const FlowDev F = smx_flow(a, prog, tp, tg, c);
      flow_forward_n<1, false, true>(F, f, rp, der);
      gL[c * nt + tid] = f[0];
      gmax = fmax(gmax, f[0]);
    }
    double se = 0.0;
    for (int c = 0; c < C; ++c) se += exp(gL[c * nt + tid] - gmax);
    const double lse = gmax + log(se);
    for (int c = 0; c < C; ++c) pL[c * nt + tid] += exp(gL[c * nt + tid] - lse);
  }
  const double is = 1.0 / (double)S;
  const int y = Y ? (int)Y[n] : -1;
  for (int c = 0; c < C; ++c) {
    const double p = pL[c * nt + tid] * is;
    Pout[(size_t)n * C + c] = p;
    if (logp && c == y) logp[n] = log(p);
  }
}

// ---------------------------------------------------------------------------------------------------
// host launchers
// ---------------------------------------------------------------------------------------------------
size_t softmax_workspace_doubles(int N, int P) { return (size_t)((N + SMX_ROWS - 1) / SMX_ROWS) * (size_t)(1 + P) + 2; }

int launch_ell_softmax(const SmxArgs& a, const FlowProg& fp, const double* theta, const double* Y, const double* mu, const double* v,
                       const double* eps, double* out, double* mu_bar, double* v_bar, double* theta_bar, double* ws,
                       hipStream_t st) {
  // as many waves (sample groups) per workgroup as a CU's LDS holds for this C and these programs, no more than there are samples
  int nt = 256;
  while (nt > 64 && (nt / 64 > a.S || smx_ell_lds(nt, a.C, fp.nblk, a.P) > 64 * 1024)) nt >>= 1;
  const size_t lds = smx_ell_lds(nt, a.C, fp.nblk, a.P);
  static size_t cur = 48 * 1024;
  if (int rc = ensure_lds(reinterpret_cast<const void*>(k_ell_softmax), lds, &cur)) return rc;
  const int nb = (a.N + SMX_ROWS - 1) / SMX_ROWS;
  int32_t* ticket = reinterpret_cast<int32_t*>(ws + (size_t)nb * (1 + a.P));
  hipError_t e = hipMemsetAsync(ticket, 0, sizeof(int32_t), st);   // a call cannot count on what an earlier one left here
  if (e != hipSuccess) return set_error(e, __FILE__, __LINE__);
  hipLaunchKernelGGL(k_ell_softmax, dim3(nb), dim3(nt), lds, st, a, fp, theta, Y, mu, v, eps, out, mu_bar, v_bar, theta_bar, ws,
                     ticket);
  LAUNCH_CHECK();
  return 0;
}

int launch_mc_normals(const SmxArgs& a, double* eps, hipStream_t st) {
  const size_t total = (size_t)a.S * a.C * a.N;
  hipLaunchKernelGGL(k_mc_normals, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, a, eps);
  LAUNCH_CHECK();
  return 0;
}

int launch_predict_softmax(const SmxArgs& a, const FlowProg& fp, const double* theta, const double* mu, const double* v,
                           const double* eps, const double* Y, double* P, double* logp, hipStream_t st) {
  const size_t lds = 16 * (size_t)(fp.nblk > 0 ? fp.nblk : 1) +
                     (2 * (size_t)(a.P > 0 ? a.P : 1) + 2 * (size_t)a.C * SMX_ROWS) * sizeof(double);
  static size_t cur = 48 * 1024;
  if (int rc = ensure_lds(reinterpret_cast<const void*>(k_predict_softmax), lds, &cur)) return rc;
  hipLaunchKernelGGL(k_predict_softmax, dim3((a.N + SMX_ROWS - 1) / SMX_ROWS), dim3(SMX_ROWS), lds, st, a, fp, theta, mu, v, eps, Y,
                     P, logp);
  LAUNCH_CHECK();
  return 0;
}

}  // namespace tgp
