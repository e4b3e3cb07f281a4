// tgp_warp.hip -- the warped-GP likelihood (likelihoods/WarpedGaussianLinearMean.py): the flow T is applied to the TARGETS.
//   k_ell_warp      t = T(y), the Gaussian closed form at t, sum log T'(y) and the adjoints of both down to theta, one launch
//   k_flow_inverse  x = T^-1(t), block by block from the last: closed forms, else a bracketed Newton iteration
//   k_predict_warp  Gauss-Hermite moments of T^-1(f), f ~ N(mu, v + noise), and the exact warped predictive log density
// The blocks are evaluated one element at a time with the library's exp / log / sinh / cosh / tanh (this is N rows x B blocks,
// no quadrature loop and no MFMA: launch- and latency-bound), with the reference's quirks the interpreter of
// tgp_dev.hpp keeps: asinh(x) = log(x + sqrt(x^2 + 1)), softplus with threshold 20, float32 pi in the Gaussian constant.
// Shared with the other kernels through tgp_dev.hpp: the per-kind tables (parameters per block, which one is softplus'ed) and
// the staging of the shared parameters into LDS (flow_params_lds); warp_block is this file's own, for its second derivative.
#include "tgp_dev.hpp"
#include "tgp_launch.hpp"

namespace tgp {

// one data row per lane.  64-lane workgroups up to this many rows (Power: 8 611 rows = 135 workgroups on 256 CUs instead of
// 34), 256-lane workgroups above (fewer partials for the last workgroup to add up)
#define WARP_SMALL_MAXN 16384
static int warp_threads(int N) { return N <= WARP_SMALL_MAXN ? 64 : 256; }
static int warp_blocks(int N) { const int t = warp_threads(N); return (N + t - 1) / t; }
// partial p of workgroup b: part[b * (3 + P) + p], p = {ell, d/d eta, logdet, theta...}; then the ticket word
size_t warp_workspace_doubles(int N, int P) {
  const size_t nb64 = (size_t)((N < WARP_SMALL_MAXN ? N : WARP_SMALL_MAXN) + 63) / 64, nb256 = (size_t)(N + 255) / 256;
  return (nb64 > nb256 ? nb64 : nb256) * (size_t)(3 + P) + 2;
}

// One block at x: value g, derivative g1 = dg/dx and (D2) g2 = d2g/dx2.  pa, pb: the two parameters of an AFFINE / SAL block
// (shared or this row's, already transformed); tp: the block's shared parameters in LDS (the other kinds).
struct WVal { double g, g1, g2; };
template <bool D2>
__device__ inline WVal warp_block(int kind, int K, int flags, const double* tp, double pa, double pb, double x) {
  const bool addf = flags & TGP_FLAG_ADD_F0;
  WVal r{0.0, 0.0, 0.0};
  if (kind == TGP_FLOW_AFFINE) {
    r.g = pa * x + pb;
    r.g1 = pa;
    return r;   // (the interpreter has no ADD_F0 for this kind either)
  }
  if (kind == TGP_FLOW_SAL) {
    const double s2 = x * x + 1.0, s = sqrt(s2), u = log(x + s), tau = pb * u - pa, sh = sinh(tau), ch = cosh(tau);
    r.g = sh;
    r.g1 = pb * ch / s;
    if (D2) r.g2 = pb * pb * sh / s2 - pb * ch * x / (s2 * s);
  } else if (kind == TGP_FLOW_STEPTANH) {
    for (int k = 0; k < K; ++k) {
      const double a = tp[4 * k], B = tp[4 * k + 1], c = tp[4 * k + 2], D = tp[4 * k + 3];
      const double th = tanh((x - c) / D), se = 1.0 - th * th;
      r.g += a + B * th;
      r.g1 += B * se / D;
      if (D2) r.g2 += -2.0 * B * th * se / (D * D);
    }
  } else if (kind == TGP_FLOW_ARCSINH) {
    const double a = tp[0], b = tp[1], c = tp[2], d = tp[3];
    const double z = (x - c) / d, s2 = z * z + 1.0, s = sqrt(s2);
    r.g = a + b * log(z + s);
    r.g1 = b / (d * s);
    if (D2) r.g2 = -b * z / (d * d * s2 * s);
  } else if (kind == TGP_FLOW_BOXCOX) {
    double lam = tp[0];
    if (lam == 0.0) lam = 1e-11;
    const double ax = fabs(x), p = exp(lam * log(ax));
    r.g = (copysign(p, x) - 1.0) / lam;
    r.g1 = p / ax;
    if (D2) r.g2 = (lam - 1.0) * p / (ax * x);
  } else if (kind == TGP_FLOW_INV_BOXCOX) {
    double lam = tp[0];
    if (lam == 0.0) lam = 1e-11;
    const double w = lam * x + 1.0, aw = fabs(w), q = exp(log(aw) / lam);
    r.g = copysign(q, w);
    r.g1 = q / aw;
    if (D2) r.g2 = (1.0 - lam) * q / (aw * w);
  } else if (kind == TGP_FLOW_SINH) {
    const double a = tp[0], b = tp[1], c = tp[2], d = tp[3];
    const double z = (x - c) / d, sh = sinh(z);
    r.g = a + b * sh;
    r.g1 = b * cosh(z) / d;
    if (D2) r.g2 = b * sh / (d * d);
  } else {  // TUKEY (the host refuses NORMCDF, EXP and SOFTPLUS as warps: they do not map onto the real line)
    double gam = tp[0];
    if (gam == 0.0) gam = 1e-11;
    const double h = tp[1], em = expm1(gam * x), eg = em + 1.0, u = em / gam, E = exp(0.5 * h * x * x);
    r.g = u * E;
    r.g1 = E * (eg + h * x * u);
    if (D2) r.g2 = h * x * r.g1 + E * (gam * eg + h * u + h * x * eg);
    return r;   // (no ADD_F0 for this kind: the API refuses it)
  }
  if (addf) { r.g += x; r.g1 += 1.0; }
  return r;
}

// a block with SHARED parameters: q = the block's parameters in LDS; only AFFINE / SAL take the two scalars (a one-parameter
// block at the end of theta must not read past its own entry)
template <bool D2>
__device__ __forceinline__ WVal warp_block_shared(int kind, int K, int flags, const double* q, double x) {
  const bool two = kind <= TGP_FLOW_SAL;
  return warp_block<D2>(kind, K, flags, q, two ? q[0] : 0.0, two ? q[1] : 0.0, x);
}

// ---------------------------------------------------------------------------------------------------
// k_ell_warp
//   ELL_w = c sum_n [-1/2 log 2pi - 1/2 eta - 1/2 e^-eta ((t_n - mu_n)^2 + v_n)] + c sum_n log T'(y_n),  t = T(y), c = scale
//   forward sweep keeps the block inputs x_{k-1} in LDS; reverse sweep with two adjoints per row, gb for the value (starts at
//   dELL/dt_n = -c e^-eta (t_n - mu_n)) and the constant c for the log-derivative sum:
//     theta_k += gb dg_k/dtheta + c dlog g_k'/dtheta      gb <- gb g_k' + c g_k''/g_k'
//   Shared-parameter sums: butterfly over the wave, lane 0 adds into the wave's LDS accumulator (one writer per address),
//   the waves in order into the workgroup's partial, the partials in order by the LAST workgroup to take a ticket: no float
//   atomics, bit-reproducible for a given N (the launch shape depends on N only).
// ---------------------------------------------------------------------------------------------------
// adjoint of parameter j of a block: wave sum of the rows' contributions into aw[j] (d(tp)/d(raw) applied)
__device__ __forceinline__ void warp_acc(double* aw, const double* tg, int j, double contrib, int lane) {
  const double s = wave_sum(contrib);
  if (lane == 0) aw[j] += s * tg[j];
}

__global__ __launch_bounds__(256) void k_ell_warp(tgp_model md, FlowProg fp, int mode, const double* __restrict__ Y,
                                                   const double* __restrict__ mu, const double* __restrict__ v,
                                                   double* __restrict__ out, double* __restrict__ g_mu,
                                                   double* __restrict__ g_v, double* __restrict__ g_theta,
                                                   double* __restrict__ t_out, double* __restrict__ part,
                                                   int32_t* __restrict__ ticket) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  double* sm = reinterpret_cast<double*>(smem_raw);
  const int tid = threadIdx.x, nt = blockDim.x, lane = tid & 63, wave = tid >> 6, nw = nt >> 6, P = md.P;
  const int Pp = P > 0 ? P : 1;
  double* tp = sm;                              // P
  double* tg = tp + Pp;                         // P
  double* accw = tg + Pp;                       // nw x P: per-wave parameter adjoints
  double* red = accw + (size_t)nw * Pp;         // 3 x 4 wave sums, then 8 x 32 words of the final reduction
  double* stack = red + 12 + 8 * 33;            // nblk x nt: block inputs
  __shared__ int s_last;
  flow_params_lds<true>(md.theta, fp, tp, tg);
  const int n = blockIdx.x * nt + tid;
  const bool valid = n < md.N;
  const int nc = valid ? n : md.N - 1;
  // ---- forward
  double x = Y[nc], ld = 0.0;
  if (mode == TGP_WARP_TARGETS) {
    for (int b = 0; b < fp.nblk; ++b) {
      const int kind = fp.blk[4 * b], K = fp.blk[4 * b + 1], poff = fp.blk[4 * b + 2], flags = fp.blk[4 * b + 3];
      x = warp_block_shared<false>(kind, K, flags, tp + poff, x).g;
    }
    if (valid) t_out[n] = x;
    if (blockIdx.x == 0 && tid == 0) *ticket = 0;   // the post-pass of this step counts its workgroups from 0
    return;
  }
  for (int i = tid; i < nw * Pp; i += nt) accw[i] = 0.0;
  for (int b = 0; b < fp.nblk; ++b) {
    const int kind = fp.blk[4 * b], K = fp.blk[4 * b + 1], poff = fp.blk[4 * b + 2], flags = fp.blk[4 * b + 3];
    stack[(size_t)b * nt + tid] = x;
    const WVal r = warp_block_shared<false>(kind, K, flags, tp + poff, x);
    x = r.g;
    ld += log(r.g1);
  }
  __syncthreads();   // accw zeroed
  const double c = md.scale, eta = md.log_var_noise[0], einv = exp(-eta);
  const double res = x - mu[nc], vn = v[nc];
  double e = 0.0, et = 0.0;
  if (valid) {
    e = -0.5 * TGP_LOG_2PI_REF - 0.5 * eta - 0.5 * einv * (res * res + vn);
    et = -0.5 + 0.5 * einv * (res * res + vn);
    if (t_out) t_out[n] = x;
    if (g_mu) g_mu[n] = c * einv * res;
    if (g_v) g_v[n] = -0.5 * c * einv;
  } else {
    ld = 0.0;
  }
  // ---- reverse
  double gb = valid ? -c * einv * res : 0.0;
  const double cw = valid ? c : 0.0;
  double* aw = accw + (size_t)wave * Pp;
  for (int b = fp.nblk - 1; b >= 0; --b) {
    const int kind = fp.blk[4 * b], K = fp.blk[4 * b + 1], poff = fp.blk[4 * b + 2], flags = fp.blk[4 * b + 3];
    const double xi = stack[(size_t)b * nt + tid];
    const double* q = tp + poff;
    double* a_ = aw + poff;
    const double* tg_ = tg + poff;
    const WVal r = warp_block_shared<true>(kind, K, flags, q, xi);
    const double ig = 1.0 / r.g1, cg = cw * ig;   // c / g': weight of d(g')/d(theta)
    if (kind == TGP_FLOW_AFFINE) {
      warp_acc(a_, tg_, 0, gb * xi + cg, lane);
      warp_acc(a_, tg_, 1, gb, lane);
    } else if (kind == TGP_FLOW_SAL) {
      const double s = sqrt(xi * xi + 1.0), u = log(xi + s), tau = q[1] * u - q[0], sh = sinh(tau), ch = cosh(tau);
      warp_acc(a_, tg_, 0, gb * (-ch) + cg * (-q[1] * sh / s), lane);
      warp_acc(a_, tg_, 1, gb * (u * ch) + cg * (ch / s + q[1] * u * sh / s), lane);
    } else if (kind == TGP_FLOW_STEPTANH) {
      for (int k = 0; k < K; ++k) {
        const double B = q[4 * k + 1], cc = q[4 * k + 2], D = q[4 * k + 3];
        const double z = (xi - cc) / D, th = tanh(z), se = 1.0 - th * th, iD = 1.0 / D;
        warp_acc(a_, tg_, 4 * k, gb, lane);
        warp_acc(a_, tg_, 4 * k + 1, gb * th + cg * (se * iD), lane);
        warp_acc(a_, tg_, 4 * k + 2, gb * (-B * se * iD) + cg * (2.0 * B * th * se * iD * iD), lane);
        warp_acc(a_, tg_, 4 * k + 3, gb * (-B * se * z * iD) + cg * (B * se * iD * iD * (2.0 * th * z - 1.0)), lane);
      }
    } else if (kind == TGP_FLOW_ARCSINH) {
      const double bb = q[1], cc = q[2], d = q[3];
      const double z = (xi - cc) / d, s2 = z * z + 1.0, s = sqrt(s2), as = log(z + s);
      warp_acc(a_, tg_, 0, gb, lane);
      warp_acc(a_, tg_, 1, gb * as + cg / (d * s), lane);
      warp_acc(a_, tg_, 2, gb * (-bb / (d * s)) + cg * (bb * z / (d * d * s2 * s)), lane);
      warp_acc(a_, tg_, 3, gb * (-bb * z / (d * s)) + cg * (-bb / (d * d * s2 * s)), lane);
    } else if (kind == TGP_FLOW_BOXCOX) {
      double lam = q[0];
      if (lam == 0.0) lam = 1e-11;
      const double ax = fabs(xi), lx = log(ax), p = exp(lam * lx), sp = copysign(p, xi);
      warp_acc(a_, tg_, 0, gb * (sp * lx / lam - (sp - 1.0) / (lam * lam)) + cg * (p / ax * lx), lane);
    } else if (kind == TGP_FLOW_INV_BOXCOX) {
      double lam = q[0];
      if (lam == 0.0) lam = 1e-11;
      const double w = lam * xi + 1.0, aw_ = fabs(w), lw = log(aw_), qq = exp(lw / lam), sq = copysign(qq, w);
      const double dl = xi / (lam * w) - lw / (lam * lam);
      warp_acc(a_, tg_, 0, gb * (sq * dl) + cg * (qq / aw_ * (dl - xi / w)), lane);
    } else if (kind == TGP_FLOW_SINH) {
      // g = a + b sinh z, g' = (b/d) cosh z, z = (x - c)/d
      const double bb = q[1], cc = q[2], d = q[3], id = 1.0 / d;
      const double z = (xi - cc) * id, sh = sinh(z), ch = cosh(z);
      warp_acc(a_, tg_, 0, gb, lane);
      warp_acc(a_, tg_, 1, gb * sh + cg * (ch * id), lane);
      warp_acc(a_, tg_, 2, gb * (-bb * ch * id) + cg * (-bb * sh * id * id), lane);
      warp_acc(a_, tg_, 3, gb * (-bb * ch * z * id) + cg * (-bb * id * id * (ch + z * sh)), lane);
    } else {  // TUKEY: u_gam = du/dgam = (x e^{gam x} - u)/gam
      double gam = q[0];
      if (gam == 0.0) gam = 1e-11;
      const double h = q[1], em = expm1(gam * xi), eg = em + 1.0, u = em / gam, E = exp(0.5 * h * xi * xi);
      const double ug = (xi * eg - u) / gam, hx2 = 0.5 * xi * xi;
      warp_acc(a_, tg_, 0, gb * (E * ug) + cg * (E * (xi * eg + h * xi * ug)), lane);
      warp_acc(a_, tg_, 1, gb * (r.g * hx2) + cg * (hx2 * r.g1 + E * xi * u), lane);
    }
    gb = gb * r.g1 + cw * r.g2 * ig;
  }
  // ---- workgroup partial
  e = wave_sum(e); et = wave_sum(et); ld = wave_sum(ld);
  if (lane == 0) { red[wave] = e; red[4 + wave] = et; red[8 + wave] = ld; }
  __syncthreads();
  const int len = 3 + P;
  double* pb = part + (size_t)blockIdx.x * len;
  if (tid < 3) {
    double s = red[4 * tid];
    for (int w = 1; w < nw; ++w) s += red[4 * tid + w];
    st_agent(pb + tid, c * s);
  }
  for (int j = tid; j < P; j += nt) {
    double s = accw[j];
    for (int w = 1; w < nw; ++w) s += accw[(size_t)w * Pp + j];
    st_agent(pb + 3 + j, s);
  }
  // ---- the last workgroup to arrive adds the partials in a fixed order
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");   // every wave's partial stores have landed
  if (tid == 0) {
    const int tk = __hip_atomic_fetch_add(ticket, 1, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
    s_last = tk == (int)gridDim.x - 1;
  }
  __syncthreads();
  if (!s_last) return;
  double* fin = red + 12;                       // [8][33]
  const int cidx = tid & 31, grp = tid >> 5, ng = nt >> 5, nb = (int)gridDim.x;
  for (int j0 = 0; j0 < len; j0 += 32) {
    const int j = j0 + cidx;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
    if (j < len) {
      int b = grp;
      for (; b + 3 * ng < nb; b += 4 * ng) {
        const double t0 = ld_agent(part + (size_t)b * len + j), t1 = ld_agent(part + (size_t)(b + ng) * len + j);
        const double t2 = ld_agent(part + (size_t)(b + 2 * ng) * len + j), t3 = ld_agent(part + (size_t)(b + 3 * ng) * len + j);
        s0 += t0; s1 += t1; s2 += t2; s3 += t3;
      }
      for (; b < nb; b += ng) s0 += ld_agent(part + (size_t)b * len + j);
    }
    __syncthreads();
    fin[grp * 33 + cidx] = (s0 + s1) + (s2 + s3);
    __syncthreads();
    if (grp == 0 && j < len) {
      double s = fin[cidx];
      for (int g = 1; g < ng; ++g) s += fin[g * 33 + cidx];
      if (mode == TGP_WARP_FULL) {
        // out[0] = ELL_w needs the sums 0 and 2 (both in the first column chunk): through two words of `red`, free by now
        if (j == 0) red[0] = s;
        if (j == 1) out[1] = s;
        if (j == 2) { out[2] = s; red[1] = s; }
      } else {
        if (j == 2) { red[1] = s; }
      }
      if (j >= 3 && g_theta) g_theta[j - 3] = s;
    }
    __syncthreads();
    if (j0 == 0 && tid == 0) {
      const double ldt = red[1];
      if (mode == TGP_WARP_FULL) out[0] = red[0] + ldt;
      else { out[0] += ldt; out[1] += ldt; }    // the step's {ELBO, ELL} gain the log-Jacobian term
    }
  }
  if (tid == 0) __hip_atomic_store(ticket, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---------------------------------------------------------------------------------------------------
// inverse of one block at target t
// ---------------------------------------------------------------------------------------------------
#define WARP_INV_MAXIT 128
// Bracketed Newton on g(x) = t, g strictly increasing.  Start at x = t; grow a bracket from it by doubling steps (first step
// max(1, |x|)); Newton steps with g', bisection whenever a step leaves the open bracket or g' is not positive and finite;
// stop when g(x) == t or a step is <= 4 ulp-ish (2^-50 max(1, |x|)).  *fail is set when either phase runs out of evaluations.
__device__ inline double warp_newton(int kind, int K, int flags, const double* tp, double pa, double pb, double t, bool* fail) {
  double x = t;
  WVal r = warp_block<false>(kind, K, flags, tp, pa, pb, x);
  if (r.g == t) return x;
  double lo, hi, step = fmax(1.0, fabs(x));
  bool ok = false;
  if (r.g < t) {
    lo = x; hi = x + step;
    for (int it = 0; it < WARP_INV_MAXIT; ++it) {
      if (warp_block<false>(kind, K, flags, tp, pa, pb, hi).g >= t) { ok = true; break; }
      lo = hi; step *= 2.0; hi = lo + step;
    }
  } else {
    hi = x; lo = x - step;
    for (int it = 0; it < WARP_INV_MAXIT; ++it) {
      if (warp_block<false>(kind, K, flags, tp, pa, pb, lo).g <= t) { ok = true; break; }
      hi = lo; step *= 2.0; lo = hi - step;
    }
  }
  if (!ok) { *fail = true; return x; }
  // TUKEY grows like e^{h x^2/2}: from a start far above the root a Newton step is only ~1/(h x) long and the bracket never
  // cuts it short.  For that kind a step that would not at least halve the one before it gives way to a bisection (the rule of
  // Numerical Recipes' rtsafe), with twice the evaluations; the other kinds iterate exactly as before.
  const bool guard = kind == TGP_FLOW_TUKEY;
  const int maxit = guard ? 2 * WARP_INV_MAXIT : WARP_INV_MAXIT;
  double dxprev = hi - lo;
  for (int it = 0; it < maxit; ++it) {
    const double fx = r.g - t;
    if (fx == 0.0) return x;
    if (fx < 0.0) lo = x; else hi = x;
    double xn = x - fx / r.g1;
    if (!(xn > lo && xn < hi) || (guard && fabs(2.0 * fx) > fabs(dxprev * r.g1))) xn = 0.5 * (lo + hi);
    const double dx = fabs(xn - x);
    dxprev = dx;
    x = xn;
    if (dx <= 8.8817841970012523e-16 * fmax(1.0, fabs(x))) return x;
    r = warp_block<false>(kind, K, flags, tp, pa, pb, x);
  }
  *fail = true;
  return x;
}

// x = T^-1(t) for one element; rp = this row's per-row parameters (raw) or nullptr
__device__ inline double warp_inverse(const FlowProg& fp, const double* tp, const double* __restrict__ rp, double t, bool* fail) {
  double x = t;
  for (int b = fp.nblk - 1; b >= 0; --b) {
    const int kind = fp.blk[4 * b], K = fp.blk[4 * b + 1], poff = fp.blk[4 * b + 2], flags = fp.blk[4 * b + 3];
    const bool addf = (flags & TGP_FLAG_ADD_F0) && kind != TGP_FLOW_AFFINE;
    double pa = 0.0, pb = 0.0;
    if (flags & TGP_FLAG_PER_ROW) {   // AFFINE / SAL only (make_prog)
      pa = rp[poff]; pb = rp[poff + 1];
      if (flags & TGP_FLAG_RESTRICT) { if (kind == TGP_FLOW_AFFINE) pa = softplus_d(pa); else pb = softplus_d(pb); }
    } else if (kind <= TGP_FLOW_SAL) {
      pa = tp[poff]; pb = tp[poff + 1];
    }
    const double* q = tp + poff;
    if (addf || kind == TGP_FLOW_STEPTANH || kind == TGP_FLOW_TUKEY) {
      x = warp_newton(kind, K, flags, q, pa, pb, x, fail);
    } else if (kind == TGP_FLOW_AFFINE) {
      x = (x - pb) / pa;
    } else if (kind == TGP_FLOW_SAL) {
      x = sinh((log(x + sqrt(x * x + 1.0)) + pa) / pb);
    } else if (kind == TGP_FLOW_ARCSINH) {
      x = q[2] + q[3] * sinh((x - q[0]) / q[1]);
    } else if (kind == TGP_FLOW_SINH) {
      x = q[2] + q[3] * asinh((x - q[0]) / q[1]);
    } else if (kind == TGP_FLOW_BOXCOX) {      // the INV_BOXCOX block of the same lam
      x = warp_block<false>(TGP_FLOW_INV_BOXCOX, 0, 0, q, 0.0, 0.0, x).g;
    } else {
      x = warp_block<false>(TGP_FLOW_BOXCOX, 0, 0, q, 0.0, 0.0, x).g;
    }
  }
  return x;
}

__global__ __launch_bounds__(256) void k_flow_inverse(tgp_model md, FlowProg fp, const double* __restrict__ t, size_t total, int N,
                                                       const double* __restrict__ rowp, double* __restrict__ xo,
                                                       int32_t* __restrict__ status) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  double* tp = reinterpret_cast<double*>(smem_raw);
  double* tg = tp + (md.P > 0 ? md.P : 1);
  flow_params_lds<true>(md.theta, fp, tp, tg);
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  bool fail = false;
  const double* rp = rowp ? rowp + (i % (size_t)N) * md.RP : nullptr;
  xo[i] = warp_inverse(fp, tp, rp, t[i], &fail);
  if (fail && status) atomicAdd(status, 1);
}

// ---------------------------------------------------------------------------------------------------
// prediction: WarpedGaussianLinearMean.marginal_moments (:93-148) and the exact warped predictive log density
// ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_predict_warp(tgp_model md, FlowProg fp, const double* __restrict__ mu,
                                                       const double* __restrict__ v, const double* __restrict__ Y, double Y_std,
                                                       double* __restrict__ m1o, double* __restrict__ m2o,
                                                       double* __restrict__ logp) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  double* tp = reinterpret_cast<double*>(smem_raw);
  double* tg = tp + (md.P > 0 ? md.P : 1);
  flow_params_lds<true>(md.theta, fp, tp, tg);
  const int n = blockIdx.x * 256 + threadIdx.x;
  if (n >= md.N) return;
  const double var = v[n] + exp(md.log_var_noise[0]), m_ = mu[n];
  if (m1o || m2o) {
    const double sq = sqrt(2.0 * var);
    double m1 = 0.0, e2 = 0.0;
    bool fail = false;
    for (int s = 0; s < md.S; ++s) {
      const double xi = warp_inverse(fp, tp, nullptr, m_ + sq * md.xs[s], &fail);
      m1 += md.wn[s] * xi;
      e2 += md.wn[s] * xi * xi;
    }
    if (fail) { m1 = NAN; e2 = NAN; }   // (no status word in this entry: a failed inversion must not pass for a moment)
    if (m1o) m1o[n] = m1;
    if (m2o) m2o[n] = e2 - m1 * m1;
  }
  if (logp && Y) {
    double x = Y[n], ld = 0.0;
    for (int b = 0; b < fp.nblk; ++b) {
      const int kind = fp.blk[4 * b], K = fp.blk[4 * b + 1], poff = fp.blk[4 * b + 2], flags = fp.blk[4 * b + 3];
      const WVal r = warp_block_shared<false>(kind, K, flags, tp + poff, x);
      x = r.g;
      ld += log(r.g1);
    }
    const double res = x - m_;
    logp[n] = -0.5 * (TGP_LOG_2PI_REF + log(var) + res * res / var) + ld - log(Y_std);
  }
}

// ---------------------------------------------------------------------------------------------------
// host launchers
// ---------------------------------------------------------------------------------------------------
int launch_ell_warp(const tgp_model& md, const FlowProg& fp, int mode, const double* Y, const double* mu, const double* v,
                    double* out, double* g_mu, double* g_v, double* g_theta, double* t_out, double* ws, hipStream_t st) {
  const int nt = warp_threads(md.N), nb = warp_blocks(md.N), Pp = md.P > 0 ? md.P : 1;
  const size_t lds = ((size_t)(2 + nt / 64) * Pp + 12 + 8 * 33 + (size_t)(fp.nblk > 0 ? fp.nblk : 1) * nt) * sizeof(double);
  static size_t cur = 48 * 1024;
  if (int rc = ensure_lds(reinterpret_cast<const void*>(k_ell_warp), lds, &cur)) return rc;
  int32_t* ticket = reinterpret_cast<int32_t*>(ws + (size_t)nb * (3 + md.P));
  if (mode == TGP_WARP_FULL) {
    // a stand-alone call cannot count on what an earlier call left in its workspace
    hipError_t e = hipMemsetAsync(ticket, 0, sizeof(int32_t), st);
    if (e != hipSuccess) return set_error(e, __FILE__, __LINE__);
  }
  hipLaunchKernelGGL(k_ell_warp, dim3(nb), dim3(nt), lds, st, md, fp, mode, Y, mu, v, out, g_mu, g_v, g_theta, t_out, ws, ticket);
  LAUNCH_CHECK();
  return 0;
}

int launch_flow_inverse(const tgp_model& md, const FlowProg& fp, const double* t, int S, int N, const double* rowp, double* x,
                        int32_t* status, hipStream_t st) {
  const size_t total = (size_t)S * N;
  const size_t lds = 2 * (size_t)(md.P > 0 ? md.P : 1) * sizeof(double);
  static size_t cur = 48 * 1024;
  if (int rc = ensure_lds(reinterpret_cast<const void*>(k_flow_inverse), lds, &cur)) return rc;
  hipLaunchKernelGGL(k_flow_inverse, dim3((unsigned)((total + 255) / 256)), dim3(256), lds, st, md, fp, t, total, N, rowp, x, status);
  LAUNCH_CHECK();
  return 0;
}

int launch_predict_warp(const tgp_model& md, const FlowProg& fp, const double* mu, const double* v, const double* Y, double Y_std,
                        double* m1, double* m2, double* logp, hipStream_t st) {
  const size_t lds = 2 * (size_t)(md.P > 0 ? md.P : 1) * sizeof(double);
  static size_t cur = 48 * 1024;
  if (int rc = ensure_lds(reinterpret_cast<const void*>(k_predict_warp), lds, &cur)) return rc;
  hipLaunchKernelGGL(k_predict_warp, dim3((md.N + 255) / 256), dim3(256), lds, st, md, fp, mu, v, Y, Y_std, m1, m2, logp);
  LAUNCH_CHECK();
  return 0;
}

}  // namespace tgp
