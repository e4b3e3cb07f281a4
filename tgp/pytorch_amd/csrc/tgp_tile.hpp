// tgp_tile.hpp -- the on-chip tile vocabulary of the stand-alone operators (tgp_cov, tgp_unwhiten, tgp_optqu, tgp_greedy, tgp_pathwise).
// A name is here because two call sites share it and none got slower by it; DESIGN.md names the candidates that stay in their kernels.
#pragma once
#include <type_traits>
#include "tgp_dev.hpp"

namespace tgp {

constexpr int TL_T = 64;    // output tile (rows and columns)
constexpr int TL_KC = 16;   // contraction indices staged or generated per step
constexpr int TL_LDN = 80;  // LDS stride (f64) of a [16 k][64 n] operand tile: the 4 k rows of one MFMA operand fall in distinct banks
constexpr int TL_LDK = 18;  // LDS stride (f64) of a [64 r][16 k] operand tile: 16 rows x 2 k of a half wave in distinct banks
constexpr int TL_LDT = 65;  // LDS stride (f64) of the 64 x 64 output tile: conflict-free along rows and along columns

// ils[d] = 1 / length-scale d for d < D and zero above, ils[16] = the output scale, ils[17] = the RQ kernel's alpha (TL_ILS doubles).
// The caller's barrier follows; tile_cov reads the covariance description back after it.
constexpr int TL_ILS = 18;
__device__ __forceinline__ void tile_scales(int kernel, int D, const double* __restrict__ raw_ls, const double* __restrict__ raw_os,
                                            double* ils) {
  const int tid = threadIdx.x;
  if (tid < 16) ils[tid] = tid < D ? 1.0 / softplus_d(raw_ls[tid]) : 0.0;
  if (tid == 64) { ils[16] = softplus_d(raw_os[0]); ils[17] = cov_alpha(kernel, raw_os); }
}
__device__ __forceinline__ Cov tile_cov(int kernel, const double* ils) { return make_cov(kernel, ils[16], ils[17]); }

// tile t of the lower block triangle, row major: (ti, tj), tj <= ti
__device__ __forceinline__ void tile_lower(int t, int& ti, int& tj) {
  ti = (int)((sqrtf(8.0f * (float)t + 1.0f) - 1.0f) * 0.5f);
  while ((ti + 1) * (ti + 2) / 2 <= t) ++ti;
  while (ti * (ti + 1) / 2 > t) --ti;
  tj = t - ti * (ti + 1) / 2;
}

// host: f(std::integral_constant<int, DP>) with the padded input dimension DP = 4, 8 or 16 that holds D
template <class F>
inline void dispatch_dp(int D, F&& f) {
  if (D <= 4) f(std::integral_constant<int, 4>{});
  else if (D <= 8) f(std::integral_constant<int, 8>{});
  else f(std::integral_constant<int, 16>{});
}

}  // namespace tgp
