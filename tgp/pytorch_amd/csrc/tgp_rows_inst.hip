// tgp_rows_inst.hip -- one translation unit per MT (compiled 8x with -DTGP_MT=1..8 so the big unrolled
// kernels build in parallel); each defines launch_rows_mt<N>().  Compiled another 8x with -DTGP_FLOWX_BUILD=1: the training
// kernels whose flow sweeps know the extended kind set (the TGP_FLOWX bit set in MODE / NW), launch_rows_mt<N>_x(), and 8x with
// -DTGP_FLOWX_BUILD=2: the same with the kinds past INV_BOXCOX compiled in as well (TGP_FLOWX2), launch_rows_mt<N>_x2().
// Compiled another 8 x 3 times with -DTGP_KT=1..3: the training kernels (mode 1 at 16 and at 10 rows per wave, plain kind set)
 // that leave out the padded k-steps of M's last tile (k_rows<.., MODE | TGP_ROWS_KT(KT), ..>), launch_rows_mt<N>_kt<K>().
#include "tgp_rows.hpp"
#include "tgp_rows4.hpp"
#include "tgp_launch.hpp"

#ifndef TGP_MT
#error "compile with -DTGP_MT=<1..8>"
#endif
#ifndef TGP_FLOWX_BUILD
#define TGP_FLOWX_BUILD 0
#endif
#define CAT_(a, b) a##b
#define CAT(a, b) CAT_(a, b)
#if TGP_FLOWX_BUILD == 2
#define TGP_XBIT TGP_FLOWX2
#define TGP_LAUNCH_MT CAT(CAT(launch_rows_mt, TGP_MT), _x2)
#elif TGP_FLOWX_BUILD
#define TGP_XBIT TGP_FLOWX
#define TGP_LAUNCH_MT CAT(CAT(launch_rows_mt, TGP_MT), _x)
#else
#define TGP_XBIT 0
#define TGP_LAUNCH_MT CAT(launch_rows_mt, TGP_MT)
#endif
// TGP_DP16_APART: this unit leaves the DP = 16 kernels to a unit of their own, compiled with -DTGP_DP16_ONLY, which defines
// launch_rows_mt<N>[_x]_dp16() (the Makefile uses it where the compiler cannot build those kernels with the others' flags)
#ifndef TGP_DP16_APART
#define TGP_DP16_APART 0
#endif
#ifndef TGP_DP16_ONLY
#define TGP_DP16_ONLY 0
#endif
#define TGP_LAUNCH_DP16 CAT(TGP_LAUNCH_MT, _dp16)
#ifndef TGP_KT
#define TGP_KT 4
#endif
#if TGP_KT != 4 && TGP_FLOWX_BUILD
#error "the trimmed units hold the plain kind set only"
#endif
#define TGP_LAUNCH_KT CAT(CAT(CAT(launch_rows_mt, TGP_MT), _kt), TGP_KT)

namespace tgp {

template <int DP, int MODE, int RW = 16>
static int launch_one(const RowArgs& a, size_t lds, hipStream_t st) {
  constexpr bool TRAIN = MODE != 0;
  auto kern = k_rows<TGP_MT, DP, MODE | TGP_XBIT | TGP_ROWS_KT(TGP_KT), RW>;
  static size_t lds_cur = 48 * 1024;
  if (int rc = ensure_lds(reinterpret_cast<const void*>(kern), lds, &lds_cur)) return rc;
  // the row blocks, then (training) the MT passenger blocks
  const int grid = a.p.nblocks + (TRAIN ? a.p.MT : 0);
  hipLaunchKernelGGL(kern, dim3(grid), dim3(256), lds, st, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return set_error(e, __FILE__, __LINE__);
  return 0;
}

#if TGP_KT != 4
// mode: 1 (16 rows per wave) or 200 (10), the two the dispatch sends here
template <int DP>
static int launch_kt(const RowArgs& a, int mode, size_t lds, hipStream_t st) {
  if (mode == 200) return launch_one<DP, 1, TGP_RW_SMALL>(a, lds, st);
  return launch_one<DP, 1>(a, lds, st);
}
int TGP_LAUNCH_KT(const RowArgs& a, int mode, size_t lds, hipStream_t st) {
  switch (a.p.DP) {
    case 4: return launch_kt<4>(a, mode, lds, st);
    case 8: return launch_kt<8>(a, mode, lds, st);
    default: return launch_kt<16>(a, mode, lds, st);
  }
}
#else
// the 4-rows-per-wave kernel (tgp_rows4.hpp): NW waves per workgroup
template <int DP, bool TRAIN, int NW>
static int launch_one4(const RowArgs& a, hipStream_t st) {
  auto kern = k_rows4<TGP_MT, DP, TRAIN, NW | TGP_XBIT>;
  const size_t lds = row4_lds(a.p, TRAIN, a.prog.nslots, NW).total * sizeof(double);
  static size_t lds_cur = 48 * 1024;
  if (int rc = ensure_lds(reinterpret_cast<const void*>(kern), lds, &lds_cur)) return rc;
  const int grid = a.p.nblocks + (TRAIN ? a.p.MT : 0);   // Plan.nblocks = ceil(N / 4 NW); then the MT passenger blocks
  hipLaunchKernelGGL(kern, dim3(grid), dim3(NW * 64), lds, st, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return set_error(e, __FILE__, __LINE__);
  return 0;
}

template <int DP>
static int launch_dp(const RowArgs& a, int mode, size_t lds, hipStream_t st) {
  switch (mode) {
    case 150 + 4: return launch_one4<DP, true, 4>(a, st);
    case 150 + 8: return launch_one4<DP, true, 8>(a, st);
    case 200: return launch_one<DP, 1, TGP_RW_SMALL>(a, lds, st);
#if TGP_FLOWX_BUILD
    case 0: return TGP_E_UNSUPPORTED;   // (moments only: no flow, the plain kernel serves every program)
#else
    case 0: return launch_one<DP, 0>(a, lds, st);
#endif
    case 1: return launch_one<DP, 1>(a, lds, st);
    default: return launch_one<DP, 2>(a, lds, st);
  }
}

#if TGP_DP16_ONLY
int TGP_LAUNCH_DP16(const RowArgs& a, int mode, size_t lds, hipStream_t st) { return launch_dp<16>(a, mode, lds, st); }
#else
#if TGP_DP16_APART
int TGP_LAUNCH_DP16(const RowArgs& a, int mode, size_t lds, hipStream_t st);
#endif
int TGP_LAUNCH_MT(const RowArgs& a, int mode, size_t lds, hipStream_t st) {
  switch (a.p.DP) {
    case 4: return launch_dp<4>(a, mode, lds, st);
    case 8: return launch_dp<8>(a, mode, lds, st);
#if TGP_DP16_APART
    default: return TGP_LAUNCH_DP16(a, mode, lds, st);
#else
    default: return launch_dp<16>(a, mode, lds, st);
#endif
  }
}
#endif

#endif   // TGP_KT == 4

#if TGP_MT == 1 && !TGP_FLOWX_BUILD && TGP_KT == 4
size_t rows4_lds_bytes(const Plan& p, bool train, int nw) {
  const Row4Lds L = row4_lds(p, train, p.nslots, nw);
  return L.nb == 0 ? (size_t)1 << 30 : L.total * sizeof(double);   // (not even one quadrature node per lane fits: not a candidate)
}
#endif

}  // namespace tgp
