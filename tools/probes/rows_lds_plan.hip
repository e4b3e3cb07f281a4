// rows_lds_plan.hip -- host only: the LDS plan of k_rows at 10 rows per wave, from the headers of the tree it is built in.
// For MT = 1 .. 8, DP = 4, 8, 16 and every flow program on stdin it prints row_lds(p, 1, nslots, 10).total in bytes, whether
// that is within the 160 KiB - 1 KiB a kernel is granted, and the rows per wave the dispatch then picks (the rule of rows_per_wave,
// tgp_rows.hip, restated below: it reads nothing of the plan but row_lds).  Built and run on two trees, the two outputs side by
// side show that a change of the carve-up loses no (plan, program) the 10-rows-per-wave kernel had (profiles/r11_rows_lds_plan.txt).
//   hipcc -std=c++17 --offload-arch=gfx950 -I tgp/pytorch_amd/csrc tools/probes/rows_lds_plan.hip -o rows_lds_plan
//   python tools/probes/rows_lds_plan.py | ./rows_lds_plan
// stdin, one program per line:  name S P RP nblk  kind K poff flags  (nblk times)
#include <cstdio>
#include "tgp_rows.hpp"

using namespace tgp;

static int rows_per_wave_rule(const Plan& p, const FlowProg& fp) {
  for (int b = 0; b < fp.nblk; ++b)
    if ((fp.blk[4 * b + 3] & TGP_FLAG_PER_ROW) && fp.blk[4 * b] != TGP_FLOW_SAL) return 16;
  if (rows_rw(p.N) != TGP_RW_SMALL || TGP_RW_SMALL * p.S > 64 * TGP_RW_NODES) return 16;
  if (row_lds(p, 1, p.nslots, TGP_RW_SMALL).total * sizeof(double) > 160 * 1024 - 1024) return 16;
  return TGP_RW_SMALL;
}

int main() {
  char name[128];
  int S, P, RP, nblk;
  std::printf("%-28s %3s %3s %3s %6s %2s %2s %8s %4s %2s\n", "program", "S", "P", "RP", "nslots", "MT", "DP", "bytes", "fits", "rw");
  while (std::scanf("%127s %d %d %d %d", name, &S, &P, &RP, &nblk) == 5) {
    FlowProg fp{};
    fp.nblk = nblk;
    for (int i = 0; i < 4 * nblk; ++i)
      if (std::scanf("%d", &fp.blk[i]) != 1) return 1;
    fp.nslots = flow_slots(fp.blk, nblk);
    for (int MT = 1; MT <= 8; ++MT)
      for (int DP = 4; DP <= 16; DP *= 2) {
        Plan p;
        make_plan(p, 8611, DP, 16 * MT - 12, S, nblk, P, RP, TGP_LIK_FLOW, 0, TGP_RW_SMALL);
        p.nslots = fp.nslots;
        const size_t bytes = row_lds(p, 1, fp.nslots, TGP_RW_SMALL).total * sizeof(double);
        std::printf("%-28s %3d %3d %3d %6d %2d %2d %8zu %4s %2d\n", name, S, P, RP, fp.nslots, MT, DP, bytes,
                    bytes <= 160 * 1024 - 1024 ? "yes" : "NO", rows_per_wave_rule(p, fp));
      }
  }
  return 0;
}
