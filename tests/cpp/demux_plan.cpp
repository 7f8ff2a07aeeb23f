// Prints yu::plan_demux (yustack_amd/csrc/yucsum_plan.h) for the batches named on
// the command line: `demux_plan n cus [...]`, one line "policy blocks name" each.
// The knobs come from the environment as in the library (YU_TUNING=1 and YU_NT /
// YU_BLOCKS_PER_CU). CPU only.
#include <stdio.h>
#include <stdlib.h>

#include "yucsum_plan.h"

int main(int argc, char **argv) {
  if (argc < 3 || (argc - 1) % 2) return 2;
  for (int i = 1; i + 1 < argc; i += 2) {
    const yu::DemuxPlan p = yu::plan_demux(strtoull(argv[i], nullptr, 10), atoi(argv[i + 1]), yu::env_knobs());
    printf("%d %u %s\n", (int)p.policy, p.blocks, p.name);
  }
  return 0;
}
