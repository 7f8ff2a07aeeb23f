// Prints yu::plan_iov (yustack_amd/csrc/yucsum_plan.h) for the batches named on
// the command line: `iov_plan n mode fill cus [n mode fill cus ...]`, one line
// "kernel policy blocks name" each. The knobs come from the environment as in
// the library (YU_TUNING=1 and YU_NT / YU_BLOCKS_PER_CU). CPU only.
#include <stdio.h>
#include <stdlib.h>

#include "yucsum_plan.h"

int main(int argc, char **argv) {
  if (argc < 5 || (argc - 1) % 4) return 2;
  for (int i = 1; i + 3 < argc; i += 4) {
    const yu::IovPlan p = yu::plan_iov(strtoull(argv[i], nullptr, 10), atoi(argv[i + 1]),
                                       atoi(argv[i + 2]) != 0, atoi(argv[i + 3]), yu::env_knobs());
    printf("%d %d %u %s\n", (int)p.kernel, (int)p.policy, p.blocks, p.name);
  }
  return 0;
}
