// Prints yu::plan_build (yustack_amd/csrc/yucsum_plan.h) for the batches named on
// the command line: `tx_build_plan n cus [...]`, one line "kernel policy blocks
// name" each. The knobs come from the environment as in the library. CPU only.
#include <stdio.h>
#include <stdlib.h>

#include "yucsum_plan.h"

int main(int argc, char **argv) {
  if ((argc - 1) % 2) return 2;
  for (int i = 1; i + 1 < argc; i += 2) {
    const uint64_t n = strtoull(argv[i], nullptr, 10);
    const yu::BuildPlan p = yu::plan_build(n, atoi(argv[i + 1]), yu::env_knobs());
    printf("%d %d %u %s\n", (int)p.kernel, (int)p.policy, p.blocks, p.name);
  }
  return 0;
}
