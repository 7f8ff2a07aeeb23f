// Prints yu::plan_iov_pack and yu::plan_iov (yustack_amd/csrc/yucsum_plan.h) for
// the batches named on the command line: `iov_pack_datagram_plan n mode fill cus
// [...]`, one line "kernel policy blocks name | kernel policy blocks name" each
// (the packing plan, then plan_iov's row for the same batch), then one line with
// the values of the yu::IovKernel enumerators in order. The knobs come from the
// environment as in the library. CPU only.
#include <stdio.h>
#include <stdlib.h>

#include "yucsum_plan.h"

int main(int argc, char **argv) {
  if ((argc - 1) % 4) return 2;
  for (int i = 1; i + 3 < argc; i += 4) {
    const uint64_t n = strtoull(argv[i], nullptr, 10);
    const int mode = atoi(argv[i + 1]), cus = atoi(argv[i + 3]);
    const bool fill = atoi(argv[i + 2]) != 0;
    const yu::IovPlan p = yu::plan_iov_pack(n, mode, fill, cus, yu::env_knobs());
    const yu::IovPlan q = yu::plan_iov(n, mode, fill, cus, yu::env_knobs());
    printf("%d %d %u %s | %d %d %u %s\n", (int)p.kernel, (int)p.policy, p.blocks, p.name, (int)q.kernel,
           (int)q.policy, q.blocks, q.name);
  }
  printf("enum %d %d %d %d %d %d %d %d %d\n", (int)yu::k_iov4, (int)yu::k_iov4_fill, (int)yu::k_iov4_dg,
         (int)yu::k_iov4_dg_fill, (int)yu::k_pack4, (int)yu::k_pack4_fill, (int)yu::k_pack4_dg,
         (int)yu::k_pack4_dg_fill, (int)yu::kIovPackEnd);
  return 0;
}
