// Prints yu::plan_group (yustack_amd/csrc/yucsum_plan.h) for the batches named on the
// command line: `group_plan n m cus [...]`, one line each:
//   digit_bits passes tile blocks lane_blocks hist_off hist_bytes sums_off sums_bytes
//   count_off count_bytes pair0_off pair0_bytes pair1_off pair1_bytes bytes name
// The knobs come from the environment as in the library. CPU only.
#include <stdio.h>
#include <stdlib.h>

#include "yucsum_plan.h"

int main(int argc, char **argv) {
  if (argc < 4 || (argc - 1) % 3) return 2;
  for (int i = 1; i + 2 < argc; i += 3) {
    const yu::GroupPlan p = yu::plan_group(strtoull(argv[i], nullptr, 10), strtoull(argv[i + 1], nullptr, 10),
                                           atoi(argv[i + 2]), yu::env_knobs());
    printf("%u %u %u %u %u", p.digit_bits, p.passes, p.tile, p.blocks, p.lane_blocks);
    const unsigned long long r[] = {p.hist_off,    p.hist_bytes,  p.sums_off,      p.sums_bytes,
                                    p.count_off,   p.count_bytes, p.pair_off[0],   p.pair_bytes[0],
                                    p.pair_off[1], p.pair_bytes[1], p.bytes};
    for (unsigned long long v : r) printf(" %llu", v);
    printf(" %s\n", p.name);
  }
  return 0;
}
