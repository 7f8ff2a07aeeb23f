// Prints yu::plan_wave (yustack_amd/csrc/yucsum_plan.h) for the batches named on
// the command line: `wave_plan family n mode fill cus [...]` (family: iov, pack,
// build or split), one line "kernel policy blocks name" each; the argument `enum` prints
// one line with the values of the yu::WaveKernel enumerators in order and their
// count. The knobs come from the environment as in the library (YU_TUNING=1 and
// YU_NT / YU_BLOCKS_PER_CU). CPU only.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "yucsum_plan.h"

int main(int argc, char **argv) {
  for (int i = 1; i < argc;) {
    if (!strcmp(argv[i], "enum")) {
      printf("enum");
#define YU_X(id, ...) printf(" %d", (int)yu::k_##id);
      YU_WAVE_KERNELS(YU_X)
#undef YU_X
      printf(" %d\n", (int)yu::kWaveKernelCount);
      i += 1;
      continue;
    }
    if (i + 4 >= argc) return 2;
    yu::WaveFamily family;
    if (!strcmp(argv[i], "iov")) family = yu::WaveFamily::Iov;
    else if (!strcmp(argv[i], "pack")) family = yu::WaveFamily::Pack;
    else if (!strcmp(argv[i], "build")) family = yu::WaveFamily::Build;
    else if (!strcmp(argv[i], "split")) family = yu::WaveFamily::Split;
    else return 2;
    const yu::WavePlan p = yu::plan_wave(family, strtoull(argv[i + 1], nullptr, 10), atoi(argv[i + 2]),
                                         atoi(argv[i + 3]) != 0, atoi(argv[i + 4]), yu::env_knobs());
    printf("%d %d %u %s\n", (int)p.kernel, (int)p.policy, p.blocks, p.name);
    i += 5;
  }
  return 0;
}
