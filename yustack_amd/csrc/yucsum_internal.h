// yucsum_internal.h — library-internal entry points shared by the translation
// units of libyucsum.so. Not part of the C ABI (include/yucsum.h).
#ifndef YUCSUM_INTERNAL_H
#define YUCSUM_INTERNAL_H

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "yucsum.h"
#include "yucsum_proto.h"

// The protocol tables shared by the kernels and the host-side field writer
// (mode_field, mode_is_tx, mode_fills, l4_field, l4_min) are yucsum_proto.h's.
namespace yu {

// Measurement knobs (YU_RAGGED, YU_VARIANT, YU_NT, YU_FILL_WB, YU_RUNS,
// YU_BLOCKS_PER_CU, YU_SEG_SMALL_BLOCKS, YU_XCD, YU_HOST_COPY_THREADS,
// YU_HOST_DIRECT_MAX, YU_HOST_SLICE_BYTES, YU_HOST_SLICE_PACKETS (where the
// host path cuts its slices, at most the compiled limits), and the fault
// injection YU_HOST_FAIL_ALLOC) force kernels, grids, cut-overs, slice seams
// and failures for tools/ and the forced-kernel and host-ledger test runs.
// They are read only when the process also sets YU_TUNING=1, so a production
// process that inherits one of them keeps the library's own choices; when the gate is open, each knob that is set is named
// once on stderr. Returns the knob's value, or NULL (gate closed or unset).
inline const char *tuning_env(const char *name) {
  static const bool on = [] {
    const char *g = getenv("YU_TUNING");
    return g && g[0] == '1' && g[1] == '\0';
  }();
  if (!on) return nullptr;
  const char *v = getenv(name);
  if (v && *v) fprintf(stderr, "yucsum: tuning knob %s=%s (YU_TUNING=1)\n", name, v);
  return v;
}

}  // namespace yu

// Enqueue on `stream` a one-thread kernel that stores `value` to `flag` (a
// device view of coherent pinned host memory) with system-scope fences, so a
// host thread polling the flag sees it only after everything enqueued before
// it on the stream has completed. Returns a YU_* status.
__attribute__((visibility("hidden"))) int yu_internal_signal(uint32_t *flag, uint32_t value,
                                                       void *stream);

#endif  // YUCSUM_INTERNAL_H
