// plan_table — prints the launch plan (yustack_amd/csrc/yucsum_plan.h) of a fixed
// list of batch shapes, one line per case:
//   <U|R> mode align stride len n fill cu | name form policy blocks ppw uf small_waves xcd
// A "# knobs: NAME=VALUE ..." line sets the measurement knobs of the cases after
// it (none: the production choices). tests/test_plan.py compares the output with
// tests/golden/launch_plans.txt. Needs no GPU and no libyucsum.so: built from this
// file and yucsum_plan.cpp alone. (plan_rows.h: the rows and the shape axes, shared
// with plan_query.)
#include "plan_rows.h"

int main() {
  knobs({});
  shape_axes();
  // the ragged picks (uniform VERIFY_RX / TX_DATAGRAM batches take them too)
  for (const char *e : {"YU_RAGGED=loop", "YU_RAGGED=seg4", "YU_RAGGED=seg16", "YU_RAGGED=seg8", "YU_FILL_WB=0",
                        "YU_SEG_SMALL_BLOCKS=0"}) {
    knobs({e});
    ragged_shapes();
    uniform(YU_MODE_VERIFY_RX, false, 0, 1500, 1500, kBig);
    uniform(YU_MODE_TX_DATAGRAM, true, 0, 1500, 1500, kBig);
  }
  knobs({"YU_RAGGED=seg4", "YU_FILL_WB=0"});
  ragged_shapes();
  // the uniform picks
  for (const char *e : {"YU_VARIANT=k_small<32,4>", "YU_VARIANT=k_seg<4", "YU_VARIANT=k_seg<8", "YU_VARIANT=k_hdr",
                        "YU_VARIANT=k_tiny<8>", "YU_VARIANT=k_lane<8>", "YU_RUNS=0", "YU_RUNS=2"}) {
    knobs({e});
    uniform_shapes();
  }
  // policy and grid: both
  for (const char *e : {"YU_NT=0", "YU_NT=1", "YU_BLOCKS_PER_CU=8", "YU_XCD=1"}) {
    knobs({e});
    uniform_shapes();
    ragged_shapes();
  }
  return 0;
}
