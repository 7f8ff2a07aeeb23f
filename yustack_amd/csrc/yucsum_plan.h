// yucsum_plan.h — the launch plan: which kernel a batch gets, in which form, with
// which load policy and on which grid. One list of kernels (YU_KERNELS) and one
// pure function (plan) hold the whole decision; yucsum_kernels.hip builds its
// function table from the same list and launches what the plan names. The
// wave-per-packet calls (scatter-gather, packing, yu_tx_build_ragged,
// yu_rx_split_ragged) have the same pair beside it: YU_WAVE_KERNELS and
// plan_wave; yu_rx_parse_ragged's header pass, a lane per packet, has plan_parse,
// yu_rx_demux's kernel, a lane per record, plan_demux, and yu_rx_reply's
// plan_reply (one rule for the three); yu_rx_group's launches and workspace have
// plan_group. yu_tx_build_iov takes yu_tx_build_ragged's plan_wave row.
// No HIP call is made here,
// so tests/cpp/plan_table.cpp and tests/cpp/wave_plan.cpp check every decision
// on a CPU.
#ifndef YUCSUM_PLAN_H
#define YUCSUM_PLAN_H

#include <stdint.h>

#pragma GCC visibility push(hidden)  // library-internal, like yucsum_internal.h's entry point
namespace yu {

constexpr uint32_t kLEMax = 131072u;     // longest packet the LE sum covers
constexpr uint32_t kOOB = 0x80000000u;   // out-of-range buffer offset (loads return zeros)

enum class Family : uint8_t { Lane, Tiny, Small, Loop, Hdr, Seg };
enum class SegKind : uint8_t { None, Plain, Tx, Rx, Dg, TxW };
// Blocks per CU (blocks_per_cu in yucsum_plan.cpp has the measurements).
enum class Grid : uint8_t {
  B64,   // MTU-size and larger packets, one-wave-per-packet and stream kernels
  B16,   // the small-packet lane-group variants (G < 16)
  B6,    // the 64-packet-step kernels (k_lane, k_tiny)
  B10U,  // 4 KiB k_seg tiles: 10 on uniform batches, 64 on ragged ones
};

// k_small runs of 16 packets per wave (one side-record load and one result
// store per run): config 3 235-246 -> 235-240 us against the interleaved
// mapping (PR = 0; equal on some boxes), 64-packet runs 248; 1M x 768 B 131.5
// -> 122.6, x 3000 B 467.8 -> 450.7; 256K x 768 B 43.8 -> 35.0. The in-place
// fill keeps the interleaved mapping (config 9: 313 vs 328 us with runs), and
// so do batches of fewer than 8 runs per CU (see plan).
// profiles/r02/kbench_ab_k_small_runs.log
constexpr int kSmallRun = 16;

// The kernels, each once: X(id, name, family, window, G, ppw, run, grid,
// own_fill, fill_plain, tile, kind, ragged_fill, targs).
//   window       bytes covered per packet step (0 = loop / stream kernel)
//   G, ppw       lanes per packet; packets per wave step (k_seg: per chunk)
//   run          packets per wave run (k_small), 0 = none
//   own_fill     writing in place is an instantiation of its own (form Fill)
//   fill_plain   writing in place, it loads by the fill policy (plain loads)
//   tile, kind   k_seg: KiB per tile and the kind
//   ragged_fill  the kernel a ragged in-place call takes instead (itself: none)
//   targs        what yucsum_kernels.hip instantiates the family's template with
// Within a family the order is the order pick_uniform tries them in.
//
// window of k_lane = the largest stride a wave step's U KiB hold (64 packets).
#define YU_K_LANE(X, U)                                                                       \
  X(lane##U, "k_lane<" #U ">", Lane, 16u * U, 1, 64, 0, B6, false, false, 0, None, lane##U, (U))
// k_tiny<8> (113..128 bytes) fills with single field stores: its whole-chunk
// instantiation would spill scalar registers
#define YU_K_TINY(X, G, OWN_FILL)                                                             \
  X(tiny##G, "k_tiny<" #G ">", Tiny, 16u * G, G, 64, 0, B6, OWN_FILL, false, 0, None, tiny##G, \
    (G, OWN_FILL))
#define YU_K_SMALL(X, G, U, GRID)                                                             \
  X(small##G##_##U, "k_small<" #G "," #U ">", Small, 16u * G * U, G, 64u / G, kSmallRun, GRID, \
    false, true, 0, None, small##G##_##U, (G, U))
#define YU_K_LOOP(X, ID, NAME) \
  X(ID, NAME, Loop, 0, 64, 1, 0, B64, false, false, 0, None, ID, (ID))
#define YU_K_SEG(X, ID, NAME, U, KIND, CH, GRID, FILL_PLAIN, RAGGED_FILL) \
  X(ID, NAME, Seg, 0, 64, CH, 0, GRID, false, FILL_PLAIN, U, KIND, RAGGED_FILL, (U, KIND, CH))

#define YU_KERNELS(X)                                                                         \
  YU_K_LANE(X, 2) YU_K_LANE(X, 3) YU_K_LANE(X, 4) YU_K_LANE(X, 5)                             \
  YU_K_LANE(X, 6) YU_K_LANE(X, 7) YU_K_LANE(X, 8)                                             \
  YU_K_TINY(X, 4, true) YU_K_TINY(X, 8, false)                                                \
  /* Ordered by window; for each window the variant with the most packets per */             \
  /* wave comes first (amortises the per-packet epilogue over more bytes). */                 \
  YU_K_SMALL(X, 4, 1, B16) YU_K_SMALL(X, 8, 1, B16) YU_K_SMALL(X, 8, 2, B16)                  \
  YU_K_SMALL(X, 16, 2, B64) YU_K_SMALL(X, 16, 3, B64) YU_K_SMALL(X, 16, 4, B64)               \
  YU_K_SMALL(X, 16, 6, B64) YU_K_SMALL(X, 32, 4, B64) YU_K_SMALL(X, 32, 6, B64)               \
  YU_K_SMALL(X, 64, 4, B64)                                                                   \
  YU_K_LOOP(X, loop_le, "k_loop<4,LE>") YU_K_LOOP(X, loop_be, "k_loop<4,BE>")                 \
  YU_K_LOOP(X, loop_rx, "k_loop<4,rx>") YU_K_LOOP(X, loop_dg, "k_loop<4,dg>")                 \
  /* plain loads by default (policy slot 2 = slot 0): for scattered 32-byte header */         \
  /* reads they beat nt ones (30.7 vs 32.5 us, kbench 12) */                                  \
  X(hdr, "k_hdr", Hdr, 0, 64, 64, 0, B64, false, false, 0, None, hdr, ())                     \
  /* 64 packets per chunk. (63 packets and a marker lane, kMarker, which drops the */         \
  /* end-point slot: small RX datagrams 27.0 -> 26.6 us, but config 4 703 -> 714 and */       \
  /* U{64..1500} 127 -> 129 from the 1.6 % more chunks; the 16-packet chunks use it. */       \
  /* profiles/r03/kbench_ab_kseg_lean.log) */                                                 \
  YU_K_SEG(X, seg4, "k_seg<4>", 4, Plain, 64, B10U, false, seg4)                              \
  YU_K_SEG(X, seg8, "k_seg<8>", 8, Plain, 64, B64, false, seg8)                               \
  YU_K_SEG(X, seg4_tx, "k_seg<4,tx>", 4, Tx, 64, B10U, false, seg4_txw)                       \
  YU_K_SEG(X, seg8_tx, "k_seg<8,tx>", 8, Tx, 64, B64, false, seg8_txw_c48)                    \
  YU_K_SEG(X, seg4_rx, "k_seg<4,rx>", 4, Rx, 64, B64, false, seg4_rx)                         \
  YU_K_SEG(X, seg8_rx, "k_seg<8,rx>", 8, Rx, 64, B64, false, seg8_rx)                         \
  /* 16-packet chunks: 4x the waves for mid-size ragged batches (see pick_ragged) */          \
  YU_K_SEG(X, seg8_c16, "k_seg<8,c16>", 8, Plain, 16, B64, false, seg8_c16)                   \
  YU_K_SEG(X, seg8_tx_c16, "k_seg<8,tx,c16>", 8, Tx, 16, B64, false, seg8_txw_c16)            \
  /* the TX kinds' in-place form for ragged batches (the whole-line write-back) */            \
  YU_K_SEG(X, seg4_txw, "k_seg<4,txw>", 4, TxW, 64, B64, false, seg4_txw)                     \
  YU_K_SEG(X, seg8_txw_c16, "k_seg<8,txw,c16>", 8, TxW, 16, B64, false, seg8_txw_c16)         \
  YU_K_SEG(X, seg8_rx_c16, "k_seg<8,rx,c16>", 8, Rx, 16, B64, false, seg8_rx_c16)             \
  /* (no 4 KiB-tile DG kind: datagram batches take the ragged picks, 8 KiB) */                \
  /* TX_DATAGRAM in place loads plainly too (fill_plain): a datagram's header line is */      \
  /* then more often still cached when its two field stores arrive (1M datagrams */           \
  /* U{40..1500}: 211.5 -> 203.1 us; the TXW kind is better off non-temporal, 48.7 */         \
  /* vs 52.1 us; profiles/r04/kbench_ab_r04k_fill_nt.log) */                                  \
  YU_K_SEG(X, seg8_dg, "k_seg<8,dg>", 8, Dg, 64, B64, true, seg8_dg_c40)                      \
  YU_K_SEG(X, seg8_dg_c16, "k_seg<8,dg,c16>", 8, Dg, 16, B64, true, seg8_dg_c16)              \
  /* In place, from 64K packets on: smaller chunks. The TXW kind at 48 packets (1M UDP */     \
  /* datagrams U{40..200}: 48.7 -> 46.3 us; U{64..1500} TCP 192.9 -> 190.4: a small */        \
  /* datagram chunk then fits one 8 KiB tile, so all its fields go out as whole */            \
  /* lines), TX_DATAGRAM at 40 (U{40..1500}: 204.3 -> 198.7 us). The read-only kinds */       \
  /* keep 64 (RX U{40..200} 26.5 vs 27.5 at 48 and 30.3 at 40; plain unchanged). */           \
  /* profiles/r04/kbench_ab_r04v_seg_chunk.log (and r04s/r04t/r04u for 32..60) */             \
  YU_K_SEG(X, seg8_txw_c48, "k_seg<8,txw,c48>", 8, TxW, 48, B64, false, seg8_txw_c48)         \
  YU_K_SEG(X, seg8_dg_c40, "k_seg<8,dg,c40>", 8, Dg, 40, B64, true, seg8_dg_c40)

enum KernelId : uint8_t {
#define YU_X(id, ...) k_##id,
  YU_KERNELS(YU_X)
#undef YU_X
  kKernelCount
};

struct KernelInfo {
  const char *name;
  Family family;
  uint32_t window, G, ppw, run;
  Grid grid;
  bool own_fill, fill_plain;
  uint32_t tile;
  SegKind kind;
  KernelId ragged_fill;
};
extern const KernelInfo kKernels[kKernelCount];

// The measurement knobs, as values. The defaults are the production choices.
struct Knobs {
  enum class Ragged : uint8_t { Auto, Loop, Seg4, Seg16, Seg8 };
  Ragged ragged = Ragged::Auto;  // YU_RAGGED (any other value acts as seg8)
  bool forced = false;           // YU_VARIANT is set
  uint8_t forced_seg = 0;        //   "k_seg<4..." / "k_seg<8...": 4 / 8
  int16_t forced_kernel = -1;    //   a k_small, k_tiny, k_lane or k_hdr name: its id
  int8_t nt = -1;                // YU_NT: load policy 0/1/2 (see bld16) for every form; -1 = unset
  bool fill_wb = true;           // YU_FILL_WB
  uint8_t runs = 1;              // YU_RUNS: 0 never, 1 measured cut-over, 2 whenever not filling
  uint16_t blocks_per_cu = 0;    // YU_BLOCKS_PER_CU: grid size in 256-thread blocks per CU; 0 = per kernel
  uint8_t seg_small_blocks = 3;  // YU_SEG_SMALL_BLOCKS
  bool xcd = false;              // YU_XCD
  bool stream_walk = false;      // YU_STREAM=walk: k_stream takes the general step for every entry (A/B, equality test)
};
// Knobs from their text form: `get` returns a knob's value, or NULL when unset.
Knobs read_knobs(const char *(*get)(const char *name));
// The process's knobs: read once, through yu::tuning_env (YU_TUNING=1 only).
const Knobs &env_knobs();

struct Shape {
  bool ragged;
  uint64_t align;  // uniform: the first packet's address, or just its low 4 bits
  uint64_t stride;
  uint32_t len;
  uint64_t n;
  int mode;
  bool fill;  // written in place
};

enum class Form : uint8_t { Plain, Runs, Inter, Fill };

struct Plan {
  KernelId kernel;
  uint8_t policy;  // load-policy slot 0 / 1 / 2 (plain, nt, hybrid: bld16)
  Form form;       // Runs / Inter: k_small with and without runs; Fill: own_fill kernels in place
  uint32_t blocks;
  uint32_t ppw;    // packets per wave (step, run or chunk)
  uint32_t uf;     // BatchArgs::uf
  uint32_t small_waves;
  uint32_t xcd;
  const char *name;  // what the yu_*_variant* calls of include/yucsum.h return
};

Plan plan(const Shape &s, int cus, const Knobs &k);

// The wave-per-packet device calls have a list and a plan of their own: the
// scatter-gather sums (k_iov, yucsum_iov.h), their packing form (k_pack, k_pack_dg:
// yucsum_iov_pack.h), yu_tx_build_ragged (k_build, yucsum_build.h) and
// yu_rx_split_ragged (k_split, yucsum_split.h). None is one of YU_KERNELS, because
// no uniform or ragged batch ever takes them. Each once:
// X(id, name, family, dg, fill, targs).
//   dg     the kind for whole IPv4 datagrams (the modes of yu::iov_dg_mode_ok)
//   fill   the instantiation that stores the checksum fields
//   targs  what yucsum_kernels.hip instantiates the family's template with
// The ids are the rows of yucsum_kernels.hip's function table, in this order.
#define YU_WAVE_KERNELS(X)                                                          \
  X(iov4, "k_iov<4>", Iov, false, false, (4, false, false))                         \
  X(iov4_fill, "k_iov<4,fill>", Iov, false, true, (4, true, false))                 \
  X(iov4_dg, "k_iov<4,dg>", Iov, true, false, (4, false, true))                     \
  X(iov4_dg_fill, "k_iov<4,dg,fill>", Iov, true, true, (4, true, true))             \
  X(pack4, "k_pack<4>", Pack, false, false, (4, false, false))                      \
  X(pack4_fill, "k_pack<4,fill>", Pack, false, true, (4, true, false))              \
  X(pack4_dg, "k_pack<4,dg>", Pack, true, false, (4, false, true))                  \
  X(pack4_dg_fill, "k_pack<4,dg,fill>", Pack, true, true, (4, true, true))          \
  X(build4, "k_build<4>", Build, false, false, (4))                                \
  X(split4, "k_split<4>", Split, false, false, (4))

enum class WaveFamily : uint8_t { Iov, Pack, Build, Split };
enum WaveKernel : uint8_t {
#define YU_X(id, ...) k_##id,
  YU_WAVE_KERNELS(YU_X)
#undef YU_X
  kWaveKernelCount
};
struct WavePlan {
  WaveKernel kernel;
  uint8_t policy;  // load-policy slot: 0 plain, 1 nt, 2 plain for a step's first slot, nt for the rest
  uint32_t blocks;
  const char *name;  // what the yu_*_variant_n calls of these families return
};
// Iov, Pack: any mode; one of the whole-datagram modes (yu::iov_dg_mode_ok) picks
// the dg kernels, every other the whole-packet ones. Build, Split: one kernel each,
// mode and fill are ignored.
WavePlan plan_wave(WaveFamily family, uint64_t n, int mode, bool fill, int cus, const Knobs &k);

// yu_rx_parse_ragged's header pass (k_parse, yucsum_parse.h) is a lane per packet,
// 64 packets per wave step, so it is a row of neither list: no uniform or ragged
// batch takes it and it is no wave-per-packet kernel. One kernel, its plan here.
struct ParsePlan {
  uint8_t policy;  // load-policy slot: 0 plain, 1 nt
  uint32_t blocks;
  const char *name;  // what yu_rx_parse_variant_n returns
};
ParsePlan plan_parse(uint64_t n, int cus, const Knobs &k);

// yu_rx_demux's kernel (k_demux, yucsum_demux.h) is the same mapping, a lane per
// record, and bound by the same thing, the latency of scattered loads (here the
// table probes), so it takes plan_parse's rule: one function behind both. The
// policy is that of the record stream; the table is always read with plain loads.
typedef ParsePlan DemuxPlan;  // name: what yu_rx_demux_variant_n returns
DemuxPlan plan_demux(uint64_t n, int cus, const Knobs &k);

// yu_rx_reply's kernel (k_reply, yucsum_reply.h) is the same mapping again, a lane
// per packet over the records, views, flags and endpoints those two calls stored, so
// it takes the same rule. The policy is that of those streams; the ep_echo table
// is always read with plain loads. The scan behind it is yu_rx_group's
// (yucsum_group.h): a block per tile of n + 1 outputs, nothing to plan.
typedef ParsePlan ReplyPlan;  // name: what yu_rx_reply_variant_n returns
ReplyPlan plan_reply(uint64_t n, int cus, const Knobs &k);

// yu_rx_group (yucsum_group.h): a stable radix partition of the packet numbers by
// endpoint, `passes` passes of a block histogram, a device-wide scan and a scatter,
// then the CSR and, with views, the grouped view table. Everything the launches
// need to agree on is here: the digit, the tile, the grids and where each region
// of the caller's workspace lies. Only lane_blocks depends on the CU count and the
// knobs (YU_BLOCKS_PER_CU), so yu_rx_group_workspace_bytes needs no device.
struct GroupPlan {
  uint32_t digit_bits;   // bits per pass digit, 1 .. 8
  uint32_t passes;       // 1 .. 4; 0 when the plan is refused (bytes == 0)
  uint32_t tile;         // packets per block of the pass kernels
  uint32_t blocks;       // blocks of the pass kernels: ceil(n / tile)
  uint32_t lane_blocks;  // grid of the lane-per-element kernels (grid-stride)
  // byte offsets into `work`, each 16-byte aligned; a region of 0 bytes is unused
  uint64_t hist_off, hist_bytes;        // pass histogram: uint32 [radix][blocks]
  uint64_t sums_off, sums_bytes;        // the scan's tile sums: uint64
  uint64_t count_off, count_bytes;      // passes > 1: m + 1 uint32 key counts
  uint64_t pair_off[2], pair_bytes[2];  // passes > 1 / > 2: n keys then n packet numbers, uint32
  uint64_t bytes;                       // yu_rx_group_workspace_bytes(n, m)
  const char *name;                     // what yu_rx_group_variant_n returns
};
GroupPlan plan_group(uint64_t n, uint64_t m, int cus, const Knobs &k);

}  // namespace yu
#pragma GCC visibility pop

#endif  // YUCSUM_PLAN_H
