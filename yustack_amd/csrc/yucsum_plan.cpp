// yucsum_plan.cpp — kernel selection and grid arithmetic (yucsum_plan.h). Every
// cut-over here was measured; the comments cite the logs.
#include "yucsum_plan.h"

#include <string.h>

#include "yucsum_internal.h"
#include "yucsum_iov.h"
#include "yucsum_group.h"  // after yucsum_internal.h, like yucsum_iov.h: YU_IOV_FN needs the HIP runtime's macros here

namespace yu {

constexpr KernelInfo kKernels[kKernelCount] = {
#define YU_X(id, name, family, window, G, ppw, run, grid, own_fill, fill_plain, tile, kind, \
             ragged_fill, targs)                                                           \
  {name, Family::family, window, G, ppw, run, Grid::grid, own_fill, fill_plain, tile,      \
   SegKind::kind, k_##ragged_fill},
    YU_KERNELS(YU_X)
#undef YU_X
};

namespace {

// The ids [begin, end) of a family (the list keeps each family together).
constexpr int family_begin(Family f) {
  int i = 0;
  while (i < kKernelCount && kKernels[i].family != f) ++i;
  return i;
}
constexpr int family_end(Family f) {
  int i = kKernelCount;
  while (i > 0 && kKernels[i - 1].family != f) --i;
  return i;
}

bool mode_is_ipv4(int m) { return m == YU_MODE_IPV4 || m == YU_MODE_VERIFY_IPV4; }

// The k_seg kind for a mode (not the IPv4 header-only modes).
KernelId seg_for(bool u8, int mode) {
  if (mode == YU_MODE_VERIFY_RX) return u8 ? k_seg8_rx : k_seg4_rx;
  if (mode == YU_MODE_TX_DATAGRAM) return k_seg8_dg;
  if (mode_is_tx(mode)) return u8 ? k_seg8_tx : k_seg4_tx;
  return u8 ? k_seg8 : k_seg4;
}

// Ragged kernel choice: the segmented stream sum with 8 KiB tiles, except for
// the IPv4 modes, which read only each packet's header (k_hdr, one lane per
// packet). 8 KiB tiles beat 4 KiB ones from ~800-byte packets up (config 4:
// 84.9 vs 83.4 % of peak, U{64..1500}: 80.5 vs 77.7 %) and lose below
// (U{40..200}: 54 vs 61-66 %). Measurement override YU_RAGGED=loop|seg4|seg16|seg8.
// Small bursts (n <= kSmallBurst, e.g. a tun read burst on the host path) go to
// k_loop instead: k_seg gives each 64-packet chunk to one wave, which streams
// the chunk's tiles one after another, so a burst of few chunks leaves the GPU
// idle and pays one memory latency per tile. One wave per packet instead
// (tools/kbench KB_N, profiles/r01/kbench_ragged_burst_size.log): 64 packets of
// U{64..1500} 8.6 -> 3.4 us, 1024 of them 10.7 -> 3.8, 2048 jumbo packets
// U{64..9000} 43.2 -> 5.7; at 4096 small packets U{40..200} the two tie (4.7);
// from 16384 packets on k_seg wins on small packets (5.4 vs 11.5). VERIFY_RX
// bursts take k_loop_rx, the same shape.
constexpr uint64_t kSmallBurst = 4096;
// the largest uniform stride k_seg's 32-bit kinds take: 63 strides plus a 65535-byte
// packet and its 3 head bytes stay under 2^31 bytes
constexpr uint64_t kSeg32Stride = ((1ull << 31) - 65535u - 3u) / 63u;
constexpr uint64_t kMidBatch = 65536;

KernelId pick_ragged(int mode, uint64_t n, const Knobs &k) {
  const bool f = k.ragged != Knobs::Ragged::Auto;
  const bool rx = mode == YU_MODE_VERIFY_RX;  // only k_seg verifies whole datagrams
  const bool dg = mode == YU_MODE_TX_DATAGRAM;  // and fills both fields of one
  const KernelId loop = rx ? k_loop_rx : (dg ? k_loop_dg : (mode == YU_MODE_RAW ? k_loop_be : k_loop_le));  // BE: exact past 131072 B
  const KernelId c16 = rx ? k_seg8_rx_c16 : (dg ? k_seg8_dg_c16 : (mode_is_tx(mode) ? k_seg8_tx_c16 : k_seg8_c16));
  if (k.ragged == Knobs::Ragged::Loop) return loop;
  if (mode_is_ipv4(mode)) return k_hdr;  // header-only: one lane per packet
  if (k.ragged == Knobs::Ragged::Seg16) return c16;
  if (n <= kSmallBurst && !f) return loop;
  // up to 64K packets: 16-packet chunks, 4x the waves (U{64..1500}: 8192
  // packets 11.2 -> 6.3 us, 32768 11.7 -> 8.7; U{40..200} 5.1 -> 4.4; jumbo
  // 44.2 -> 17.0; VERIFY_RX 13.3 -> 7.1); from 65536 on 64-packet chunks win
  // again (13.1 vs 14.7 us; profiles/r01/kbench_kseg_chunk16_sweep.log)
  if (n < kMidBatch && !f) return c16;
  return seg_for(k.ragged != Knobs::Ragged::Seg4, mode);
}

// Ragged in place: the TX kinds of k_seg take their TXW form (the whole-line
// write-back, 1M UDP datagrams U{40..200}: 67.5 -> 48.9 us, kbench 8, DESIGN.md
// §5.4) unless YU_FILL_WB=0, and 64-packet TX_DATAGRAM chunks their 40-packet
// form (the list in yucsum_plan.h). Ragged calls only: a uniform in-place batch
// that pick_uniform sends to k_seg keeps the read-only pick, whose TX and DG
// kinds store each field on its own.
KernelId pick_ragged_fill(int mode, uint64_t n, bool fill, const Knobs &k) {
  const KernelId v = pick_ragged(mode, n, k);
  if (!fill) return v;
  const KernelId w = kKernels[v].ragged_fill;
  return kKernels[w].kind == SegKind::TxW && !k.fill_wb ? v : w;
}

// Tuning override (measurement only): YU_VARIANT=<name> forces a k_small
// variant whenever it covers the shape.
KernelId pick_uniform(uint64_t base, uint64_t stride, uint32_t len, uint64_t n, int mode,
                      const Knobs &k) {
  const uint64_t need = mode_is_ipv4(mode) ? (len < 60u ? len : 60u) : len;
  // the window starts at floor4(start): up to 3 extra bytes in front
  const bool aligned4 = ((base | (n > 1 ? stride : 0)) & 3u) == 0;
  const uint64_t span = need + (aligned4 ? 0 : 3);
  // lane window offsets are 32-bit: (64/G - 1) strides + the window
  auto fits = [&](const KernelInfo &v) {
    return span <= v.window && v.ppw * stride + v.window < kOOB;
  };
  // k_tiny: no junk bytes (4-aligned starts, no TX field, no IPv4 header walk)
  const bool tiny_ok = aligned4 && !mode_is_ipv4(mode) && mode != YU_MODE_VERIFY_RX &&
                       mode != YU_MODE_TX_DATAGRAM;
  // k_lane: the same modes, one wave step = 64 whole strides in LDS, so only
  // where gaps between packets waste at most half the bytes it loads
  auto lane_fits = [&](const KernelInfo &v) {
    return tiny_ok && (stride & 3u) == 0 && len >= 1u && len <= stride && stride <= v.window &&
           2u * stride <= 3u * (uint64_t)len;
  };
  constexpr int lane0 = family_begin(Family::Lane), lane1 = family_end(Family::Lane);
  constexpr int tiny0 = family_begin(Family::Tiny), tiny1 = family_end(Family::Tiny);
  constexpr int small0 = family_begin(Family::Small), small1 = family_end(Family::Small);
  if (mode == YU_MODE_VERIFY_RX || mode == YU_MODE_TX_DATAGRAM) {
    // k_seg's RX / DG kinds keep positions in 32 bits: a 64-packet chunk must
    // span less than 2 GiB, so sparser uniform batches take a wave per datagram
    if (n > 1 && stride > kSeg32Stride) return mode == YU_MODE_VERIFY_RX ? k_loop_rx : k_loop_dg;
    return pick_ragged(mode, n, k);
  }
  // IPv4 header-only modes: one lane per packet (1M x 1500-B datagrams:
  // 29.9 us vs 36.9 with k_small<4,1>, kbench 13)
  if (mode_is_ipv4(mode) && !k.forced) return k_hdr;
  if (k.forced) {
    if (!mode_is_ipv4(mode) && k.forced_seg && (n < 2 || stride <= kSeg32Stride))
      return seg_for(k.forced_seg == 8, mode);
    if (k.forced_kernel >= 0) {
      const KernelId id = (KernelId)k.forced_kernel;
      const KernelInfo &v = kKernels[id];
      if (v.family == Family::Hdr ? mode_is_ipv4(mode)
          : v.family == Family::Small ? fits(v)
          : v.family == Family::Tiny  ? tiny_ok && fits(v)
                                      : lane_fits(v))
        return id;
    }
  }
  // k_lane up to 112 bytes (72-byte UDP datagrams: 16.4 vs 20.0 us with
  // k_tiny<8>; 64-byte packets, config 2: 14.2 vs 14.8 with k_tiny<4>),
  // k_tiny<8> above, where all its lanes load (128 bytes: 23.6 vs 24.6 us;
  // tools/kbench 2 and 14); k_tiny<4> for sparse small packets
  if (len <= 112u)
    for (int i = lane0; i < lane1; ++i)
      if (lane_fits(kKernels[i])) return (KernelId)i;
  if (tiny_ok)
    for (int i = tiny0; i < tiny1; ++i)
      if (fits(kKernels[i])) return (KernelId)i;
  // Dense packets up to 704 bytes that k_lane / k_tiny do not take (129..704
  // bytes, or not 4-aligned): the segmented stream sum beats per-packet lane
  // groups, whose loads scatter over partly used windows (160 B: 34.6 vs 50.0 us;
  // 320: 58-66 vs 88-89; 512: 87 vs 103; 704: 116 vs 120; unaligned 66 B: 26.8
  // vs 38.6; from 768 on k_small is as fast or faster; tools/kbench 14,
  // profiles/r01/kbench_uniform_size_sweep.log)
  // (k_seg gives one wave to 64 packets: only batches of 64K packets or more
  // have enough of them to fill the GPU; smaller ones keep the per-packet shapes)
  const bool dense = 2u * stride <= 3u * (uint64_t)len && n >= kMidBatch;
  if (len <= 704u && dense) return seg_for(len >= 448u, mode);
  // and above 3 KiB, where it streams 8 KiB tiles past k_small<64,4> and the
  // one-wave-per-packet k_loop (4096 B: 636 vs 664 us; 9000 B: 1373 vs 1464;
  // 16 KiB: 0.88 vs 0.81 of peak) — given enough 64-packet chunks to fill the
  // GPU (one wave each); a few huge packets keep k_loop's wave per packet
  if (len > 3072u && dense) return seg_for(true, mode);
  for (int i = small0; i < small1; ++i)
    if (fits(kKernels[i])) return (KernelId)i;
  return len > kLEMax ? k_loop_be : k_loop_le;
}

// Grid size in 256-thread blocks per CU. The grid is deliberately larger than
// what is resident at once (5-8 blocks/CU): finished blocks are replaced by
// fresh ones, which evens out the per-CU tail. Measured optimum on MI355X
// (tools/kbench, round 1): 64 for MTU-size and larger packets, 16 for the
// small-packet lane-group variants (G < 16). The 64-packet-step kernels
// (k_lane, k_tiny: Grid::B6) run best on 6 (round 2, each wave then streams
// about 4 steps with the next in flight): 1M x 64 B 14.2 -> 13.4 us, 72 B 16.0
// -> 14.8, 32 B 10.4 -> 8.4, 100 B 21.7 -> 20.8, 124 B 25.0 -> 23.8
// (profiles/r02/kbench_ab_lane_grid.log).
// Uniform batches on 4 KiB k_seg tiles (dense 129..447-byte packets, Grid::B10U)
// run on 10: each wave then streams 2-3 chunks with the next tile in flight
// instead of one chunk per wave (1M UDP datagrams, medians of 6 launches of
// 30: 136 B 33.0 -> 30.5 us, 160 B 34.5 -> 32.9, 256 B 50.2 -> 47.8, 320 B
// 58.8 -> 56.9, 384 B 70.3 -> 66.7, 200 and 420 B within 1 %;
// profiles/r02/kbench_grid_mid_uniform_{a,b}.log).
uint32_t blocks_per_cu(Grid g, bool ragged, const Knobs &k) {
  if (k.blocks_per_cu) return k.blocks_per_cu;
  switch (g) {
    case Grid::B10U: return ragged ? 64 : 10;
    case Grid::B6: return 6;
    case Grid::B16: return 16;
    default: return 64;
  }
}

int knob_int(const char *s, int lo, int hi, int dflt) {
  if (!s || !*s) return dflt;
  const int x = atoi(s);
  return (x >= lo && x <= hi) ? x : dflt;
}

}  // namespace

Knobs read_knobs(const char *(*get)(const char *name)) {
  Knobs k;
  if (const char *f = get("YU_RAGGED"))
    k.ragged = strcmp(f, "loop") == 0    ? Knobs::Ragged::Loop
               : strcmp(f, "seg4") == 0  ? Knobs::Ragged::Seg4
               : strcmp(f, "seg16") == 0 ? Knobs::Ragged::Seg16
                                         : Knobs::Ragged::Seg8;
  if (const char *f = get("YU_VARIANT")) {
    k.forced = true;
    if (strncmp(f, "k_seg<", 6) == 0) k.forced_seg = f[6] == '8' ? 8 : 4;
    for (int i = 0; i < kKernelCount; ++i) {
      const Family fam = kKernels[i].family;
      if (fam != Family::Loop && fam != Family::Seg && strcmp(kKernels[i].name, f) == 0)
        k.forced_kernel = (int16_t)i;
    }
  }
  k.nt = (int8_t)knob_int(get("YU_NT"), 0, 2, -1);
  // The ragged in-place writer of k_seg's TX kind (wbk): 0 = one 2-byte store per
  // field; 1 = the fields patched into the parked tile and their 128-byte lines
  // stored whole. YU_FILL_WB overrides.
  k.fill_wb = knob_int(get("YU_FILL_WB"), 0, 1, 1) != 0;
  k.runs = (uint8_t)knob_int(get("YU_RUNS"), 0, 2, 1);
  k.blocks_per_cu = (uint16_t)knob_int(get("YU_BLOCKS_PER_CU"), 1, 1024, 0);
  // YU_SEG_SMALL_BLOCKS: blocks per CU that work on a small-packet ragged
  // batch (seg_waves); 0 = the whole grid.
  k.seg_small_blocks = (uint8_t)knob_int(get("YU_SEG_SMALL_BLOCKS"), 0, 64, 3);
  // YU_XCD: 1 = XCD-aware block order (grid_wave), 0 (default) = plain blockIdx.
  // Measured (round 1, tools/ab.sh): no gain on any config — these kernels
  // share at most one line between neighbouring blocks, and the Infinity Cache
  // already absorbs its second fetch — and -1..3 % on configs 2/3, so it is off.
  k.xcd = knob_int(get("YU_XCD"), 0, 1, 0) != 0;
  // YU_STREAM=walk: k_stream without its plain runs, one general step per queue entry.
  if (const char *f = get("YU_STREAM")) k.stream_walk = strcmp(f, "walk") == 0;
  return k;
}

// Tuning knobs (read once, measurement only, and only under YU_TUNING=1:
// yu::tuning_env).
const Knobs &env_knobs() {
  static const Knobs k = read_knobs(tuning_env);
  return k;
}

Plan plan(const Shape &s, int cus, const Knobs &k) {
  const KernelId id = s.ragged ? pick_ragged_fill(s.mode, s.n, s.fill, k)
                               : pick_uniform(s.align, s.stride, s.len, s.n, s.mode, k);
  const KernelInfo &v = kKernels[id];
  Plan p;
  p.kernel = id;
  p.name = v.name;
  // k_small: runs from 8 runs per CU up (1500-B packets, runs vs interleaved:
  // 16384 packets 8.0 vs 7.2 us, 32768 11.3 vs 12.5, 131072 35.3 vs 38.8; 768-B
  // packets 6.6 vs 5.0, 7.5 vs 8.2, 19.7 vs 22.0; kbench_ab_k_small_runs.log)
  // (YU_RUNS: 0 never, 2 whenever not filling — measurement only)
  const bool runs = v.run && !s.fill &&
                    (k.runs == 2 || (k.runs == 1 && s.n / v.run >= 8u * (uint64_t)cus));
  p.form = v.run ? (runs ? Form::Runs : Form::Inter) : (s.fill && v.own_fill ? Form::Fill : Form::Plain);
  // Load policy: the hybrid one (2, see bld16). k_small writing the field in
  // place loads plainly unless YU_NT says otherwise: the
  // field's line is then more often still cached when the 2-byte store reaches it
  // (config 9: 320.9 -> 312.2 us on one box, 326.2 -> 321.2 on another; all-nt 330.2;
  // k_lane's 72-byte writer gains nothing, 29.9 vs 30.8; profiles/r03/kbench_ab_fill_nt.log)
  p.policy = (uint8_t)(k.nt >= 0 ? k.nt : (s.fill && v.fill_plain ? 0 : 2));
  p.ppw = runs ? v.run : v.ppw;
  const uint64_t waves_per_block = 4;
  const uint64_t cap = (uint64_t)cus * blocks_per_cu(v.grid, s.ragged, k);
  const uint64_t waves = (s.n + p.ppw - 1) / p.ppw;
  uint64_t blocks = (waves + waves_per_block - 1) / waves_per_block;
  if (blocks > cap) blocks = cap;
  if (blocks < 1) blocks = 1;
  p.blocks = (uint32_t)blocks;
  p.uf = 0;
  if (!s.ragged) {
    if (v.family == Family::Lane || v.family == Family::Tiny)
      p.uf = s.len >= 16u * v.G ? 1u : 0u;  // k_tiny: all chunks whole?
    else if (v.family == Family::Small)
      p.uf = mode_is_ipv4(s.mode) ? 0u : s.len / (16u * v.G);
  }
  p.xcd = k.xcd;
  p.small_waves = (uint32_t)cus * 4u * k.seg_small_blocks;
  return p;
}

// The wave-per-packet kernels: a wave per packet, four per block, on the over-
// subscribed grid of the other wave-per-packet kernels (64 blocks per CU,
// YU_BLOCKS_PER_CU overrides); the load policy is YU_NT's, else slot 2 (k_pack's
// source side is k_iov's, and k_build and k_split read each packet once). `mode` picks the
// kind: the whole-packet sums share one kernel, the modes that parse an IPv4 header
// out of the packet (IPV4, VERIFY_IPV4, VERIFY_RX, TX_DATAGRAM) take the dg one;
// the grid is the same.
WavePlan plan_wave(WaveFamily family, uint64_t n, int mode, bool fill, int cus, const Knobs &k) {
  struct Row {
    const char *name;
    WaveFamily family;
    bool dg, fill;
  };
  static constexpr Row rows[kWaveKernelCount] = {
#define YU_X(id, name, family, dg, fill, targs) {name, WaveFamily::family, dg, fill},
      YU_WAVE_KERNELS(YU_X)
#undef YU_X
  };
  const bool single = family == WaveFamily::Build || family == WaveFamily::Split;  // one kernel: no kinds
  const bool dg = !single && iov_dg_mode_ok(mode);
  fill = fill && !single;
  int id = 0;  // every (family, dg, fill) a call can ask for has its row
  while (rows[id].family != family || rows[id].dg != dg || rows[id].fill != fill) ++id;
  WavePlan p;
  p.kernel = (WaveKernel)id;
  p.name = rows[id].name;
  p.policy = (uint8_t)(k.nt >= 0 ? k.nt : 2);
  const uint64_t cap = (uint64_t)cus * (k.blocks_per_cu ? k.blocks_per_cu : 64u);
  uint64_t blocks = (n + 3) / 4;  // 4 waves per block, a wave per packet
  if (blocks > cap) blocks = cap;
  if (blocks < 1) blocks = 1;
  p.blocks = (uint32_t)blocks;
  return p;
}

// The lane-per-packet kernels (k_parse, k_demux): a wave step takes 64 packets
// and a block 256. The grid is 8 blocks per CU, every wave slot of a SIMD (these
// kernels are bound by the latency of scattered loads, not by arithmetic), and
// larger batches stride over it; YU_BLOCKS_PER_CU overrides. Plain loads of the
// packet stream unless YU_NT is 1.
static ParsePlan plan_lane_per_packet(const char *name, uint64_t n, int cus, const Knobs &k) {
  ParsePlan p;
  p.name = name;
  p.policy = (uint8_t)(k.nt == 1 ? 1 : 0);
  const uint64_t cap = (uint64_t)cus * (k.blocks_per_cu ? k.blocks_per_cu : 8u);
  uint64_t blocks = (n + 255) / 256;
  if (blocks > cap) blocks = cap;
  if (blocks < 1) blocks = 1;
  p.blocks = (uint32_t)blocks;
  return p;
}

// k_parse: the scattered loads are the packets' headers. Plain by default because a
// small packet shares its 128-byte line with its neighbours, which other lanes of
// the same step read (k_hdr's finding for scattered header reads).
ParsePlan plan_parse(uint64_t n, int cus, const Knobs &k) { return plan_lane_per_packet("k_parse", n, cus, k); }

// k_demux: the scattered loads are the table probes, always plain (the table is what
// is reused); the policy is that of the record stream (yucsum_plan.h).
DemuxPlan plan_demux(uint64_t n, int cus, const Knobs &k) { return plan_lane_per_packet("k_demux", n, cus, k); }

// k_reply: every load but the ep_echo byte is a stream read once, lane after lane.
ReplyPlan plan_reply(uint64_t n, int cus, const Knobs &k) { return plan_lane_per_packet("k_reply", n, cus, k); }

// yu_rx_group: the digit and the pass count follow from m alone (keys are 0 .. m),
// the tile and the pass kernels' grid from n alone (yucsum_group.h), so the
// workspace layout is the same on every device. Regions in the order hist, sums,
// count, pair[0], pair[1], each rounded up to 16 bytes. The histogram is allotted
// group_blocks_cap(n) blocks, not group_blocks(n): the latter drops where the tile
// grows, and the workspace must not shrink as n grows. The tile sums serve the
// longest scan of the call: a pass histogram, the m + 2 entries of `first`, or the
// n + 1 of q_offsets. The lane-per-element kernels (the view gather, `first` from
// the histogram) take plan_parse's grid rule.
GroupPlan plan_group(uint64_t n, uint64_t m, int cus, const Knobs &k) {
  static const char *const names[4] = {"k_group<1>", "k_group<2>", "k_group<3>", "k_group<4>"};
  GroupPlan p = {};
  p.name = "none";
  if (m > kGroupMaxEndpoints || n >= (1ull << 32)) return p;
  p.passes = group_passes(m);
  p.digit_bits = group_digit_bits(m);
  p.name = names[p.passes - 1];
  p.tile = group_tile(n);
  p.blocks = group_blocks(n);
  p.lane_blocks = plan_lane_per_packet(p.name, n > m + 2 ? n : m + 2, cus, k).blocks;
  const uint64_t hist = ((uint64_t)1 << p.digit_bits) * group_blocks_cap(n);
  uint64_t longest = hist > m + 2 ? hist : m + 2;
  if (n + 1 > longest) longest = n + 1;
  p.hist_bytes = group_align16(4u * hist);
  p.sums_bytes = group_align16(8u * group_scan_tiles(longest));
  p.count_bytes = p.passes > 1 ? group_align16(4u * (m + 1)) : 0u;
  p.pair_bytes[0] = p.passes > 1 ? group_align16(8u * n) : 0u;
  p.pair_bytes[1] = p.passes > 2 ? group_align16(8u * n) : 0u;
  p.hist_off = 0;
  p.sums_off = p.hist_off + p.hist_bytes;
  p.count_off = p.sums_off + p.sums_bytes;
  p.pair_off[0] = p.count_off + p.count_bytes;
  p.pair_off[1] = p.pair_off[0] + p.pair_bytes[0];
  p.bytes = p.pair_off[1] + p.pair_bytes[1];
  return p;
}

}  // namespace yu
