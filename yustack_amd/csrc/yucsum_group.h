// yucsum_group.h — the arithmetic of yu_rx_group (include/yucsum.h): the packet
// numbers of a batch grouped by the endpoint yu_rx_demux chose for each, in
// arrival order inside a group, and the CSR of the groups. That is what the
// reference's deliverPacketLocked ends in, ep.HandlePacket appending the packet
// to the endpoint's queue (rcvList.PushBack, segmentQueue.enqueue), for a batch.
//
// Key: ep[i] when it is below m, else m ("no endpoint"), so keys are 0 .. m and
// have bitlen(m) bits. The grouping is a stable least-significant-digit radix
// partition of (key, packet number) on `passes` digits of `digit_bits` bits:
//   passes     = max(1, ceil(bitlen(m) / 8))
//   digit_bits = max(1, ceil(bitlen(m) / passes))
// one pass up to m = 255, two up to 65535, three below 2^24 and four at 2^24.
//
// One pass, three steps:
//   histogram  block b takes the packets [b * tile, (b + 1) * tile) and stores
//              its count of every digit at hist[digit * blocks + b]: digit-major,
//              so ONE exclusive scan over the array gives each block the place
//              where its packets of each digit start.
//   scan       the device-wide exclusive scan below, in place.
//   scatter    wave w of a block takes the w-th quarter of the tile and walks
//              it in steps of 64 consecutive packets, lane l the l-th: lane order
//              is packet order. place = scanned hist + the earlier waves' count
//              of the digit + the earlier steps' + the number of lower lanes of
//              this step with the digit. Every place is compared with n before
//              the store.
// The scan (group_scan_*) is three launches without any wait between blocks:
// per-tile sums, an exclusive scan of those sums by one block (thread t takes
// the t-th run of them), and the add-back. It also turns the key counts into
// `first` and the grouped view lengths into `q_offsets`.
//
// No HIP call is made here: the kernels, yu::plan_group and
// tests/cpp/rx_group.cpp all use these functions.
#ifndef YUCSUM_GROUP_H
#define YUCSUM_GROUP_H

#include <stdint.h>

#include "yucsum.h"
#include "yucsum_iov.h"

#pragma GCC visibility push(hidden)
namespace yu {

constexpr uint32_t kGroupMaxEndpoints = YU_DEMUX_MAX_ENDPOINTS;
constexpr uint32_t kGroupThreads = 256u;      // one block: four waves
constexpr uint32_t kGroupWaves = 4u;
constexpr uint32_t kGroupRadixMax = 256u;     // digits of at most 8 bits
constexpr uint32_t kGroupTile = 1024u;        // packets per block, up to kGroupMaxBlocks blocks: four steps per wave
constexpr uint32_t kGroupMaxBlocks = 8192u;   // beyond that the tile grows instead
constexpr uint32_t kGroupScanPer = 8u;        // consecutive elements per thread of a scan block
constexpr uint32_t kGroupScanTile = kGroupThreads * kGroupScanPer;

YU_IOV_FN uint32_t group_bitlen(uint64_t m) {
  uint32_t b = 0;
  while (m) {
    ++b;
    m >>= 1;
  }
  return b;
}
YU_IOV_FN uint32_t group_passes(uint64_t m) {
  const uint32_t b = group_bitlen(m);
  return b <= 8u ? 1u : (b + 7u) / 8u;
}
YU_IOV_FN uint32_t group_digit_bits(uint64_t m) {
  const uint32_t b = group_bitlen(m), p = group_passes(m);
  return b == 0u ? 1u : (b + p - 1u) / p;
}

// The key of a packet, and the digit a pass sorts by.
YU_IOV_FN uint32_t group_key(uint32_t ep, uint32_t m) { return ep < m ? ep : m; }
YU_IOV_FN uint32_t group_digit(uint32_t key, uint32_t pass, uint32_t digit_bits) {
  return (key >> (pass * digit_bits)) & ((1u << digit_bits) - 1u);
}

// Packets per block: a multiple of kGroupTile, so a wave's quarter is a whole
// number of 64-packet steps, and the least that leaves at most kGroupMaxBlocks blocks.
YU_IOV_FN uint32_t group_tile(uint64_t n) {
  const uint64_t span = (uint64_t)kGroupTile * kGroupMaxBlocks;
  const uint64_t k = n <= span ? 1u : (n + span - 1u) / span;
  return (uint32_t)(k * kGroupTile);
}
YU_IOV_FN uint32_t group_blocks(uint64_t n) {
  const uint64_t t = group_tile(n);
  return (uint32_t)((n + t - 1u) / t);
}
// What the workspace allots a histogram's blocks: at least group_blocks(n), and
// monotone in n, which group_blocks is not where the tile grows.
YU_IOV_FN uint32_t group_blocks_cap(uint64_t n) {
  const uint64_t b = (n + kGroupTile - 1u) / kGroupTile;
  return (uint32_t)(b < kGroupMaxBlocks ? b : kGroupMaxBlocks);
}

// Wave w's quarter of block b's tile: [begin, begin + tile / 4), cut to n by the
// lanes themselves.
YU_IOV_FN uint64_t group_wave_begin(uint32_t b, uint32_t w, uint32_t tile) {
  return (uint64_t)b * tile + (uint64_t)w * (tile / kGroupWaves);
}
YU_IOV_FN uint32_t group_wave_steps(uint32_t tile) { return tile / kGroupWaves / 64u; }

// Where block b's count of `digit` lies in a pass histogram.
YU_IOV_FN uint64_t group_hist_at(uint32_t digit, uint32_t b, uint32_t blocks) {
  return (uint64_t)digit * blocks + b;
}

// The scan: tiles of kGroupScanTile outputs, thread t of a tile's block takes the
// kGroupScanPer consecutive elements from tile * kGroupScanTile + t * kGroupScanPer.
// Inputs at and past n_in count as 0, so n_out = n_in + 1 also yields the total.
YU_IOV_FN uint64_t group_scan_tiles(uint64_t n_out) { return (n_out + kGroupScanTile - 1u) / kGroupScanTile; }
// The middle launch: thread t of its one block takes the sums [t * run, (t + 1) * run).
YU_IOV_FN uint64_t group_scan_run(uint64_t tiles) { return (tiles + kGroupThreads - 1u) / kGroupThreads; }

YU_IOV_FN uint64_t group_align16(uint64_t x) { return (x + 15u) & ~(uint64_t)15u; }

}  // namespace yu
#pragma GCC visibility pop

#endif  // YUCSUM_GROUP_H
