// yucsum_dense.h — k_small's dense fetch: when a uniform batch has no gaps
// (stride == len), the 64/G packets of a wave step are one contiguous byte
// range, and the wave asks memory for it as whole 128-byte lines: lane L's
// load u takes 16-byte chunk 64u + L of the range that starts at the line
// holding the step's first byte, so every line of a step is requested once,
// whole, by one instruction. The chunks are parked in the wave's LDS slice
// and each group reads its packet's window back from there.
//
// This header holds the predicate and the geometry only and makes no HIP
// call: the kernel and tests/cpp/dense_geom.cpp both use it.
#ifndef YUCSUM_DENSE_H
#define YUCSUM_DENSE_H

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define YU_DENSE_FN __host__ __device__ __forceinline__
#else
#define YU_DENSE_FN inline
#endif

#pragma GCC visibility push(hidden)
namespace yu {

constexpr uint32_t kDenseLine = 128u;   // bytes per memory line
constexpr uint32_t kDensePiece = 1024u; // bytes one load instruction covers (64 lanes x 16)
constexpr uint32_t kDenseOOB = 0x80000000u;  // == kOOB (yucsum_plan.h)

// The k_small instantiations that carry the dense path (and its LDS slice).
// <16,6> (dense 1025..1536-byte packets, config 3) is the measured one.
constexpr bool dense_inst(int G, int U) { return G == 16 && U == 6; }

// Whether a batch takes the dense path on k_small<G, U>. `data` is the first
// packet's address. With 16-aligned data and len % 4 == 0 every packet starts
// 4-aligned (window base == packet start) and every 16-byte chunk of a step's
// range lies on a 16-byte boundary of the buffer, so a chunk is wholly inside
// or wholly outside the batch's first byte. The last condition keeps a step's
// range (up to 124 lead-in bytes, then 64/G packets) inside the U pieces.
YU_DENSE_FN bool dense_ok(int G, int U, uint64_t data, bool ragged, uint64_t stride, uint32_t len,
                          bool fill, bool ipv4) {
  return dense_inst(G, U) && !ragged && stride == len && !fill && !ipv4 && (data & 15u) == 0 &&
         len != 0 && (len & 3u) == 0 &&
         (uint64_t)(64 / G) * len + (kDenseLine - 4u) <= (uint64_t)kDensePiece * (uint32_t)U;
}

// One wave step: packets [pb, pb + gpw) of n. Offsets are relative to `base`.
struct DenseStep {
  uint64_t base;  // floor128(address of packet pb): the descriptor's base
  uint32_t lead;  // packet pb starts at base + lead
  uint32_t lo;    // chunks below lo begin before the batch's first byte: not loaded
  uint32_t hi;    // chunks at or past hi are not loaded
};

// hi: the end of the last line the step's packets touch, or, for the batch's
// last step, the batch's end (nothing is loaded for a packet >= n; the chunk
// holding the end is cut at ceil4(end) by the descriptor). pb >= n loads nothing.
YU_DENSE_FN DenseStep dense_step(uint64_t data, uint32_t len, uint64_t n, uint64_t pb,
                                 uint32_t gpw) {
  DenseStep s;
  const uint64_t start = data + pb * len;
  s.base = start & ~(uint64_t)(kDenseLine - 1u);
  s.lead = (uint32_t)(start - s.base);
  s.lo = data > s.base ? (uint32_t)(data - s.base) : 0u;
  s.hi = 0u;
  if (pb < n) {
    const uint64_t rem = n - pb;
    const uint32_t bytes = s.lead + (uint32_t)(rem < gpw ? rem : gpw) * len;
    s.hi = rem > gpw ? (bytes + kDenseLine - 1u) & ~(kDenseLine - 1u) : bytes;
  }
  return s;
}

// Lane `lane`'s load u is chunk 64u + lane of the range. Counted from lo, the
// chunk at x = dense_x0 + u * kDensePiece is loaded if x < dense_lim (a chunk
// below lo wraps to a large x), from buffer offset lo + x.
YU_DENSE_FN uint32_t dense_x0(const DenseStep &s, uint32_t lane) { return 16u * lane - s.lo; }
YU_DENSE_FN uint32_t dense_lim(const DenseStep &s) { return s.hi > s.lo ? s.hi - s.lo : 0u; }

// Buffer offset of lane `lane`'s load u, or out of range.
YU_DENSE_FN uint32_t dense_chunk(const DenseStep &s, uint32_t u, uint32_t lane) {
  const uint32_t x = dense_x0(s, lane) + u * kDensePiece;
  return x < dense_lim(s) ? s.lo + x : kDenseOOB;
}

// Where the window of group gw's packet pb + gw (base floor4(start) == start)
// begins in the wave's LDS slice, which mirrors the step's range from `base`
// on: the step's lead-in, then gw packets.
YU_DENSE_FN uint32_t dense_window(uint64_t data, uint32_t len, uint64_t pb, uint32_t gw) {
  return (((uint32_t)data + (uint32_t)pb * len) & (kDenseLine - 1u)) + gw * len;
}

// A group reads its whole 16*G*U-byte window, and the last group's may end past
// the 1 KiB * U slice (only in bytes past its packet, which the sum masks):
// bytes to pad the LDS array with so that the last wave's reads stay inside it.
constexpr uint32_t dense_pad(int G, int U) {
  const uint32_t gpw = 64u / (uint32_t)G, slice = kDensePiece * (uint32_t)U;
  const uint32_t lmax = ((slice - (kDenseLine - 4u)) / gpw) & ~3u;  // longest dense_ok packet
  const uint32_t reach = (kDenseLine - 4u) + (gpw - 1u) * lmax + 16u * (uint32_t)G * (uint32_t)U;
  return reach > slice ? (reach - slice + 15u) & ~15u : 0u;
}

}  // namespace yu
#pragma GCC visibility pop

#endif  // YUCSUM_DENSE_H
