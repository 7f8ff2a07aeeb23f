// yucsum_hostgeom.h — the geometry of the host path (yucsum_host.cpp) and its
// field writer: where a host batch is cut into slices, which batches go direct,
// how a _multi call is cut into shards, and which bytes of a packet in host
// memory take a TX result. No HIP call is made here: yucsum_host.cpp and
// tests/cpp/host_geom.cpp (a plain C++ program) both use these functions.
//
// Slices. A host batch crosses PCIe in slices of whole, consecutive packets.
// A slice holds at most `pkts` packets and, unless it is one packet, at most
// `bytes` bytes of packet memory:
//   ragged, views: packets are taken in order while the count is below `pkts`
//     and the next one still fits in `bytes`; the first packet of a slice is
//     always taken, so a packet longer than `bytes` is a slice of its own.
//     Empty packets count as packets and add no bytes.
//   uniform: every slice but the last holds the same count,
//     min(n, pkts, max(1, bytes / max(stride, 1))), and spans
//     (count - 1) * stride + len bytes, the gap after the last packet left out
//     (so with stride < len a slice's span may pass `bytes` by less than len).
// The limits are YU_HOST_SLICE_BYTES and YU_HOST_SLICE_PACKETS of
// include/yucsum.h; the measurement knobs of the same names lower them
// (slice_knob) for cutting only.
//
// Route. A batch that is one slice of at most direct_max bytes is a burst: the
// kernel reads it in place (or from one staging slot) through a burst context
// of 1 slot; every other batch takes the copies through a bulk context of 3.
//
// Shards. A _multi call gives device i of ndev the packets [b[i], b[i+1]):
// uniform and view batches b[i] = floor(n * i / ndev); ragged batches the first
// packet boundary whose offset is at or above offsets[0] + floor(total * i /
// ndev), never below b[i-1]. b[0] = 0 and b[ndev] = n.
#ifndef YUCSUM_HOSTGEOM_H
#define YUCSUM_HOSTGEOM_H

#include <stdint.h>
#include <stdlib.h>

#include <algorithm>
#include <vector>

#include "yucsum.h"
#include "yucsum_proto.h"

namespace yu {
namespace hostgeom {

struct SliceLimits {
  uint64_t bytes, pkts;
};

// A slice-limit knob's value: a number in [1, compiled]; anything else (unset,
// not a number, 0, above the compiled constant) leaves the constant.
inline uint64_t slice_knob(const char *v, uint64_t compiled) {
  if (!v || !*v) return compiled;
  char *end = nullptr;
  const unsigned long long k = strtoull(v, &end, 10);
  if (*end || k < 1 || k > compiled) return compiled;
  return (uint64_t)k;
}

// Packets per slice of a uniform batch.
inline uint64_t uniform_slice(uint64_t stride, uint64_t n, const SliceLimits &lim) {
  const uint64_t pstride = stride ? stride : 1;
  uint64_t slice = lim.bytes / pstride;
  if (slice > lim.pkts) slice = lim.pkts;
  if (slice < 1) slice = 1;
  if (slice > n) slice = n;
  return slice;
}
inline uint64_t uniform_count(uint64_t n, uint64_t slice, uint64_t first) {
  return n - first < slice ? n - first : slice;
}
inline uint64_t uniform_bytes(uint64_t stride, uint32_t len, uint64_t cnt) {
  return (cnt - 1) * stride + len;
}

// Slices of whole packets, each up to lim.bytes (a longer packet is a
// slice of its own); `span(i)` = bytes of packet i.
template <class Span>
uint64_t byte_slice(uint64_t first, uint64_t n, const Span &span, const SliceLimits &lim) {
  uint64_t cnt = 0, b = 0;
  while (first + cnt < n && cnt < lim.pkts) {
    const uint64_t l = span(first + cnt);
    if (cnt && b + l > lim.bytes) break;
    b += l;
    ++cnt;
  }
  return cnt;
}

inline uint64_t ragged_count(const uint64_t *off, uint64_t n, uint64_t first, const SliceLimits &lim) {
  return byte_slice(first, n, [&](uint64_t i) { return off[i + 1] - off[i]; }, lim);
}
inline uint64_t ragged_bytes(const uint64_t *off, uint64_t first, uint64_t cnt) {
  return off[first + cnt] - off[first];
}

inline uint64_t iov_plen(const yu_iovec *iov, const uint64_t *first_iov, uint64_t i) {
  uint64_t l = 0;
  for (uint64_t v = first_iov[i]; v < first_iov[i + 1]; ++v) l += iov[v].len;
  return l;
}
inline uint64_t iov_count(const yu_iovec *iov, const uint64_t *first_iov, uint64_t n, uint64_t first,
                          const SliceLimits &lim) {
  return byte_slice(first, n, [&](uint64_t i) { return iov_plen(iov, first_iov, i); }, lim);
}
inline uint64_t iov_bytes(const yu_iovec *iov, const uint64_t *first_iov, uint64_t first, uint64_t cnt) {
  uint64_t b = 0;
  for (uint64_t i = first; i < first + cnt; ++i) b += iov_plen(iov, first_iov, i);
  return b;
}

// The burst predicate: the batch's largest slice is the whole batch (max_pk
// packets of n, max_b bytes) and small enough to be read over PCIe in place.
inline bool is_burst(uint64_t max_pk, uint64_t n, uint64_t max_b, uint64_t direct_max) {
  return max_pk == n && max_b <= direct_max;
}

// Even packet counts (uniform, iovec).
inline std::vector<uint64_t> even_bounds(uint64_t n, int ndev) {
  std::vector<uint64_t> b(ndev + 1);
  for (int i = 0; i <= ndev; ++i) b[i] = (uint64_t)((unsigned __int128)n * i / ndev);
  return b;
}

// Packet boundaries closest below an even split of the bytes (ragged), as
// yustack_amd/shard.py does for the device-resident bench.
inline std::vector<uint64_t> byte_bounds(const uint64_t *off, uint64_t n, int ndev) {
  std::vector<uint64_t> b(ndev + 1);
  const uint64_t o0 = off[0], tot = off[n] - off[0];
  b[0] = 0;
  b[ndev] = n;
  for (int i = 1; i < ndev; ++i) {
    const uint64_t target = o0 + (uint64_t)((unsigned __int128)tot * i / ndev);
    uint64_t k = (uint64_t)(std::lower_bound(off, off + n + 1, target) - off);
    if (k > n) k = n;
    b[i] = std::max(k, b[i - 1]);
  }
  return b;
}

// ---------------------------------------------------------------------
// The field writer's rule. `at(i, k)` is byte k of packet i through a layout's
// accessor (nullptr past the packet). The same rule as the device writer
// decides when a field is stored: it must lie inside the packet (IPv4: inside
// min(len, IHL*4)).
// ---------------------------------------------------------------------
template <class At>
void put_field(const At &at, uint64_t i, uint32_t f, uint16_t v) {
  uint8_t *hi = at(i, f), *lo = at(i, f + 1);
  if (!hi || !lo) return;
  *hi = (uint8_t)(v >> 8);
  *lo = (uint8_t)v;
}

// TX_DATAGRAM: both fields of datagram i where the device defined them
// (include/yucsum.h): the contract 20 <= HeaderLength() <= TotalLength() <=
// len read from the bytes, the transport field when the protocol has one and
// the segment holds its header — the rule the kernels apply.
template <class At>
void put_datagram_fields(const At &at, uint64_t i, const uint16_t *res) {
  const uint8_t *b0 = at(i, 0), *b2 = at(i, 2), *b3 = at(i, 3), *b9 = at(i, 9);
  if (!at(i, 19)) return;  // shorter than 20 bytes
  const uint32_t hl = (uint32_t)(*b0 & 0xFu) * 4u, tl = (uint32_t)*b2 << 8 | *b3;
  if (hl < 20u || hl > tl || !at(i, tl - 1u)) return;
  put_field(at, i, 10, res[2 * i]);
  const uint32_t proto = *b9;
  const uint32_t fo = l4_field(proto);
  if (fo && tl - hl >= l4_min(proto)) put_field(at, i, hl + fo, res[2 * i + 1]);
}

// Packet i of a fill call in `mode`: its result(s) of `res` into its field(s).
template <class At>
void put_packet_fields(int mode, uint64_t i, const uint16_t *res, const At &at) {
  const uint32_t f = mode_field(mode);
  if (mode == YU_MODE_TX_DATAGRAM) {
    put_datagram_fields(at, i, res);
    return;
  }
  if (mode == YU_MODE_IPV4) {  // the field must lie inside the header
    const uint8_t *b0 = at(i, 0);
    if (!b0 || (uint32_t)(*b0 & 0xFu) * 4u < f + 2u) return;
  }
  put_field(at, i, f, res[i]);
}

// The three layouts' accessors.
struct UniformAt {
  uint8_t *h_data;
  uint64_t stride;
  uint32_t len;
  uint8_t *operator()(uint64_t i, uint32_t k) const { return k < len ? h_data + i * stride + k : nullptr; }
};
struct RaggedAt {
  uint8_t *h_data;
  const uint64_t *off;
  uint8_t *operator()(uint64_t i, uint32_t k) const {
    return k < off[i + 1] - off[i] ? h_data + off[i] + k : nullptr;
  }
};
// byte k of packet i: walk its views (the field may straddle two of them)
struct IovAt {
  const yu_iovec *iov;
  const uint64_t *first_iov;
  uint8_t *operator()(uint64_t i, uint32_t k) const {
    uint64_t at = k;
    for (uint64_t v = first_iov[i]; v < first_iov[i + 1]; ++v) {
      if (at < iov[v].len) return (uint8_t *)iov[v].base + at;
      at -= iov[v].len;
    }
    return nullptr;
  }
};

}  // namespace hostgeom
}  // namespace yu

#endif  // YUCSUM_HOSTGEOM_H
