// yucsum_demux.h — the arithmetic of k_demux, the kernel of yu_rx_demux
// (include/yucsum.h), and of yu_demux_table_fill, which builds its table:
// transport demultiplexing, the step after Nic.DeliverTransportPacket has read
// the ports. A registered endpoint is a TransportEndpointId plus its protocol
// (yu_endpoint_id); a received packet's record (yu_tx_record, as
// yu_rx_parse_ragged stores it) is looked up three times in the fixed order of
// deliverPacketLocked: all four fields, then the remote part emptied, then the
// local address emptied as well. The first hit is the packet's endpoint.
//
// The table is open-addressed with linear probing. `slots` is a power of two, at
// least 16 and at least twice the number of ids, so half the slots are empty and
// every probe chain of a filled table ends. A slot is four dwords, 16-byte
// aligned, so a probe is one 16-byte load:
//   {local address, remote address, local_port | remote_port << 16, tag}
//   tag = index << 8 | kind << 4 | (proto == 17 ? 2 : 1); tag == 0: empty.
// Addresses are the four wire bytes read as one little-endian dword, which is
// what a dword load of a record or of an id gives. The low byte of the tag is
// the `code`: it keeps the three kinds and the two protocols apart, so a
// connection from 0.0.0.0:0 and a listener never match each other's key.
//
// One packet, one lane: the lane builds the three keys from record dwords 0 .. 2
// and the protocol byte, and walks one probe chain per key (demux_lookup), at
// most `slots` probes each, every probe at 16 * (index & (slots - 1)), inside
// the table whatever the table holds. An index read from a slot is clamped to
// the number of ids (demux_clamp), so the counter it selects exists.
//
// No HIP call is made here: the kernel, the fill and tests/cpp/rx_demux.cpp all
// use these functions.
#ifndef YUCSUM_DEMUX_H
#define YUCSUM_DEMUX_H

#include <stdint.h>
#include <string.h>

#include <new>

#include "yucsum.h"
#include "yucsum_iov.h"

#pragma GCC visibility push(hidden)
namespace yu {

constexpr uint32_t kDemuxNone = YU_DEMUX_NONE;
constexpr uint32_t kDemuxMax = YU_DEMUX_MAX_ENDPOINTS;
constexpr uint32_t kDemuxSlotBytes = 16u;
constexpr uint32_t kDemuxMinSlots = 16u;
constexpr uint32_t kDemuxPerWave = 64u;  // packets per wave step, one per lane
constexpr uint32_t kDemuxSplit = 16u;    // YU_RX_SPLIT: the record is defined

// Slots of a table of m ids, m <= kDemuxMax: the power of two that is at least
// 16 and at least 2m (at most 2^25).
YU_IOV_FN uint32_t demux_slots(uint64_t m) {
  uint32_t s = kDemuxMinSlots;
  while ((uint64_t)s < 2u * m) s <<= 1;
  return s;
}
YU_IOV_FN uint64_t demux_table_bytes(uint64_t m) {
  return m > kDemuxMax ? 0ull : (uint64_t)demux_slots(m) * kDemuxSlotBytes;
}

// The low byte of a tag; never zero.
YU_IOV_FN uint32_t demux_code(uint32_t kind, uint32_t proto) { return kind << 4 | (proto == 17u ? 2u : 1u); }
YU_IOV_FN uint32_t demux_tag(uint32_t index, uint32_t code) { return index << 8 | code; }

// The three words and the code a lookup compares.
struct DemuxKey {
  uint32_t local, remote, ports, code;
};

// murmur3's 32-bit finaliser.
YU_IOV_FN uint32_t demux_fmix(uint32_t h) {
  h ^= h >> 16;
  h *= 0x85EBCA6Bu;
  h ^= h >> 13;
  h *= 0xC2B2AE35u;
  h ^= h >> 16;
  return h;
}
// The hash of a key: the finaliser word by word, the code last. The home slot
// is demux_hash & (slots - 1).
YU_IOV_FN uint32_t demux_hash(const DemuxKey &k) {
  uint32_t h = demux_fmix(k.local + 0x9E3779B9u);
  h = demux_fmix(h ^ k.remote);
  h = demux_fmix(h ^ k.ports);
  return demux_fmix(h ^ k.code);
}

// The key of a registered id: its fields as they stand. An id the table takes
// (demux_id_ok) has the fields its kind empties zero, which is what demux_rec_key
// puts there on the packet's side.
YU_IOV_FN DemuxKey demux_id_key(const yu_endpoint_id &id) {
  uint32_t la, ra;
  memcpy(&la, id.local_addr, 4);
  memcpy(&ra, id.remote_addr, 4);
  return {la, ra, (uint32_t)id.local_port | (uint32_t)id.remote_port << 16, demux_code(id.kind, id.proto)};
}

// Is an id one the table takes? proto 6 or 17, kind 0 .. 2, what its kind
// empties zero, reserved zero.
YU_IOV_FN bool demux_id_ok(const yu_endpoint_id &id) {
  if (id.proto != 6u && id.proto != 17u) return false;
  if (id.kind > 2u || id.reserved != 0u) return false;
  const DemuxKey k = demux_id_key(id);
  if (id.kind >= 1u && (k.remote != 0u || id.remote_port != 0u)) return false;
  if (id.kind == 2u && k.local != 0u) return false;
  return true;
}

// Packet side. w0, w1, w2: record dwords 0 .. 2 (src, dst, sport | dport << 16);
// proto: the record's protocol byte. On receive dst is local: the id is
// {LocalPort: dport, LocalAddress: dst, RemotePort: sport, RemoteAddress: src}.
YU_IOV_FN uint32_t demux_rec_proto(uint32_t w6) { return w6 & 0xFFu; }
YU_IOV_FN DemuxKey demux_rec_key(uint32_t kind, uint32_t w0, uint32_t w1, uint32_t w2, uint32_t proto) {
  const uint32_t dport = w2 >> 16, sport = w2 & 0xFFFFu;
  return {kind == 2u ? 0u : w1, kind == 0u ? w0 : 0u, kind == 0u ? dport | sport << 16 : dport,
          demux_code(kind, proto)};
}

// Does the packet reach the demultiplexer? DeliverTransportPacket finds a
// transport protocol for TCP and UDP only; with a flags array, every bit of
// need | YU_RX_SPLIT must be set.
YU_IOV_FN bool demux_eligible(uint32_t proto, bool have_flags, uint32_t flags, uint32_t need) {
  const uint32_t want = (need | kDemuxSplit) & 0xFFFFu;
  return (proto == 6u || proto == 17u) && (!have_flags || (flags & want) == want);
}

// One slot as loaded.
struct DemuxSlot {
  uint32_t local, remote, ports, tag;
};
YU_IOV_FN bool demux_match(const DemuxSlot &s, const DemuxKey &k) {
  return s.local == k.local && s.remote == k.remote && s.ports == k.ports && (s.tag & 0xFFu) == k.code;
}
YU_IOV_FN bool demux_empty(const DemuxSlot &s) { return s.tag == 0u; }
YU_IOV_FN uint32_t demux_next(uint32_t i, uint32_t slots) { return (i + 1u) & (slots - 1u); }
// An index as a result: one the table's ids do not have is no endpoint.
YU_IOV_FN uint32_t demux_clamp(uint32_t index, uint32_t m) { return index < m ? index : kDemuxNone; }

// One lookup. ld(i), i < slots, loads slot i (the 16 bytes at 16 * i). The chain
// starts at the home slot and ends at a match, at an empty slot, or after
// `slots` probes (a table without an empty slot). Returns the slot's index
// field, or kDemuxNone.
template <typename Ld>
YU_IOV_FN uint32_t demux_lookup(Ld &ld, uint32_t slots, const DemuxKey &k) {
  uint32_t i = demux_hash(k) & (slots - 1u);
  for (uint32_t t = 0; t < slots; ++t) {
    const DemuxSlot s = ld(i);
    if (demux_match(s, k)) return s.tag >> 8;
    if (demux_empty(s)) return kDemuxNone;
    i = demux_next(i, slots);
  }
  return kDemuxNone;
}

// deliverPacketLocked for one eligible packet: the three lookups in order, the
// first hit clamped to m.
template <typename Ld>
YU_IOV_FN uint32_t demux_deliver(Ld &ld, uint32_t slots, uint32_t m, uint32_t w0, uint32_t w1, uint32_t w2,
                                 uint32_t proto) {
  for (uint32_t kind = 0; kind < 3u; ++kind) {
    const uint32_t e = demux_lookup(ld, slots, demux_rec_key(kind, w0, w1, w2, proto));
    if (e != kDemuxNone) return demux_clamp(e, m);
  }
  return kDemuxNone;
}

// The counter a result adds to: ep_count[e], or ep_count[m] for no endpoint.
YU_IOV_FN uint32_t demux_counter(uint32_t e, uint32_t m) { return e == kDemuxNone ? m : e; }

// yu_demux_table_fill without its argument checks: the table of ids[0, m) into
// `table` (demux_table_bytes(m) bytes). Returns m when every id went in, else
// the index of the first id that is malformed or equals an earlier one (the
// reference's ErrPortInUse), and then `table` is not written: the slots are
// built in a block of their own and copied at the end. Returns m + 1 when that
// block cannot be allocated. Host only.
inline uint64_t demux_fill(const yu_endpoint_id *ids, uint64_t m, void *table) {
  const uint32_t slots = demux_slots(m);
  DemuxSlot *t = new (std::nothrow) DemuxSlot[slots]();
  if (!t) return m + 1;
  uint64_t bad = m;
  for (uint64_t j = 0; j < m; ++j) {
    if (!demux_id_ok(ids[j])) {
      bad = j;
      break;
    }
    const DemuxKey k = demux_id_key(ids[j]);
    uint32_t i = demux_hash(k) & (slots - 1u);
    while (!demux_empty(t[i]) && !demux_match(t[i], k)) i = demux_next(i, slots);  // at most m of 2m slots are taken
    if (!demux_empty(t[i])) {
      bad = j;
      break;
    }
    t[i] = {k.local, k.remote, k.ports, demux_tag((uint32_t)j, k.code)};
  }
  if (bad == m && table) memcpy(table, t, (size_t)slots * kDemuxSlotBytes);
  delete[] t;
  return bad;
}

}  // namespace yu
#pragma GCC visibility pop

#endif  // YUCSUM_DEMUX_H
