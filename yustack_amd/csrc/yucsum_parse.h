// yucsum_parse.h — the arithmetic of k_parse, the kernel of yu_rx_parse_ragged
// (include/yucsum.h): received IPv4 datagrams parsed where they lie. It is
// yu_rx_split_ragged without the payload copy: the same 32-byte record and the
// same YU_RX_SPLIT bit, and instead of a copied payload one yu_iovec that
// points at the payload in the batch.
//
// One packet, one lane. The parse, the delivery tests and the record read only
// the packet's first min(len, 80) bytes (yucsum_split.h), so a lane holds that
// window itself: it starts at floor4(address), window dword j is loaded when
// 4j < split_hdr_lim, every other window dword is zero, and packet dword k is
// split_pkt_dword of window dwords k and k + 1, exactly what lane k of k_split
// holds. With IHL 5 the transport header's first four dwords t0 .. t3 are
// packet dwords 5 .. 8, so window dwords 0 .. 9 (parse_fixed) hold everything;
// any other IHL takes window dwords IHL .. IHL + 4 as well (parse_opt), named
// by value, never by indexing what is already held. A packet shorter than 20
// bytes is invalid whatever its first byte says and takes no second load.
// split_parse and split_record then give k_split's decision and record by
// construction.
//
// No HIP call is made here: the kernel and tests/cpp/rx_parse.cpp both use
// these functions.
#ifndef YUCSUM_PARSE_H
#define YUCSUM_PARSE_H

#include "yucsum_split.h"

#pragma GCC visibility push(hidden)
namespace yu {

constexpr uint32_t kParseFix = 10u;       // window dwords 0 .. 9: packet dwords 0 .. 8 at any phase
constexpr uint32_t kParseOpt = 5u;        // window dwords IHL .. IHL + 4: packet dwords IHL .. IHL + 3
constexpr uint32_t kParsePerWave = 64u;   // packets per wave step, one per lane
constexpr uint32_t kParseHdrBits = 8u | kSplitFlag;  // YU_RX_INVALID | YU_RX_SPLIT: what the header alone decides

// Is window dword j (the dword at floor4(addr) + 4j) loaded? lim: split_hdr_lim.
YU_IOV_FN bool parse_loads(uint32_t j, uint32_t lim) { return 4u * j < lim; }
// Are window dwords 0 .. kParseFix - 1 all loaded (a packet of 37 bytes or more)?
// Then they may be fetched as wider loads: the same dwords, nothing past them.
YU_IOV_FN bool parse_whole(uint32_t lim) { return parse_loads(kParseFix - 1u, lim); }

// The packet dwords split_parse and split_record read.
struct ParseHdr {
  uint32_t d0, d1, d2, d3, d4;  // packet dwords 0 .. 4
  uint32_t t0, t1, t2, t3;      // packet dwords HL / 4 .. HL / 4 + 3
};

// From window dwords 0 .. 9 (zero where not loaded), s = address & 3: d0 .. d4,
// and t0 .. t3 as they are with IHL 5.
YU_IOV_FN void parse_fixed(ParseHdr &P, const uint32_t (&w)[kParseFix], uint32_t s) {
  P.d0 = split_pkt_dword(w[1], w[0], s);
  P.d1 = split_pkt_dword(w[2], w[1], s);
  P.d2 = split_pkt_dword(w[3], w[2], s);
  P.d3 = split_pkt_dword(w[4], w[3], s);
  P.d4 = split_pkt_dword(w[5], w[4], s);
  P.t0 = split_pkt_dword(w[6], w[5], s);
  P.t1 = split_pkt_dword(w[7], w[6], s);
  P.t2 = split_pkt_dword(w[8], w[7], s);
  P.t3 = split_pkt_dword(w[9], w[8], s);
}
YU_IOV_FN uint32_t parse_ihl(const ParseHdr &P) { return P.d0 & 15u; }
// Does the packet take the second load? Under 20 bytes it is invalid and its
// t0 .. t3 are never read.
YU_IOV_FN bool parse_needs_opt(const ParseHdr &P, uint32_t len) { return len >= kBuildIp && parse_ihl(P) != 5u; }
// The window dword its k-th load, k < kParseOpt, takes.
YU_IOV_FN uint32_t parse_opt_dword(const ParseHdr &P, uint32_t k) { return parse_ihl(P) + k; }
// t0 .. t3 from those five (zero where not loaded).
YU_IOV_FN void parse_opt(ParseHdr &P, const uint32_t (&x)[kParseOpt], uint32_t s) {
  P.t0 = split_pkt_dword(x[1], x[0], s);
  P.t1 = split_pkt_dword(x[2], x[1], s);
  P.t2 = split_pkt_dword(x[3], x[2], s);
  P.t3 = split_pkt_dword(x[4], x[3], s);
}

// The two results the header alone decides: YU_RX_INVALID (iov_dg_value's
// `valid`) and YU_RX_SPLIT.
YU_IOV_FN uint32_t parse_hdr_bits(const SplitDg &S, uint32_t len) {
  const bool valid = (S.D.meta & kIovDgOk) && S.D.tl <= len;
  return (valid ? 0u : 8u) | (S.split ? kSplitFlag : 0u);
}

// The view: yu_iovec's two members. addr: split_src's address of the packet.
struct ParseView {
  uint64_t base, len;
};
YU_IOV_FN ParseView parse_view(const SplitDg &S, uint64_t addr) {
  return {S.split ? addr + S.lo : 0ull, S.split ? (uint64_t)S.L : 0ull};
}

}  // namespace yu
#pragma GCC visibility pop

#endif  // YUCSUM_PARSE_H
