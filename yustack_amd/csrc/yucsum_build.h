// yucsum_build.h — the arithmetic of k_build, the kernel of yu_tx_build_ragged
// (include/yucsum.h): outgoing IPv4 datagrams built on the device from a payload
// and one 32-byte record per packet, what sendUDP, sendTCP / sendTCPWithOptions
// and sendICMPv4 do with a payload and a few numbers before WritePacket adds the
// IPv4 header (transport/udp/endpoint.go:164-187, transport/tcp/connect.go:
// 556-586 and 288-322, network/ipv4/icmp.go:36-45, network/ipv4/ipv4.go:80-97).
//
// One packet, one wave. The payload is a single view: yucsum_iov.h's walk cuts
// it into 1-KiB slots at floor4(base), started at packet offset 20 + H (H: the
// transport header's bytes), which is even and a multiple of 4, so a byte's
// class follows from its address parity as ever and header and payload share
// the destination phase. Each slot goes through yucsum_iov_pack.h's plan, shift
// and masked stores as it is summed. The header is never loaded: its 20 + H <=
// 40 bytes are encoded from the record into at most ten little-endian dwords
// (build_hdr_src), its sums are arithmetic on the record's numbers
// (build_ip_sum, build_pseudo_sum, build_l4_sum), and once the payload's class
// sums are known the two fields are composed (build_values) and the header is
// stored last, once, with both fields in place: lane J < 11 owns destination
// dword J of the packet, bytes [4J - delta, 4J - delta + 4) of the header
// (build_hdr_dst from source dwords J - 1 and J), cut to the header's end and
// the packet's room by the same byte mask a payload dword gets (build_hdr_plan
// makes the plan iov_pack_mask reads). No byte is held back and none is stored
// twice: the destination dword that holds the header's last bytes and the
// payload's first gets two partial stores with disjoint masks.
//
// No HIP call is made here: the kernel and tests/cpp/tx_build.cpp both use
// these functions.
#ifndef YUCSUM_BUILD_H
#define YUCSUM_BUILD_H

#include "yucsum_iov_pack.h"

#pragma GCC visibility push(hidden)
namespace yu {

constexpr uint32_t kBuildIp = 20u;          // IPv4MinimumSize: WritePacket encodes IHL 5
constexpr uint32_t kBuildHdrMax = 40u;      // 20 + TCPMinimumSize
constexpr uint32_t kBuildHdrDwords = 11u;   // destination dwords 40 bytes touch at phase 3

// yu_tx_record as the eight dwords a little-endian load gives.
struct BuildRec {
  uint32_t w[8];
};
YU_IOV_FN uint32_t build_src(const BuildRec &R) { return R.w[0]; }  // wire bytes
YU_IOV_FN uint32_t build_dst(const BuildRec &R) { return R.w[1]; }
YU_IOV_FN uint32_t build_sport(const BuildRec &R) { return R.w[2] & 0xFFFFu; }
YU_IOV_FN uint32_t build_dport(const BuildRec &R) { return R.w[2] >> 16; }
YU_IOV_FN uint32_t build_seq(const BuildRec &R) { return R.w[3]; }
YU_IOV_FN uint32_t build_ack(const BuildRec &R) { return R.w[4]; }
YU_IOV_FN uint32_t build_window(const BuildRec &R) { return R.w[5] & 0xFFFFu; }
YU_IOV_FN uint32_t build_flags(const BuildRec &R) { return (R.w[5] >> 16) & 0xFFu; }
YU_IOV_FN uint32_t build_doff(const BuildRec &R) { return R.w[5] >> 24; }
YU_IOV_FN uint32_t build_proto(const BuildRec &R) { return R.w[6] & 0xFFu; }
YU_IOV_FN uint32_t build_ttl(const BuildRec &R) { return (R.w[6] >> 8) & 0xFFu; }
YU_IOV_FN uint32_t build_ip_id(const BuildRec &R) { return R.w[6] >> 16; }
YU_IOV_FN uint32_t build_tos(const BuildRec &R) { return R.w[7] & 0xFFu; }
YU_IOV_FN uint32_t build_frag(const BuildRec &R) { return R.w[7] >> 16; }

// H: the transport header the call encodes (TCP's options are payload bytes).
YU_IOV_FN uint32_t build_l4_len(uint32_t proto) {
  return proto == 6u ? 20u : (proto == 17u ? 8u : (proto == 1u ? 4u : 0u));
}
// TCP.Encode's data-offset byte, (doff / 4) << 4, as a byte whatever doff is.
YU_IOV_FN uint32_t build_doff_byte(const BuildRec &R) { return ((build_doff(R) >> 2) << 4) & 0xFFu; }

// A 16-bit / 32-bit number as its big-endian bytes read little-endian.
YU_IOV_FN uint32_t build_be16(uint32_t x) { return ((x & 0xFFu) << 8) | ((x >> 8) & 0xFFu); }
YU_IOV_FN uint32_t build_be32(uint32_t x) {
  return (x >> 24) | ((x >> 8) & 0xFF00u) | ((x << 8) & 0xFF0000u) | (x << 24);
}

// The IPv4 header's big-endian sum, its field taken as 0 (IPv4.Encode,
// header/ipv4.go:146-157; T: TotalLength). Never 0: the first word is 0x45xx.
YU_IOV_FN uint32_t build_ip_sum(const BuildRec &R, uint32_t T) {
  return (0x4500u | build_tos(R)) + (T & 0xFFFFu) + build_ip_id(R) + build_frag(R) +
         ((build_ttl(R) << 8) | build_proto(R)) + iov_be_words(build_src(R)) + iov_be_words(build_dst(R));
}
// PseudoHeaderChecksum plus the transport length (H + L); ICMP has none.
YU_IOV_FN uint32_t build_pseudo_sum(const BuildRec &R, uint32_t H, uint32_t L) {
  const uint32_t proto = build_proto(R);
  if (proto != 6u && proto != 17u) return 0u;
  return iov_be_words(build_src(R)) + iov_be_words(build_dst(R)) + proto + ((H + L) & 0xFFFFu);
}
// The transport header's own big-endian words, its field taken as 0.
YU_IOV_FN uint32_t build_l4_sum(const BuildRec &R, uint32_t L) {
  const uint32_t proto = build_proto(R);
  if (proto == 6u)
    return build_sport(R) + build_dport(R) + (build_seq(R) >> 16) + (build_seq(R) & 0xFFFFu) +
           (build_ack(R) >> 16) + (build_ack(R) & 0xFFFFu) + ((build_doff_byte(R) << 8) | build_flags(R)) +
           build_window(R);
  if (proto == 17u) return build_sport(R) + build_dport(R) + ((8u + L) & 0xFFFFu);
  if (proto == 1u) return build_sport(R);  // type << 8 | code
  return 0u;
}

// The two fields of the image with H + L transport bytes: ipsum is YU_MODE_IPV4's
// value, xsum YU_MODE_TX_DATAGRAM's second ((sA, sB): the payload's class sums,
// sA the swapped class). The sums are sums of the segment's own bytes and
// cannot wrap, so xsum is 0xFFFF exactly when everything summed is zero (an
// all-zero ICMP segment) and a sum of 0xFFFF gives 0x0000 as it is (UDP: no
// substitution). No transport header: xsum 0.
YU_IOV_FN void build_values(const BuildRec &R, uint32_t H, uint32_t L, uint32_t sA, uint32_t sB, uint32_t &ipsum,
                            uint32_t &xsum) {
  ipsum = (~iov_fold(build_ip_sum(R, kBuildIp + H + L))) & 0xFFFFu;
  const uint32_t seg = iov_residue(sA, sB) + build_pseudo_sum(R, H, L) + build_l4_sum(R, L);
  xsum = H ? (~iov_fold(seg)) & 0xFFFFu : 0u;
}

// Source dword k of the header: bytes [4k, 4k + 4) of the image as a
// little-endian load would read them; 0 from the header's end on (k >= 5 + H / 4).
YU_IOV_FN uint32_t build_hdr_src(const BuildRec &R, uint32_t H, uint32_t L, uint32_t ipsum, uint32_t xsum,
                                 uint32_t k) {
  const uint32_t proto = build_proto(R);
  const uint32_t T = kBuildIp + H + L;
  const uint32_t ports = build_be16(build_sport(R)) | (build_be16(build_dport(R)) << 16);
  const uint32_t xs = build_be16(xsum);
  uint32_t h5 = 0, h6 = 0, h7 = 0, h8 = 0, h9 = 0;
  if (proto == 6u) {  // TCP.Encode, header/tcp.go:176-186 (urgent pointer 0)
    h5 = ports;
    h6 = build_be32(build_seq(R));
    h7 = build_be32(build_ack(R));
    h8 = build_doff_byte(R) | (build_flags(R) << 8) | (build_be16(build_window(R)) << 16);
    h9 = xs;
  } else if (proto == 17u) {  // UDP.Encode, header/udp.go:78-83
    h5 = ports;
    h6 = build_be16(8u + L) | (xs << 16);
  } else if (proto == 1u) {  // type, code, checksum
    h5 = build_be16(build_sport(R)) | (xs << 16);
  }
  switch (k) {
    case 0: return 0x45u | (build_tos(R) << 8) | (build_be16(T) << 16);
    case 1: return build_be16(build_ip_id(R)) | (build_be16(build_frag(R)) << 16);
    case 2: return build_ttl(R) | (proto << 8) | (build_be16(ipsum) << 16);
    case 3: return build_src(R);
    case 4: return build_dst(R);
    case 5: return h5;
    case 6: return h6;
    case 7: return h7;
    case 8: return h8;
    case 9: return h9;
    default: return 0u;
  }
}

// The header as a first slot of 20 + H bytes whose window byte 0 is packet
// offset 0: the plan of lane 0, whose destination dword j = 0 .. 10
// (iov_pack_mask(P, j), at (P.pa & ~3) + 4j) is the one lane j of the wave stores.
YU_IOV_FN void build_hdr_plan(IovPackPlan &P, const IovPackDst &D, uint32_t H) {
  iov_pack_plan(P, (kBuildIp + H) | kIovFirst, D, 0, 0u);
}
// Destination dword J's header bytes from source dwords J - 1 (lo; J == 0: none)
// and J (hi).
YU_IOV_FN uint32_t build_hdr_dst(uint32_t hi, uint32_t lo, uint32_t delta) { return iov_pack_shift(hi, lo, delta); }

// In contract (include/yucsum.h): the payload's offsets do not decrease and stay
// inside payload[0, pay_offsets[n]) (ranged), T <= 65535 (the walk took all L
// bytes: !over), T fits the room, and TCP's doff is a header length the payload
// holds the options of.
YU_IOV_FN bool build_in_contract(const BuildRec &R, bool ranged, bool over, uint32_t L, uint32_t room) {
  const uint32_t proto = build_proto(R), doff = build_doff(R);
  const uint32_t T = kBuildIp + build_l4_len(proto) + L;
  const bool tcp_ok = proto != 6u || (doff >= 20u && doff <= 60u && (doff & 3u) == 0u && doff - 20u <= L);
  return ranged && !over && T <= kIovLimit && T <= room && tcp_ok;
}

// yu_tx_build_iov: a packet whose destination span is empty is skipped by
// definition (its view is not walked, its record is ignored, nothing is stored,
// its out pair is {0, 0}), so a table with empty entries, as yu_rx_reply leaves
// for the packets it does not answer, is passed as it stands.
YU_IOV_FN bool build_iov_skipped(uint64_t o0, uint64_t o1) { return o1 == o0; }

}  // namespace yu
#pragma GCC visibility pop

#endif  // YUCSUM_BUILD_H
