// yucsum_reply.h — the arithmetic of k_reply, the kernel of yu_rx_reply
// (include/yucsum.h): which received packets are answered, with which record,
// and how long each answer is. It is the step that joins the receive half
// (yu_rx_parse_ragged, yu_rx_demux) to the send half (yu_tx_build_iov): what
// sample/tun_udp_echo does with ep.Read and ep.Write(v, &fullAddr), which ends
// in sendUDP(route, v, e.id.LocalPort, to.Port) with the addresses and ports
// turned round (transport/udp/endpoint.go:138-187), and what ipv4.handleICMP
// does with an Echo, sendICMPv4(r, ICMPv4EchoReply, 0, v) after
// vv.TrimFront(ICMPv4MinimumSize) (network/ipv4/icmp.go:28-63).
//
// One packet, one lane. The lane holds its record as eight dwords (two 16-byte
// loads), its view's length, and where given its flags, its endpoint number and
// one byte of ep_echo, which it loads only when reply_reads_echo says its index
// lies in the table. It leaves the reply record (two 16-byte stores, 32 zero
// bytes for no reply) and T, the reply datagram's length, or 0. The exclusive
// sum of T over the batch is the scan of yucsum_group.h, in place over the
// array the lanes stored T into.
//
// No HIP call is made here: the kernel, yu_rx_reply_workspace_bytes and
// tests/cpp/rx_reply.cpp all use these functions.
#ifndef YUCSUM_REPLY_H
#define YUCSUM_REPLY_H

#include <stdint.h>

#include "yucsum.h"
#include "yucsum_build.h"
#include "yucsum_demux.h"
#include "yucsum_group.h"

#pragma GCC visibility push(hidden)
namespace yu {

constexpr uint32_t kReplyIcmpEcho = YU_REPLY_ICMP_ECHO;
constexpr uint32_t kReplyUdpEcho = YU_REPLY_UDP_ECHO;
constexpr uint32_t kReplyKnown = kReplyIcmpEcho | kReplyUdpEcho;
constexpr uint32_t kReplyPerWave = 64u;   // packets per wave step, one per lane
constexpr uint32_t kReplyTtl = 64u;       // WritePacket's TTL (network/ipv4/ipv4.go:89)
constexpr uint32_t kReplyIcmpEchoType = 8u;  // header.ICMPv4Echo; the reply's type is 0, ICMPv4EchoReply

// The scratch of the call: the tile sums of one scan over n + 1 outputs.
YU_IOV_FN uint64_t reply_workspace_bytes(uint64_t n) { return group_align16(8u * group_scan_tiles(n + 1u)); }

// yu_rx_demux's gate without its protocol test: with a flags array every bit of
// need | YU_RX_SPLIT must be set.
YU_IOV_FN bool reply_gate(bool have_flags, uint32_t flags, uint32_t need) {
  const uint32_t want = (need | kDemuxSplit) & 0xFFFFu;
  return !have_flags || (flags & want) == want;
}

// What a gated packet may be answered as: kReplyIcmpEcho (an Echo request; only
// Type() is tested, icmp.go:57), kReplyUdpEcho (any UDP datagram), or 0. w2:
// record dword 2, sport | dport << 16, where ICMP's sport is type << 8 | code.
YU_IOV_FN uint32_t reply_kind(uint32_t what, bool gate, uint32_t proto, uint32_t w2) {
  if (!gate) return 0u;
  if ((what & kReplyIcmpEcho) && proto == 1u && ((w2 & 0xFFFFu) >> 8) == kReplyIcmpEchoType) return kReplyIcmpEcho;
  if ((what & kReplyUdpEcho) && proto == 17u) return kReplyUdpEcho;
  return 0u;
}

// Does the lane read ep[i]? Only a UDP candidate has an endpoint to ask.
YU_IOV_FN bool reply_reads_ep(uint32_t kind) { return kind == kReplyUdpEcho; }
// Does it read ep_echo[e]? Only with a table, and only at an index inside it.
YU_IOV_FN bool reply_reads_echo(uint32_t kind, bool have_echo, uint32_t e, uint32_t m) {
  return kind == kReplyUdpEcho && have_echo && e < m;
}

// The reply of one packet. in: its record; L: its view's length; kind:
// reply_kind's; e: ep[i] (anything when the lane did not read it); echo: the
// ep_echo byte (anything when the lane did not read it). Stores the reply
// record, or eight zero dwords, and returns T = 20 + H + L, or 0.
YU_IOV_FN uint64_t reply_make(BuildRec &out, const BuildRec &in, uint64_t L, uint32_t kind, bool have_echo,
                              uint32_t e, uint32_t m, uint32_t echo) {
  out = BuildRec{{0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u}};
  uint32_t proto = 0u;
  if (kind == kReplyIcmpEcho) proto = 1u;
  if (kind == kReplyUdpEcho && e < m && (!have_echo || echo != 0u)) proto = 17u;
  const uint32_t H = build_l4_len(proto);
  if (proto == 0u || L > (uint64_t)(kIovLimit - kBuildIp - H)) return 0u;
  out.w[0] = in.w[1];  // src = the request's dst: FindRoute with one address and an empty bindAddr
  out.w[1] = in.w[0];
  out.w[2] = proto == 17u ? (in.w[2] >> 16) | (in.w[2] << 16) : 0u;  // ports turned round; EchoReply, code 0
  out.w[6] = proto | (kReplyTtl << 8);
  return (uint64_t)(kBuildIp + H) + L;
}

}  // namespace yu
#pragma GCC visibility pop

#endif  // YUCSUM_REPLY_H
