// yucsum_split.h — the arithmetic of k_split, the kernel of yu_rx_split_ragged
// (include/yucsum.h): received IPv4 datagrams taken apart on the device into a
// 32-byte record, a payload and VERIFY_RX's flags, what ipv4.HandlePacket
// (network/ipv4/ipv4.go:62-77), Nic.DeliverTransportPacket (stack/nic.go:125-153),
// segment.parse (transport/tcp/segment.go:81-109) and udp.endpoint.HandlePacket
// (transport/udp/endpoint.go:191-199) do with a datagram before its payload is
// queued. It is k_build (yucsum_build.h) run backwards.
//
// One packet, one wave. A packet is one source range, so its header needs no
// gather: lane j loads window dword j of the packet's first min(len, 80) bytes
// (the window starts at floor4(address), as every window does), which covers an
// IPv4 header of IHL <= 15 plus TCP's 20 fixed bytes; split_pkt_dword shifts two
// neighbouring window dwords to packet dword k = bytes [4k, 4k + 4) of the
// packet, held by lane k. The parse (split_parse) is VERIFY_RX's (iov_dg_parse)
// plus the reference's delivery tests; the record's eight little-endian dwords
// (split_record) are build_hdr_src inverted. The IPv4 header, the pseudo
// header's addresses and the H fixed transport bytes are summed big-endian from
// the lanes (split_ip_term, split_seg_term); the rest of the segment, packet
// offsets [HL + H, TL), is the payload: one view, walked by yucsum_iov.h in
// 1-KiB slots, each summed and, when the packet splits, stored through
// yucsum_iov_pack.h's plan, shift and masked stores with nothing held back (no
// field is written). HL + H is a multiple of 4, so a byte's class (address
// parity XOR its packet offset) is its class in the payload counted from 0,
// and the payload is walked as a packet of its own that starts at offset 0
// (split_dst: where that offset goes and the room it has; no room, nothing
// stored). The header sums are already big-endian and enter the value on the
// unswapped side (split_value), which gives exactly VERIFY_RX's bits.
//
// No HIP call is made here: the kernel and tests/cpp/rx_split.cpp both use
// these functions.
#ifndef YUCSUM_SPLIT_H
#define YUCSUM_SPLIT_H

#include "yucsum_build.h"

#pragma GCC visibility push(hidden)
namespace yu {

constexpr uint32_t kSplitHdr = 80u;        // packet bytes the lanes hold: IHL <= 15 and TCPMinimumSize
constexpr uint32_t kSplitWinDwords = 21u;  // window dwords 80 bytes touch at phase 1..3
constexpr uint32_t kSplitFlag = 16u;       // == YU_RX_SPLIT

// Packet i's bytes, whatever its offsets say: cut to data[0, offsets[n]) and to
// kIovLimit ((o0, o1, oN): offsets[i], offsets[i + 1], offsets[n]). No bytes: the
// address is data's own and nothing is loaded.
YU_IOV_FN void split_src(uint64_t data, uint64_t o0, uint64_t o1, uint64_t oN, uint64_t &addr, uint32_t &len) {
  const uint64_t e = o1 < oN ? o1 : oN;
  const uint64_t l = e > o0 ? e - o0 : 0;
  len = l < kIovLimit ? (uint32_t)l : kIovLimit;
  addr = data + (len ? o0 : 0);
}
// Window bytes of the header load: lane j < kSplitWinDwords loads the dword at
// floor4(addr) + 4j when 4j < split_hdr_lim.
YU_IOV_FN uint32_t split_hdr_lim(uint64_t addr, uint32_t len) {
  return len ? ((uint32_t)addr & 3u) + (len < kSplitHdr ? len : kSplitHdr) : 0u;
}
// Packet dword k from window dwords k (lo) and k + 1 (hi), s = address & 3.
YU_IOV_FN uint32_t split_pkt_dword(uint32_t hi, uint32_t lo, uint32_t s) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_alignbyte(hi, lo, s);
#else
  return (uint32_t)((((uint64_t)hi << 32) | lo) >> (8u * s));
#endif
}

// What the parse of a packet's first dwords fixes before its walk starts.
struct SplitDg {
  IovDg D;            // VERIFY_RX's parse (D.lo, D.hi, D.f are not used here)
  uint32_t H;         // k_build's transport header length for Protocol()
  uint32_t L;         // payload bytes, slen - H (0 without YU_RX_SPLIT)
  uint32_t lo, hi;    // packet offsets the walk takes: [HL + H, TL), or none
  uint32_t flo, fhi;  // packet offsets of the transport bytes the lanes sum: [HL, min(HL + H, TL)), or none
  bool split;         // YU_RX_SPLIT
};

// len: the packet's bytes; d0, d2: packet dwords 0 and 2; t1, t3: packet dwords
// HL / 4 + 1 and HL / 4 + 3 (UDP's Length(), TCP's data-offset byte; anything
// where the packet does not hold them: they are read only when it does).
YU_IOV_FN void split_parse(SplitDg &S, uint32_t len, uint32_t d0, uint32_t d2, uint32_t t1, uint32_t t3) {
  const uint32_t have = len < kIovHdr ? len : kIovHdr;
  iov_dg_parse(S.D, 8, have, d0 & 0xFFu, (d0 >> 16) & 0xFFu, d0 >> 24, (d2 >> 8) & 0xFFu);
  const uint32_t hl = iov_dg_hl(S.D.meta), tl = S.D.tl, proto = iov_dg_proto(S.D.meta);
  const bool valid = (S.D.meta & kIovDgOk) && tl <= len;  // IsValid, header/ipv4.go:126-138
  const bool l4 = (S.D.meta & kIovDgL4) != 0;
  const uint32_t H = build_l4_len(proto);
  const uint32_t slen = valid ? tl - hl : 0u;
  bool split = valid && hl >= kBuildIp && slen >= H;  // stack/nic.go:133
  if (split && proto == 6u) {                         // segment.go:94-97
    const uint32_t doff = ((t3 & 0xFFu) >> 4) * 4u;
    split = doff >= 20u && doff <= slen;
  }
  if (split && proto == 17u) split = build_be16(t1 & 0xFFFFu) <= slen;  // udp/endpoint.go:194
  S.H = H;
  S.L = split ? slen - H : 0u;
  S.split = split;
  S.lo = hl + H;
  S.hi = valid && (split || l4) && tl > hl + H ? tl : S.lo;
  S.flo = hl;
  S.fhi = valid && l4 ? (hl + H < tl ? hl + H : tl) : hl;
}

// Lane k's share (pd: packet dword k) of the IPv4 header's big-endian sum over
// b[:min(HL, len)], and of what the lanes add to the segment's: the H fixed
// transport bytes the packet holds and, but for ICMP, the pseudo header's
// {src, dst}.
YU_IOV_FN uint32_t split_ip_term(const SplitDg &S, uint32_t k, uint32_t pd) {
  return iov_be_words(pd & iov_win_mask((int32_t)(4u * k), 0u, iov_dg_hn(S.D.meta)));
}
YU_IOV_FN uint32_t split_seg_term(const SplitDg &S, uint32_t k, uint32_t pd) {
  const uint32_t ps = (k == 3u || k == 4u) && iov_dg_proto(S.D.meta) != 1u ? iov_be_words(pd) : 0u;
  return ps + iov_be_words(pd & iov_win_mask((int32_t)(4u * k), S.flo, S.fhi));
}

// out[i]: VERIFY_RX's bits plus YU_RX_SPLIT. hs, xs: the lanes' sums above;
// (sA, sB): the walk's class sums (sA the swapped class). xs is big-endian
// already and at most 14 words, so it joins the unswapped class without a wrap,
// and the segment's sum stays 0 exactly when every byte of it is zero.
YU_IOV_FN uint32_t split_value(const SplitDg &S, uint32_t len, uint32_t hs, uint32_t xs, uint32_t sA, uint32_t sB) {
  uint32_t r0, r1;
  bool st0, st1;
  iov_dg_value(S.D, 8, len, hs, 0u, sA, sB + xs, r0, r1, st0, st1);
  return r0 | (S.split ? kSplitFlag : 0u);
}

// The record: build_hdr_src inverted. d0 .. d4: packet dwords 0 .. 4; t0 .. t3:
// packet dwords HL / 4 .. HL / 4 + 3. Without YU_RX_SPLIT: eight zero dwords.
YU_IOV_FN void split_record(BuildRec &R, const SplitDg &S, uint32_t d0, uint32_t d1, uint32_t d2, uint32_t d3,
                            uint32_t d4, uint32_t t0, uint32_t t1, uint32_t t2, uint32_t t3) {
  for (int k = 0; k < 8; ++k) R.w[k] = 0u;
  if (!S.split) return;
  const uint32_t proto = iov_dg_proto(S.D.meta);
  R.w[0] = d3;
  R.w[1] = d4;
  if (proto == 6u || proto == 17u) R.w[2] = build_be16(t0 & 0xFFFFu) | (build_be16(t0 >> 16) << 16);
  if (proto == 1u) R.w[2] = build_be16(t0 & 0xFFFFu);  // type << 8 | code
  if (proto == 6u) {
    R.w[3] = build_be32(t1);
    R.w[4] = build_be32(t2);
    R.w[5] = build_be16(t3 >> 16) | (((t3 >> 8) & 0xFFu) << 16) | ((((t3 & 0xFFu) >> 4) * 4u) << 24);
  }
  R.w[6] = proto | ((d2 & 0xFFu) << 8) | (build_be16(d1 & 0xFFFFu) << 16);
  R.w[7] = ((d0 >> 8) & 0xFFu) | (build_be16(d1 >> 16) << 16);
}

// The payload as a packet of its own: its byte 0 (packet offset HL + H) goes to
// pay + pay_offsets[i], with the room of the packet's span ((p0, p1, pN):
// pay_offsets[i], pay_offsets[i + 1], pay_offsets[n]); a packet that does not
// split has no room, so the store side stores nothing of it.
YU_IOV_FN IovPackDst split_dst(const SplitDg &S, uint64_t pay, uint64_t p0, uint64_t p1, uint64_t pN) {
  return {pay + p0, S.split ? iov_pack_room(p0, p1, pN) : 0u};
}
// Starts the walk over the payload of the packet at addr: W.off counts the
// payload's own bytes from 0. Returns iov_pack_view's packet offset of the
// view's window byte 0.
YU_IOV_FN int32_t split_walk(IovWalk &W, const SplitDg &S, uint64_t addr) {
  iov_walk_reset(W);
  const uint64_t a = addr + S.lo;
  iov_walk_view(W, a, S.hi - S.lo, false, 0u);
  return iov_pack_view(a, 0u);
}

}  // namespace yu
#pragma GCC visibility pop

#endif  // YUCSUM_SPLIT_H
