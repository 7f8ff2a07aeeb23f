// k_split on a CPU: the parse, the delivery tests, the record, the header sums
// and the value of yustack_amd/csrc/yucsum_split.h, the single-view walk of
// yucsum_iov.h and the destination geometry of yucsum_iov_pack.h, driven here
// exactly as the kernel drives them (the header as one window dword per lane,
// packet dword k from lanes k and k + 1; the payload by iov_model.h's
// range_walk: steps of U = 4 slots, 64 lanes of 16 bytes, each lane's previous
// source dword taken from its neighbour, lane 0's from lane 63 of the slot
// before), against a byte-by-byte restatement of what
// ipv4.HandlePacket, Nic.DeliverTransportPacket, segment.parse and
// udp.endpoint.HandlePacket do with a datagram, its checksums by the scalar
// library's yu_checksum.
//
// The packet sits in an exact-size heap block rounded out to whole dwords (what
// the kernel's descriptors let it read: under AddressSanitizer a read past it
// is a report). The payload is stored into an exact-size block between 0xA5
// canaries; a store is counted per byte, so a byte stored twice, a slack byte or
// a canary touched, a store outside the block or a misaligned store is a
// failure.
//
// Well-formed: every L in 0..96 and 1016..1032 x source address mod 4 x
// destination mod 4 x {UDP, ICMP, protocol 47, TCP doff 20 / 24 / 60} x
//   IHL 5, 6, 15 x {random bytes with 0..3 trailing bytes past TL, all-0x00,
//   all-0xFF} with exact room, and
//   IHL 5, random bytes x room with slack 1..5 and short by 1..45.
// (A TCP kind whose doff the segment cannot hold is counted where it stands: it
// does not split.) Malformed: len 0..19; IHL 0..4; HL > TL; TL > len; a damaged
// IPv4 sum; a damaged transport sum; slen = H - 1 for each protocol; TCP doff 16
// and doff past slen; UDP Length() = slen + 1 and slen - 1. Then the limits and
// the device test's contract batch. The program prints, before its last line,
// the number of packets of each of these three groups.
#include "iov_model.h"
#include "yucsum_iov_pack.h"
#include "yucsum_split.h"

namespace {

constexpr size_t kCanary = 48;

struct Result {
  uint32_t out, pay_len;
  yu::BuildRec R;
};

// One packet as k_split<4, *> handles it. data: the call's data pointer; (o0, o1,
// oN): offsets[i], [i + 1], [n]; pay: the call's pay pointer; (p0, p1, pN):
// pay_offsets[i], [i + 1], [n].
Result kernel_split(Store &st, uint64_t data, uint64_t o0, uint64_t o1, uint64_t oN, uint64_t pay, uint64_t p0,
                    uint64_t p1, uint64_t pN) {
  uint64_t addr;
  uint32_t len;
  yu::split_src(data, o0, o1, oN, addr, len);
  const uint32_t lim = yu::split_hdr_lim(addr, len), s = (uint32_t)addr & 3u;
  const yu::IovSlot hs_slot = {addr & ~3ull, lim};
  uint32_t hw[64], pd[64];
  for (uint32_t lane = 0; lane < 64; ++lane) hw[lane] = 4u * lane < lim ? load_dword(hs_slot, 4u * lane, lim) : 0u;
  for (uint32_t lane = 0; lane < 64; ++lane) pd[lane] = yu::split_pkt_dword(hw[(lane + 1u) & 63u], hw[lane], s);
  const uint32_t q = pd[0] & 15u;
  yu::SplitDg S;
  yu::split_parse(S, len, pd[0], pd[2], pd[q + 1], pd[q + 3]);
  uint32_t hs = 0, xs = 0;
  for (uint32_t lane = 0; lane < 64; ++lane) {
    hs += yu::split_ip_term(S, lane, pd[lane]);
    xs += yu::split_seg_term(S, lane, pd[lane]);
  }
  const yu::IovPackDst D = yu::split_dst(S, pay, p0, p1, pN);
  yu::IovWalk W;
  const int32_t vpk = yu::split_walk(W, S, addr);
  uint32_t A, B;
  range_walk(W, vpk, D, st, A, B);
  Result r;
  r.out = yu::split_value(S, len, hs, xs, A, B);
  r.pay_len = S.L;
  yu::split_record(r.R, S, pd[0], pd[1], pd[2], pd[3], pd[4], pd[q], pd[q + 1], pd[q + 2], pd[q + 3]);
  return r;
}

uint32_t l4_len(uint32_t proto) { return proto == 6 ? 20 : (proto == 17 ? 8 : (proto == 1 ? 4 : 0)); }
uint32_t rd16(const uint8_t *p) { return ((uint32_t)p[0] << 8) | p[1]; }
uint32_t rd32(const uint8_t *p) { return (rd16(p) << 16) | rd16(p + 2); }

struct Want {
  uint32_t out = 0, L = 0;
  yu_tx_record rec;
  const uint8_t *pay = nullptr;
};

// What the reference does with the received datagram b[0, len), step by step.
Want reference(const uint8_t *b, uint32_t len) {
  Want w;
  memset(&w.rec, 0, sizeof w.rec);
  uint32_t r[2];
  int field[2];
  scalar_value(b, len, YU_MODE_VERIFY_RX, r, field);  // the checksums: include/yucsum.h's VERIFY_RX
  w.out = r[0];
  // ipv4.HandlePacket: IsValid (header/ipv4.go:126-138), then the header is trimmed
  if (len < 20) return w;
  const uint32_t hl = (b[0] & 15u) * 4u, tl = rd16(b + 2);
  if (hl > tl || tl > len) return w;
  if (hl < 20) return w;  // the address bytes would not be header bytes
  const uint8_t *seg = b + hl;
  const uint32_t slen = tl - hl, proto = b[9], H = l4_len(proto);
  // Nic.DeliverTransportPacket (stack/nic.go:133): the transport header's minimum size
  if (slen < H) return w;
  yu_tx_record rec;
  memset(&rec, 0, sizeof rec);
  memcpy(rec.src, b + 12, 4);
  memcpy(rec.dst, b + 16, 4);
  rec.proto = (uint8_t)proto, rec.ttl = b[8], rec.ip_id = (uint16_t)rd16(b + 4), rec.tos = b[1];
  rec.frag = (uint16_t)rd16(b + 6);
  if (proto == 6) {  // segment.parse (transport/tcp/segment.go:81-109)
    const uint32_t doff = (uint32_t)(seg[12] >> 4) * 4u;
    if (doff < 20 || doff > slen) return w;
    rec.sport = (uint16_t)rd16(seg), rec.dport = (uint16_t)rd16(seg + 2);
    rec.seq = rd32(seg + 4), rec.ack = rd32(seg + 8);
    rec.flags = seg[13], rec.window = (uint16_t)rd16(seg + 14), rec.doff = (uint8_t)doff;
  } else if (proto == 17) {  // udp.endpoint.HandlePacket (transport/udp/endpoint.go:191-199)
    if (rd16(seg + 4) > slen) return w;
    rec.sport = (uint16_t)rd16(seg), rec.dport = (uint16_t)rd16(seg + 2);
  } else if (proto == 1) {
    rec.sport = (uint16_t)rd16(seg);
  }
  w.out |= YU_RX_SPLIT;
  w.rec = rec;
  w.L = slen - H;
  w.pay = seg + H;
  return w;
}

struct Case {
  uint32_t salign = 0, dalign = 0;
  int64_t room = -1;        // the packet's span in pay (< 0: exact, L)
  bool decreasing = false;  // pay_offsets decreases at the packet
  int src_fault = 0;        // 1: offsets decreases at the packet, 2: it ends past offsets[n], 3: one byte over the limit
};

void run(const std::vector<uint8_t> &pkt, uint32_t len, const Case &c, const char *what) {
  const View v = place(pkt.data(), len, c.salign);
  uint64_t o0 = 4096 + c.salign, o1 = o0 + len, oN = o1;
  const uint64_t data = v.addr - o0;
  uint32_t use = len;  // the bytes the kernel may take
  if (c.src_fault == 1) o1 = o0 - 1, oN = o0, use = 0;
  if (c.src_fault == 2) o1 = o0 + len + 77;
  if (c.src_fault == 3) use = len - 1;  // len is 65536 here
  const Want want = reference(pkt.data(), use);

  const uint64_t want_room = c.room >= 0 ? (uint64_t)c.room : want.L;
  const uint64_t room = c.decreasing ? 0 : (want_room < 65535 ? want_room : 65535);
  const size_t inner = (size_t)(want_room > want.L ? want_room : want.L);
  Store st;
  st.total = kCanary + c.dalign + inner + kCanary;
  st.blk = (uint8_t *)malloc(st.total);
  memset(st.blk, 0xA5, st.total);
  st.cnt.assign(st.total, 0);
  const size_t at = kCanary + c.dalign;  // malloc's blocks are 16-aligned
  const uint64_t p0 = 1000;
  uint64_t p1 = p0 + want_room;
  const uint64_t pN = p0 + want_room + 64;
  if (c.decreasing) p1 = p0 - 1;
  const uint64_t pay = (uint64_t)(uintptr_t)st.blk + at - p0;
  const Result got = kernel_split(st, data, o0, o1, oN, pay, p0, p1, pN);
  ++checks;

  bool ok = !st.bad && got.out == want.out && got.pay_len == want.L && memcmp(got.R.w, &want.rec, 32) == 0;
  const size_t in = want.L < room ? want.L : (size_t)room;  // the in-room bytes
  for (size_t i = 0; i < in; ++i) ok = ok && st.cnt[at + i] == 1 && st.blk[at + i] == want.pay[i];
  for (size_t i = 0; i < st.total; ++i)
    if (i < at || i >= at + in) ok = ok && st.cnt[i] == 0 && st.blk[i] == 0xA5;
  if (!ok) {
    fprintf(stderr, "%s: len %u salign %u dalign %u room %lld dec %d src_fault %d: out %x (want %x) pay_len %u (want %u) "
            "store-bad %d\n", what, len, c.salign, c.dalign, (long long)c.room, (int)c.decreasing, c.src_fault, got.out,
            want.out, got.pay_len, want.L, (int)st.bad);
    if (++fails > 10) exit(1);
  }
  free(st.blk);
  free(v.blk);
}

void put16(std::vector<uint8_t> &v, size_t at, uint32_t x) {
  v[at] = (uint8_t)(x >> 8);
  v[at + 1] = (uint8_t)x;
}

// Both checksum fields of the datagram as the reference's senders store them.
void fill_sums(std::vector<uint8_t> &b) {
  const uint32_t hl = (b[0] & 15u) * 4u, tl = rd16(&b[2]), proto = b[9], sl = tl - hl;
  put16(b, 10, 0);
  put16(b, 10, (uint16_t)~yu_checksum(b.data(), hl, 0));
  const uint32_t f = proto == 6 ? 16u : (proto == 17 ? 6u : (proto == 1 ? 2u : 0u));
  if (!f || sl < f + 2u) return;
  put16(b, hl + f, 0);
  uint16_t x = 0;
  if (proto != 1) {
    x = yu_pseudo_header_checksum(proto, &b[12], 4, &b[16], 4);
    const uint8_t lb[2] = {(uint8_t)(sl >> 8), (uint8_t)sl};
    x = yu_checksum(lb, 2, x);
  }
  put16(b, hl + f, (uint16_t)~yu_checksum(&b[hl], sl, x));
}

// A received datagram with payload L: fill 0 random (its sums filled in), 1 all
// 0x00, 2 all 0xFF; `trail` bytes past TotalLength. Returns its length.
uint32_t datagram_of(std::vector<uint8_t> &b, std::mt19937_64 &rng, uint32_t proto, uint32_t doff, uint32_t ihl,
                     uint32_t L, int fill, uint32_t trail) {
  const uint32_t hl = 4 * ihl, tl = hl + l4_len(proto) + L, len = tl + trail;
  b.assign(len + 1, 0);
  for (auto &x : b) x = fill == 0 ? (uint8_t)rng() : (fill == 1 ? 0x00 : 0xFF);
  b[0] = (uint8_t)(0x40u | ihl);
  put16(b, 2, tl);
  b[9] = (uint8_t)proto;
  if (proto == 6) b[hl + 12] = (uint8_t)(((doff / 4) << 4) | (b[hl + 12] & 15u));
  if (proto == 17) put16(b, hl + 4, 8 + L);
  if (fill == 0) fill_sums(b);
  return len;
}

const struct {
  uint8_t proto, doff;
} kKinds[6] = {{17, 20}, {1, 20}, {47, 20}, {6, 20}, {6, 24}, {6, 60}};

}  // namespace

int main() {
  std::mt19937_64 rng(20261020);
  std::vector<uint8_t> b;
  std::vector<uint32_t> lens;
  for (uint32_t l = 0; l <= 96; ++l) lens.push_back(l);
  for (uint32_t l = 1016; l <= 1032; ++l) lens.push_back(l);

  // ---- well-formed ----
  for (uint32_t L : lens)
    for (const auto &k : kKinds)
      for (uint32_t sa = 0; sa < 4; ++sa)
        for (uint32_t da = 0; da < 4; ++da) {
          Case c;
          c.salign = sa, c.dalign = da;
          for (uint32_t ihl : {5u, 6u, 15u}) {
            for (uint32_t trail = 0; trail < 4; ++trail)
              run(b, datagram_of(b, rng, k.proto, k.doff, ihl, L, 0, trail), c, "exact room");
            run(b, datagram_of(b, rng, k.proto, k.doff, ihl, L, 1, 0), c, "all 0x00");
            run(b, datagram_of(b, rng, k.proto, k.doff, ihl, L, 2, 0), c, "all 0xFF");
          }
          const uint32_t len = datagram_of(b, rng, k.proto, k.doff, 5, L, 0, 0);
          const int64_t Lp = reference(b.data(), len).L;  // 0 where the kind's doff does not fit
          for (int64_t slack = 1; slack <= 5; ++slack) {
            c.room = Lp + slack;
            run(b, len, c, "slack");
          }
          for (int64_t shrt = 1; shrt <= 45; ++shrt) {
            c.room = Lp > shrt ? Lp - shrt : 0;
            run(b, len, c, "short room");
          }
        }
  printf("%llu well-formed\n", (unsigned long long)checks);
  const uint64_t before_malformed = checks;

  // ---- malformed ----
  for (uint32_t sa = 0; sa < 4; ++sa)
    for (uint32_t da = 0; da < 4; ++da) {
      Case c;
      c.salign = sa, c.dalign = da;
      for (uint32_t len = 0; len < 20; ++len) {
        datagram_of(b, rng, 17, 20, 5, 40, 0, 0);
        run(b, len, c, "len below 20");
      }
      for (const auto &k : kKinds)
        for (uint32_t L : {0u, 7u, 64u, 1021u}) {
          for (uint32_t ihl = 0; ihl < 5; ++ihl) {  // HL < 20 (IsValid accepts)
            const uint32_t len = datagram_of(b, rng, k.proto, k.doff, 5, L, 0, 0);
            b[0] = (uint8_t)(0x40u | ihl);
            run(b, len, c, "HL below 20");
          }
          uint32_t len = datagram_of(b, rng, k.proto, k.doff, 5, L, 0, 0);
          put16(b, 2, 19);
          run(b, len, c, "HL > TL");
          len = datagram_of(b, rng, k.proto, k.doff, 5, L, 0, 0);
          put16(b, 2, len + 1);
          run(b, len, c, "TL > len");
          len = datagram_of(b, rng, k.proto, k.doff, 5, L, 0, 0);
          b[10] ^= 0x40;
          run(b, len, c, "damaged IPv4 sum");
          len = datagram_of(b, rng, k.proto, k.doff, 5, L, 0, 0);
          b[len > 20 ? len - 1 : 11] ^= 0x04;
          run(b, len, c, "damaged transport sum");
        }
      for (uint32_t ihl : {5u, 6u, 15u})
        for (uint32_t proto : {6u, 17u, 1u}) {  // slen = H - 1
          const uint32_t len = datagram_of(b, rng, proto, 20, ihl, 0, 0, 0) - 1;
          put16(b, 2, len);
          fill_sums(b);
          run(b, len, c, "slen = H - 1");
        }
      for (uint32_t L : {0u, 4u, 7u, 36u}) {
        uint32_t len = datagram_of(b, rng, 6, 16, 5, L, 0, 0);
        run(b, len, c, "TCP doff 16");
        len = datagram_of(b, rng, 6, ((20 + L) / 4 + 1) * 4, 5, L, 0, 0);
        run(b, len, c, "TCP doff past slen");
      }
      for (uint32_t L : {0u, 7u, 64u, 1021u})
        for (int d : {1, -1}) {
          const uint32_t len = datagram_of(b, rng, 17, 20, 5, L, 0, 0);
          put16(b, 24, (uint32_t)((int)(8 + L) + d));
          fill_sums(b);
          run(b, len, c, d > 0 ? "UDP Length() = slen + 1" : "UDP Length() = slen - 1");
        }
    }
  printf("%llu malformed\n", (unsigned long long)(checks - before_malformed));
  const uint64_t before_limits = checks;

  // ---- the limits and the device test's contract batch ----
  for (uint32_t sa = 0; sa < 4; ++sa)
    for (uint32_t da = 0; da < 4; ++da) {
      Case c;
      c.salign = sa, c.dalign = da;
      uint32_t len = datagram_of(b, rng, 6, 24, 5, 65535 - 40, 0, 0);
      run(b, len, c, "65535 bytes");
      for (uint32_t L : {1459u, 1460u, 1461u, 4099u, 9000u}) run(b, datagram_of(b, rng, 6, 20, 5, L, 0, 0), c, "long");
      Case f = c;
      f.src_fault = 3;  // a 65536-byte packet: its first 65535 bytes are taken (TL: 65535)
      len = datagram_of(b, rng, 17, 20, 5, 65535 - 28, 0, 1);
      run(b, len, f, "65536 bytes");
      f.src_fault = 1;
      run(b, datagram_of(b, rng, 17, 20, 5, 700, 0, 0), f, "offsets decreases");
      f.src_fault = 2;
      run(b, datagram_of(b, rng, 17, 20, 5, 700, 0, 0), f, "ends past offsets[n]");
      Case s3 = c;
      s3.room = 700 - 3;
      run(b, datagram_of(b, rng, 17, 20, 5, 700, 0, 0), s3, "room short by 3");
      Case dec = c;
      dec.decreasing = true;
      run(b, datagram_of(b, rng, 17, 20, 5, 700, 0, 0), dec, "pay_offsets decreases");
    }
  printf("%llu limits\n", (unsigned long long)(checks - before_limits));
  return finish();
}
