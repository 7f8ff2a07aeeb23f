// k_build on a CPU: the header encode, sums and contract test of
// yustack_amd/csrc/yucsum_build.h, the single-view walk of yucsum_iov.h and the
// destination geometry of yucsum_iov_pack.h, driven here exactly as the kernel
// drives them (the payload by iov_model.h's range_walk: steps of U = 4 slots, 64
// lanes of 16 bytes, each lane's previous source dword taken from its neighbour,
// lane 0's from lane 63 of the slot before; the header stored last, lane J < 11
// its destination dword J, the neighbour's source dword by a row shift), against
// an image assembled byte by byte with the scalar library's yu_checksum.
//
// Each datagram is built into an exact-size heap block with 0xA5 canaries on
// both sides; a store is counted per byte, so a byte stored twice, a slack byte
// or a canary touched, a store outside the block or a misaligned store is a
// failure (and, for the block's ends, a report under AddressSanitizer). The
// payload sits in an exact-size heap block rounded out to whole dwords.
//
// Every L in 0..96 and 1016..1032 x payload address mod 4 x destination mod 4 x
// UDP, ICMP, protocol 47 and TCP with doff 20, 24 and 60 x room exact, slack
// 1..5 and short by 1..45 (a cut in the middle of the header included); random
// payloads and records, and all-0x00 / all-0xFF ones. Then the cases of the
// device test's contract batch (T = 65535, T = 65536, room short by 3,
// decreasing dst_offsets, doff 24 with L = 2), a span cut by dst_offsets[n] and
// payload offsets that decrease or pass pay_offsets[n].
#include "iov_model.h"
#include "yucsum_build.h"
#include "yucsum_iov_pack.h"

namespace {

constexpr size_t kCanary = 48;

struct Result {
  uint32_t ipsum, xsum;  // as computed (the kernel stores {0, 0} to out when !ok)
  bool ok;               // build_in_contract
};

// One packet as k_build<4, *> handles it. payload: the call's payload pointer;
// (p0, p1, poN): pay_offsets[i], [i + 1], [n]; dst: the call's dst pointer; (o0,
// o1, oN): dst_offsets[i], [i + 1], [n].
Result kernel_build(Store &st, uint64_t payload, uint64_t p0, uint64_t p1, uint64_t poN, const yu::BuildRec &R,
                    uint64_t dst, uint64_t o0, uint64_t o1, uint64_t oN) {
  const uint32_t H = yu::build_l4_len(yu::build_proto(R));
  const bool ranged = p0 <= p1 && p1 <= poN;
  const uint64_t pe = p1 < poN ? p1 : poN;
  const uint64_t plen = pe > p0 ? pe - p0 : 0;
  const uint64_t addr = payload + (plen ? p0 : 0);
  const yu::IovPackDst D = {dst + o0, yu::iov_pack_room(o0, o1, oN)};
  yu::IovWalk W;
  yu::iov_walk_reset(W);
  W.off = yu::kBuildIp + H;
  const int32_t vpk = yu::iov_pack_view(addr, W.off);
  yu::iov_walk_view(W, addr, plen, false, 0u);
  const uint32_t L = W.off - (yu::kBuildIp + H);
  uint32_t A, B;
  range_walk(W, vpk, D, st, A, B);
  Result r;
  yu::build_values(R, H, L, A, B, r.ipsum, r.xsum);
  uint32_t hw[64];
  for (uint32_t lane = 0; lane < 64; ++lane) hw[lane] = yu::build_hdr_src(R, H, L, r.ipsum, r.xsum, lane);
  yu::IovPackPlan P;
  yu::build_hdr_plan(P, D, H);
  for (uint32_t lane = 0; lane < 64; ++lane) {
    const uint32_t hprev = (lane & 15u) ? hw[lane - 1] : 0u;  // row_shr:1, a row's first lane gets 0
    const uint32_t m = lane < yu::kBuildHdrDwords ? yu::iov_pack_mask(P, lane) : 0u;
    if (m) yu::iov_pack_store(st, (P.pa & ~3ull) + 4u * lane, yu::build_hdr_dst(hw[lane], hprev, P.delta), m);
  }
  r.ok = yu::build_in_contract(R, ranged, W.over != 0u, L, D.room);
  return r;
}

struct Rec {  // yu_tx_record's fields as numbers
  uint8_t src[4], dst[4];
  uint16_t sport, dport;
  uint32_t seq, ack;
  uint16_t window;
  uint8_t flags, doff, proto, ttl;
  uint16_t ip_id;
  uint8_t tos;
  uint16_t frag;
};

yu::BuildRec as_dwords(const Rec &r) {
  yu_tx_record t;
  memset(&t, 0, sizeof t);
  memcpy(t.src, r.src, 4);
  memcpy(t.dst, r.dst, 4);
  t.sport = r.sport, t.dport = r.dport, t.seq = r.seq, t.ack = r.ack, t.window = r.window;
  t.flags = r.flags, t.doff = r.doff, t.proto = r.proto, t.ttl = r.ttl, t.ip_id = r.ip_id, t.tos = r.tos;
  t.frag = r.frag;
  yu::BuildRec R;
  static_assert(sizeof t == sizeof R.w, "the record is eight dwords");
  memcpy(R.w, &t, sizeof t);
  return R;
}

void be16(std::vector<uint8_t> &v, size_t at, uint32_t x) {
  v[at] = (uint8_t)(x >> 8);
  v[at + 1] = (uint8_t)x;
}
void be32(std::vector<uint8_t> &v, size_t at, uint32_t x) {
  be16(v, at, x >> 16);
  be16(v, at + 2, x & 0xFFFFu);
}

uint32_t l4_len(uint32_t proto) { return proto == 6 ? 20 : (proto == 17 ? 8 : (proto == 1 ? 4 : 0)); }

// The image byte by byte, the two fields by yu_checksum over it (include/yucsum.h).
std::vector<uint8_t> scalar_image(const Rec &r, const uint8_t *pay, uint32_t L, uint32_t &ipsum, uint32_t &xsum) {
  const uint32_t H = l4_len(r.proto);
  const uint32_t T = 20 + H + L;
  std::vector<uint8_t> v(T, 0);
  v[0] = 0x45, v[1] = r.tos;
  be16(v, 2, T), be16(v, 4, r.ip_id), be16(v, 6, r.frag);
  v[8] = r.ttl, v[9] = r.proto;
  memcpy(&v[12], r.src, 4);
  memcpy(&v[16], r.dst, 4);
  size_t f = 0;
  if (r.proto == 6) {
    be16(v, 20, r.sport), be16(v, 22, r.dport), be32(v, 24, r.seq), be32(v, 28, r.ack);
    v[32] = (uint8_t)((r.doff / 4) << 4), v[33] = r.flags;
    be16(v, 34, r.window);
    f = 36;
  } else if (r.proto == 17) {
    be16(v, 20, r.sport), be16(v, 22, r.dport), be16(v, 24, 8 + L);
    f = 26;
  } else if (r.proto == 1) {
    v[20] = (uint8_t)(r.sport >> 8), v[21] = (uint8_t)r.sport;
    f = 22;
  }
  if (L) memcpy(&v[20 + H], pay, L);
  ipsum = (uint16_t)~yu_checksum(v.data(), 20, 0);
  xsum = 0;
  if (f) {
    uint16_t x = 0;
    if (r.proto != 1) {
      x = yu_pseudo_header_checksum(r.proto, r.src, 4, r.dst, 4);
      const uint8_t lb[2] = {(uint8_t)((H + L) >> 8), (uint8_t)(H + L)};
      x = yu_checksum(lb, 2, x);
    }
    xsum = (uint16_t)~yu_checksum(v.data() + 20, H + L, x);
    be16(v, f, xsum);
  }
  be16(v, 10, ipsum);
  return v;
}

struct Case {
  uint32_t palign = 0, dalign = 0;
  int64_t room = -1;       // the packet's span is [0, room) of the block (< 0: exact, T)
  bool decreasing = false;  // dst_offsets decreases at the packet
  bool cut_by_end = false;  // dst_offsets[n] cuts the span to `room`
  int pay_fault = 0;        // 1: pay_offsets decreases at the packet, 2: it passes pay_offsets[n]
};

void run(const Rec &rec, const uint8_t *pay, uint32_t L, const Case &c, const char *what) {
  const uint64_t T = 20ull + l4_len(rec.proto) + L;
  // the payload in an exact-size block rounded out to whole dwords
  const size_t psz = (c.palign + L + 3u) & ~(size_t)3;
  uint8_t *pblk = (uint8_t *)malloc(psz ? psz : 4);
  memset(pblk, 0xA5, psz ? psz : 4);
  if (L) memcpy(pblk + c.palign, pay, L);
  uint64_t p0 = 4096 + c.palign, p1 = p0 + L, poN = p1;
  const uint64_t payload = (uint64_t)(uintptr_t)pblk + c.palign - p0;
  if (c.pay_fault == 1) p1 = p0 - 1, poN = p0;
  if (c.pay_fault == 2) p1 = p0 + L + 77;
  const uint32_t Luse = c.pay_fault == 1 ? 0 : L;  // the bytes the kernel may take
  const uint64_t Tuse = T - L + Luse;

  const uint64_t want_room = c.room >= 0 ? (uint64_t)c.room : T;
  const uint64_t room = c.decreasing ? 0 : (want_room < 65535 ? want_room : 65535);  // bytes the call may store
  const size_t inner = (size_t)(want_room > T ? want_room : T);  // the block between the canaries
  Store st;
  st.total = kCanary + c.dalign + inner + kCanary;
  st.blk = (uint8_t *)malloc(st.total);
  memset(st.blk, 0xA5, st.total);
  st.cnt.assign(st.total, 0);
  const size_t at = kCanary + c.dalign;  // malloc's blocks are 16-aligned
  const uint64_t o0 = 1000;
  uint64_t o1 = o0 + want_room, oN = o1 + 64;
  if (c.decreasing) o1 = o0 - 1;
  if (c.cut_by_end) {
    oN = o0 + want_room;
    o1 = oN + 7;
  }
  const uint64_t dst = (uint64_t)(uintptr_t)st.blk + at - o0;
  const yu::BuildRec R = as_dwords(rec);
  const Result got = kernel_build(st, payload, p0, p1, poN, R, dst, o0, o1, oN);
  ++checks;

  const bool tcp_ok =
      rec.proto != 6 || (rec.doff >= 20 && rec.doff <= 60 && rec.doff % 4 == 0 && rec.doff - 20u <= Luse);
  const bool fits = Tuse <= 65535 && Tuse <= room && !c.decreasing && c.pay_fault == 0;
  bool ok = !st.bad && got.ok == (fits && tcp_ok);
  if (Tuse <= 65535) {
    uint32_t ipsum, xsum;
    const std::vector<uint8_t> img = scalar_image(rec, pay, Luse, ipsum, xsum);
    const size_t in = Tuse < room ? (size_t)Tuse : (size_t)room;  // the in-room bytes
    // every in-room byte exact (a doff fault: but for the two field bytes) and stored exactly once
    for (size_t i = 0; i < in; ++i) {
      ok = ok && st.cnt[at + i] == 1;
      if (!tcp_ok && (i == 36 || i == 37)) continue;
      ok = ok && st.blk[at + i] == img[i];
    }
    for (size_t i = in; i < inner; ++i) ok = ok && st.cnt[at + i] == 0 && st.blk[at + i] == 0xA5;  // slack, or past the room
    if (fits && tcp_ok) ok = ok && got.ipsum == ipsum && got.xsum == xsum;
  } else {
    // over the limit: only inside the span, no byte twice
    for (size_t i = 0; i < inner; ++i) {
      ok = ok && st.cnt[at + i] <= 1;
      if (i >= room) ok = ok && st.cnt[at + i] == 0 && st.blk[at + i] == 0xA5;
    }
  }
  for (size_t i = 0; i < at; ++i) ok = ok && st.cnt[i] == 0 && st.blk[i] == 0xA5;
  for (size_t i = at + inner; i < st.total; ++i) ok = ok && st.cnt[i] == 0 && st.blk[i] == 0xA5;
  if (!ok) {
    fprintf(stderr, "%s: L %u proto %u doff %u palign %u dalign %u room %lld dec %d cut %d pay_fault %d: "
            "ipsum %04x xsum %04x in-contract %d, store-bad %d\n", what, L, rec.proto, rec.doff, c.palign, c.dalign,
            (long long)c.room, (int)c.decreasing, (int)c.cut_by_end, c.pay_fault, got.ipsum, got.xsum, (int)got.ok,
            (int)st.bad);
    if (++fails > 10) exit(1);
  }
  free(st.blk);
  free(pblk);
}

Rec random_rec(std::mt19937_64 &rng, int kind) {
  Rec r;
  uint8_t raw[32];
  for (auto &x : raw) x = kind == 0 ? (uint8_t)rng() : (kind == 1 ? 0x00 : 0xFF);
  memcpy(r.src, raw, 4);
  memcpy(r.dst, raw + 4, 4);
  memcpy(&r.sport, raw + 8, 2), memcpy(&r.dport, raw + 10, 2), memcpy(&r.seq, raw + 12, 4);
  memcpy(&r.ack, raw + 16, 4), memcpy(&r.window, raw + 20, 2);
  r.flags = raw[22], r.ttl = raw[23], r.tos = raw[24];
  memcpy(&r.ip_id, raw + 26, 2), memcpy(&r.frag, raw + 28, 2);
  r.doff = 20, r.proto = 17;
  return r;
}

}  // namespace

int main() {
  std::mt19937_64 rng(20261020);
  static const struct {
    uint8_t proto, doff;
  } kKinds[6] = {{17, 20}, {1, 20}, {47, 20}, {6, 20}, {6, 24}, {6, 60}};
  std::vector<uint32_t> lens;
  for (uint32_t l = 0; l <= 96; ++l) lens.push_back(l);
  for (uint32_t l = 1016; l <= 1032; ++l) lens.push_back(l);
  for (uint32_t L : lens)
    for (int kind = 0; kind < 3; ++kind) {  // random, all 0x00 (ICMP: the all-zero segment), all 0xFF
      std::vector<uint8_t> pay(L + 1);
      for (auto &x : pay) x = kind == 0 ? (uint8_t)rng() : (kind == 1 ? 0x00 : 0xFF);
      for (const auto &k : kKinds) {
        Rec rec = random_rec(rng, kind);
        rec.proto = k.proto, rec.doff = k.doff;
        const int64_t T = 20 + l4_len(k.proto) + L;
        for (uint32_t pa = 0; pa < 4; ++pa)
          for (uint32_t da = 0; da < 4; ++da) {
            Case c;
            c.palign = pa, c.dalign = da;
            run(rec, pay.data(), L, c, "exact room");
            if (kind != 0) continue;
            for (int64_t slack = 1; slack <= 5; ++slack) {
              c.room = T + slack;
              run(rec, pay.data(), L, c, "slack");
            }
            for (int64_t shrt = 1; shrt <= 45 && shrt <= T; ++shrt) {
              c.room = T - shrt;
              run(rec, pay.data(), L, c, "short room");
            }
          }
      }
    }
  // a UDP datagram whose sum is 0xFFFF keeps 0x0000 in its field: all-zero
  // addresses and ports, and a payload word that completes the sum
  {
    Rec rec = random_rec(rng, 1);
    rec.proto = 17;
    const uint8_t pay[2] = {0xFF, (uint8_t)(0xFF - 17 - 10 - 10)};  // less proto and 8 + L, twice
    uint32_t ipsum, xsum;
    scalar_image(rec, pay, 2, ipsum, xsum);
    if (xsum != 0) {
      fprintf(stderr, "udp zero sum: the case does not sum to 0xFFFF (%04x)\n", xsum);
      ++fails;
    }
    run(rec, pay, 2, Case(), "udp zero sum");
  }
  // the device test's contract batch, the limit, and long payloads, at every phase pair
  {
    std::vector<uint8_t> pay(65600);
    for (auto &x : pay) x = (uint8_t)rng();
    for (uint32_t pa = 0; pa < 4; ++pa)
      for (uint32_t da = 0; da < 4; ++da) {
        Case c;
        c.palign = pa, c.dalign = da;
        Rec udp = random_rec(rng, 0), tcp = random_rec(rng, 0);
        tcp.proto = 6, tcp.doff = 24;
        run(udp, pay.data(), 65507, c, "T = 65535");
        Case over = c;
        over.room = 65536;
        run(udp, pay.data(), 65508, over, "T = 65536");
        over.room = 70000;
        run(udp, pay.data(), 65590, over, "T past the limit, room too");
        Case s3 = c;
        s3.room = 20 + 8 + 700 - 3;
        run(udp, pay.data(), 700, s3, "room short by 3");
        Case dec = c;
        dec.decreasing = true;
        run(udp, pay.data(), 700, dec, "dst_offsets decreases");
        run(tcp, pay.data(), 2, c, "doff 24, L = 2");
        Case cut = c;
        cut.cut_by_end = true, cut.room = 300;
        run(udp, pay.data(), 700, cut, "cut by dst_offsets[n]");
        Case pf = c;
        pf.pay_fault = 1;
        run(udp, pay.data(), 700, pf, "pay_offsets decreases");
        pf.pay_fault = 2;
        run(udp, pay.data(), 700, pf, "pay_offsets passes pay_offsets[n]");
        tcp.doff = 20;
        for (uint32_t L : {1459u, 1460u, 1461u, 4099u, 9000u}) run(tcp, pay.data(), L, c, "long");
      }
  }
  return finish();
}
