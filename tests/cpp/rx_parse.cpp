// k_parse on a CPU: one lane's work as yustack_amd/csrc/yucsum_kernels.hip does
// it, with the arithmetic of yucsum_parse.h (which window dwords are loaded, the
// packet dwords d0 .. d4 and t0 .. t3 out of them, the header bits, the view) and
// yucsum_split.h's split_src, split_hdr_lim, split_parse and split_record, held
// against a byte-by-byte restatement of what ipv4.HandlePacket,
// Nic.DeliverTransportPacket, segment.parse and udp.endpoint.HandlePacket do with a
// datagram before its payload is queued.
//
// The batch sits in an exact-size heap block rounded out to whole dwords, so under
// AddressSanitizer a read outside the dwords holding data[0, offsets[n]) is a
// report. Every load goes through `load`, which also records it: a dword outside
// the window of the packet's first min(len, 80) bytes, outside the batch, loaded
// twice by the first pass or a sixteenth load is a failure.
//
// Cases, each at address phase 0 .. 3 (the program prints each group's count):
//   well-formed   IHL 5 .. 15 x {UDP, ICMP, protocol 47, TCP doff 20 / 24 / 60 / 16}
//                 x payload 0, 1, 7, 40, 100 x {the batch ends with the packet;
//                 3 trailing bytes past TL and 5 more batch bytes behind it}
//   short header  IHL 0 .. 4 x the seven kinds x payload 0, 7, 64
//   short packet  len 0 .. 19
//   total length  TL = HL - 1 and TL = len + 1, the seven kinds x payload 0, 7, 64
//   slen = H - 1  TCP, UDP, ICMP x IHL 5, 6, 15
//   doff          TCP doff one dword past slen x IHL 5, 6, 15 x payload 0, 4, 7, 36
//   UDP Length()  slen + 1 and slen - 1 x IHL 5, 6, 15 x payload 0, 7, 64
//   batch end     len 20 .. 100 x IHL 5, 6, 15: TL = len, nothing behind the packet
//   limits        65535 bytes; the contract batch's 65536 bytes, decreasing offsets
//                 and an end past offsets[n]
#include "iov_model.h"
#include "yucsum_parse.h"

namespace {

struct Loads {
  std::vector<uint64_t> at;
  size_t first = 0;  // how many of them the first pass made
  uint32_t operator()(uint64_t a) {
    at.push_back(a);
    uint32_t x;
    memcpy(&x, (const void *)(uintptr_t)a, 4);
    return x;
  }
};

struct Result {
  uint32_t bits;
  yu::BuildRec R;
  yu::ParseView V;
  uint64_t addr;
  uint32_t len;
};

// One lane of k_parse. data: the call's data pointer; (o0, o1, oN): offsets[i],
// [i + 1], [n].
Result kernel_parse(Loads &load, uint64_t data, uint64_t o0, uint64_t o1, uint64_t oN) {
  Result r;
  yu::split_src(data, o0, o1, oN, r.addr, r.len);
  const uint32_t lim = yu::split_hdr_lim(r.addr, r.len), s = (uint32_t)r.addr & 3u;
  const uint64_t base = r.addr & ~3ull;
  uint32_t w[yu::kParseFix];
  const bool whole = yu::parse_whole(lim);  // the kernel's wide loads: the same ten dwords
  for (uint32_t j = 0; j < yu::kParseFix; ++j) w[j] = whole || yu::parse_loads(j, lim) ? load(base + 4u * j) : 0u;
  load.first = load.at.size();
  yu::ParseHdr H;
  yu::parse_fixed(H, w, s);
  if (yu::parse_needs_opt(H, r.len)) {
    uint32_t x[yu::kParseOpt];
    for (uint32_t k = 0; k < yu::kParseOpt; ++k) {
      const uint32_t j = yu::parse_opt_dword(H, k);
      x[k] = yu::parse_loads(j, lim) ? load(base + 4u * j) : 0u;
    }
    yu::parse_opt(H, x, s);
  }
  yu::SplitDg S;
  yu::split_parse(S, r.len, H.d0, H.d2, H.t1, H.t3);
  yu::split_record(r.R, S, H.d0, H.d1, H.d2, H.d3, H.d4, H.t0, H.t1, H.t2, H.t3);
  r.V = yu::parse_view(S, r.addr);
  r.bits = yu::parse_hdr_bits(S, r.len);
  return r;
}

uint32_t l4_len(uint32_t proto) { return proto == 6 ? 20 : (proto == 17 ? 8 : (proto == 1 ? 4 : 0)); }
uint32_t rd16(const uint8_t *p) { return ((uint32_t)p[0] << 8) | p[1]; }
uint32_t rd32(const uint8_t *p) { return (rd16(p) << 16) | rd16(p + 2); }

struct Want {
  uint32_t bits = YU_RX_INVALID;
  yu_tx_record rec;
  uint32_t pay_at = 0, L = 0;  // the payload: packet offset and length
};

// What the reference does with the received datagram b[0, len), step by step (its
// checksums aside: the header pass computes none).
Want reference(const uint8_t *b, uint32_t len) {
  Want w;
  memset(&w.rec, 0, sizeof w.rec);
  // ipv4.HandlePacket: IsValid (header/ipv4.go:126-138), then the header is trimmed
  if (len < 20) return w;
  const uint32_t hl = (b[0] & 15u) * 4u, tl = rd16(b + 2);
  if (hl > tl || tl > len) return w;
  w.bits = 0;
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
  w.bits = YU_RX_SPLIT;
  w.rec = rec;
  w.pay_at = hl + H;
  w.L = slen - H;
  return w;
}

uint64_t max_loads = 0, opt_packets = 0;

// The packet b[0, len) at address phase sa, `after` more batch bytes behind it.
// src_fault: 1 offsets decreases at the packet, 2 it ends past offsets[n], 3 it is
// one byte over the limit (len is 65536).
void run(const std::vector<uint8_t> &b, uint32_t len, uint32_t sa, uint32_t after, int src_fault, const char *what) {
  std::vector<uint8_t> bytes(b.begin(), b.begin() + len);
  bytes.resize(len + after, 0x5A);
  const View v = place(bytes.data(), len + after, sa);
  uint64_t o0 = 4096 + sa, o1 = o0 + len, oN = o1 + after;
  const uint64_t data = v.addr - o0;
  uint32_t use = len;  // the bytes the lane may take
  if (src_fault == 1) o1 = o0 - 1, oN = o0, use = 0;
  if (src_fault == 2) o1 = o0 + len + 77;
  if (src_fault == 3) use = len - 1;
  const Want want = reference(b.data(), use);
  Loads load;
  const Result got = kernel_parse(load, data, o0, o1, oN);
  ++checks;

  const uint64_t want_base = (want.bits & YU_RX_SPLIT) ? data + o0 + want.pay_at : 0;
  bool ok = got.bits == want.bits && memcmp(got.R.w, &want.rec, 32) == 0 && got.V.base == want_base &&
            got.V.len == want.L && got.len == use;
  // the loads: inside the window of the first min(len, 80) bytes and inside the batch
  const uint64_t a0 = (data + o0) & ~3ull;
  const uint64_t win_end = data + o0 + (use < yu::kSplitHdr ? use : yu::kSplitHdr);  // one past the last byte
  const uint64_t batch_end = data + oN;
  bool loads_ok = load.at.size() <= yu::kParseFix + yu::kParseOpt;
  for (size_t i = 0; i < load.at.size(); ++i) {
    const uint64_t a = load.at[i];
    loads_ok = loads_ok && use > 0 && (a & 3u) == 0 && a >= a0 && a < win_end && a < batch_end;
    for (size_t k = 0; k < i && i < load.first; ++k) loads_ok = loads_ok && load.at[k] != a;
  }
  if (load.at.size() > max_loads) max_loads = load.at.size();
  if (load.at.size() > load.first) ++opt_packets;
  if (!ok || !loads_ok) {
    fprintf(stderr, "%s: len %u phase %u after %u src_fault %d: bits %x (want %x) view %llx+%llu (want %llx+%u) loads %zu %s\n",
            what, len, sa, after, src_fault, got.bits, want.bits, (unsigned long long)got.V.base,
            (unsigned long long)got.V.len, (unsigned long long)want_base, want.L, load.at.size(),
            loads_ok ? "" : "LOADS OUT OF BOUNDS");
    if (++fails > 10) exit(1);
  }
  free(v.blk);
}

void put16(std::vector<uint8_t> &v, size_t at, uint32_t x) {
  v[at] = (uint8_t)(x >> 8);
  v[at + 1] = (uint8_t)x;
}

// A received datagram with payload L, random bytes, `trail` bytes past TotalLength.
// Returns its length.
uint32_t datagram_of(std::vector<uint8_t> &b, std::mt19937_64 &rng, uint32_t proto, uint32_t doff, uint32_t ihl,
                     uint32_t L, uint32_t trail) {
  const uint32_t hl = 4 * ihl, tl = hl + l4_len(proto) + L, len = tl + trail;
  b.assign(len + 1, 0);
  for (auto &x : b) x = (uint8_t)rng();
  b[0] = (uint8_t)(0x40u | ihl);
  put16(b, 2, tl);
  b[9] = (uint8_t)proto;
  if (proto == 6) b[hl + 12] = (uint8_t)(((doff / 4) << 4) | (b[hl + 12] & 15u));
  if (proto == 17) put16(b, hl + 4, 8 + L);
  return len;
}

const struct {
  uint8_t proto, doff;
} kKinds[7] = {{17, 20}, {1, 20}, {47, 20}, {6, 20}, {6, 24}, {6, 60}, {6, 16}};

uint64_t group(const char *name, uint64_t before) {
  printf("%llu %s\n", (unsigned long long)(checks - before), name);
  return checks;
}

}  // namespace

int main() {
  std::mt19937_64 rng(20261021);
  std::vector<uint8_t> b;
  uint64_t mark = 0;

  for (uint32_t sa = 0; sa < 4; ++sa)
    for (uint32_t ihl = 5; ihl <= 15; ++ihl)
      for (const auto &k : kKinds)
        for (uint32_t L : {0u, 1u, 7u, 40u, 100u}) {
          run(b, datagram_of(b, rng, k.proto, k.doff, ihl, L, 0), sa, 0, 0, "well-formed");
          run(b, datagram_of(b, rng, k.proto, k.doff, ihl, L, 3), sa, 5, 0, "well-formed, bytes behind");
        }
  mark = group("well-formed", mark);

  for (uint32_t sa = 0; sa < 4; ++sa)
    for (uint32_t ihl = 0; ihl < 5; ++ihl)  // HL < 20 (IsValid accepts)
      for (const auto &k : kKinds)
        for (uint32_t L : {0u, 7u, 64u}) {
          const uint32_t len = datagram_of(b, rng, k.proto, k.doff, 5, L, 0);
          b[0] = (uint8_t)(0x40u | ihl);
          run(b, len, sa, 0, 0, "HL below 20");
        }
  mark = group("short header", mark);

  for (uint32_t sa = 0; sa < 4; ++sa)
    for (uint32_t len = 0; len < 20; ++len) {
      datagram_of(b, rng, 17, 20, 5, 40, 0);
      put16(b, 2, len);  // TL <= len: the length alone makes it invalid
      run(b, len, sa, 0, 0, "len below 20");
    }
  mark = group("short packet", mark);

  for (uint32_t sa = 0; sa < 4; ++sa)
    for (const auto &k : kKinds)
      for (uint32_t L : {0u, 7u, 64u}) {
        uint32_t len = datagram_of(b, rng, k.proto, k.doff, 5, L, 0);
        put16(b, 2, 19);
        run(b, len, sa, 0, 0, "TL below HL");
        len = datagram_of(b, rng, k.proto, k.doff, 5, L, 0);
        put16(b, 2, len + 1);
        run(b, len, sa, 0, 0, "TL past len");
      }
  mark = group("total length", mark);

  for (uint32_t sa = 0; sa < 4; ++sa)
    for (uint32_t ihl : {5u, 6u, 15u})
      for (uint32_t proto : {6u, 17u, 1u}) {
        const uint32_t len = datagram_of(b, rng, proto, 20, ihl, 0, 0) - 1;
        put16(b, 2, len);
        run(b, len, sa, 0, 0, "slen = H - 1");
      }
  mark = group("slen = H - 1", mark);

  for (uint32_t sa = 0; sa < 4; ++sa)
    for (uint32_t ihl : {5u, 6u, 15u})
      for (uint32_t L : {0u, 4u, 7u, 36u})
        run(b, datagram_of(b, rng, 6, ((20 + L) / 4 + 1) * 4, ihl, L, 0), sa, 0, 0, "TCP doff past slen");
  mark = group("doff", mark);

  for (uint32_t sa = 0; sa < 4; ++sa)
    for (uint32_t ihl : {5u, 6u, 15u})
      for (uint32_t L : {0u, 7u, 64u})
        for (int d : {1, -1}) {
          const uint32_t len = datagram_of(b, rng, 17, 20, ihl, L, 0);
          put16(b, 4 * ihl + 4, (uint32_t)((int)(8 + L) + d));
          run(b, len, sa, 0, 0, d > 0 ? "UDP Length() = slen + 1" : "UDP Length() = slen - 1");
        }
  mark = group("UDP Length()", mark);

  for (uint32_t sa = 0; sa < 4; ++sa)
    for (uint32_t len = 20; len <= 100; ++len)
      for (uint32_t ihl : {5u, 6u, 15u}) {
        static const uint32_t kProtos[4] = {6u, 17u, 1u, 47u};
        const uint32_t proto = kProtos[len & 3u];
        b.assign(len + 1, 0);
        for (auto &x : b) x = (uint8_t)rng();
        b[0] = (uint8_t)(0x40u | ihl);
        put16(b, 2, len);
        b[9] = (uint8_t)proto;
        if (proto == 6 && 4 * ihl + 12 < len) b[4 * ihl + 12] = 0x50;
        if (proto == 17 && 4 * ihl + 5 < len) put16(b, 4 * ihl + 4, 8);
        run(b, len, sa, 0, 0, "batch end");
      }
  mark = group("batch end", mark);

  for (uint32_t sa = 0; sa < 4; ++sa) {
    run(b, datagram_of(b, rng, 6, 24, 5, 65535 - 40, 0), sa, 0, 0, "65535 bytes");
    run(b, datagram_of(b, rng, 17, 20, 5, 65535 - 28, 1), sa, 0, 3, "65536 bytes");  // its first 65535 bytes are taken
    run(b, datagram_of(b, rng, 17, 20, 5, 700, 0), sa, 0, 1, "offsets decreases");
    run(b, datagram_of(b, rng, 17, 20, 5, 700, 0), sa, 0, 2, "ends past offsets[n]");
  }
  mark = group("limits", mark);

  // the second load is taken exactly by the packets whose IHL is not 5, and no lane
  // ever makes more than fifteen loads
  printf("%llu packets took the second load, at most %llu loads\n", (unsigned long long)opt_packets,
         (unsigned long long)max_loads);
  if (max_loads != yu::kParseFix + yu::kParseOpt || opt_packets == 0) ++fails;
  return finish();
}
